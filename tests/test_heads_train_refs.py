"""The fp64 reference of the all-heads training kernels (tests/test_gpu_heads_train_kernels.py), checked without a GPU.
The reference is torch.autograd through the oracle's canonical MLP on the state whose output_linear.0 is (4H, 256); it is
compared with the references of tests/test_train_kernel_refs.py driven with the wide head layer (what the GPU tests
use), with the SUM of the single-head references over the heads (the gradient is linear in the incoming planes), and
with central finite differences."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import multihead_cases as mc
from tests.heads_train_cases import HEAD_COUNTS, head_problem, make_heads_problem, wide_gradient
from tests.test_train_kernel_refs import CNL_NAMES, ref_mlp, ref_mlp_grads


def oracle_heads_grads(pr):
    """Autograd through oracle.canonical_mlp on the multi-head state for the loss sum_h <raw_h, g_h>:
    dict(out (P, 4H), hidden, masks, d_x, dW [9], db [9], dZ [8])."""
    st = dict(pr['st'])
    st[mc.W_KEY], st[mc.B_KEY] = pr['ws'][-1], pr['bs'][-1]
    assert mc.n_heads_of(st) == pr['H']
    st = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for k, v in st.items()}
    x = torch.from_numpy(pr['x']).double().requires_grad_(True)
    hidden = []
    out = oracle.canonical_mlp(st, oracle.fourier_pe(x, 10), hidden)
    for hd in hidden:
        hd.retain_grad()
    (out * torch.from_numpy(wide_gradient(pr['g'])).double()).sum().backward()
    masks = [(hd > 0).double().detach() for hd in hidden]
    return dict(out=out.detach(), hidden=hidden, masks=masks, d_x=x.grad,
                dW=[st[n + '.weight'].grad for n in CNL_NAMES], db=[st[n + '.bias'].grad for n in CNL_NAMES],
                dZ=[hd.grad * m for hd, m in zip(hidden, masks)])


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('H', HEAD_COUNTS)
def test_all_heads_reference_is_the_oracle_and_the_sum_of_the_single_head_references(H):
    P = 129
    pr = make_heads_problem(H, P, 40 + H)
    o = oracle_heads_grads(pr)
    # (a) the wide-head reference the GPU tests use
    r = ref_mlp_grads(pr, o['masks'], wide_gradient(pr['g']))
    assert tuple(r['out'].shape) == (P, 4 * H) and close(r['out'].detach(), o['out'])
    assert close(r['d_x'], o['d_x'])
    for l in range(9):
        assert close(r['dW'][l], o['dW'][l]) and close(r['db'][l], o['db'][l]), l
    for l in range(8):
        assert close(r['dZ'][l], o['dZ'][l]), l
    # the planes of the forward: the multi-head twin of tests/multihead_cases.py, head by head
    raws = mc.heads_raw64(dict(pr['st'], **{mc.W_KEY: pr['ws'][-1], mc.B_KEY: pr['bs'][-1]}), xyz=pr['x'])
    for h in range(H):
        assert close(torch.from_numpy(raws[h]), o['out'][:, 4 * h:4 * h + 4])
    # (b) linearity: the single-head references summed over the heads; the head layer's rows are each head's own
    singles = [ref_mlp_grads(head_problem(pr, h), o['masks']) for h in range(H)]
    assert close(sum(s['d_x'] for s in singles), o['d_x'])
    for l in range(8):
        assert close(sum(s['dW'][l] for s in singles), o['dW'][l]) and close(sum(s['db'][l] for s in singles), o['db'][l]), l
        assert close(sum(s['dZ'][l] for s in singles), o['dZ'][l]), l
    for h, s in enumerate(singles):
        assert close(s['dW'][8], o['dW'][8][4 * h:4 * h + 4]) and close(s['db'][8], o['db'][8][4 * h:4 * h + 4]), h
        assert close(s['out'].detach(), o['out'][:, 4 * h:4 * h + 4]), h


def test_all_heads_reference_matches_finite_differences():
    """Central differences of the masked forward (piecewise linear in the weights), as
    test_mlp_reference_matches_oracle_autograd_and_finite_differences does: a trunk weight, the skip layer, one weight of
    the first and of the last head, and two coordinates."""
    H, P = 5, 129
    pr = make_heads_problem(H, P, 77)
    o = oracle_heads_grads(pr)
    g = torch.from_numpy(wide_gradient(pr['g'])).double()
    rs = np.random.RandomState(0)

    def loss_at(mut):
        q = dict(pr, ws=[w.astype(np.float64) for w in pr['ws']], bs=[b.astype(np.float64) for b in pr['bs']],
                 x=pr['x'].astype(np.float64))
        mut(q)
        with torch.no_grad():
            return float((ref_mlp(q, o['masks'])['out'] * g).sum())
    picks = [(0, rs.randint(256), rs.randint(63)), (5, rs.randint(256), rs.randint(319)), (8, 1, rs.randint(256)),
             (8, 4 * (H - 1) + 3, rs.randint(256))]
    for l, r_, c_ in picks:
        def bump(q, s, l=l, r_=r_, c_=c_):
            q['ws'][l] = q['ws'][l].copy()
            q['ws'][l][r_, c_] += s
        fd = (loss_at(lambda q: bump(q, 1e-4)) - loss_at(lambda q: bump(q, -1e-4))) / 2e-4
        assert abs(fd - float(o['dW'][l][r_, c_])) <= 1e-7 * max(1.0, abs(fd)), (l, r_, c_)
    for s_i, ax in ((0, 0), (P - 1, 2)):
        def bump(q, s, s_i=s_i, ax=ax):
            q['x'] = q['x'].copy()
            q['x'][s_i, ax] += s
        fd = (loss_at(lambda q: bump(q, 1e-6)) - loss_at(lambda q: bump(q, -1e-6))) / 2e-6
        assert abs(fd - float(o['d_x'][s_i, ax])) <= 1e-5 * max(1.0, abs(fd)), (s_i, ax)
