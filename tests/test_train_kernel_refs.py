"""fp64 references of the training kernels (tests/test_gpu_train_kernels.py) and the checks of those references that
need no GPU: they are compared here with torch.autograd through the oracle's own, independently written forwards and
with central finite differences, and the blocked-layout helpers are checked to be inverse to each other."""
import numpy as np
import pytest
import torch

from oracle import oracle

CNL_NAMES = [f'cnl_mlp.module.pts_linears.{i}' for i in (0, 2, 4, 6, 8, 10, 12, 14)] + ['cnl_mlp.module.output_linear.0']
NR_NAMES = [f'non_rigid_mlp.module.block_mlps.{i}' for i in (0, 2, 4, 6, 8, 10, 12)]
# hidden layers, width, mask words per sample, head outputs, real PE columns, skip layer and the order of its input
SPECS = {'canonical': dict(L=8, W=256, nb=8, n_out=4, npe=63, skip=5, order='pe_first', names=CNL_NAMES),
         'nonrigid': dict(L=6, W=128, nb=4, n_out=3, npe=36, skip=4, order='h_first', names=NR_NAMES)}


def make_problem(kind, P, seed, regime=None, dense_g=False):
    """Weights (tests/test_gpu_parity.py::_mlp_states, optionally in one of the non-rigid regimes), positions and an
    incoming gradient for one MLP: numpy fp32."""
    from tests.test_gpu_parity import _apply_regime, _mlp_states
    rs = np.random.RandomState(seed)
    st = _mlp_states(rs)
    if regime is not None:
        st = _apply_regime(st, regime, rs)
    spec = SPECS[kind]
    pr = dict(kind=kind, P=P, st=st, ws=[st[n + '.weight'] for n in spec['names']], bs=[st[n + '.bias'] for n in spec['names']])
    if kind == 'canonical':
        pr['x'] = rs.uniform(-1.2, 1.2, (P, 3)).astype(np.float32)
        keep = np.ones((P, 1)) if dense_g else (rs.uniform(size=(P, 1)) > 0.3)
        pr['g'] = (rs.standard_normal((P, 4)) * keep).astype(np.float32)
    else:
        pr['x'] = rs.uniform(-1.0, 1.0, (P, 3)).astype(np.float32)
        pr['g'] = rs.standard_normal((P, 3)).astype(np.float32)
        pr['cond'] = (rs.standard_normal(69) * 0.3).astype(np.float32)
        pr['hann'] = np.array([1.0, 1.0, 0.75, 0.25, 0.0, 0.0], np.float32)
    return pr


def ref_mlp(pr, masks=None, grad=False):
    """Both MLPs in plain torch, fp64 (mlp_rgb_sigma.py:132-198 / mlp_offset.py:74-114 on fourier.py / hannw_fourier.py).
    masks: per hidden layer a (P, W) 0/1 matrix applied INSTEAD of relu (the kernel's own sign pattern, so that a
    pre-activation within rounding of zero cannot flip a whole term of a gradient); None: relu.
    Returns dict(x, ws, bs: the leaves; pe; acts: post-activation of every hidden layer; out: raw / xyz; offsets)."""
    spec = SPECS[pr['kind']]
    leaf = lambda a: torch.from_numpy(a).double().requires_grad_(grad)
    x, ws, bs = leaf(pr['x']), [leaf(w) for w in pr['ws']], [leaf(b) for b in pr['bs']]
    if pr['kind'] == 'canonical':
        pe = oracle.fourier_pe(x, 10)
        h = pe
    else:
        pe = oracle.hann_pe(x, torch.from_numpy(pr['hann']).double())
        h = torch.cat([torch.from_numpy(pr['cond']).double().expand(x.shape[0], 69), pe], -1)
    acts = []
    for l in range(spec['L']):
        if l == spec['skip']:
            h = torch.cat([pe, h], -1) if spec['order'] == 'pe_first' else torch.cat([h, pe], -1)
        z = torch.nn.functional.linear(h, ws[l], bs[l])
        h = torch.relu(z) if masks is None else z * masks[l]
        acts.append(h)
    out = torch.nn.functional.linear(h, ws[-1], bs[-1])
    res = dict(x=x, ws=ws, bs=bs, pe=pe, acts=acts, out=out, offsets=None)
    if pr['kind'] == 'nonrigid':
        res['offsets'], res['out'] = out, x + out
    return res


def ref_mlp_grads(pr, masks, g=None):
    """fp64 autograd of ref_mlp for the loss <out, g>: dict(d_x, dW [L + 1], db [L + 1], dZ [L]: the gradient at every
    hidden layer's pre-activation) plus the forward."""
    r = ref_mlp(pr, masks, grad=True)
    for a in r['acts']:
        a.retain_grad()
    r['out'].backward(torch.from_numpy(pr['g'] if g is None else g).double())
    r.update(d_x=r['x'].grad, dW=[w.grad for w in r['ws']], db=[b.grad for b in r['bs']],
             dZ=[a.grad * masks[l] for l, a in enumerate(r['acts'])])      # acts = z * mask: dL/dz = dL/dacts * mask
    return r


def ref_weight_grads_from_operands(spec, dZ, acts, pe, g):
    """dW / db of every layer as fp64 products of GIVEN operands (the values the kernels saved): dZ [L] (P, W) un-scaled,
    acts [L] (P, W), pe (P, npe), g (P, n_out) the gradient at the head.  The layer-0 weight of the non-rigid MLP is
    returned without its condition-code columns."""
    L = spec['L']
    dW, db = [], []
    for l in range(L):
        if l == 0:
            X = pe
        elif l == spec['skip']:
            X = torch.cat([pe, acts[l - 1]], -1) if spec['order'] == 'pe_first' else torch.cat([acts[l - 1], pe], -1)
        else:
            X = acts[l - 1]
        dW.append(dZ[l].T @ X)
        db.append(dZ[l].sum(0))
    dW.append(g.T @ acts[L - 1])
    db.append(g.sum(0))
    return dW, db


def composite_problem(R, S, regime, seed=5):
    """Inputs of hnrf_composite_bwd.  'sparse': tests/test_gpu_grad.py::test_composite_bwd_kernel's.  'dense' / 'opaque':
    mask = 1 on the middle third of the ray and 0 elsewhere with sigma ~ N(200, 20) / N(2e4, 20): the transmittance
    collapses with live samples behind it; in 'opaque' exp(-sigma dist) underflows and 1 - alpha + 1e-10 is the floor."""
    rs = np.random.RandomState(seed)
    raw = rs.randn(R, S, 4).astype(np.float32) * 2
    mask = rs.uniform(0, 1.1, (R, S)).astype(np.float32)
    if regime == 'sparse':
        raw[..., 3] = rs.randn(R, S) * 20 + 5
    else:
        raw[..., 3] = rs.randn(R, S) * 20 + (200.0 if regime == 'dense' else 2e4)
        mask[:] = 0.0
        mask[:, S // 3:max(S // 3 + 1, 2 * S // 3)] = 1.0
    z = np.sort(1 + rs.uniform(0, 3, (R, S)).astype(np.float32), axis=1)
    rays_d = rs.randn(R, 3).astype(np.float32)
    bg = np.array([200., 100., 30.], dtype=np.float32)
    g_rgb, g_a, g_d = rs.randn(R, 3).astype(np.float32), rs.randn(R).astype(np.float32), rs.randn(R).astype(np.float32)
    return dict(raw=raw, mask=mask, z=z, rays_d=rays_d, bg=bg, g_rgb=g_rgb, g_a=g_a, g_d=g_d)


def ref_composite_grads(c, dtype=torch.float64, with_alpha_depth=True):
    """(d_raw, d_mask): torch.autograd through oracle.raw2outputs in ``dtype`` on the CPU."""
    t = lambda a: torch.from_numpy(a).to(dtype)
    R, S = c['z'].shape
    rt, mt = t(c['raw']).requires_grad_(True), t(c['mask']).requires_grad_(True)
    o = oracle.raw2outputs(rt, mt, t(c['z']), t(c['rays_d']), torch.zeros(R, S, 3, dtype=dtype), t(c['bg']))
    loss = (o['rgb'] * t(c['g_rgb'])).sum()
    if with_alpha_depth:
        loss = loss + (o['alpha'] * t(c['g_a'])).sum() + (o['depth'] * t(c['g_d'])).sum()
    loss.backward()
    return rt.grad, mt.grad


def ref_pe_grad(x, g, n_bands, hann_w):
    """d <PE(x), g> / dx in fp64; hann_w None: fourier.py with the input term, else hannw_fourier.py."""
    xt = torch.from_numpy(x).double().requires_grad_(True)
    pe = oracle.fourier_pe(xt, n_bands) if hann_w is None else oracle.hann_pe(xt, torch.from_numpy(hann_w).double())
    (pe * torch.from_numpy(g).double()).sum().backward()
    return xt.grad


# ------------------------------------------------------------------------------------------------ checks (no GPU)
@pytest.mark.parametrize('W', [128, 256])
@pytest.mark.parametrize('P', [1, 127, 128, 129, 777])
def test_blocked_layout_helpers_are_inverse(P, W):
    from tests.test_gpu_grad import _rows, _to_blocked
    m = torch.from_numpy(np.random.RandomState(P + W).standard_normal((P, W)).astype(np.float32)).half()
    b = _to_blocked(m)
    assert b.shape == ((P + 127) // 128 * 128, W)
    assert torch.equal(_rows(b, P, True), m)
    full = _rows(b, b.shape[0], True)
    assert torch.equal(full[:P], m) and float(full[P:].abs().max() if full.shape[0] > P else 0.0) == 0.0
    # a permutation of the padded matrix, and not the identity: every value is somewhere, rows really move
    assert torch.equal(b.flatten().sort().values, full.flatten().sort().values)
    if P >= 127:
        assert not torch.equal(b[:P], m)


@pytest.mark.parametrize('kind', ['canonical', 'nonrigid'])
def test_mlp_reference_matches_oracle_autograd_and_finite_differences(kind):
    """ref_mlp / ref_mlp_grads at P = 129 against (a) the oracle's own forward of the same MLP (oracle.canonical_mlp /
    non_rigid_mlp: written separately, from the state dict) and torch.autograd through it, (b) central differences."""
    P = 129
    pr = make_problem(kind, P, 31, 'scaled' if kind == 'nonrigid' else None)
    spec = SPECS[kind]
    st = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in pr['st'].items()}
    x = torch.from_numpy(pr['x']).double().requires_grad_(True)
    hidden = []
    if kind == 'canonical':
        out = oracle.canonical_mlp(st, oracle.fourier_pe(x, 10), hidden)
    else:
        out, _ = oracle.non_rigid_mlp(st, oracle.hann_pe(x, torch.from_numpy(pr['hann']).double()),
                                      torch.from_numpy(pr['cond']).double()[None], x, hidden)
    g = torch.from_numpy(pr['g']).double()
    for hd in hidden:
        hd.retain_grad()
    (out * g).sum().backward()
    masks = [(hd > 0).double().detach() for hd in hidden]
    r = ref_mlp_grads(pr, masks)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert len(hidden) == spec['L'] and close(r['out'].detach(), out.detach())
    assert all(close(a.detach(), b.detach()) for a, b in zip(r['acts'], hidden))
    assert close(r['d_x'], x.grad)
    for l, n in enumerate(spec['names']):
        assert close(r['dW'][l], st[n + '.weight'].grad) and close(r['db'][l], st[n + '.bias'].grad), n
    for l in range(spec['L']):      # relu: dL/dz = dL/dh where h > 0
        assert close(r['dZ'][l], hidden[l].grad * masks[l])
    # the operand products: db is the column sum of dZ, dW its product with the layer's input
    pe = r['pe'].detach()
    dW, db = ref_weight_grads_from_operands(spec, r['dZ'], [a.detach() for a in r['acts']], pe, g)
    for l in range(spec['L'] + 1):
        want = r['dW'][l] if not (kind == 'nonrigid' and l == 0) else r['dW'][0][:, 69:]
        assert close(dW[l], want) and close(db[l], r['db'][l]), l
    if kind == 'nonrigid':           # the condition-code columns: the same vector for every sample
        assert close(db[0][:, None] * torch.from_numpy(pr['cond']).double()[None], r['dW'][0][:, :69])
    # central differences of the masked forward (piecewise linear in the weights: step size is uncritical)
    rs = np.random.RandomState(0)

    def loss_at(mut):
        q = dict(pr, ws=[w.astype(np.float64) for w in pr['ws']], bs=[b.astype(np.float64) for b in pr['bs']],
                 x=pr['x'].astype(np.float64))
        mut(q)
        with torch.no_grad():
            return float((ref_mlp(q, masks)['out'] * g).sum())
    for l in (0, spec['skip'], spec['L']):
        o, i = rs.randint(pr['ws'][l].shape[0]), rs.randint(pr['ws'][l].shape[1])
        def bump(q, s, l=l, o=o, i=i):
            q['ws'][l] = q['ws'][l].copy()
            q['ws'][l][o, i] += s
        fd = (loss_at(lambda q: bump(q, 1e-4)) - loss_at(lambda q: bump(q, -1e-4))) / 2e-4
        assert abs(fd - float(r['dW'][l][o, i])) <= 1e-7 * max(1.0, abs(fd)), (l, o, i)
    for s_i, ax in ((0, 0), (P - 1, 2)):
        def bump(q, s, s_i=s_i, ax=ax):
            q['x'] = q['x'].copy()
            q['x'][s_i, ax] += s
        fd = (loss_at(lambda q: bump(q, 1e-6)) - loss_at(lambda q: bump(q, -1e-6))) / 2e-6
        assert abs(fd - float(r['d_x'][s_i, ax])) <= 1e-5 * max(1.0, abs(fd)), (s_i, ax)


@pytest.mark.parametrize('regime', ['sparse', 'dense', 'opaque'])
def test_composite_reference_matches_closed_form(regime):
    """ref_composite_grads (autograd through oracle.raw2outputs) at R = 3, S = 129 against the closed form of the same
    derivative written out sample by sample in numpy fp64 (the formula in csrc/hnrf_backward.hip's header comment), and
    the fp32 evaluation that serves as the noise floor of the dense regimes is finite."""
    c = composite_problem(3, 129, regime)
    d_raw, d_mask = ref_composite_grads(c)
    R, S = c['z'].shape
    raw, mask, z = c['raw'].astype(np.float64), c['mask'].astype(np.float64), c['z'].astype(np.float64)
    want_raw, want_mask = np.zeros((R, S, 4)), np.zeros((R, S))
    for r in range(R):
        dist = np.append(z[r, 1:] - z[r, :-1], 1e10) * np.linalg.norm(c['rays_d'][r].astype(np.float64))
        e = np.exp(-np.maximum(raw[r, :, 3], 0) * dist)
        a = (1 - e) * mask[r]
        t = 1 - a + 1e-10
        T = np.append(1.0, np.cumprod(t)[:-1])
        col = 1 / (1 + np.exp(-raw[r, :, :3]))
        gw = (col - c['bg'].astype(np.float64) / 255) @ c['g_rgb'][r].astype(np.float64) + c['g_a'][r] + c['g_d'][r] * z[r]
        w = a * T
        for i in range(S):
            da = T[i] * gw[i] - (gw[i + 1:] * w[i + 1:]).sum() / t[i]
            want_raw[r, i, :3] = w[i] * c['g_rgb'][r] * col[i] * (1 - col[i])
            want_raw[r, i, 3] = da * mask[r, i] * dist[i] * e[i] if raw[r, i, 3] > 0 else 0.0
            want_mask[r, i] = da * (1 - e[i])
    for got, want in ((d_raw.numpy(), want_raw), (d_mask.numpy(), want_mask)):
        assert np.isfinite(got).all()
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    f_raw, f_mask = ref_composite_grads(c, torch.float32)
    assert bool(torch.isfinite(f_raw).all()) and bool(torch.isfinite(f_mask).all())
    # without the optional upstream gradients: the same as zeros for them
    n_raw, n_mask = ref_composite_grads(c, with_alpha_depth=False)
    z_raw, z_mask = ref_composite_grads(dict(c, g_a=c['g_a'] * 0, g_d=c['g_d'] * 0))
    assert torch.equal(n_raw, z_raw) and torch.equal(n_mask, z_mask)


def test_pe_reference_matches_finite_differences():
    rs = np.random.RandomState(3)
    P = 129
    x = rs.uniform(-1.2, 1.2, (P, 3)).astype(np.float32)
    for nb, hw in ((10, None), (6, np.array([1, 1, 0.7, 0.2, 0, 0], dtype=np.float32))):
        C = 6 * nb + (3 if hw is None else 0)
        g = rs.randn(P, C).astype(np.float32)
        got = ref_pe_grad(x, g, nb, hw)
        x64, g64 = torch.from_numpy(x).double(), torch.from_numpy(g).double()
        f = lambda xx: ((oracle.fourier_pe(xx, nb) if hw is None else oracle.hann_pe(xx, torch.from_numpy(hw).double())) * g64).sum(-1)
        for ax in range(3):
            d = torch.zeros(3, dtype=torch.float64)
            d[ax] = 1e-6
            fd = (f(x64 + d) - f(x64 - d)) / 2e-6
            assert float((fd - got[:, ax]).abs().max()) <= 1e-5 * float(got.abs().max())
