"""LPIPS-VGG16 without a GPU: the fp64 / fp32 restatement of include/hnrf.h "LPIPS" in plain torch ops, pinned to the
reference's own class through tests/golden/lpips_seeded.npz (tests/make_golden_lpips.py), and the per-kernel references
that tests/test_gpu_lpips.py holds the HIP kernels against.

Bounds (the convention of tests/test_gpu_render_kernels.py): 4 x the error of torch's CPU fp32 evaluation of the same
function against fp64 on the same inputs, computed here, with the lower bounds
    value     1e-6 of the value           (CPU fp32 vs fp64 measured 4.6e-8 .. 3.9e-7 relative)
    gradient  2e-5 of its norm, norm-wise (measured 3.1e-6 .. 5.3e-6)
about 3 x the worst measured case: one case's own floor can by luck lie far below what another summation order gives."""
import functools
import os

import numpy as np
import pytest
import torch

from humannerf_amd.lpips import CONV_IDX, POOL_BEFORE, SCALE, SHIFT, TAP_LAYERS, LpipsVGG, seeded_trunk
from humannerf_amd.ops import LPIPS_CONVS, LPIPS_TAPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 32, 32, 0), (1, 37, 45, 0), (1, 16, 16, 0), (3, 17, 16, 2)]
VALUE_FLOOR, GRAD_FLOOR = 1e-6, 2e-5
F = torch.nn.functional


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'lpips_seeded.npz')))


@functools.lru_cache(maxsize=None)
def trunk(seed=0):
    return seeded_trunk(seed)


def heads():
    return [torch.from_numpy(golden()['lin%d' % t]) for t in range(5)]


def head_state():
    return {'lin%d.model.1.weight' % t: v.reshape(1, -1, 1, 1) for t, v in enumerate(heads())}


def case_key(case):
    return 'n%d_h%d_w%d_s%d' % case


def reference_lpips(trunk_state, lins, in0, in1, dtype=torch.float64, per_layer=False):
    """The arithmetic of hnrf.h "LPIPS" in plain torch ops on the CPU (or any device): in0, in1 (N,3,H,W) -> (N,1,1,1).
    ``lins``: five (C) vectors.  Differentiable; this is what the tests hold the kernels against in fp64."""
    shift = torch.tensor(SHIFT, dtype=dtype, device=in0.device)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=dtype, device=in0.device)[None, :, None, None]
    F = torch.nn.functional

    def taps(x):
        h, outs = (x.to(dtype) - shift) / scale, []
        for l, i in enumerate(CONV_IDX):
            if l in POOL_BEFORE:
                h = F.max_pool2d(h, 2, 2)
            w = trunk_state.get('features.%d.weight' % i, trunk_state.get('%d.weight' % i))
            b = trunk_state.get('features.%d.bias' % i, trunk_state.get('%d.bias' % i))
            h = F.relu(F.conv2d(h, w.to(h), b.to(h), padding=1))
            if l in TAP_LAYERS:
                outs.append(h)
        return outs

    def normalize(f):
        return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True) + 1e-10) + 1e-10)

    vals = []
    for f0, f1, w in zip(taps(in0), taps(in1), lins):
        d = (normalize(f0) - normalize(f1)) ** 2
        vals.append((d * w.to(d).reshape(1, -1, 1, 1)).sum(1, keepdim=True).mean([2, 3], keepdim=True))
    total = vals[0]
    for v in vals[1:]:
        total = total + v
    return (total, vals) if per_layer else total


def value_and_grad(in0, in1, dtype, weight=None, state=None):
    """value (N) and d sum_n weight[n] value[n] / d in0 (N,3,H,W) of the restatement, as numpy fp64."""
    a = torch.as_tensor(in0).to(dtype).requires_grad_(True)
    v = reference_lpips(state or trunk(), heads(), a, torch.as_tensor(in1).to(dtype), dtype).reshape(-1)
    wt = torch.ones_like(v) if weight is None else torch.as_tensor(weight).to(v)
    g, = torch.autograd.grad((v * wt).sum(), a)
    return v.detach().double().numpy(), g.double().numpy()


@functools.lru_cache(maxsize=None)
def case_ref(case):
    """(value64, grad64, value32, grad32) of a fixture case, computed once per session and never modified."""
    g = golden()
    in0, in1 = g[case_key(case) + '_in0'], g[case_key(case) + '_in1']
    return value_and_grad(in0, in1, torch.float64) + value_and_grad(in0, in1, torch.float32)


def check_value(name, got, v64, v32):
    got, v64, v32 = (np.asarray(a, np.float64).reshape(-1) for a in (got, v64, v32))
    tol = np.maximum(4 * np.abs(v32 - v64), VALUE_FLOOR * np.abs(v64))
    err = np.abs(got - v64)
    print('%s value: err/|v| %s  cpu-fp32 floor/|v| %s  err/bound %.3f' % (name, err / np.abs(v64), np.abs(v32 - v64) / np.abs(v64),
                                                                           float((err / tol).max())))
    assert (err <= tol).all(), (name, err, tol)


def check_grad(name, got, g64, g32):
    got, g64, g32 = (np.asarray(a, np.float64) for a in (got, g64, g32))
    nrm = np.linalg.norm(g64)
    tol = max(4 * np.linalg.norm(g32 - g64), GRAD_FLOOR * nrm)
    err = np.linalg.norm(got - g64)
    print('%s grad: err/|g| %.3g  cpu-fp32 floor/|g| %.3g  err/bound %.3f' % (name, err / nrm, np.linalg.norm(g32 - g64) / nrm, err / tol))
    assert err <= tol, (name, err, tol)


# ------------------------------------------------------------------------------------- per-kernel references (NHWC)
def layer_weights(layer, seed=0):
    i = CONV_IDX[layer]
    return trunk(seed)['features.%d.weight' % i], trunk(seed)['features.%d.bias' % i]


def conv_fwd_ref(x, layer, dtype=torch.float64, scale_input=False, relu=True, absolute=False):
    """x (N,H,W,Cin) -> (N,H,W,Cout).  ``absolute``: conv(|x|, |w|) + |b|, the scale of the rounding-error bound."""
    w, b = layer_weights(layer)
    h = torch.as_tensor(x).to(dtype).permute(0, 3, 1, 2)
    if scale_input:
        h = (h - torch.tensor(SHIFT, dtype=dtype)[None, :, None, None]) / torch.tensor(SCALE, dtype=dtype)[None, :, None, None]
    if absolute:
        return (F.conv2d(h.abs(), w.to(dtype).abs(), b.to(dtype).abs(), padding=1)).permute(0, 2, 3, 1)
    y = F.conv2d(h, w.to(dtype), b.to(dtype), padding=1)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


def conv_bwd_ref(dy, y_saved, layer, dtype=torch.float64, unscale=False, absolute=False):
    """dy (N,H,W,Cout), y_saved (same or None) -> dx (N,H,W,Cin) = conv_transpose(dy * (y_saved > 0))."""
    w, _ = layer_weights(layer)
    g = torch.as_tensor(dy).to(dtype)
    if y_saved is not None:
        g = g * (torch.as_tensor(y_saved) > 0).to(dtype)
    g, w = g.permute(0, 3, 1, 2), w.to(dtype)
    if absolute:
        g, w = g.abs(), w.abs()
    dx = F.conv_transpose2d(g, w, padding=1)
    if unscale:
        dx = dx / torch.tensor(SCALE, dtype=dtype)[None, :, None, None]
    return dx.permute(0, 2, 3, 1)


def conv_bound(absref, K):
    """Rounding-error bound of a K-term fp32 fma chain with u = 2^-24: certainly <= K u sum|a b|, and it behaves like
    sqrt(K) u sum|a b|; the bound is 4 sqrt(K) u sum|a b| (+ one rounding of the result)."""
    return (4 * np.sqrt(K) + 1) * 2.0 ** -24 * np.asarray(absref, np.float64) + 1e-37


def pool_fwd_ref(x):
    return F.max_pool2d(torch.as_tensor(x).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)


def pool_bwd_ref(x, dy):
    """torch's CPU autograd of max_pool2d: the gradient goes to the first maximum in row-major scan order."""
    a = torch.as_tensor(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.max_pool2d(a, 2, 2)
    g, = torch.autograd.grad(y, a, torch.as_tensor(dy).permute(0, 3, 1, 2).contiguous())
    return g.permute(0, 2, 3, 1)


def head_ref(f, w, dtype=torch.float64, go=None):
    """f (2N,P,C), w (C) -> v (N); with ``go`` (N) also d sum(go v) / d f[:N] (N,P,C)."""
    f = torch.as_tensor(f).to(dtype)
    N = f.shape[0] // 2
    f0, f1 = f[:N].clone().requires_grad_(go is not None), f[N:]
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(-1, keepdim=True) + 1e-10) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(-1, keepdim=True) + 1e-10) + 1e-10)
    v = (((n0 - n1) ** 2) * torch.as_tensor(w).to(dtype)).sum(-1).mean(-1)
    if go is None:
        return v
    g, = torch.autograd.grad((v * torch.as_tensor(go).to(dtype)).sum(), f0)
    return v.detach(), g


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('case', CASES, ids=case_key)
def test_restatement_reproduces_the_reference_class(case):
    g = golden()
    v64, g64, v32, g32 = case_ref(case)
    for name, v, gr in (('fp64', v64, g64), ('fp32', v32, g32)):
        check_value(case_key(case) + ' ' + name, g[case_key(case) + '_value'], v, v32 if name == 'fp64' else v64)
        check_grad(case_key(case) + ' ' + name, g[case_key(case) + '_grad'], gr, g32 if name == 'fp64' else g64)
    assert g[case_key(case) + '_value'].shape == (case[0],)


def test_fixture_is_what_the_issue_recorded():
    v = golden()['n2_h32_w32_s0_value']
    assert abs(v[0] - 0.00566884) < 5e-9 and abs(v[1] - 0.00536851) < 5e-9
    for t, (_, c) in enumerate(LPIPS_TAPS):
        assert golden()['lin%d' % t].shape == (c,)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'lpips_seeded.npz')) < 256 * 1024


def test_identical_inputs_give_zero():
    x = torch.from_numpy(golden()['n1_h16_w16_s0_in0'])
    for dt in (torch.float32, torch.float64):
        assert float(reference_lpips(trunk(), heads(), x, x.clone(), dt).abs().max()) == 0.0


def test_folding_the_shift_into_the_bias_is_wrong_on_the_border():
    """conv((x - shift) / scale) zero-pads the SCALED image; conv'(x) with w' = w / scale, b' = b - sum w shift / scale
    zero-pads x itself, which is the scaled value shift / scale != 0: equal inside, different on every border pixel."""
    x = torch.from_numpy(golden()['n1_h16_w16_s0_in0']).double()
    w, b = (t.double() for t in layer_weights(0))
    sh, sc = torch.tensor(SHIFT).double()[None, :, None, None], torch.tensor(SCALE).double()[None, :, None, None]
    right = F.conv2d((x - sh) / sc, w, b, padding=1)
    folded = F.conv2d(x, w / sc, b - (w * sh / sc).sum((1, 2, 3)), padding=1)
    diff = (right - folded).abs()
    assert float(diff[:, :, 1:-1, 1:-1].max()) < 1e-12
    border = torch.ones(16, 16, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert float(diff.amax(1)[0][border].min()) > 1e-3


def test_seeded_trunk_recipe():
    rs = np.random.RandomState(0)
    w0 = (rs.standard_normal((64, 3, 3, 3)) * np.sqrt(2. / 27)).astype(np.float32)
    b0 = (rs.standard_normal(64) * 0.05).astype(np.float32)
    assert np.array_equal(trunk()['features.0.weight'].numpy(), w0) and np.array_equal(trunk()['features.0.bias'].numpy(), b0)
    assert [tuple(trunk()['features.%d.weight' % i].shape[:2][::-1]) for i in CONV_IDX] == LPIPS_CONVS
    assert TAP_LAYERS == (1, 3, 6, 9, 12) and POOL_BEFORE == (2, 4, 7, 10)


def test_state_dict_keys():
    st = trunk()
    a = LpipsVGG(st, head_state())
    b = LpipsVGG({k[len('features.'):]: v for k, v in st.items()}, head_state())
    assert all(torch.equal(x, y) for x, y in zip(a.weights + a.biases + a.lins, b.weights + b.biases + b.lins))
    assert len(a.weights) == 13 and len(a.lins) == 5 and a.lins[4].shape == (512,)
    missing = {k: v for k, v in st.items() if k != 'features.17.bias'}
    with pytest.raises(KeyError, match='features.17.bias'):
        LpipsVGG(missing, head_state())
    bad = dict(st)
    bad['features.5.weight'] = torch.zeros(128, 64, 3, 2)
    with pytest.raises(ValueError, match='features.5.weight'):
        LpipsVGG(bad, head_state())
    hs = head_state()
    del hs['lin3.model.1.weight']
    with pytest.raises(KeyError, match='lin3.model.1.weight'):
        LpipsVGG(st, hs)
    hs = head_state()
    hs['lin0.model.1.weight'] = torch.zeros(1, 65, 1, 1)
    with pytest.raises(ValueError, match='lin0.model.1.weight'):
        LpipsVGG(st, hs)


def test_load_reads_plain_state_dicts(tmp_path):
    torch.save(trunk(), str(tmp_path / 'vgg16.pth'))
    torch.save(head_state(), str(tmp_path / 'vgg.pth'))
    lp = LpipsVGG.load(str(tmp_path / 'vgg16.pth'), str(tmp_path / 'vgg.pth'))
    assert torch.equal(lp.weights[12], trunk()['features.28.weight']) and torch.equal(lp.lins[2], heads()[2])


def test_sizes_below_16_are_refused():
    from humannerf_amd import _lib
    lp = LpipsVGG(trunk(), head_state())
    for shape in ((1, 3, 15, 16), (1, 3, 16, 15)):
        with pytest.raises(ValueError, match='>= 16'):
            lp(torch.zeros(shape), torch.zeros(shape))
    lib = _lib.load()
    assert lib.hnrf_lpips_workspace_bytes(1, 15, 16, 0) == 0 and lib.hnrf_lpips_workspace_bytes(1, 16, 15, 1) == 0
    assert lib.hnrf_lpips_workspace_bytes(1, 16, 16, 1) > lib.hnrf_lpips_workspace_bytes(1, 16, 16, 0) > 0
    assert lib.hnrf_lpips_fwd(256, 256, 256, 1, 15, 16, 0, 256, 1 << 30, 256, None, None) == -2
    assert '15' in lib.hnrf_last_error().decode()
    assert lib.hnrf_lpips_bwd(256, 256, 1, 16, 15, 256, 1 << 30, 256, None) == -2


def test_abi_argument_errors_do_not_need_a_gpu():
    from humannerf_amd import _lib
    lib = _lib.load()
    err = lambda: lib.hnrf_last_error().decode()
    assert lib.hnrf_lpips_packed_bytes() > 2 * 4 * 14710464          # both images of the 14.7 M trunk weights
    assert lib.hnrf_lpips_pack(None, None, None, None, None) == -1 and 'null pointer' in err()
    assert lib.hnrf_conv3x3_fwd(None, 256, 0, 1, 4, 4, 0, 256, None) == -1 and 'null pointer' in err()
    assert lib.hnrf_conv3x3_fwd(256, 256, 13, 1, 4, 4, 0, 256, None) == -2 and 'layer 13' in err()
    assert lib.hnrf_conv3x3_fwd(256, 256, 1, 1, 4, 4, 1, 256, None) == -2 and 'scaling layer' in err()
    assert lib.hnrf_conv3x3_fwd(256, 256, 1, 1, 0, 4, 0, 256, None) == -2
    assert lib.hnrf_conv3x3_fwd(256, 256, 12, 64, 512, 512, 0, 256, None) == -2 and '31 bits' in err()
    assert lib.hnrf_conv3x3_fwd(260, 256, 1, 1, 4, 4, 0, 256, None) == -1 and 'aligned' in err()
    assert lib.hnrf_conv3x3_bwd_data(256, None, 256, 0, 1, 4, 4, 0, None, None) == -1
    assert lib.hnrf_conv3x3_bwd_data(256, None, 256, -1, 1, 4, 4, 0, 256, None) == -2
    assert lib.hnrf_conv3x3_bwd_data(256, None, 256, 2, 1, 4, 4, 1, 256, None) == -2
    assert lib.hnrf_maxpool2_fwd(None, 1, 4, 4, 64, 256, None) == -1
    assert lib.hnrf_maxpool2_fwd(256, 1, 4, 4, 6, 256, None) == -2 and 'C=6' in err()
    assert lib.hnrf_maxpool2_bwd(256, None, 1, 4, 4, 64, 256, None) == -1
    assert lib.hnrf_maxpool2_bwd(256, 256, 1, 4, 4, 3, 256, None) == -2
    assert lib.hnrf_lpips_head_fwd(256, 256, 1, 4, 64, None, 256, 0, None, None) == -1
    assert lib.hnrf_lpips_head_fwd(256, 256, 1, 4, 96, 256, 256, 0, None, None) == -2 and 'C=96' in err()
    assert lib.hnrf_lpips_head_bwd(256, 256, None, 1, 4, 64, 256, 0, None) == -1
    assert lib.hnrf_lpips_head_bwd(256, 256, 256, 1, 0, 64, 256, 0, None) == -2
    assert lib.hnrf_lpips_fwd(256, None, 256, 1, 16, 16, 0, 256, 1 << 30, 256, None, None) == -1
    assert lib.hnrf_lpips_fwd(256, 256, 256, 1, 16, 16, 0, 256, 16, 256, None, None) == -4 and 'workspace' in err()
    assert lib.hnrf_lpips_fwd(256, 256, 256, 1, 16, 16, 0, 264, 1 << 30, 256, None, None) == -1 and 'aligned' in err()
    assert lib.hnrf_lpips_bwd(None, 256, 1, 16, 16, 256, 1 << 30, 256, None) == -1
    assert lib.hnrf_lpips_bwd(256, 256, 1, 16, 16, 256, 16, 256, None) == -4
