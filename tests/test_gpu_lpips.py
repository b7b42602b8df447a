"""LPIPS-VGG16 on the GPU (include/hnrf.h "LPIPS", humannerf_amd/csrc/hnrf_lpips.hip): every kernel on its own against
fp64, then the whole path against the reference's own class (tests/golden/lpips_seeded.npz) and the fp64 restatement,
then the training and metric glue.  References and bounds: tests/test_lpips_refs.py.  Every check prints its error-to-bound
ratio before it asserts (run with -s)."""
import os

import numpy as np
import pytest
import torch

from tests import test_lpips_refs as refs

pytestmark = pytest.mark.gpu

NAN = float('nan')
# trunk layer of every (Cin, Cout) pair of VGG16
PAIR_LAYER = {(3, 64): 0, (64, 64): 1, (64, 128): 2, (128, 128): 3, (128, 256): 4, (256, 256): 5, (256, 512): 7, (512, 512): 8}
SMALL_SHAPES = [(1, 1, 1), (1, 2, 2), (2, 3, 5), (1, 7, 9)]              # 1, 4, 30, 63 pixels
CONV_CASES = [(l, s) for l in PAIR_LAYER.values() for s in SMALL_SHAPES]
CONV_CASES += [(l, s) for l in (0, 1, 2, 3, 4) for s in [(3, 16, 16), (1, 33, 31)]] + [(8, (3, 16, 16))]
# the two large tilings start at 128 tiles per image (hnrf_lpips.hip): 256 x 64 tiles for 64 output channels at
# H W > 32512, 128 x 128 tiles for 128 at H W > 16256 and for 256 at H W > 8064; the last tile of each is ragged
BIG_CASES = [(1, (1, 181, 181)), (3, (1, 127, 130)), (5, (1, 90, 91))]
CONV_IDS = lambda c: 'L%d_%dx%dx%d' % ((c[0],) + c[1])


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lp():
    from humannerf_amd.lpips import LpipsVGG
    return LpipsVGG(refs.trunk(), refs.head_state())


@pytest.fixture(scope='module')
def packed(lp):
    return lp.packed(dev())


def _guarded(shape, fill):
    """A tensor of ``shape`` inside a larger buffer filled with ``fill``; returns (view, guard region)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 1024,), fill, device=dev())
    return buf[:n].view(shape), buf[n:]


def _conv_inputs(layer, shape, seed):
    from humannerf_amd.ops import LPIPS_CONVS
    ci, co = LPIPS_CONVS[layer]
    rs = np.random.RandomState(1000 * layer + seed + shape[1] * 7 + shape[2])
    x = rs.standard_normal(shape + (ci,)).astype(np.float32)
    dy = rs.standard_normal(shape + (co,)).astype(np.float32)
    ys = np.maximum(rs.standard_normal(shape + (co,)), 0).astype(np.float32)      # about half of the mask is zero
    return x, dy, ys


def _check_conv(name, got, ref, absref, K):
    err = np.abs(got.double().cpu().numpy() - ref.numpy())
    tol = refs.conv_bound(absref.numpy(), K)
    print('%s: max err %.3g, err/bound %.3f' % (name, err.max(), float((err / tol).max())))
    assert np.isfinite(got.cpu().numpy()).all()
    assert (err <= tol).all(), (name, float((err / tol).max()))


@pytest.mark.parametrize('case', CONV_CASES + BIG_CASES, ids=CONV_IDS)
def test_conv3x3_forward_against_fp64(case, packed):
    from humannerf_amd import ops
    layer, shape = case
    x, _, _ = _conv_inputs(layer, shape, 0)
    y_nan, guard = _guarded(shape + (ops.LPIPS_CONVS[layer][1],), NAN)
    ops.conv3x3_fwd(torch.from_numpy(x).to(dev()), packed, layer, scale_input=(layer == 0), out=y_nan)
    y_zero, _ = _guarded(y_nan.shape, 0.0)
    ops.conv3x3_fwd(torch.from_numpy(x).to(dev()), packed, layer, scale_input=(layer == 0), out=y_zero)
    torch.cuda.synchronize()
    assert torch.equal(y_nan, y_zero) and bool(torch.isnan(guard).all())
    _check_conv('conv fwd ' + CONV_IDS(case), y_nan, refs.conv_fwd_ref(x, layer, scale_input=(layer == 0)),
                refs.conv_fwd_ref(x, layer, scale_input=(layer == 0), absolute=True), 9 * ops.LPIPS_CONVS[layer][0] + 1)


def test_conv3x3_first_layer_without_the_scaling_layer(packed):
    from humannerf_amd import ops
    x, _, _ = _conv_inputs(0, (2, 5, 6), 3)
    y = ops.conv3x3_fwd(torch.from_numpy(x).to(dev()), packed, 0)
    _check_conv('conv fwd L0 unscaled', y, refs.conv_fwd_ref(x, 0), refs.conv_fwd_ref(x, 0, absolute=True), 28)


@pytest.mark.parametrize('case', CONV_CASES + BIG_CASES, ids=CONV_IDS)
def test_conv3x3_backward_data_against_fp64(case, packed):
    """dx of the reversed channel pair (64 -> 3 included), the incoming gradient masked by a saved output with zeros."""
    from humannerf_amd import ops
    layer, shape = case
    _, dy, ys = _conv_inputs(layer, shape, 1)
    assert (ys == 0).any() or ys.size < 64
    d_nan, guard = _guarded(shape + (ops.LPIPS_CONVS[layer][0],), NAN)
    args = (torch.from_numpy(dy).to(dev()), torch.from_numpy(ys).to(dev()), packed, layer)
    ops.conv3x3_bwd_data(*args, unscale_output=(layer == 0), out=d_nan)
    d_zero, _ = _guarded(d_nan.shape, 0.0)
    ops.conv3x3_bwd_data(*args, unscale_output=(layer == 0), out=d_zero)
    torch.cuda.synchronize()
    assert torch.equal(d_nan, d_zero) and bool(torch.isnan(guard).all())
    _check_conv('conv bwd ' + CONV_IDS(case), d_nan, refs.conv_bwd_ref(dy, ys, layer, unscale=(layer == 0)),
                refs.conv_bwd_ref(dy, ys, layer, unscale=(layer == 0), absolute=True), 9 * ops.LPIPS_CONVS[layer][1] + 1)


def test_conv3x3_backward_data_without_a_mask(packed):
    from humannerf_amd import ops
    _, dy, _ = _conv_inputs(2, (2, 3, 5), 2)
    dx = ops.conv3x3_bwd_data(torch.from_numpy(dy).to(dev()), None, packed, 2)
    _check_conv('conv bwd L2 unmasked', dx, refs.conv_bwd_ref(dy, None, 2), refs.conv_bwd_ref(dy, None, 2, absolute=True), 9 * 128)


@pytest.mark.parametrize('shape', [(2, 3, 5, 64), (1, 7, 9, 128), (1, 16, 16, 512)], ids=str)
def test_maxpool2_forward_and_backward_bit_for_bit(shape):
    """Floor mode (3 x 5 -> 1 x 2, 7 x 9 -> 3 x 4); integer-valued inputs with exact ties: the gradient goes where
    torch's CPU autograd sends it, the first maximum in row-major scan order."""
    from humannerf_amd import ops
    rs = np.random.RandomState(shape[3])
    N, H, W, C = shape
    for x in (rs.standard_normal(shape).astype(np.float32), rs.randint(0, 3, shape).astype(np.float32)):
        y, guard = _guarded((N, H // 2, W // 2, C), NAN)
        ops.maxpool2_fwd(torch.from_numpy(x).to(dev()), out=y)
        assert torch.equal(y.cpu(), refs.pool_fwd_ref(x)) and bool(torch.isnan(guard).all())
        dy = rs.standard_normal(tuple(y.shape)).astype(np.float32)
        dx, guard = _guarded(shape, NAN)
        ops.maxpool2_bwd(torch.from_numpy(x).to(dev()), torch.from_numpy(dy).to(dev()), out=dx)
        assert torch.equal(dx.cpu(), refs.pool_bwd_ref(x, dy)) and bool(torch.isnan(guard).all())


def _head_inputs(C, P, N=2):
    rs = np.random.RandomState(C + P)
    f = (np.maximum(rs.standard_normal((2 * N, P, C)), 0) * 5).astype(np.float32)
    f[0, 0] = 0                                          # an all-zero pixel vector in the first image only,
    f[N + 1, P - 1] = 0                                  # in the second image only,
    if P > 2:
        f[1, 1] = 0                                      # and in both
        f[N + 1, 1] = 0
    w = refs.heads()[{64: 0, 128: 1, 256: 2, 512: 3}[C]].numpy()
    go = rs.uniform(0.5, 1.5, N).astype(np.float32)
    return f, w, go


@pytest.mark.parametrize('P', [1, 4, 63, 1024])
@pytest.mark.parametrize('C', [64, 128, 256, 512])
def test_head_forward_and_backward_against_fp64(C, P):
    from humannerf_amd import ops
    f, w, go = _head_inputs(C, P)
    ft, wt, got = (torch.from_numpy(a).to(dev()) for a in (f, w, go))
    prev = torch.tensor([0.25, -1.0], device=dev())
    out, val = ops.lpips_head_fwd(ft, wt)
    out2, val2 = ops.lpips_head_fwd(ft, wt, out=prev.clone(), accumulate=True)
    assert torch.equal(out, val) and torch.equal(val, val2) and torch.equal(out2, prev + val)
    v64, g64 = refs.head_ref(f, w, torch.float64, go)
    v32, g32 = refs.head_ref(f, w, torch.float32, go)
    refs.check_value('head C%d P%d' % (C, P), val.cpu().numpy(), v64.numpy(), v32.numpy())
    dx_nan, guard = _guarded((2, P, C), NAN)
    ops.lpips_head_bwd(ft, wt, got, out=dx_nan)
    assert bool(torch.isnan(guard).all()) and bool(torch.isfinite(dx_nan).all())
    refs.check_grad('head C%d P%d' % (C, P), dx_nan.cpu().numpy(), g64.numpy(), g32.numpy())
    base = torch.from_numpy(np.random.RandomState(1).standard_normal((2, P, C)).astype(np.float32)).to(dev())
    acc = ops.lpips_head_bwd(ft, wt, got, out=base.clone(), accumulate=True)
    assert torch.equal(acc, base + dx_nan)
    if P > 2:
        assert bool((dx_nan[1, 1] == 0).all())           # both vectors zero: no gradient


@pytest.mark.parametrize('C', [64, 512])
def test_head_of_equal_maps_is_exactly_zero(C):
    from humannerf_amd import ops
    f, w, go = _head_inputs(C, 63)
    f = np.concatenate([f[:2], f[:2]])
    ft, wt, got = (torch.from_numpy(a).to(dev()) for a in (f, w, go))
    out, _ = ops.lpips_head_fwd(ft, wt)
    dx = ops.lpips_head_bwd(ft, wt, got)
    assert bool((out == 0).all()) and bool((dx == 0).all())


# --------------------------------------------------------------------------------------------------- whole path
def _run(lp, in0, in1, weight=None):
    """value (N) and the gradient (N,3,H,W) of sum_n weight[n] value[n] through LpipsVGG.__call__."""
    a = torch.as_tensor(in0).to(dev()).requires_grad_(True)
    v = lp(a, torch.as_tensor(in1).to(dev()))
    assert v.shape == (a.shape[0], 1, 1, 1)
    wt = torch.ones_like(v) if weight is None else torch.as_tensor(weight).to(v).reshape(v.shape)
    (v * wt).sum().backward()
    return v.detach().reshape(-1), a.grad


@pytest.mark.parametrize('case', refs.CASES, ids=refs.case_key)
def test_whole_path_against_the_reference_class_and_fp64(case, lp):
    g, key = refs.golden(), refs.case_key(case)
    v64, g64, v32, g32 = refs.case_ref(case)
    v, gr = _run(lp, g[key + '_in0'], g[key + '_in1'])
    v2, gr2 = _run(lp, g[key + '_in0'], g[key + '_in1'])
    assert torch.equal(v, v2) and torch.equal(gr, gr2)                       # run to run: bit-identical
    v, gr = v.cpu().numpy(), gr.cpu().numpy()
    refs.check_value(key + ' vs fp64', v, v64, v32)
    refs.check_grad(key + ' vs fp64', gr, g64, g32)
    # the reference's class evaluated in fp32 on the CPU is itself one floor away from fp64
    tol = np.maximum(4 * np.abs(v32 - v64), refs.VALUE_FLOOR * np.abs(v64)) + np.abs(g[key + '_value'] - v64)
    assert (np.abs(v - g[key + '_value']) <= tol).all()
    gtol = max(4 * np.linalg.norm(g32 - g64), refs.GRAD_FLOOR * np.linalg.norm(g64)) + np.linalg.norm(g[key + '_grad'] - g64)
    assert np.linalg.norm(gr - g[key + '_grad']) <= gtol
    per = lp.layers(torch.from_numpy(g[key + '_in0']).to(dev()), torch.from_numpy(g[key + '_in1']).to(dev()))
    _, vals = refs.reference_lpips(refs.trunk(), refs.heads(), torch.from_numpy(g[key + '_in0']), torch.from_numpy(g[key + '_in1']),
                                   torch.float64, per_layer=True)
    want = torch.stack([t.reshape(-1) for t in vals]).numpy()
    assert per.shape == (5, case[0]) and np.abs(per.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert np.abs(per.double().sum(0).cpu().numpy() - v).max() <= 1e-6 * np.abs(v).max()


def test_weighted_upstream_gradient(lp):
    case = refs.CASES[3]
    g, key = refs.golden(), refs.case_key(case)
    wt = np.array([0.5, -2.0, 3.0], np.float32)
    _, gr = _run(lp, g[key + '_in0'], g[key + '_in1'], wt)
    _, g64 = refs.value_and_grad(g[key + '_in0'], g[key + '_in1'], torch.float64, wt)
    _, g32 = refs.value_and_grad(g[key + '_in0'], g[key + '_in1'], torch.float32, wt)
    refs.check_grad(key + ' weighted', gr.cpu().numpy(), g64, g32)


def test_identical_images_give_exactly_zero(lp):
    x = refs.golden()['n2_h32_w32_s0_in0']
    v, gr = _run(lp, x, x.copy())
    assert bool((v == 0).all()) and bool((gr == 0).all())


def test_a_pair_does_not_depend_on_its_batch(lp):
    g, key = refs.golden(), refs.case_key(refs.CASES[3])
    v3, g3 = _run(lp, g[key + '_in0'], g[key + '_in1'])
    v1, g1 = _run(lp, g[key + '_in0'][:1], g[key + '_in1'][:1])
    assert torch.equal(v3[:1], v1) and torch.equal(g3[:1], g1)


def test_views_metric_and_refusals(lp):
    g = refs.golden()
    in0, in1 = (torch.from_numpy(g['n1_h37_w45_s0_' + k]).to(dev()) for k in ('in0', 'in1'))
    nhwc = in0.permute(0, 2, 3, 1).contiguous()
    view = nhwc.permute(0, 3, 1, 2)                                          # what train.image_loss passes
    assert lp._nhwc(view).data_ptr() == nhwc.data_ptr()                      # taken as is
    with torch.no_grad():
        a, b = lp(in0, in1), lp(view, in1)
        assert torch.equal(a, b)
        p, t = (in0.permute(0, 2, 3, 1) + 1) / 2, (in1.permute(0, 2, 3, 1) + 1) / 2
        m = lp.metric(p, t)
        assert m.dim() == 0 and torch.equal(m, torch.mean(lp(p.permute(0, 3, 1, 2) * 2. - 1., t.permute(0, 3, 1, 2) * 2. - 1.)))
        assert torch.equal(lp.metric(p[0].cpu().numpy(), t[0].cpu()), m)     # (H,W,3), numpy or CPU tensors
    with pytest.raises(ValueError, match='first argument'):
        lp(in0, in1.clone().requires_grad_(True))
    z = torch.zeros(1, 3, 15, 16, device=dev())
    with pytest.raises(ValueError, match='>= 16'):
        lp(z, z)
    with pytest.raises(ValueError, match='>= 16'):
        lp.metric(torch.zeros(16, 15, 3), torch.zeros(16, 15, 3))


def test_poisoned_workspace_and_bounds(lp, packed):
    """NaN-filled workspace and outputs give the bits of zero-filled ones; nothing is written past the stated sizes."""
    from humannerf_amd import _lib, ops
    g = refs.golden()
    in0, in1 = (torch.from_numpy(g['n3_h17_w16_s2_' + k]).to(dev()).permute(0, 2, 3, 1).contiguous() for k in ('in0', 'in1'))
    N, H, W = 3, 17, 16
    lib = _lib.load()
    res = []
    for want_grad in (0, 1):
        need = lib.hnrf_lpips_workspace_bytes(N, H, W, want_grad)
        assert need % 256 == 0
        for fill in (NAN, 0.0):
            buf = torch.full((need // 4 + 64 + 1024,), fill, device=dev())
            off = (-buf.data_ptr() % 256) // 4
            ws, guard = buf[off:off + need // 4], buf[off + need // 4:]
            out, per, _ = ops.lpips_fwd(in0, in1, packed, want_grad=want_grad, workspace=ws, want_layers=True)
            d = ops.lpips_bwd(torch.ones(N, device=dev()), packed, ws, N, H, W) if want_grad else None
            torch.cuda.synchronize()
            assert bool((guard != guard).all() if fill != fill else (guard == 0).all())
            res.append((out, per, d))
    assert all(torch.equal(res[0][0], r[0]) and torch.equal(res[0][1], r[1]) for r in res[1:])
    assert torch.equal(res[2][2], res[3][2]) and bool(torch.isfinite(res[2][2]).all())
    with pytest.raises(_lib.HnrfError, match='workspace'):
        ops.lpips_fwd(in0, in1, packed, want_grad=True, workspace=torch.empty(64 + 1024, device=dev())[:1024])


# ------------------------------------------------------------------------------------------------- training glue
def test_image_loss_with_lpips(lp):
    """train.image_loss = 1.0 LPIPS + 0.2 MSE (default.yaml:278-281) on a GPU prediction that requires grad."""
    from humannerf_amd.train import image_loss
    g = refs.golden()
    q = lambda a: np.round((a.transpose(0, 2, 3, 1).astype(np.float64) + 1) / 2 * 65536) / 65536     # 2 p - 1 is exact in fp32
    p, t = q(g['n2_h32_w32_s0_in0']).astype(np.float32), q(g['n2_h32_w32_s0_in1']).astype(np.float32)
    pred = torch.from_numpy(p).to(dev()).requires_grad_(True)
    loss, parts = image_loss(pred, torch.from_numpy(t).to(dev()), lp)
    loss.backward()
    assert set(parts) == {'mse', 'lpips'}

    def ref(dtype):
        a = torch.from_numpy(p).to(dtype).requires_grad_(True)
        b = torch.from_numpy(t).to(dtype)
        lpv = 1.0 * torch.mean(refs.reference_lpips(refs.trunk(), refs.heads(), a.permute(0, 3, 1, 2) * 2. - 1.,
                                                    b.permute(0, 3, 1, 2) * 2. - 1., dtype))
        mse = 0.2 * torch.mean((a - b) ** 2)
        gr, = torch.autograd.grad(lpv + mse, a)
        return float(lpv), float(mse), gr.double().numpy()
    l64, m64, g64 = ref(torch.float64)
    l32, m32, g32 = ref(torch.float32)
    refs.check_value('image_loss lpips', [float(parts['lpips'])], [l64], [l32])
    refs.check_value('image_loss mse', [float(parts['mse'])], [m64], [m32])
    refs.check_value('image_loss total', [float(loss)], [l64 + m64], [l32 + m32])
    refs.check_grad('image_loss', pred.grad.cpu().numpy(), g64, g32)


def test_one_training_step_with_lpips(seeded_params, golden_dir):
    """Trainer.train_step on 3 patches of 16 x 16, 32 samples per ray, with the seeded trunk as lpips_fn."""
    from humannerf_amd import dataset
    from humannerf_amd.config import cfg
    from humannerf_amd.lpips import LpipsVGG
    from humannerf_amd.network import Network
    from humannerf_amd.train import Trainer
    old = (cfg.patch.N_patches, cfg.patch.size, cfg.N_samples)
    cfg.patch.N_patches, cfg.patch.size, cfg.N_samples = 3, 16, 32
    try:
        assert cfg.train.lossweights.lpips == 1.0
        subj = dataset.Subject(os.path.join(golden_dir, 'subject_synth'))
        net = Network()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params.items()})
        net = net.to(dev())
        tr = Trainer(net, lpips_fn=LpipsVGG.seeded(0))
        assert tr.objective == '1*lpips + 0.2*mse'
        stream = dataset.FrameStream(subj, rank=0, world=1, seed=0, device=dev())
        try:
            batch = next(iter(stream))
        finally:
            stream.close()
        loss, parts = tr.train_step(batch)
        assert np.isfinite(float(loss)) and set(parts) == {'mse', 'lpips'} and float(parts['lpips']) > 0
        moved = [k for k, v in net.state_dict().items() if not torch.equal(v.cpu(), torch.from_numpy(seeded_params[k]))]
        assert len(moved) >= 50
    finally:
        cfg.patch.N_patches, cfg.patch.size, cfg.N_samples = old


def test_metrics_writer_with_lpips(tmp_path, lp):
    from humannerf_amd.render import MetricsWriter
    g = refs.golden()
    p = (g['n1_h37_w45_s0_in0'][0].transpose(1, 2, 0) + 1) / 2
    t = (g['n1_h37_w45_s0_in1'][0].transpose(1, 2, 0) + 1) / 2
    mw = MetricsWriter(str(tmp_path), 'exp', 'synthetic', metrics=['psnr', 'lpips'], lpips_fn=lp.metric)
    mw.append('frame_000000', p, t)
    avg = mw.finalize()
    want = 1000 * float(lp.metric(p, t))
    assert mw.name2metrics['frame_000000']['lpips'] == want and avg['lpips'] == want and 1 < want < 20
    with open(str(tmp_path / 'exp-metrics.perimg.txt')) as f:
        assert 'lpips-%.4f' % want in f.read()
    with open(str(tmp_path / 'exp-metrics.average.txt')) as f:
        assert 'l:%.4f' % want in f.read()
