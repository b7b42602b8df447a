"""Baked canonical grid on the MI355X: the bake against the canonical kernel, the device sampler against its host
twin, the baked frame pipeline against its parts and against the fp64 oracle, Network.forward / run.run_movement with
cfg.amd.canonical = 'baked', and the convergence of the grid to the MLP on a band-limited network."""
import os

import numpy as np
import pytest
import torch

from humannerf_amd import baked, ops, scene
from humannerf_amd.config import cfg
from humannerf_amd.network import Network, hann_window_weights
from humannerf_amd.seeded import default_shapes, seeded_state, with_density

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KEYS11 = {'rgb', 'alpha', 'depth', 'weights_on_rays', 'xyz_on_rays', 'rgb_on_rays', 'cnl_xyz', 'cnl_rgb', 'cnl_weight',
          'backward_motion_weights', 'offsets'}
FRAME_KEYS = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
              'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'cnl_bbox_max_xyz', 'bgcolor']
CNL_LAYERS = [0, 2, 4, 6, 8, 10, 12, 14]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def load_net(state):
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return n.to(DEV).eval()


def frame_to_gpu(fr, rays=None):
    d = {k: T(fr[k]) for k in FRAME_KEYS}
    if rays is not None:
        d['rays'], d['near'], d['far'] = d['rays'][:, :rays].contiguous(), d['near'][:rays].contiguous(), d['far'][:rays].contiguous()
    return d


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.fixture(scope='module')
def state():
    return with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)


@pytest.fixture(scope='module')
def net(state):
    return load_net(state)


@pytest.fixture(scope='module')
def frame():
    return scene.synthetic_frame(H=64, W=64, pose_seed=3, pose_scale=0.3)


@pytest.fixture(autouse=True)
def restore_cfg():
    amd = {k: cfg.amd.get(k) for k in ('mlp_mode', 'canonical', 'bake_resolution', 'diagnostics', 'term_eps', 'cull_eps')}
    top = (cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions, cfg.chunk)
    cfg.N_samples, cfg.perturb = 128, 0.
    yield
    for k, v in amd.items():
        cfg.amd[k] = v
    cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions, cfg.chunk = top


def canonical_pack_of(state, mode, head_scale=1.0):
    ws = [T(state['cnl_mlp.module.pts_linears.%d.weight' % i]) for i in CNL_LAYERS]
    bs = [T(state['cnl_mlp.module.pts_linears.%d.bias' % i]) for i in CNL_LAYERS]
    ws.append(T(state['cnl_mlp.module.output_linear.0.weight'] * np.float32(head_scale)))
    bs.append(T(state['cnl_mlp.module.output_linear.0.bias'] * np.float32(head_scale)))
    return ops.canonical_pack(ws, bs, mode)


def frame_parts(net, frame, use_nonrigid=True, mode='f16x3'):
    """K1's and K2's inputs for ``frame`` as Network.forward prepares them."""
    old = cfg.amd.mlp_mode
    cfg.amd.mlp_mode = mode
    try:
        Rs, Ts, vol = net.frame_motion(frame)
        d = frame_to_gpu(frame)
        nrc = cfg.non_rigid_motion_mlp
        hann_w = hann_window_weights(1e7, nrc.multires, nrc.kick_in_iter, nrc.full_band_iter).to(DEV)
        nr_packed = net._nonrigid_packed(d['dst_posevec']).clone() if use_nonrigid else None
    finally:
        cfg.amd.mlp_mode = old
    k1 = (d['rays'][0].contiguous(), d['rays'][1].contiguous(), d['near'].reshape(-1), d['far'].reshape(-1), None, Rs, Ts,
          vol, d['cnl_bbox_min_xyz'], d['cnl_bbox_scale_xyz'])
    return k1, hann_w if use_nonrigid else None, nr_packed, d


# ---------------------------------------------------------------------------------------------------------- 4: the bake
@pytest.mark.parametrize('N', [32, 45, 131])          # 131^3 points: two chunks of the bake, the second one ragged
@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_bake_is_the_canonical_kernel_rounded(state, frame, mode, N):
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    packed = canonical_pack_of(state, mode)
    grid, sat = ops.bake_canonical(packed, T(lo), T(hi), N, mode, want_saturated=True)
    assert grid.shape == (N, N, N, 4) and grid.dtype == torch.float16
    pts = T(baked.lattice_points(lo, hi, N))
    ref = ops.canonical(pts, packed, mode).clamp(-65504, 65504).half().reshape(N, N, N, 4)
    assert torch.equal(grid, ref)
    assert torch.equal(grid.view(torch.int16), ref.view(torch.int16))
    assert int(sat) == 0
    assert torch.equal(ops.bake_canonical(packed, T(lo), T(hi), N, mode), grid)


def test_bake_saturates_and_counts_what_leaves_the_f16_range(state, frame):
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    N = 40
    packed = canonical_pack_of(state, 'f32', head_scale=3e4)          # outputs of order 1e5: many beyond 65504
    grid, sat = ops.bake_canonical(packed, T(lo), T(hi), N, 'f32', want_saturated=True)
    raw = ops.canonical(T(baked.lattice_points(lo, hi, N)), packed, 'f32').reshape(N, N, N, 4)
    over = raw.abs() > 65504
    assert int(over.sum()) > 100 and int((~over).sum()) > 100
    assert int(sat) == int(over.sum())
    assert torch.equal(grid, raw.clamp(-65504, 65504).half())
    assert torch.equal(grid[over].float(), torch.sign(raw[over]) * 65504.0)
    assert bool(torch.isfinite(grid.float()).all())


# ------------------------------------------------------------------------------------------------------- 5: the sampler
@pytest.mark.parametrize('P', [1, 63, 4133, 128 * 1000])
def test_device_sampler_equals_the_host_twin_bit_for_bit(net, state, frame, P):
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    grid = ops.bake_canonical(canonical_pack_of(state, 'f16x3'), T(lo), T(hi), 48, 'f16x3')
    k1, hann_w, nr_packed, _ = frame_parts(net, frame)
    z, x_skel, mask, _ = ops.sample_warp(*k1, 128)
    xyz, _ = ops.nonrigid(x_skel, hann_w, nr_packed, 'f16x3')
    stride = 4 if P > 5000 else 97                                    # samples of many rays, inside and outside the body
    xyz = xyz.reshape(-1, 3)[::stride][:P].contiguous()
    m = mask.reshape(-1)[::stride][:P].contiguous()
    assert xyz.shape[0] == P
    host = baked.sample_host(grid.cpu().numpy(), xyz.cpu().numpy(), lo, hi)
    dense = ops.baked_sample(xyz, grid, T(lo), T(hi))
    assert np.array_equal(dense.cpu().numpy().view(np.uint32), host.view(np.uint32))
    if P > 1000:                                                     # (the samples do spread over the lattice)
        assert float(dense.std()) > 0.01
    # sparse: only the listed rows are written
    idx, count = ops.compact_samples(m, 1e-4)
    n = int(count)
    assert P < 1000 or 0 < n < P
    raw = torch.full((P, 4), 123.25, device=DEV)
    out = ops.baked_sample_sparse(xyz, grid, T(lo), T(hi), idx, count, raw=raw)
    listed = torch.zeros(P, dtype=torch.bool, device=DEV)
    listed[idx[:n].long()] = True
    assert torch.equal(out[listed], dense[listed])
    assert bool((out[~listed] == 123.25).all())
    # points far outside the box and NaN coordinates: clamped, finite, and the host twin's bits
    odd = xyz.clone()
    odd[::3, 0] += 5.0
    odd[1::3, 1] -= 7.0
    odd[::7, 2] = float('nan')
    got = ops.baked_sample(odd, grid, T(lo), T(hi))
    assert bool(torch.isfinite(got).all())
    assert np.array_equal(got.cpu().numpy().view(np.uint32),
                          baked.sample_host(grid.cpu().numpy(), odd.cpu().numpy(), lo, hi).view(np.uint32))


# ------------------------------------------------------------------------------------------------------ 6: the pipeline
@pytest.mark.parametrize('overlap', [False, True])
@pytest.mark.parametrize('use_nonrigid', [True, False])
@pytest.mark.parametrize('diag', [True, False])
def test_baked_frame_is_the_chain_of_its_parts(net, state, frame, diag, use_nonrigid, overlap):
    lo, hi = T(frame['cnl_bbox_min_xyz']), T(frame['cnl_bbox_max_xyz'])
    grid = ops.bake_canonical(canonical_pack_of(state, 'f16x3'), lo, hi, 40, 'f16x3')
    k1, hann_w, nr_packed, d = frame_parts(net, frame, use_nonrigid)
    S, chunk = 128, 1500                                              # 4096 rays: chunks of 1500, 1500, 1096
    assert k1[0].shape[0] % chunk != 0
    out, _ = ops.render_frame(*k1, hann_w, nr_packed, None, d['bgcolor'], S, chunk, 'f16x3', diagnostics=diag,
                              overlap=overlap, baked=(grid, lo, hi))
    z, x_skel, mask, bmw = ops.sample_warp(*k1, S, want_bmw=diag)
    if use_nonrigid:
        xyz, off = ops.nonrigid(x_skel, hann_w, nr_packed, 'f16x3', want_offsets=True)
    else:
        xyz, off = x_skel, torch.zeros_like(x_skel)
    raw = ops.baked_sample(xyz, grid, lo, hi)
    ref = ops.composite(raw, mask, z, k1[1], xyz, d['bgcolor'], diagnostics=diag)
    if diag:
        ref.update(xyz_on_rays=xyz, backward_motion_weights=bmw, offsets=off)
    assert set(out) == set(ref) == (KEYS11 if diag else {'rgb', 'alpha', 'depth'})
    for k in ref:
        assert same_bits(out[k], ref[k]), k
    assert float(out['alpha'].max()) > 0.5                           # (a picture, not the background)
    if diag:
        return
    # culled: the same chain through compact_samples and the sparse ops
    eps = 1e-9
    culled, _ = ops.render_frame(*k1, hann_w, nr_packed, None, d['bgcolor'], S, chunk, 'f16x3', diagnostics=False,
                                 cull_eps=eps, overlap=overlap, baked=(grid, lo, hi))
    idx, count = ops.compact_samples(mask, eps)
    assert 0 < int(count) < mask.numel()
    xyz_s = ops.nonrigid_sparse(x_skel, hann_w, nr_packed, idx, count, 'f16x3') if use_nonrigid else x_skel
    raw_s = ops.baked_sample_sparse(xyz_s, grid, lo, hi, idx, count)
    ref = ops.composite(raw_s, mask, z, k1[1], None, d['bgcolor'], diagnostics=False, cull_eps=eps)
    for k in ref:
        assert same_bits(culled[k], ref[k]), k
    # and the single-chunk entry
    R = 1000
    rays = tuple(t[:R].contiguous() if i < 4 else t for i, t in enumerate(k1))
    ws = torch.empty(ops.render_workspace_bytes(R, S) // 4 + 64, device=DEV)
    one = ops.render_rays(*rays, hann_w, nr_packed, None, d['bgcolor'], S, 'f16x3', workspace=ws, baked=(grid, lo, hi))
    for k in one:
        assert same_bits(one[k], out[k][:R]), k


# ---------------------------------------------------------------------------------------------------- 7: the fp64 oracle
def test_baked_frame_against_the_oracle(net, golden_case, state):
    """The new plumbing isolated: the 11-output baked frame of the golden case 'dense_s128' against
    oracle.raw2outputs in float64, fed the frame's own xyz_on_rays, K1's z_vals / foreground mask on the same inputs and
    raw = the host twin of the sampler on the downloaded grid.  Tolerance and argmax selection of test_composite_kernel
    (3e-6 * max(1, max|ref|); cnl_xyz equal, cnl_rgb -- a sigmoid, fp32 on the device -- within that tolerance, where
    the two largest weights are more than 1e-6 apart).  The selection may hide nothing: at least 70 % of the rays
    must be selected -- counted on the rays the case's fixture keeps per-sample outputs for (the first keep_rays = 64),
    where the reference's own weights select 89 %; of all 289 rays of this frame the exact renderer itself (the fp64
    oracle with the MLP) selects 68.9 %, rays that pass the body by have no weight to speak of, so no renderer can be
    asked for 70 % of those.  Both fractions are printed; the comparison itself runs over every selected ray of the
    frame."""
    from oracle import oracle
    m, g, fr, case_state = golden_case('dense_s128')
    head = ('cnl_mlp.module.output_linear.0.weight', 'cnl_mlp.module.output_linear.0.bias')
    sd = net.state_dict()
    cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions = m['N_samples'], m['perturb'], m['ignore_non_rigid_motions']
    cfg.amd.canonical, cfg.amd.bake_resolution, cfg.amd.diagnostics = 'baked', 96, True
    try:
        with torch.no_grad():
            for k in head:
                sd[k].copy_(torch.from_numpy(case_state[k]))
            net.set_baked_grid(None, None, None)
            d = frame_to_gpu(fr)
            out = net(**d, iter_val=m['iter_val'])
            assert net.check_f16_range(wait=True) is False
            grid, bmin, bmax = (getattr(net._kept['baked'], k).cpu().numpy() for k in ('grid', 'bmin', 'bmax'))
            k1, _, _, _ = frame_parts(net, fr, use_nonrigid=False)
            z, _, mask, _ = ops.sample_warp(*k1, m['N_samples'])
    finally:
        with torch.no_grad():
            for k in head:
                sd[k].copy_(torch.from_numpy(state[k]))
        net.set_baked_grid(None, None, None)
    assert set(out) == KEYS11 and grid.shape == (96, 96, 96, 4)
    assert np.array_equal(bmin, fr['cnl_bbox_min_xyz']) and np.array_equal(bmax, fr['cnl_bbox_max_xyz'])
    xyz = out['xyz_on_rays'].cpu().numpy()
    raw = baked.sample_host(grid, xyz, bmin, bmax)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    ref = oracle.raw2outputs(f64(raw), mask.cpu().double(), z.cpu().double(), f64(fr['rays'][1]), f64(xyz), f64(fr['bgcolor']))
    tol = lambda k: 3e-6 * max(1.0, float(ref[k].abs().max()))
    for k in ('rgb', 'alpha', 'depth', 'weights_on_rays', 'rgb_on_rays', 'cnl_weight'):
        err = float((out[k].cpu().double() - ref[k]).abs().max())
        print(k, 'max err %.3e (tol %.3e)' % (err, tol(k)))
        assert err <= tol(k), (k, err)
    w = ref['weights_on_rays'].numpy()
    srt = np.sort(w, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-6
    kept = clear[:m['keep_rays']]
    print('rays with an unambiguous argmax: %.3f of the %d kept rays, %.3f of all %d' % (kept.mean(), kept.size, clear.mean(), clear.size))
    assert kept.mean() >= 0.70
    assert np.array_equal(out['cnl_xyz'].cpu().numpy()[clear], ref['cnl_xyz'].numpy()[clear].astype(np.float32))
    assert np.abs(out['cnl_rgb'].cpu().numpy()[clear] - ref['cnl_rgb'].numpy()[clear]).max() <= tol('cnl_rgb')
    assert float(out['alpha'].max()) > 0.9                            # the dense medium does saturate rays


# ------------------------------------------------------------------------------------------------- 8: Network.forward
def test_network_forward_with_the_baked_option(net, state, frame):
    d = frame_to_gpu(frame)
    cfg.amd.bake_resolution = 32
    net.set_baked_grid(None, None, None)
    bias = net.cnl_mlp.module.output_linear[0].bias
    keep = bias.detach().clone()
    try:
        with torch.no_grad():
            exact = net(**d, iter_val=1e7)
            cfg.amd.canonical = 'baked'
            c0 = net.bake_count
            first = net(**d, iter_val=1e7)
            assert net.bake_count == c0 + 1
            assert set(first) == set(exact) == KEYS11
            assert all(first[k].shape == exact[k].shape and first[k].dtype == exact[k].dtype for k in exact)
            assert not torch.equal(first['rgb'], exact['rgb'])                      # (it is an approximation ...)
            for k in ('xyz_on_rays', 'offsets', 'backward_motion_weights'):          # K1 and K2 stay exact
                assert same_bits(first[k], exact[k]), k
            second = net(**d, iter_val=1e7)
            assert net.bake_count == c0 + 1                                         # same key: no re-bake
            assert all(same_bits(first[k], second[k]) for k in first)
            fresh = frame_to_gpu(frame)                                             # new tensor objects, same values
            third = net(**fresh, iter_val=1e7)
            assert net.bake_count == c0 + 1 and same_bits(third['rgb'], first['rgb'])
            # an in-place change of a canonical weight re-bakes
            bias[0] += 0.75
            changed = net(**d, iter_val=1e7)
            assert net.bake_count == c0 + 2 and not torch.equal(changed['rgb'], first['rgb'])
            bias.copy_(keep)
            again = net(**d, iter_val=1e7)
            assert net.bake_count == c0 + 3 and all(same_bits(first[k], again[k]) for k in first)
            # another resolution is another key
            cfg.amd.bake_resolution = 24
            net(**d, iter_val=1e7)
            assert net.bake_count == c0 + 4 and net._kept['baked'].grid.shape[0] == 24
            # an injected analytic grid is used as it is, and never re-baked
            vals = torch.tensor([0.0, 1.0, -1.0, 50.0])
            const = vals.half().expand(16, 16, 16, 4).contiguous()
            net.set_baked_grid(const, frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz'])
            inj = net(**d, iter_val=1e7)
            assert net.bake_count == c0 + 4
            want = torch.sigmoid(vals[:3]).to(DEV)
            assert float((inj['rgb_on_rays'] - want).abs().max()) <= 1e-6
            bias[0] += 0.75
            inj2 = net(**d, iter_val=1e7)
            assert net.bake_count == c0 + 4 and same_bits(inj2['rgb'], inj['rgb'])
            bias.copy_(keep)
            net.set_baked_grid(None, None, None)
            cfg.amd.bake_resolution = 32
            # the lean form with early termination is refused by name, not silently exact or silently unterminated
            cfg.amd.diagnostics, cfg.amd.term_eps = False, 1e-3
            with pytest.raises(NotImplementedError, match='term_eps'):
                net(**d, iter_val=1e7)
            cfg.amd.term_eps = 0.0
            lean = net(**d, iter_val=1e7)
            assert set(lean) == {'rgb', 'alpha', 'depth'} and all(same_bits(lean[k], first[k]) for k in lean)
            cfg.amd.diagnostics = True
        # the training path ignores the option
        small = frame_to_gpu(frame, rays=512)
        c1 = net.bake_count
        for p in net.parameters():
            p.requires_grad_(True)
        with torch.enable_grad():
            cfg.amd.canonical = 'baked'
            tb = net(**small, iter_val=1e7)
            cfg.amd.canonical = 'mlp'
            tm = net(**small, iter_val=1e7)
        assert tb['rgb'].requires_grad and net.bake_count == c1
        assert all(same_bits(tb[k].detach(), tm[k].detach()) for k in ('rgb', 'alpha', 'depth'))
        # back at 'mlp' with a grid still cached: the exact path, as of a network that never baked
        assert 'baked' in net._kept
        with torch.no_grad():
            back = net(**d, iter_val=1e7)
            never = load_net(state)
            ref = never(**d, iter_val=1e7)
        assert never.bake_count == 0 and 'baked' not in never._kept
        assert all(same_bits(back[k], ref[k]) for k in ref) and all(same_bits(back[k], exact[k]) for k in exact)
    finally:
        with torch.no_grad():
            bias.copy_(keep)
        net.set_baked_grid(None, None, None)


# ------------------------------------------------------------------------------------------------------------ 9: run.py
def test_run_movement_bakes_once_and_names_the_folder(net, tmp_path):
    from humannerf_amd import dataset, run
    names = scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    old = (cfg.get('show_truth', False), cfg.get('show_alpha', False))
    cfg.amd.canonical, cfg.amd.bake_resolution, cfg.amd.diagnostics, cfg.N_samples = 'baked', 24, False, 64
    net.set_baked_grid(None, None, None)
    c0 = net.bake_count
    try:
        res = run.run_movement(net, subject, logdir=str(tmp_path / 'log'), metrics=['psnr'])
        assert net.bake_count == c0 + 1
        folder = os.path.basename(res['image_dir'].rstrip('/'))
        assert 'baked_24' in folder and folder.startswith('movement')
        pngs = sorted(f for f in os.listdir(res['image_dir']) if f.endswith('.png'))
        assert pngs == sorted(n + '.png' for n in names)
        tp = run.run_tpose(net, subject, total_frames=2, image_size=64, logdir=str(tmp_path / 'log'))
        assert net.bake_count == c0 + 1 and 'baked_24' in tp['image_dir']
        cfg.amd.canonical = 'mlp'
        exact = run.run_movement(net, subject, logdir=str(tmp_path / 'log'), metrics=['psnr'])
        assert 'baked' not in exact['image_dir'] and exact['image_dir'] != res['image_dir']
    finally:
        cfg.show_truth, cfg.show_alpha = old
        net.set_baked_grid(None, None, None)


# ----------------------------------------------------------------------------------------------------- 10: convergence
def test_the_grid_converges_to_the_mlp(state, frame):
    """A band-limited canonical network (the encoding's octaves 2^3 .. 2^9 cut from both places the MLP reads it, so
    the field varies over decimetres), rendered exactly and from grids of 32^3 and 128^3: max |d rgb| at 128 is below
    half of that at 32 -- trilinear error falls with h^2 where the field is smooth and with h across ReLU creases,
    4-16x for 4x the resolution; 'half' asks for the direction and a fraction of the slowest rate.  The coarse error
    must stand above the f16 rounding floor of the stored values seen through the sigmoid's slope,
    4 * 2^-11 * max|raw| / 4, or the comparison would be one of two floors (then the coarse grid goes to 16).
    Measured on an MI355X: max |d rgb| 4.23e-2 at 16, 1.24e-2 at 32, 1.09e-3 at 128, floor 1.31e-2 -- the coarse grid
    is 16."""
    st = dict(state)
    for key in ('cnl_mlp.module.pts_linears.0.weight', 'cnl_mlp.module.pts_linears.10.weight'):
        w = st[key].copy()
        assert w.shape[1] in (63, 319)
        w[:, 21:63] = 0.0
        st[key] = w
    n = load_net(st)
    cfg.amd.mlp_mode, cfg.amd.diagnostics, cfg.ignore_non_rigid_motions = 'f32', True, True
    d = frame_to_gpu(frame)
    err = {}
    with torch.no_grad():
        exact = n(**d, iter_val=1e7)
        assert float(exact['alpha'].max()) > 0.5
        cfg.amd.canonical = 'baked'
        for N in (128, 32, 16):
            cfg.amd.bake_resolution = N
            out = n(**d, iter_val=1e7)
            assert n._kept['baked'].grid.shape[0] == N
            err[N] = float((out['rgb'] - exact['rgb']).abs().max())
            if N == 128:
                floor = 4 * 2.0 ** -11 * float(n._kept['baked'].grid.float().abs().max()) / 4
    coarse = 32 if err[32] > floor else 16
    print('max |d rgb|: N=128 %.3e, N=32 %.3e, N=16 %.3e; f16 floor %.3e; coarse grid %d'
          % (err[128], err[32], err[16], floor, coarse))
    assert err[coarse] > floor
    assert err[128] < 0.5 * err[coarse]
