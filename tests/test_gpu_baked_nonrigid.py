"""Baked non-rigid offset field on the MI355X (cfg.amd.nonrigid = 'baked'): the bake against the non-rigid kernel, the
fused sampler against its host twin and against the chain of existing ops, the frame pipeline against its parts,
Network.forward's option handling and re-bake key, the convergence of the grid to the MLP, and run.run_movement.
Fixtures and helpers are those of test_gpu_baked.py: the seeded state with density bias + 5,
synthetic_frame(64, 64, pose_seed=3, pose_scale=0.3), 128 samples per ray."""
import os

import numpy as np
import pytest
import torch

from humannerf_amd import baked, ops, scene
from humannerf_amd.config import cfg
from test_gpu_baked import (DEV, KEYS11, T, canonical_pack_of, frame, frame_parts, frame_to_gpu, load_net, net,  # noqa: F401
                            same_bits, state)

pytestmark = pytest.mark.gpu
S = 128
AMD_KEYS = ('mlp_mode', 'canonical', 'bake_resolution', 'nonrigid', 'nonrigid_bake_resolution', 'diagnostics', 'term_eps',
            'cull_eps')


@pytest.fixture(autouse=True)
def restore_cfg():
    amd = {k: cfg.amd.get(k) for k in AMD_KEYS}
    top = (cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions, cfg.chunk)
    cfg.N_samples, cfg.perturb = S, 0.
    yield
    for k, v in amd.items():
        cfg.amd[k] = v
    cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions, cfg.chunk = top


def u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.fixture(scope='module')
def parts(net, frame):
    """K1 of the frame once for the module (never written to): the packed non-rigid images of both modes, the Hann
    weights, and z / x_skel / fg_mask / bmw of all 4096 x 128 samples."""
    k1, hann_w, nr16, d = frame_parts(net, frame, True, 'f16x3')
    _, _, nr32, _ = frame_parts(net, frame, True, 'f32')
    z, x_skel, mask, bmw = ops.sample_warp(*k1, S, want_bmw=True)
    lo, hi = T(frame['cnl_bbox_min_xyz']), T(frame['cnl_bbox_max_xyz'])
    return dict(k1=k1, hann_w=hann_w, nr={'f16x3': nr16, 'f32': nr32}, d=d, z=z, x_skel=x_skel, mask=mask, bmw=bmw,
                lo=lo, hi=hi)


@pytest.fixture(scope='module')
def grids(parts, state):
    """An offset grid (M = 24) and a canonical grid (N = 48), baked once for the module."""
    off = ops.bake_nonrigid(parts['nr']['f16x3'], parts['hann_w'], parts['lo'], parts['hi'], 24, 'f16x3')
    cnl = ops.bake_canonical(canonical_pack_of(state, 'f16x3'), parts['lo'], parts['hi'], 48, 'f16x3')
    return (off, parts['lo'], parts['hi']), (cnl, parts['lo'], parts['hi'])


@pytest.fixture(scope='module')
def convergence(parts):
    """Test 5's measurement, shared with test 4: max |interpolated - exact K2 offset| (metres, 'f32' arithmetic) over
    the frame's samples with fg_mask >= 1e-4, for device grids of M = 128 and 32; and max |exact offset| there."""
    x, m = parts['x_skel'], parts['mask'] >= 1e-4
    _, exact = ops.nonrigid(x, parts['hann_w'], parts['nr']['f32'], 'f32', want_offsets=True)
    err = {}
    for M in (128, 32):
        grid = ops.bake_nonrigid(parts['nr']['f32'], parts['hann_w'], parts['lo'], parts['hi'], M, 'f32')
        got = ops.baked_sample(x, grid, parts['lo'], parts['hi'])[..., :3]
        err[M] = float((got - exact)[m].abs().max())
    err['max_offset'] = float(exact[m].abs().max())
    err['samples'] = int(m.sum())
    return err


# ------------------------------------------------------------------------------------------------------------ 1: the bake
@pytest.mark.parametrize('M', [32, 45, 131])          # 131^3 points: two chunks of the bake, the second one ragged
@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_bake_is_the_nonrigid_kernel_rounded(parts, frame, mode, M):
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    assert M ** 3 <= (1 << 21) or 0 < M ** 3 % (1 << 21) < (1 << 21)
    grid, sat = ops.bake_nonrigid(parts['nr'][mode], parts['hann_w'], parts['lo'], parts['hi'], M, mode,
                                  want_saturated=True)
    assert grid.shape == (M, M, M, 4) and grid.dtype == torch.float16
    pts = T(baked.lattice_points(lo, hi, M))
    _, off = ops.nonrigid(pts, parts['hann_w'], parts['nr'][mode], mode, want_offsets=True)
    ref = off.half().reshape(M, M, M, 3)
    assert torch.equal(grid[..., :3].contiguous().view(torch.int16), ref.view(torch.int16))
    assert float(ref.float().abs().max()) > 1e-3                      # (offsets of millimetres at least: not a zero field)
    assert not bool(grid[..., 3].contiguous().view(torch.int16).any())           # the pad lane is +0
    assert int(sat) == 0
    again = ops.bake_nonrigid(parts['nr'][mode], parts['hann_w'], parts['lo'], parts['hi'], M, mode)
    assert torch.equal(again.view(torch.int16), grid.view(torch.int16))


# --------------------------------------------------------------------------------------------------- 2: the fused sampler
@pytest.mark.parametrize('P', [1, 63, 4133, 128 * 1000])
def test_fused_sampler_equals_the_host_twin_and_the_chain(parts, grids, frame, P):
    off, cnl = grids
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    stride = 4 if P > 5000 else 97                                    # samples of many rays, inside and outside the body
    x = parts['x_skel'].reshape(-1, 3)[::stride][:P].contiguous()
    m = parts['mask'].reshape(-1)[::stride][:P].contiguous()
    assert x.shape[0] == P
    og, cg = off[0].cpu().numpy(), cnl[0].cpu().numpy()
    h_raw, h_xyz, h_off = baked.warp_sample_host(og, cg, x.cpu().numpy(), (lo, hi))
    raw, xyz, offs = ops.baked_warp_sample(x, off, cnl, want_xyz=True, want_offsets=True)
    assert np.array_equal(u32(raw), h_raw.view(np.uint32))
    assert np.array_equal(u32(xyz), h_xyz.view(np.uint32))
    assert np.array_equal(u32(offs), h_off.view(np.uint32))
    lean = ops.baked_warp_sample(x, off, cnl)                         # neither xyz nor offsets written
    assert same_bits(lean, raw)
    # the three-call chain of existing ops
    c_off = ops.baked_sample(x, *off)[..., :3].contiguous()
    c_xyz = x + c_off
    c_raw = ops.baked_sample(c_xyz, *cnl)
    assert same_bits(offs, c_off) and same_bits(xyz, c_xyz) and same_bits(raw, c_raw)
    if P > 1000:                                                     # (the samples do spread over both lattices)
        assert float(raw.std()) > 0.01 and float(offs.std()) > 1e-4
    # sparse: only the listed rows are written, of all three outputs
    idx, count = ops.compact_samples(m, 1e-4)
    n = int(count)
    assert P < 1000 or 0 < n < P
    fill = lambda c: torch.full((P, c), 123.25, device=DEV)
    s_raw, s_xyz, s_off = fill(4), fill(3), fill(3)
    out = ops.baked_warp_sample_sparse(x, off, cnl, idx, count, raw=s_raw, xyz=s_xyz, offsets=s_off)
    assert out is s_raw
    listed = torch.zeros(P, dtype=torch.bool, device=DEV)
    listed[idx[:n].long()] = True
    for got, dense in ((s_raw, raw), (s_xyz, xyz), (s_off, offs)):
        assert torch.equal(got[listed], dense[listed])
        assert bool((got[~listed] == 123.25).all())
    s_lean = ops.baked_warp_sample_sparse(x, off, cnl, idx, count)
    assert torch.equal(s_lean[listed], raw[listed]) and not bool(s_lean[~listed].any())
    # points far outside the box and NaN coordinates: clamped, raw and offsets finite, and the host twin's bits
    odd = x.clone()
    odd[::3, 0] += 5.0
    odd[1::3, 1] -= 7.0
    odd[::7, 2] = float('nan')
    g_raw, g_xyz, g_off = ops.baked_warp_sample(odd, off, cnl, want_xyz=True, want_offsets=True)
    assert bool(torch.isfinite(g_raw).all()) and bool(torch.isfinite(g_off).all())
    t_raw, t_xyz, t_off = baked.warp_sample_host(og, cg, odd.cpu().numpy(), (lo, hi))
    assert np.array_equal(u32(g_raw), t_raw.view(np.uint32)) and np.array_equal(u32(g_off), t_off.view(np.uint32))
    assert np.array_equal(g_xyz.cpu().numpy(), t_xyz, equal_nan=True)            # (NaN + offset stays NaN in both)
    # a constant offset grid c: xyz = x_skel + c exactly; an all-zero one: the plain sampler at x_skel
    c = torch.tensor([0.25, -0.125, 0.5, 0.0])
    const = (c.half().expand(16, 16, 16, 4).contiguous().to(DEV), off[1], off[2])
    k_raw, k_xyz, k_off = ops.baked_warp_sample(x, const, cnl, want_xyz=True, want_offsets=True)
    assert same_bits(k_xyz, x + c[:3].to(DEV)) and torch.equal(k_off, c[:3].to(DEV).expand(P, 3))
    assert same_bits(k_raw, ops.baked_sample((x + c[:3].to(DEV)).contiguous(), *cnl))
    zero = (torch.zeros(8, 8, 8, 4, dtype=torch.float16, device=DEV), off[1], off[2])
    z_raw, z_xyz, _ = ops.baked_warp_sample(x, zero, cnl, want_xyz=True)
    assert same_bits(z_raw, ops.baked_sample(x, *cnl)) and same_bits(z_xyz, x)


# -------------------------------------------------------------------------------------------------------- 3: the pipeline
@pytest.mark.parametrize('overlap', [False, True])
@pytest.mark.parametrize('diag', [True, False])
def test_baked_nonrigid_frame_is_the_chain_of_its_parts(parts, grids, diag, overlap):
    off, cnl = grids
    k1, bg = parts['k1'], parts['d']['bgcolor']
    chunk = 1500                                                      # 4096 rays: chunks of 1500, 1500, 1096
    assert k1[0].shape[0] == 4096
    out, _ = ops.render_frame(*k1, None, None, None, bg, S, chunk, 'f16x3', diagnostics=diag, overlap=overlap, baked=cnl,
                              baked_nr=off)
    z, x_skel, mask, bmw = parts['z'], parts['x_skel'], parts['mask'], parts['bmw']
    raw, xyz, offs = ops.baked_warp_sample(x_skel, off, cnl, want_xyz=True, want_offsets=True)
    ref = ops.composite(raw, mask, z, k1[1], xyz, bg, diagnostics=diag)
    if diag:
        ref.update(xyz_on_rays=xyz, backward_motion_weights=bmw, offsets=offs)
    assert set(out) == set(ref) == (KEYS11 if diag else {'rgb', 'alpha', 'depth'})
    for k in ref:
        assert same_bits(out[k], ref[k]), k
    assert float(out['alpha'].max()) > 0.5                           # (a picture, not the background)
    if diag:
        return
    # culled: the same chain through compact_samples and the sparse sampler
    eps = 1e-9
    culled, _ = ops.render_frame(*k1, None, None, None, bg, S, chunk, 'f16x3', diagnostics=False, cull_eps=eps,
                                 overlap=overlap, baked=cnl, baked_nr=off)
    idx, count = ops.compact_samples(mask, eps)
    assert 0 < int(count) < mask.numel()
    raw_s = ops.baked_warp_sample_sparse(x_skel, off, cnl, idx, count)
    ref = ops.composite(raw_s, mask, z, k1[1], None, bg, diagnostics=False, cull_eps=eps)
    for k in ref:
        assert same_bits(culled[k], ref[k]), k
    # and the single-chunk entry
    R = 1000
    rays = tuple(t[:R].contiguous() if i < 4 else t for i, t in enumerate(k1))
    ws = torch.empty(ops.render_workspace_bytes(R, S) // 4 + 64, device=DEV)
    one = ops.render_rays(*rays, None, None, None, bg, S, 'f16x3', workspace=ws, baked=cnl, baked_nr=off)
    for k in one:
        assert same_bits(one[k], out[k][:R]), k
    with pytest.raises(Exception, match='needs baked'):               # no offset grid in front of the canonical MLP
        ops.render_rays(*rays, None, None, None, bg, S, 'f16x3', workspace=ws, baked_nr=off)


# ----------------------------------------------------------------------------------------------------- 4: Network.forward
def test_network_forward_with_both_options_baked(net, state, frame, convergence):
    d = frame_to_gpu(frame)
    cfg.amd.bake_resolution, cfg.amd.nonrigid_bake_resolution = 32, 32
    net.set_baked_grid(None, None, None)
    w = net.non_rigid_mlp.module.linears()[-1].bias
    keep = w.detach().clone()
    try:
        with torch.no_grad():
            exact = net(**d, iter_val=1e7)
            cfg.amd.canonical = 'baked'
            today = net(**d, iter_val=1e7)                                          # today's baked frame
            cfg.amd.nonrigid = 'baked'
            c0, b0 = net.nonrigid_bake_count, net.bake_count
            first = net(**d, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 1 and net.bake_count == b0
            assert net._kept['baked_nr'].grid.shape == (32, 32, 32, 4)
            assert set(first) == set(exact) == KEYS11
            assert all(first[k].shape == exact[k].shape and first[k].dtype == exact[k].dtype for k in exact)
            assert same_bits(first['backward_motion_weights'], exact['backward_motion_weights'])     # K1 stays exact
            # the offsets are interpolated: not the exact ones, but within test 5's measurement at this M on the samples
            # it covers (there in 'f32', here in 'f16x3', which agrees with 'f32' to ~1e-6 m: 1e-5 on top)
            assert not torch.equal(first['offsets'], exact['offsets'])
            m = first['backward_motion_weights'].sum(-1) >= 1e-4
            err = float((first['offsets'] - exact['offsets'])[m].abs().max())
            print('max |d offset| on fg samples %.3e m (test 5 at M = 32: %.3e m)' % (err, convergence[32]))
            assert 0 < err <= convergence[32] + 1e-5
            second = net(**d, iter_val=1e7)                                         # same dst_posevec tensor: no re-bake
            assert net.nonrigid_bake_count == c0 + 1
            assert all(same_bits(first[k], second[k]) for k in first)
            d['dst_posevec'] += 0.05                                                # in place: one re-bake
            moved = net(**d, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 2 and not torch.equal(moved['offsets'], first['offsets'])
            net(**d, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 2
            d['dst_posevec'].copy_(T(frame['dst_posevec']))
            again = net(**d, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 3 and all(same_bits(first[k], again[k]) for k in first)
            w[0] += 0.01                                                            # a non-rigid weight, in place
            shifted = net(**d, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 4 and not torch.equal(shifted['offsets'], first['offsets'])
            w.copy_(keep)
            net(**d, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 5
            fresh = dict(d, dst_posevec=d['dst_posevec'].clone())                   # a fresh tensor simply re-bakes
            other = net(**fresh, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 6 and all(same_bits(first[k], other[k]) for k in first)
            cfg.amd.nonrigid_bake_resolution = 24                                   # another M is another key
            net(**fresh, iter_val=1e7)
            assert net.nonrigid_bake_count == c0 + 7 and net._kept['baked_nr'].grid.shape[0] == 24
            cfg.amd.nonrigid_bake_resolution = 32
            assert net.bake_count == b0                                             # (the canonical grid never moved)
            # the lean form: the same picture
            cfg.amd.diagnostics = False
            lean = net(**d, iter_val=1e7)
            assert set(lean) == {'rgb', 'alpha', 'depth'} and all(same_bits(lean[k], first[k]) for k in lean)
            cfg.amd.term_eps = 1e-3
            with pytest.raises(NotImplementedError, match='term_eps'):
                net(**d, iter_val=1e7)
            cfg.amd.term_eps, cfg.amd.diagnostics = 0.0, True
            # offsets from a grid without a canonical grid: refused, both options named
            cfg.amd.canonical = 'mlp'
            with pytest.raises(ValueError) as e:
                net(**d, iter_val=1e7)
            assert 'cfg.amd.nonrigid' in str(e.value) and 'cfg.amd.canonical' in str(e.value)
            cfg.amd.canonical = 'baked'
            # ignore_non_rigid_motions: nothing is baked, and the frame is today's baked t-pose frame
            c1 = net.nonrigid_bake_count
            cfg.ignore_non_rigid_motions = True
            tp = net(**d, iter_val=1e7)
            cfg.amd.nonrigid = 'mlp'
            tp_today = net(**d, iter_val=1e7)
            cfg.ignore_non_rigid_motions = False
            assert net.nonrigid_bake_count == c1 and all(same_bits(tp[k], tp_today[k]) for k in tp_today)
            assert not bool(tp['offsets'].any())
            # the option back at 'mlp': today's baked frame, bit for bit
            back = net(**d, iter_val=1e7)
            assert net.nonrigid_bake_count == c1 and all(same_bits(back[k], today[k]) for k in today)
            assert net.check_f16_range(wait=True) is False
        # the training path ignores the option
        small = frame_to_gpu(frame, rays=512)
        for p in net.parameters():
            p.requires_grad_(True)
        with torch.enable_grad():
            cfg.amd.canonical, cfg.amd.nonrigid = 'baked', 'baked'
            tb = net(**small, iter_val=1e7)
            cfg.amd.canonical, cfg.amd.nonrigid = 'mlp', 'mlp'
            tm = net(**small, iter_val=1e7)
        assert tb['rgb'].requires_grad and net.nonrigid_bake_count == c1
        assert all(same_bits(tb[k].detach(), tm[k].detach()) for k in ('rgb', 'alpha', 'depth'))
    finally:
        with torch.no_grad():
            w.copy_(keep)
        net.set_baked_grid(None, None, None)


# --------------------------------------------------------------------------------------------------------- 5: convergence
def test_the_offset_grid_converges_to_the_mlp(convergence):
    """Exact K2 offsets ('f32') on the frame's samples with fg_mask >= 1e-4 against device grids of M = 128 and 32.
    The coarse error must stand 100 x above the f16 rounding of the stored values, 2^-11 max |offset|, so that the
    comparison is not one of two rounding floors; the fine one must be below half of it (on uniform points the fp64
    oracle alone gives a ratio of 0.16: a half asks for the direction with margin).
    Measured on an MI355X: 2.26e-3 m at M = 128, 1.49e-2 m at 32 (ratio 0.15) on 116 951 samples; max |offset| 0.107 m,
    f16 floor 5.2e-5 m."""
    e = convergence
    floor = 2.0 ** -11 * e['max_offset']
    print('max |d offset| (m) on %d samples: M=128 %.3e, M=32 %.3e; max |offset| %.3e, f16 floor %.3e'
          % (e['samples'], e[128], e[32], e['max_offset'], floor))
    assert e['samples'] > 10000
    assert e[32] > 100 * floor
    assert e[128] < 0.5 * e[32]


# ------------------------------------------------------------------------------------------------------------- 6: run.py
def test_run_movement_bakes_the_offsets_per_frame_and_names_the_folder(net, tmp_path):
    from humannerf_amd import dataset, run
    names = scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    old = (cfg.get('show_truth', False), cfg.get('show_alpha', False))
    cfg.amd.diagnostics, cfg.N_samples = False, 64
    net.set_baked_grid(None, None, None)
    listing = lambda p: sorted((f, os.stat(os.path.join(p, f)).st_mtime_ns) for f in os.listdir(p))
    try:
        exact = run.run_movement(net, subject, logdir=str(tmp_path / 'log'), metrics=['psnr'])
        assert 'baked' not in exact['image_dir'] and '_nr' not in os.path.basename(exact['image_dir'].rstrip('/'))
        before = listing(exact['image_dir'])
        assert len(before) >= 3
        cfg.amd.canonical, cfg.amd.bake_resolution = 'baked', 24
        cfg.amd.nonrigid, cfg.amd.nonrigid_bake_resolution = 'baked', 16
        c0, b0 = net.nonrigid_bake_count, net.bake_count
        res = run.run_movement(net, subject, logdir=str(tmp_path / 'log'), metrics=['psnr'])
        assert net.nonrigid_bake_count == c0 + 3 and net.bake_count == b0 + 1
        folder = os.path.basename(res['image_dir'].rstrip('/'))
        assert 'baked_24_nr16' in folder and folder.startswith('movement')
        pngs = sorted(f for f in os.listdir(res['image_dir']) if f.endswith('.png'))
        assert pngs == sorted(n + '.png' for n in names)
        assert res['image_dir'] != exact['image_dir'] and listing(exact['image_dir']) == before
        tp = run.run_tpose(net, subject, total_frames=2, image_size=64, logdir=str(tmp_path / 'log'))
        assert net.nonrigid_bake_count == c0 + 3 and 'baked_24' in tp['image_dir']
        assert '_nr' not in os.path.basename(tp['image_dir'].rstrip('/'))
        assert net.check_f16_range(wait=True) is False
    finally:
        cfg.show_truth, cfg.show_alpha = old
        net.set_baked_grid(None, None, None)
