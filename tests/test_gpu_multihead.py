"""The multi-head canonical MLP on the GPU: every head of one trunk pass (hnrf_canonical_heads_fwd and the frame entry
hnrf_render_frame_heads_fwd) against the fp64 twin of tests/multihead_cases.py, against the single-head kernels bit for
bit, and against the reference's outputs (tests/golden/multihead.npz).  Needs an MI355X: ``pytest -m gpu``."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import multihead_cases as mc

pytestmark = pytest.mark.gpu

IDX = [0, 2, 4, 6, 8, 10, 12, 14]


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _layers(st):
    ws = [st[f'cnl_mlp.module.pts_linears.{i}.weight'] for i in IDX] + [st[mc.W_KEY]]
    bs = [st[f'cnl_mlp.module.pts_linears.{i}.bias'] for i in IDX] + [st[mc.B_KEY]]
    return [T(w) for w in ws], [T(b) for b in bs]


def _kernel_state(rs, H, tiny_head=None):
    """Xavier-scaled canonical weights as test_gpu_parity._mlp_states draws them, the head layer (4H, 256) with every
    head at the scale of the single head there; ``tiny_head``: that head's weights are U(+-1e-5) instead (the scale the
    reference initialises last layers with, mlp_offset.py:60-66) -- its power-of-two lift differs from its neighbours'."""
    from humannerf_amd.seeded import default_shapes
    st = {}
    for k, s in default_shapes().items():
        if k.startswith('cnl_mlp'):
            if k == mc.W_KEY:
                s = (4 * H, 256)
            elif k == mc.B_KEY:
                s = (4 * H,)
            b = np.sqrt(6.0 / (4 + 256 if k == mc.W_KEY else sum(s[:2]))) * np.sqrt(2) if len(s) == 2 else 0.1
            st[k] = rs.uniform(-b, b, s).astype(np.float32)
    if tiny_head is not None:
        st[mc.W_KEY][4 * tiny_head:4 * tiny_head + 4] = rs.uniform(-1e-5, 1e-5, (4, 256)).astype(np.float32)
    return st


@functools.lru_cache(maxsize=None)
def _kernel_case(P, H):
    """(state, xyz, fp64 raw per head, CPU-fp32 raw per head): computed once, shared by both modes."""
    from oracle import oracle
    rs = np.random.RandomState(1000 * H + P)
    st = _kernel_state(rs, H)
    xyz = rs.uniform(-1.3, 1.3, (P, 3)).astype(np.float32)
    ref64 = mc.heads_raw64(st, xyz=xyz)
    out32 = oracle.canonical_mlp({k: torch.from_numpy(v) for k, v in st.items()},
                                 oracle.fourier_pe(torch.from_numpy(xyz), 10)).numpy()
    return st, xyz, ref64, [out32[:, 4 * h:4 * h + 4] for h in range(H)]


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('H', [2, 3, 8])
@pytest.mark.parametrize('P', [1, 31, 128, 1000, 4133])
def test_heads_kernel_matches_fp64(P, H, mode):
    """Every head of the all-heads launch vs the fp64 twin, at the tolerance of test_canonical_mlp_kernel (each head is
    the same dot product): ragged sample counts; H = 3 leaves lane half 1 one head short, puts a real bias into float 8 of
    the head's record and zero rows behind the heads; H = 8 fills the tile."""
    from humannerf_amd import ops
    st, xyz, ref64, ref32 = _kernel_case(P, H)
    ws, bs = _layers(st)
    packed = ops.canonical_heads_pack(ws, bs, H, mode)
    raw = ops.canonical_heads(T(xyz), packed, H, mode).cpu().numpy()
    assert raw.shape == (H, P, 4)
    for h in range(H):
        scale = max(1.0, np.abs(ref64[h]).max())
        e_hip, e_cpu = np.abs(raw[h] - ref64[h]).max() / scale, np.abs(ref32[h] - ref64[h]).max() / scale
        print('heads', mode, P, H, h, 'rel err hip %.2e cpu-fp32 %.2e' % (e_hip, e_cpu))
        assert e_hip <= 2e-5, (h, e_hip, e_cpu)
        assert e_hip <= 4 * e_cpu + 1e-6, (h, e_hip, e_cpu)


@pytest.mark.parametrize('mode', ['f32', 'f16x3', 'f16x3+noguard'])
@pytest.mark.parametrize('H,tiny', [(3, None), (3, 1), (8, None), (8, 6)])
def test_head_equals_single_head_kernel_bitwise(H, tiny, mode):
    """Head h of the all-heads launch == the single-head kernel on the image packed from rows 4h .. 4h+3, bit for bit,
    for every h; also with one head at +-1e-5 between normal ones (the exponent is taken per head)."""
    from humannerf_amd import ops
    rs = np.random.RandomState(7 + H)
    st = _kernel_state(rs, H, tiny_head=tiny)
    xyz = T(rs.uniform(-1.3, 1.3, (1000, 3)).astype(np.float32))
    base = mode.partition('+')[0]
    ws, bs = _layers(st)
    raw = ops.canonical_heads(xyz, ops.canonical_heads_pack(ws, bs, H, base), H, mode)
    for h in range(H):
        w1, b1 = _layers(mc.head_state(st, h))
        one = ops.canonical(xyz, ops.canonical_pack(w1, b1, base), mode)
        assert torch.equal(raw[h], one), (h, float((raw[h] - one).abs().max()))
    if tiny is not None:
        assert float(raw[tiny].abs().max()) > 0.0


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_heads_sparse_launch(mode):
    """The sparse launch equals the dense launch's listed rows bit for bit, leaves the unlisted rows of every plane
    untouched, and writes nothing for *count == 0."""
    from humannerf_amd import ops
    H, P = 3, 1000
    st, xyz, _, _ = _kernel_case(P, H)
    ws, bs = _layers(st)
    packed = ops.canonical_heads_pack(ws, bs, H, mode)
    x = T(xyz)
    dense = ops.canonical_heads(x, packed, H, mode)
    rs = np.random.RandomState(3)
    mask = T((rs.uniform(0, 1, P) < 0.37).astype(np.float32))
    idx, count = ops.compact_samples(mask, 0.5)
    n = int(count.item())
    assert 0 < n < P
    fill = 12345.0
    raw = torch.full((H, P, 4), fill, device=dev())
    ops.canonical_heads_sparse(x, packed, H, idx, count, mode, raw=raw)
    listed = mask > 0.5
    assert torch.equal(raw[:, listed], dense[:, listed])
    assert bool((raw[:, ~listed] == fill).all())
    idx0, count0 = ops.compact_samples(torch.zeros(P, device=dev()), 0.5)
    assert int(count0.item()) == 0
    raw0 = torch.full((H, P, 4), fill, device=dev())
    ops.canonical_heads_sparse(x, packed, H, idx0, count0, mode, raw=raw0)
    assert bool((raw0 == fill).all())


def test_heads_entries_refuse_bad_arguments():
    """H outside 2..8, a null plane and a misaligned raw are refused before any launch."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_heads()
    st, xyz, _, _ = _kernel_case(31, 3)
    ws, bs = _layers(st)
    packed = ops.canonical_heads_pack(ws, bs, 3, 'f32')
    x = T(xyz)
    raw = torch.zeros(3 * 31 * 4 + 4, device=dev())
    E_ARG = -1
    for bad in (1, 9, 0, -1):
        assert lib.hnrf_canonical_heads_fwd(x.data_ptr(), packed.data_ptr(), 0, 31, bad, raw.data_ptr(), None) != 0
        assert b'n_heads' in lib.hnrf_last_error()
        assert lib.hnrf_canonical_heads_pack(ops._ptr_array(ws), ops._ptr_array(bs), bad, 0, packed.data_ptr(), None) != 0
        assert lib.hnrf_render_frame_heads_workspace_bytes(96, 16, bad) == 0
    assert lib.hnrf_canonical_heads_fwd(x.data_ptr(), packed.data_ptr(), 0, 31, 3, raw.data_ptr() + 4, None) != 0
    assert b'aligned' in lib.hnrf_last_error()
    assert lib.hnrf_canonical_heads_fwd(x.data_ptr(), packed.data_ptr(), 0, 31, 3, None, None) != 0
    assert lib.hnrf_canonical_heads_fwd(x.data_ptr(), packed.data_ptr(), 7, 31, 3, raw.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert bool((raw == 0).all())
    with pytest.raises(_lib.HnrfError):
        ops.canonical_heads_pack(ws, bs, 4, 'f32')              # (12, 256) is not 4 heads
    assert E_ARG == lib.hnrf_canonical_heads_fwd(x.data_ptr(), packed.data_ptr(), 0, 31, 9, raw.data_ptr(), None)


# ------------------------------------------------------------------ the frame
H_FRAME, N_FRAME, CHUNK = 3, 200, 96                 # chunks of 96, 96, 8: a ragged last chunk
PER_HEAD = ('rgb', 'alpha', 'depth', 'weights_on_rays', 'rgb_on_rays', 'cnl_xyz', 'cnl_rgb', 'cnl_weight')


@pytest.fixture(scope='module')
def fixture_npz(golden_dir):
    return np.load(os.path.join(golden_dir, 'multihead.npz'))


@pytest.fixture(scope='module')
def heads_net(seeded_params):
    """A Network with H_FRAME heads on the fixture's weights; the configuration is restored when the module is done."""
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    keep = (cfg.get('multihead'), cfg.canonical_mlp.get('multihead'))
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': H_FRAME, 'split': 'view'}
    try:
        net = Network()
    finally:
        for node, key, val in ((cfg, 'multihead', keep[0]), (cfg.canonical_mlp, 'multihead', keep[1])):
            if val is None:
                node.pop(key)
            else:
                node[key] = val
    state = mc.multihead_state(seeded_params, H_FRAME)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return net.to(dev()).eval().deploy_mlps_to_secondary_gpus()


@pytest.fixture(scope='module')
def heads_frame(golden_frame):
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    d = {k: T(golden_frame[k]) for k in keys}
    d['rays'] = d['rays'][:, :N_FRAME].contiguous()
    d['near'], d['far'] = d['near'][:N_FRAME].contiguous(), d['far'][:N_FRAME].contiguous()
    return d


class _Options:
    """cfg values of a test, put back afterwards."""

    def __init__(self, **amd):
        self.amd = amd

    def __enter__(self):
        from humannerf_amd.config import cfg
        self.keep = (cfg.N_samples, cfg.perturb, cfg.chunk, {k: cfg.amd[k] for k in self.amd})
        cfg.N_samples, cfg.perturb, cfg.chunk = mc.FIXTURE_S, 0.0, CHUNK
        for k, v in self.amd.items():
            cfg.amd[k] = v
        return cfg

    def __exit__(self, *exc):
        from humannerf_amd.config import cfg
        cfg.N_samples, cfg.perturb, cfg.chunk = self.keep[:3]
        for k, v in self.keep[3].items():
            cfg.amd[k] = v


@pytest.mark.parametrize('diag', [True, False])
@pytest.mark.parametrize('mode', ['f16x3', 'f32'])
def test_frame_all_heads(mode, diag, heads_net, heads_frame, fixture_npz):
    """forward(head_id=-1)[k][h] is bit-equal to forward(head_id=h)[k] (share_underflow off), within 2e-5 (rgb, alpha)
    of the reference's frame of head h; xyz_on_rays / offsets / backward_motion_weights are the single-head run's."""
    net = heads_net
    with _Options(mlp_mode=mode, diagnostics=diag, share_underflow=False), torch.no_grad():
        every = net(**heads_frame, head_id=-1)
        keys = [k for k in PER_HEAD if diag or k in ('rgb', 'alpha', 'depth')]
        assert set(every) == set(keys) | ({'xyz_on_rays', 'backward_motion_weights', 'offsets'} if diag else set())
        for h in range(H_FRAME):
            one = net(**heads_frame, head_id=torch.tensor(h))
            for k in keys:
                assert isinstance(every[k], list) and len(every[k]) == H_FRAME
                assert torch.equal(every[k][h], one[k]), (k, h, float((every[k][h] - one[k]).abs().max()))
            if diag:
                assert isinstance(every['xyz_on_rays'], list) and len(every['xyz_on_rays']) == H_FRAME
                assert torch.equal(every['xyz_on_rays'][h], one['xyz_on_rays'])
                assert torch.equal(every['offsets'], one['offsets'])
                assert torch.equal(every['backward_motion_weights'], one['backward_motion_weights'])
            for k in ('rgb', 'alpha'):
                err = np.abs(every[k][h].cpu().numpy() - fixture_npz['H%d/%s' % (H_FRAME, k)][h]).max()
                print('frame', mode, diag, k, h, 'err vs reference %.2e' % err)
                assert err <= 2e-5, (k, h, err)
        assert net.check_f16_range(wait=True) is False
        # the heads differ (a test that compared a head with itself would pass on anything)
        assert not torch.equal(every['rgb'][0], every['rgb'][1])
        # a 0-d tensor on the device is read once, then remembered
        hid = torch.tensor(1, device=dev())
        a = net(**heads_frame, head_id=hid)
        b = net(**heads_frame, head_id=hid)
        assert net._kept['head_id'].inputs[0][0]() is hid and torch.equal(a['rgb'], every['rgb'][1]) and torch.equal(b['rgb'], a['rgb'])


def test_frame_all_heads_direct_abi(heads_net, heads_frame):
    """hnrf_render_frame_heads_fwd called directly (ctypes, no ops wrapper, a workspace of exactly the stated size): every
    head's planes equal hnrf_render_frame_fwd on that head's single-head image, with and without the diagnostic outputs."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_heads()
    net, fr, S, B, H = heads_net, heads_frame, mc.FIXTURE_S, heads_net.total_bones, H_FRAME
    mode = 'f16x3'
    with _Options(mlp_mode=mode, diagnostics=True, share_underflow=False), torch.no_grad():
        rvec, cond, hann_host, hann_w, _ = net._conditioning(fr['dst_posevec'], 1e7, dev(), True)
        from humannerf_amd.network import motion_basis
        Rs, Ts = motion_basis(fr['dst_Rs'], fr['dst_Ts'], fr['cnl_gtfms'], rvec)
        vol = net._weight_volume(fr['motion_weights_priors'])
        nr_packed = net._nonrigid_packed(cond).clone()
        lin = net.cnl_mlp.module.linears()
        ws, bs = [l.weight.detach() for l in lin], [l.bias.detach() for l in lin]
        all_packed = ops.canonical_heads_pack(ws, bs, H, mode)
        rays_o, rays_d = fr['rays'][0].contiguous(), fr['rays'][1].contiguous()
        args = (rays_o, rays_d, fr['near'], fr['far'], None, Rs.contiguous(), Ts.contiguous(), vol,
                fr['cnl_bbox_min_xyz'], fr['cnl_bbox_scale_xyz'], hann_w, nr_packed)
        N, G = rays_o.shape[0], vol.shape[-1]
        need = lib.hnrf_render_frame_heads_workspace_bytes(CHUNK, S, H)
        assert need > lib.hnrf_render_frame_workspace_bytes(CHUNK, S) + (H - 1) * CHUNK * S * 16
        ws_buf = torch.empty(need // 4, device=dev())
        for diag in (True, False):
            shapes = ops.output_shapes(S, B, diag)
            planes = {k: torch.full((H, N) + shapes[k], -7.0, device=dev()) for k in PER_HEAD if k in shapes}
            single = {k: torch.full((N,) + v, -7.0, device=dev()) for k, v in shapes.items() if k not in PER_HEAD}
            arr = lambda k: (ctypes.c_void_p * H)(*[planes[k][h].data_ptr() for h in range(H)]) if k in planes else None
            p = lambda t: None if t is None else t.data_ptr()
            rc = lib.hnrf_render_frame_heads_fwd(
                *map(p, args), all_packed.data_ptr(), fr['bgcolor'].data_ptr(), ops._mode_arg(mode), 0.0, N, S, B, G, CHUNK, H,
                ws_buf.data_ptr(), need, *[arr(k) for k in PER_HEAD], p(single.get('xyz_on_rays')),
                p(single.get('backward_motion_weights')), p(single.get('offsets')), None, None, None,
                torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.hnrf_last_error()
            for h in range(H):
                one_packed = ops.canonical_pack(ws[:8] + [ws[8][4 * h:4 * h + 4]], bs[:8] + [bs[8][4 * h:4 * h + 4]], mode)
                one, _ = ops.render_frame(*args, one_packed, fr['bgcolor'], S, CHUNK, mode, diagnostics=diag, overlap=False)
                for k, v in planes.items():
                    assert torch.equal(v[h], one[k]), (diag, k, h)
                for k, v in single.items():
                    assert torch.equal(v, one[k]), (diag, k)
            # a null plane and a workspace one byte short are refused before anything runs
            bad = (ctypes.c_void_p * H)(*([planes['rgb'][0].data_ptr()] * (H - 1) + [None]))
            rest = [arr(k) for k in PER_HEAD[1:]]
            tail = (p(single.get('xyz_on_rays')), p(single.get('backward_motion_weights')), p(single.get('offsets')), None,
                    None, None, torch.cuda.current_stream().cuda_stream)
            head = (*map(p, args), all_packed.data_ptr(), fr['bgcolor'].data_ptr(), ops._mode_arg(mode), 0.0, N, S, B, G, CHUNK)
            assert lib.hnrf_render_frame_heads_fwd(*head, H, ws_buf.data_ptr(), need, bad, *rest, *tail) == -1
            assert lib.hnrf_render_frame_heads_fwd(*head, H, ws_buf.data_ptr(), need - 1, arr('rgb'), *rest, *tail) != 0
            assert lib.hnrf_render_frame_heads_fwd(*head, 9, ws_buf.data_ptr(), need, arr('rgb'), *rest, *tail) == -1


def test_all_heads_refusals_and_cull(heads_net, heads_frame):
    """head_id = -1 is the exact MLP path only: the baked canonical grid and early ray termination raise; sample culling
    works through the sparse launch and equals the single-head culled frame; a training-mode forward raises."""
    net = heads_net
    with _Options(mlp_mode='f16x3', diagnostics=False, share_underflow=False, canonical='mlp', term_eps=0.0,
                  cull_eps=0.0) as cfg, torch.no_grad():
        cfg.amd.cull_eps = 1e-3
        every = net(**heads_frame, head_id=-1)
        for h in range(H_FRAME):
            one = net(**heads_frame, head_id=h)
            for k in ('rgb', 'alpha', 'depth'):
                assert torch.equal(every[k][h], one[k]), (k, h)
        cfg.amd.cull_eps = 0.0
        cfg.amd.term_eps = 1e-3
        with pytest.raises(NotImplementedError, match='term_eps'):
            net(**heads_frame, head_id=-1)
        cfg.amd.term_eps = 0.0
        cfg.amd.canonical = 'baked'
        with pytest.raises(NotImplementedError, match='baked'):
            net(**heads_frame, head_id=-1)
        cfg.amd.canonical = 'mlp'
    with _Options(mlp_mode='f16x3'):
        with pytest.raises(NotImplementedError, match='inference only'):
            net(**heads_frame, head_id=0)                   # grad mode on, parameters require grad


def test_selected_head_outside_forward(heads_net, heads_frame):
    """select_head(h) packs head h for the passes outside forward; no selection raises instead of using head 0."""
    from humannerf_amd import ops
    net = heads_net
    verts = T(np.random.RandomState(2).uniform(-0.5, 0.5, (77, 3)).astype(np.float32))
    with _Options(mlp_mode='f16x3'):
        net.select_head(None)
        with pytest.raises(RuntimeError, match='select_head'):
            net.vertex_colors(verts)
        lin = net.cnl_mlp.module.linears()
        ws, bs = [l.weight.detach() for l in lin], [l.bias.detach() for l in lin]
        raw = ops.canonical_heads(verts, ops.canonical_heads_pack(ws, bs, H_FRAME, 'f16x3'), H_FRAME, 'f16x3')
        cols = []
        for h in range(H_FRAME):
            cols.append(net.select_head(h).vertex_colors(verts))
            assert torch.equal(cols[-1], torch.sigmoid(raw[h][:, :3]))
        assert not torch.equal(cols[0], cols[1])
        with torch.no_grad():
            one = net(**heads_frame)                        # no head_id: the selected head (the last one)
            assert torch.equal(one['rgb'], net(**heads_frame, head_id=H_FRAME - 1)['rgb'])
        net.select_head(None)
        with pytest.raises(ValueError):
            net.select_head(H_FRAME)


def test_run_heads_on_a_subject_directory(heads_net, golden_dir, tmp_path):
    """run.run_heads over the synthetic subject directory: one folder per head with the reference's names
    (<load_net><tag>_h<i>/<folder>), one metrics line per head and frame, and head i's picture equal to run_movement's
    after select_head(i)."""
    from PIL import Image
    from humannerf_amd import dataset, run
    from humannerf_amd.config import cfg
    net = heads_net
    subj = dataset.Subject(os.path.join(golden_dir, 'subject_synth'))
    old = (cfg.N_samples, cfg.get('show_truth', False), cfg.get('show_alpha', False), cfg.bgcolor)
    names = ['frame_000003.png', 'frame_000010.png', 'frame_000042.png']
    with _Options(mlp_mode='f16x3', diagnostics=False, share_underflow=False, video='none', maps=[]):
        cfg.N_samples, cfg.show_alpha, cfg.bgcolor, cfg.chunk = 64, False, [255., 255., 255.], 32768
        try:
            res = run.run_heads(net, subj, kind='movement', logdir=str(tmp_path), metrics=['psnr'])
            tp = run.run_heads(net, subj, kind='tpose', total_frames=2, image_size=64, logdir=str(tmp_path))
            assert cfg.ignore_non_rigid_motions is False and cfg.perturb == 0.0
            one = run.run_movement(net.select_head(1), subj, logdir=str(tmp_path / 'single'), metrics=['psnr'])
            cfg.amd.video = 'mjpeg'
            with pytest.raises(ValueError, match='video'):
                run.run_heads(net, subj, logdir=str(tmp_path))
            cfg.amd.video, cfg.amd.maps = 'none', ['depth']
            with pytest.raises(ValueError, match='maps'):
                run.run_heads(net, subj, logdir=str(tmp_path))
        finally:
            net.select_head(None)
            cfg.N_samples, cfg.show_truth, cfg.show_alpha, cfg.bgcolor = old
    assert len(res) == H_FRAME == len(tp)
    pictures = []
    for h in range(H_FRAME):
        root = tmp_path / ('latest_h%d' % h)
        assert res[h]['image_dir'] == str(root / 'movement') and sorted(os.listdir(root / 'movement')) == names
        lines = [l for l in open(root / 'movement-metrics.perimg.txt').read().splitlines() if ': psnr-' in l]
        assert [l.split(':')[0] for l in lines] == [n[:-4] for n in names]
        assert open(root / 'movement-metrics.average.txt').read().splitlines()[-1].startswith('p:')
        assert res[h]['metrics']['psnr'] > 3.0
        pictures.append([np.asarray(Image.open(root / 'movement' / n)) for n in names])
        assert pictures[-1][0].shape == (64, 2 * 48, 3)                # render | truth
        assert sorted(os.listdir(root / 'tpose')) == ['000000.png', '000001.png']
    assert not np.array_equal(pictures[0][1], pictures[1][1])          # the heads paint different pictures
    for i, n in enumerate(names):
        single = np.asarray(Image.open(tmp_path / 'single' / 'latest' / 'movement' / n))
        assert np.array_equal(single, pictures[1][i])
    assert abs(one['metrics']['psnr'] - res[1]['metrics']['psnr']) < 1e-9
