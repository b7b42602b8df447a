"""Shared by the view-dependent-colour tests and tests/make_golden_viewdir.py: the seeded view layers, the frame of the
fixture, and the fp64 twin of the reference's view branch (mlp_rgb_sigma.py:85-96, 168-178) built from the CPU oracle's
own functions.  The twin evaluates the branch LAYERED, as the reference writes it -- density = Wd h + bd,
rgb = W3 (W2 [W1 h + b1 ; e(d)] + b2) + b3 -- so it does not depend on the fold the code under test uses."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle

P = 'cnl_mlp.module.'
VIEW_LAYERS = ('output_linear_density.0', 'output_linear_rgb_1.0', 'output_linear_rgb_2.0', 'output_linear_rgb_2.1')
VIEW_SEED = 40
BANDS = 4                       # canonical_mlp.multires_dir of the fixture: 3 + 6 * 4 = 27 columns
# the fixture's frame: the first 200 rays of the default golden frame (tests/golden/meta.json 'frame') at S = 16, iter 1e7;
# sigma scaled to its sample spacing like tests/multihead_cases.SIGMA_SCALE
N_RAYS, N_POINTS, FIXTURE_S = 200, 300, 16
SIGMA_SCALE = FIXTURE_S / 128.0
# the gradient case: the scene of grad_s64 (S = 64)
TRAIN_SIGMA_SCALE = 64 / 128.0
FRAME_KEYS = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
              'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']


def view_tensors(bands=BANDS, seed=VIEW_SEED, sigma_scale=1.0):
    """name -> float32 array of the four view layers from a stream of their own.  Density: the sigma row of
    humannerf_amd.seeded's head (logits x 3, x SIGMA_GAIN, bias + SIGMA_BIAS), then x ``sigma_scale``; the colour layers
    Xavier-uniform with unit gain (nothing non-linear follows them), the last one x 3 like the seeded head's logits."""
    from humannerf_amd.seeded import SIGMA_BIAS, SIGMA_GAIN
    rs = np.random.RandomState(seed + bands)
    E = 3 + 6 * bands
    out = {}
    for name, (n_out, n_in), gain in zip(VIEW_LAYERS, ((1, 256), (256, 256), (256, 256 + E), (3, 256)),
                                         (math.sqrt(2.0) * 3.0 * SIGMA_GAIN * sigma_scale, 1.0, 1.0, 3.0)):
        b = gain * math.sqrt(6.0 / (n_out + n_in))
        out[P + name + '.weight'] = rs.uniform(-b, b, size=(n_out, n_in)).astype(np.float32)
        out[P + name + '.bias'] = rs.uniform(-0.05, 0.05, size=(n_out,)).astype(np.float32)
    k = P + VIEW_LAYERS[0] + '.bias'
    out[k] = ((out[k] + SIGMA_BIAS) * sigma_scale).astype(np.float32)
    return out


def view_state(base_state, bands=BANDS, sigma_scale=SIGMA_SCALE, seed=VIEW_SEED):
    """``base_state`` (seeded.seeded_state of the default shapes) without output_linear, with the seeded view layers."""
    st = {k: v for k, v in base_state.items() if '.output_linear.' not in k}
    st.update(view_tensors(bands, seed, sigma_scale))
    return st


def camera_rotation():
    """The fixed rotation (about 40 degrees about (1, 2, 3)) between row 1 and row 2 of the fixture's rays, float64."""
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    a = math.radians(40.0)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx.dot(Kx)


def with_camera_row(frame, n_rays=None):
    """``frame`` (scene.synthetic_frame) cut to its first ``n_rays`` rays, the third row of ``rays`` = row 1 turned by
    camera_rotation(), so that view_dir_camera_only True and False must differ."""
    fr = dict(frame)
    n = frame['rays'].shape[1] if n_rays is None else n_rays
    rays = np.array(frame['rays'][:, :n], dtype=np.float32)
    rays[2] = (rays[1].astype(np.float64) @ camera_rotation().T).astype(np.float32)
    fr['rays'], fr['near'], fr['far'] = rays, frame['near'][:n].copy(), frame['far'][:n].copy()
    return fr


def fixture_frame(golden_dir):
    import json
    import os
    from humannerf_amd import scene
    with open(os.path.join(golden_dir, 'meta.json')) as f:
        args = {k: v for k, v in json.load(f)['frame'].items() if k != 'seed'}
    return with_camera_row(scene.synthetic_frame(**args), N_RAYS)


def embed(dirs, bands=BANDS):
    """e(d) = PE_L(normalize(d)) (network.py:499-507 + fourier.py), in dirs' dtype."""
    return oracle.fourier_pe(F.normalize(dirs, dim=-1), bands)


def canonical_view_raw(state, pe, dirs, bands=BANDS):
    """The reference's CanonicalMLP(view_dir=True).forward, layered: pe (P, 63), dirs (P, 3) -> raw (P, 4) = rgb | density.
    The trunk is oracle.canonical_mlp's (its last hidden activation); differentiable in the state's tensors."""
    st = dict(state)
    st[P + 'output_linear.0.weight'], st[P + 'output_linear.0.bias'] = pe.new_zeros(1, 256), pe.new_zeros(1)
    hidden = []
    oracle.canonical_mlp(st, pe, hidden)
    h = hidden[-1]
    density = oracle._lin(state, P + VIEW_LAYERS[0], h)
    feat = torch.cat([oracle._lin(state, P + VIEW_LAYERS[1], h), embed(dirs, bands)], dim=1)
    rgb = oracle._lin(state, P + VIEW_LAYERS[3], oracle._lin(state, P + VIEW_LAYERS[2], feat))
    return torch.cat([rgb, density], dim=1)


def t64(state, prefix=''):
    return {k: torch.as_tensor(np.asarray(v)).double() for k, v in state.items() if k.startswith(prefix)}


def fold_parts(state, dtype=np.float64):
    """(A | Wd (4, 256), c | bd (4,), B (3, E)) written out in numpy from the four layers, in ``dtype``."""
    g = lambda n, w: np.asarray(state[P + n + '.' + w]).astype(dtype)
    Wd, bd = g(VIEW_LAYERS[0], 'weight'), g(VIEW_LAYERS[0], 'bias')
    W1, b1 = g(VIEW_LAYERS[1], 'weight'), g(VIEW_LAYERS[1], 'bias')
    W2, b2 = g(VIEW_LAYERS[2], 'weight'), g(VIEW_LAYERS[2], 'bias')
    W3, b3 = g(VIEW_LAYERS[3], 'weight'), g(VIEW_LAYERS[3], 'bias')
    n = W1.shape[0]
    A, B = W3 @ W2[:, :n] @ W1, W3 @ W2[:, n:]
    c = W3 @ (W2[:, :n] @ b1 + b2) + b3
    return np.concatenate([A, Wd]), np.concatenate([c, bd]), B


def render_view(state, data, bands=BANDS, camera_only=False, iter_val=1e7, dtype=torch.float64, **overrides):
    """oracle.render with the view branch: Network.forward (network.py:647-789) of a view_dir network, one chunk, from
    the oracle's stages.  ``state``: arrays, or tensors (leaves that require grad stay leaves when ``dtype`` is theirs)."""
    opt = dict(oracle.DEFAULTS)
    opt.update(overrides)
    d = {k: torch.as_tensor(data[k]).to(dtype) for k in FRAME_KEYS}
    state = {k: torch.as_tensor(v).to(dtype) for k, v in state.items()}
    fr = oracle.per_frame_setup(state, d, iter_val, opt)
    rays_o, rays_d = d['rays'][0].reshape(-1, 3), d['rays'][1].reshape(-1, 3)
    dirs = d['rays'][2].reshape(-1, 3) if camera_only else rays_d
    R, S = rays_o.shape[0], opt['N_samples']
    z = oracle.z_values(d['near'], d['far'], S)
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]
    x_skel, mask, _ = oracle.sample_motion_fields(pts.reshape(-1, 3), fr['Rs'], fr['Ts'], fr['vol'], d['cnl_bbox_min_xyz'],
                                                  d['cnl_bbox_scale_xyz'])
    xyz, _ = oracle.non_rigid_mlp(state, oracle.hann_pe(x_skel, fr['hann_w']), fr['cond'], x_skel)
    raw = canonical_view_raw(state, oracle.fourier_pe(xyz, opt['cnl_multires']), dirs.repeat_interleave(S, dim=0), bands)
    out = oracle.raw2outputs(raw.view(R, S, 4), mask.view(R, S), z, rays_d, xyz.view(R, S, 3), d['bgcolor'])
    out['_raw'] = raw.view(R, S, 4)
    return out


def gradients(state, data, lw, bands=BANDS, camera_only=False, iter_val=1e7, N_samples=64, dtype=torch.float64):
    """Gradients of tests.test_grad_oracle.reference_loss by torch.autograd through render_view: name -> ndarray, loss."""
    from tests.test_grad_oracle import reference_loss
    leaves = {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    out = render_view(leaves, data, bands, camera_only, iter_val, dtype, N_samples=N_samples)
    loss = reference_loss(out, lw)
    loss.backward()
    return {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in leaves.items()}, float(loss.detach())


def compare_to_fixture(grads, g, rel_norm, cos_min, n_tensors=None):
    """tests.test_grad_oracle.compare_grads for a fixture of any number of tensors: every ``norm/<name>`` of the npz
    ``g`` against ``grads`` in norm, and in cosine against the stored ``grad/`` (whole) or ``head/`` (first 4096)."""
    checked, worst_norm, worst_cos = 0, (0.0, None), (1.0, None)
    for key in g.files:
        if not key.startswith('norm/'):
            continue
        name = key[5:]
        ref_norm, got = float(g[key]), grads[name]
        gn = float(np.linalg.norm(got.astype(np.float64)))
        assert abs(gn - ref_norm) <= rel_norm * max(ref_norm, 1e-8), (name, gn, ref_norm)
        if ref_norm > 0:
            worst_norm = max(worst_norm, (abs(gn - ref_norm) / ref_norm, name))
        a = got.reshape(-1)
        ref = g['grad/' + name] if 'grad/' + name in g.files else None
        if ref is None and 'head/' + name in g.files:
            ref, a = g['head/' + name], a[:4096]
        if ref is not None and np.linalg.norm(ref) > 0:
            r = ref.reshape(-1).astype(np.float64)
            cos = float(a.astype(np.float64) @ r / (np.linalg.norm(a) * np.linalg.norm(r) + 1e-300))
            assert cos >= cos_min, (name, cos)
            worst_cos = min(worst_cos, (cos, name))
        checked += 1
    assert n_tensors is None or checked == n_tensors, checked
    return {'worst_rel_norm_err': worst_norm, 'worst_cosine': worst_cos}


class view_config:
    """``with view_config(camera_only=..., N_samples=..., chunk=..., **amd) as cfg``: the global cfg with view-dependent
    colour on (BANDS bands), cfg.perturb = 0 and the given top-level / cfg.amd values; everything is put back on exit."""
    TOP = ('N_samples', 'perturb', 'chunk', 'ignore_non_rigid_motions')
    CM = ('view_dir', 'view_embed', 'multires_dir', 'view_dir_camera_only')

    def __init__(self, camera_only=False, bands=BANDS, N_samples=None, chunk=None, **amd):
        self.camera_only, self.bands, self.N_samples, self.chunk, self.amd = camera_only, bands, N_samples, chunk, amd

    def __enter__(self):
        from humannerf_amd.config import cfg
        self.cfg = cfg
        self.keep_top = {k: cfg.get(k) for k in self.TOP}
        self.keep_cm = {k: cfg.canonical_mlp.get(k) for k in self.CM}
        self.keep_amd = {k: cfg.amd.get(k) for k in ('view_dir',) + tuple(self.amd)}
        cm = cfg.canonical_mlp
        cm.view_dir, cm.view_embed, cm.multires_dir, cm.view_dir_camera_only = True, 'mlp', self.bands, self.camera_only
        cfg.amd.view_dir = True
        cfg.perturb, cfg.ignore_non_rigid_motions = 0.0, False
        if self.N_samples is not None:
            cfg.N_samples = self.N_samples
        if self.chunk is not None:
            cfg.chunk = self.chunk
        for k, v in self.amd.items():
            cfg.amd[k] = v
        return cfg

    def __exit__(self, *exc):
        cfg = self.cfg
        for node, keep in ((cfg, self.keep_top), (cfg.canonical_mlp, self.keep_cm), (cfg.amd, self.keep_amd)):
            for k, v in keep.items():
                if v is None:
                    node.pop(k, None)
                else:
                    node[k] = v
        return False
