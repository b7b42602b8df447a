"""Mesh extraction on the MI355X: the device route against the host route (bit for bit), the density lattice against
the canonical kernel and a grid_sample restatement of the gate, vertex colours against the fp64 oracle, forward
skinning, and run.run_mesh on a synthetic subject."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from humannerf_amd import mesh, ops, scene
from humannerf_amd.config import cfg
from humannerf_amd.network import Network, rodrigues
from humannerf_amd.seeded import default_shapes, seeded_state, with_density

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LO, HI = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
LEVEL = 10.0           # with the sigma bias raised by 5 (with_density): the surface where the gate fg is about 1/2


def field(N, f):
    ax = mesh.lattice_axes(LO, HI, N)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return f(x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)).astype(np.float32)


def lattice_points(bmin, bmax, N):
    ax = mesh.lattice_axes(bmin, bmax, N)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return np.stack([x, y, z], -1).reshape(-1, 3)


@pytest.fixture(scope='module')
def state():
    return with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)


@pytest.fixture(scope='module')
def net(state):
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return n.to(DEV).eval()


@pytest.fixture(scope='module')
def frame():
    return scene.synthetic_frame(H=64, W=64, pose_seed=3, pose_scale=0.3)


@pytest.fixture
def mode_is():
    old = cfg.amd.mlp_mode

    def set_mode(m):
        cfg.amd.mlp_mode = m
    yield set_mode
    cfg.amd.mlp_mode = old


def bbox(frame):
    return frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']


def assert_same_mesh(dev_mesh, host_mesh):
    v, f = (t.cpu().numpy() for t in dev_mesh)
    vh, fh = host_mesh
    assert f.dtype == np.int32 and np.array_equal(f, fh)
    assert np.array_equal(v, vh)


@pytest.mark.parametrize('case', ['sphere', 'torus', 'two_spheres', 'level_on_values', 'empty'])
def test_device_route_equals_host_route_on_analytic_grids(case):
    level = 0.0
    if case == 'sphere':
        d = field(96, lambda x, y, z: 0.8 - np.sqrt(x * x + y * y + z * z))
    elif case == 'torus':
        d = field(64, lambda x, y, z: 0.04 - (np.sqrt(x * x + y * y) - 0.5) ** 2 - z * z)
    elif case == 'two_spheres':
        d = field(64, lambda x, y, z: np.maximum(0.3 - np.sqrt((x - 0.45) ** 2 + y * y + z * z),
                                                 0.3 - np.sqrt((x + 0.45) ** 2 + y * y + z * z)))
    elif case == 'level_on_values':
        d, level = np.rint(field(32, lambda x, y, z: 4.0 * (0.6 - np.sqrt(x * x + y * y + z * z)))), 1.0
    else:
        d = np.full((16, 16, 16), -1.0, np.float32)
    dt = torch.from_numpy(d).to(DEV)
    first = mesh.mesh_from_density(dt, LO, HI, level)
    assert_same_mesh(first, mesh.mesh_from_density_host(d, LO, HI, level))
    second = mesh.mesh_from_density(dt, LO, HI, level)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_density_grid_is_the_canonical_kernel_times_the_gate(net, frame, mode, mode_is):
    mode_is(mode)
    N = 48
    bmin, bmax = bbox(frame)
    density, sigma, fg = net.canonical_density_grid(bmin, bmax, frame['motion_weights_priors'], resolution=N,
                                                    cnl_bbox_scale_xyz=frame['cnl_bbox_scale_xyz'], return_parts=True)
    assert density.shape == (N, N, N)
    pts = torch.from_numpy(lattice_points(bmin, bmax, N)).to(DEV)
    raw = ops.canonical(pts, net._canonical_packed(), mode)
    assert torch.equal(sigma.reshape(-1), raw[:, 3])
    assert torch.equal(density, torch.relu(sigma) * fg)
    # the gate: grid_sample (align_corners, zeros) of the bone channels at the lattice points, summed
    with torch.no_grad():
        vol = net._weight_volume(torch.from_numpy(frame['motion_weights_priors']).to(DEV))
        scale = torch.from_numpy(frame['cnl_bbox_scale_xyz']).to(DEV)
        g = (pts - torch.from_numpy(bmin).to(DEV)) * scale - 1.0
        ref = F.grid_sample(vol[None, :-1], g[None, None, None], mode='bilinear', padding_mode='zeros',
                            align_corners=True)[0, :, 0, 0].sum(0)
    assert float((fg.reshape(-1) - ref).abs().max()) <= 1e-6
    assert float(fg.max()) > 0.5 and float(fg.min()) < 1e-3          # the gate does cut the lattice
    assert float(density.max()) > LEVEL and float(density.min()) < LEVEL


def test_network_mesh_equals_host_route_and_colours_match_the_oracle(net, state, frame):
    from oracle import oracle
    bmin, bmax = bbox(frame)
    verts, faces, colors = net.extract_canonical_mesh(bmin, bmax, frame['motion_weights_priors'], resolution=96,
                                                      level=LEVEL)
    assert faces.shape[0] > 1000 and colors.shape == verts.shape
    density = net.canonical_density_grid(bmin, bmax, frame['motion_weights_priors'], resolution=96)
    assert_same_mesh((verts, faces), mesh.mesh_from_density_host(density.cpu().numpy(), bmin, bmax, LEVEL))
    again = net.extract_canonical_mesh(bmin, bmax, frame['motion_weights_priors'], resolution=96, level=LEVEL)
    assert all(torch.equal(a, b) for a, b in zip((verts, faces, colors), again))
    # colours: sigmoid(raw[:3]) of the canonical MLP, against the oracle in fp64 at 1000 vertices
    idx = np.linspace(0, verts.shape[0] - 1, 1000).astype(np.int64)
    x = verts[idx].cpu().double()
    s64 = {k: torch.from_numpy(v).double() for k, v in state.items()}
    ref = torch.sigmoid(oracle.canonical_mlp(s64, oracle.fourier_pe(x, 10))[:, :3])
    assert float((colors[idx].cpu().double() - ref).abs().max()) <= 2e-5


def test_pose_vertices_identity_and_one_bone():
    gen = torch.Generator().manual_seed(0)
    G, B = 32, 24
    bmin = torch.tensor([-1.0, -1.2, -0.4])
    scale = 2.0 / torch.tensor([2.0, 2.4, 0.8])
    verts = (bmin + torch.rand(5000, 3, generator=gen) * torch.tensor([2.0, 2.4, 0.8]) * 0.98 + 0.01).float()
    vol = torch.softmax(torch.randn(B + 1, G, G, G, generator=gen) * 3.0, dim=0)
    d = lambda t: t.contiguous().to(DEV)
    eye = torch.eye(3).expand(B, 3, 3)
    out = ops.forward_skin(d(verts), d(eye), d(torch.zeros(B, 3)), d(vol), d(bmin), d(scale)).cpu()
    assert float((out - verts).abs().max()) <= 1e-6
    # one-hot volume on bone 5: that bone's inverse rigid map
    k = 5
    onehot = torch.zeros(B + 1, G, G, G)
    onehot[k] = 1.0
    Rs = rodrigues(torch.randn(B, 3, generator=gen)).float()
    Ts = torch.randn(B, 3, generator=gen).float()
    out = ops.forward_skin(d(verts), d(Rs), d(Ts), d(onehot), d(bmin), d(scale)).cpu().double()
    ref = (verts.double() - Ts[k].double()) @ torch.linalg.inv(Rs[k].double()).T
    assert float((out - ref).abs().max()) <= 1e-5


def test_pose_vertices_on_a_synthetic_pose(net, frame):
    from oracle import oracle
    bmin, bmax = bbox(frame)
    verts, faces, _ = net.extract_canonical_mesh(bmin, bmax, frame['motion_weights_priors'], resolution=64, level=LEVEL)
    posed = net.pose_vertices(verts, frame).cpu().double()
    Rs, Ts, vol = (t.cpu().double() for t in net.frame_motion(frame))
    x = verts.cpu().double()
    g = (x - torch.from_numpy(bmin).double()) * torch.from_numpy(frame['cnl_bbox_scale_xyz']).double() - 1.0
    w = torch.stack([oracle.trilinear_zeros(vol[b], g) for b in range(Rs.shape[0])], -1)
    xb = torch.einsum('bij,vbj->vbi', torch.linalg.inv(Rs), x[:, None, :] - Ts[None])
    ref = (w[..., None] * xb).sum(1) / w.sum(1, keepdim=True).clamp(min=1e-4)
    assert float((posed - ref).abs().max()) <= 1e-5
    assert float((posed - x).abs().max()) > 1e-2                       # (the pose does move the body)


def test_run_mesh_writes_the_canonical_and_posed_meshes(net, tmp_path):
    from humannerf_amd import dataset, run
    names = scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=2, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    out = run.run_mesh(net, subject, frames=(0, names[1]), resolution=64, level=LEVEL, logdir=str(tmp_path / 'log'))
    assert set(out) == {'canonical', names[0], names[1]}
    v0, f0, c0 = mesh.read_ply(out['canonical'])
    assert os.path.dirname(out['canonical']).endswith('mesh') and f0.shape[0] > 100 and c0.shape == v0.shape
    for n in names:
        v, f, c = mesh.read_ply(out[n])
        assert os.path.basename(out[n]) == n + '.ply'
        assert v.shape == v0.shape and np.array_equal(f, f0) and np.array_equal(c, c0)
        assert np.all(np.isfinite(v)) and not np.array_equal(v, v0)
