"""Training a multi-head canonical MLP end to end on the GPU (cfg.amd.train_heads): Network.forward in training mode
with head_id = h and head_id = -1 against the reference's gradients (tests/golden/multihead_grad_h1.npz,
multihead_grad_all.npz, from tests/make_golden_multihead_train.py) and against fp64 autograd through the oracle, one
Trainer step per kind of item, and the training forward against the inference render.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from tests import heads_train_cases as hc
from tests import multihead_cases as mc
from tests.test_grad_oracle import compare_exact, compare_grads, grad_frame, reference_loss

pytestmark = pytest.mark.gpu

KEYS = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
        'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
H = hc.TRAIN_HEADS
# what tests/test_gpu_grad.py::test_network_gradients_match_reference asks, and the reference's own distance from fp64
# those numbers were set against (tests/test_grad_oracle.py::test_reference_gradient_noise_floor)
REL_NORM, COS_MIN, FLOOR_NORM = 6e-3, 0.99998, 4.4e-3


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def meta(golden_dir):
    with open(os.path.join(golden_dir, 'meta.json')) as f:
        return json.load(f)['grad_s64']


@pytest.fixture(scope='module')
def case(seeded_params, meta):
    """The weights, the frame on the device, the per-head loss weights."""
    fr = grad_frame(meta)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev()) for k in KEYS}
    return dict(state=hc.train_state(seeded_params), data=data, lw=hc.head_loss_weights(meta['n_rays']))


@pytest.fixture(scope='module')
def exact(case, meta):
    """fp64 autograd through the oracle, one pass per head (CPU): [H] dicts name -> gradient of head h's loss."""
    from tests.make_golden_multihead_train import oracle_head_gradients
    return [oracle_head_gradients(case['state'], meta, case['lw'], [h], torch.float64)[0] for h in range(H)]


@pytest.fixture()
def heads_run(meta):
    """cfg of the 3-head training run at the fixture's sampling for the duration of a test; yields cfg."""
    from humannerf_amd.config import cfg
    keep = (cfg.get('multihead'), cfg.canonical_mlp.get('multihead'))
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': H, 'split': 'argmin'}
    cfg.amd.train_heads = True
    cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions = meta['N_samples'], 0.0, False
    try:
        yield cfg
    finally:
        for node, key, val in ((cfg, 'multihead', keep[0]), (cfg.canonical_mlp, 'multihead', keep[1])):
            if val is None:
                node.pop(key, None)
            else:
                node[key] = val
        cfg.amd.train_heads = False
        cfg.N_samples, cfg.perturb = 128, 1.0
        cfg.amd.train_mlp_mode = cfg.amd.train_dw_mode = cfg.amd.train_chain_mode = 'f16x3'
        cfg.amd.train_operands = 'f16'


def make_net(case, train=True):
    from humannerf_amd.network import Network
    net = Network()
    assert net.head_num == H
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case['state'].items()}, strict=True)
    net = net.to(dev())
    return net.train() if train else net.eval()


def heads_loss(out, lw, heads):
    """sum over ``heads`` of grad_s64's loss with that head's weights; ``out``: one head's dict, or the all-heads lists."""
    if not isinstance(out['rgb'], list):
        return reference_loss(out, torch.from_numpy(lw[heads[0]]).to(dev()))
    return sum(reference_loss({k: out[k][h] for k in ('rgb', 'alpha', 'depth')}, torch.from_numpy(lw[h]).to(dev())) for h in heads)


@pytest.mark.parametrize('train_mode,operands', [('f32', 'f32'), ('f16x3', 'f32'), ('f16x3', 'f16')])
@pytest.mark.parametrize('head_id', [1, -1])
def test_multihead_gradients_match_reference(head_id, train_mode, operands, case, meta, exact, golden_dir, heads_run):
    """forward(head_id = 1) and forward(head_id = -1) in training mode, in the three arithmetic settings of
    tests/test_gpu_grad.py::test_network_gradients_match_reference, against the reference's own autograd (the fixture) and
    against fp64 autograd through the oracle.  Bounds: that test's, 6e-3 in norm and cosine 0.99998 for every tensor (pose
    decoder against fp64: 1e-2 / 0.99997).  They hold as they stand while the reference's distance from fp64 recorded with
    the fixture is within the 4.4e-3 they were set against; a larger one scales them by recorded / 4.4e-3.  Recorded
    (tests/make_golden_multihead_train.py; the loss weights: heads_train_cases.LOSS_SEED): see the printed line.
    head_id = 1: the gradient rows of heads 0 and 2 are exactly zero."""
    from humannerf_amd.network import full_gradient
    cfg = heads_run
    g = np.load(os.path.join(golden_dir, 'multihead_grad_h1.npz' if head_id == 1 else 'multihead_grad_all.npz'))
    heads = [1] if head_id == 1 else list(range(H))
    assert list(g['heads']) == heads
    cfg.amd.train_mlp_mode = cfg.amd.train_dw_mode = cfg.amd.train_chain_mode = train_mode
    cfg.amd.train_operands = operands
    net = make_net(case)
    out = net(**case['data'], head_id=head_id, iter_val=meta['iter_val'])
    assert len(out) == 11
    if head_id == -1:
        assert all(isinstance(out[k], list) and len(out[k]) == H for k in ('rgb', 'alpha', 'depth', 'weights_on_rays'))
        assert not out['weights_on_rays'][0].requires_grad and out['rgb'][2].requires_grad
    loss = heads_loss(out, case['lw'], heads)
    loss.backward()
    print('loss', float(loss), 'reference', float(g['loss']))
    assert abs(float(loss) - float(g['loss'])) <= 2e-4 * max(1.0, abs(float(g['loss'])))
    grads = {k: (full_gradient(p).cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
             for k, p in net.named_parameters()}
    if head_id == 1:
        for key in (mc.W_KEY, mc.B_KEY):
            assert float(np.abs(grads[key][0:4]).max()) == 0.0 and float(np.abs(grads[key][8:12]).max()) == 0.0
            assert float(np.abs(grads[key][4:8]).max()) > 0.0
    r = c = max(1.0, float(g['noise_floor']) / FLOOR_NORM)
    print('bounds: norm %.3e cosine %.6f (recorded floor %.2e / %.7f)'
          % (REL_NORM * r, 1.0 - (1.0 - COS_MIN) * c, float(g['noise_floor']), float(g['noise_floor_cos'])))
    want = {k: sum(exact[h][k] for h in heads) for k in exact[0]}
    vs_exact = compare_exact(grads, want, rel_norm=REL_NORM * r, cos_min=1.0 - (1.0 - COS_MIN) * c,
                             loose=('pose_decoder.', 1e-2 * r, 1.0 - 3e-5 * c))
    print('head_id', head_id, train_mode, operands, '| vs fp64', vs_exact)
    vs_ref = compare_grads(grads, g, rel_norm=REL_NORM * r, cos_min=1.0 - (1.0 - COS_MIN) * c)
    print('head_id', head_id, train_mode, operands, '| vs reference', vs_ref)


def flat_item(case, meta, head_id, seed=3):
    """A training item of flat rays with per-ray targets (Trainer.backward_step's second form) and its t_rand."""
    rs = np.random.RandomState(seed)
    n = meta['n_rays']
    item = dict(case['data'], head_id=head_id,
                target_rgbs=torch.from_numpy(rs.uniform(0, 1, (n, 3)).astype(np.float32)).to(dev()),
                t_rand=torch.from_numpy(rs.uniform(0, 1, (n, meta['N_samples'])).astype(np.float32)).to(dev()))
    return item


def test_train_step_on_one_head_leaves_the_other_heads_rows_unchanged(case, meta, heads_run):
    """One Trainer.train_step from fresh Adam state on a head_id = 1 item: rows 0..3 and 8..11 of output_linear.0 (and of
    its bias) keep their bits -- a zero gradient through Adam's first step is a zero update -- and rows 4..7 move."""
    from humannerf_amd.train import Trainer
    heads_run.train.lossweights = {'lpips': 0.0, 'mse': 0.2, 'l1': 0.0}
    try:
        net = make_net(case)
        lin = net.cnl_mlp.module.output_linear[0]
        w0, b0 = lin.weight.detach().clone(), lin.bias.detach().clone()
        trunk0 = net.cnl_mlp.module.linears()[0].weight.detach().clone()
        tr = Trainer(net)
        loss, parts = tr.train_step(flat_item(case, meta, 1))
        assert bool(torch.isfinite(loss)) and 'mse' in parts and tr.best_head is None
        w1, b1 = lin.weight.detach(), lin.bias.detach()
        for rows in (slice(0, 4), slice(8, 12)):
            assert torch.equal(w1[rows], w0[rows]) and torch.equal(b1[rows], b0[rows])
        assert not torch.equal(w1[4:8], w0[4:8]) and not torch.equal(b1[4:8], b0[4:8])
        assert not torch.equal(net.cnl_mlp.module.linears()[0].weight.detach(), trunk0)
    finally:
        heads_run.train.lossweights = {'lpips': 1.0, 'mse': 0.2, 'l1': 0.0}


def test_argmin_step_reports_the_head_a_render_without_gradient_selects(case, meta, heads_run):
    """One 'argmin' step (head_id = -1, perturbed sampling): best_head is the argmin of the per-head criteria computed
    here from a no_grad head_id = -1 render of the same weights with the same t_rand; every head's trunk gradient arrives,
    and with the default zero unselected weights only the best head's rows of output_linear.0 move."""
    from humannerf_amd.train import Trainer
    cfg = heads_run
    cfg.perturb = 1.0
    cfg.train.lossweights = {'lpips': 0.0, 'mse': 0.2, 'l1': 0.0}
    try:
        item = flat_item(case, meta, -1)
        net = make_net(case)
        with torch.no_grad():
            ref = net(**item, iter_val=1.0)
        crit = [0.2 * float(((rgb - item['target_rgbs']) ** 2).mean()) for rgb in ref['rgb']]
        gap = np.diff(np.sort(crit)).min()
        assert gap > 1e-4 * max(crit), crit                          # the heads are told apart far above 2e-5 per ray
        lin = net.cnl_mlp.module.output_linear[0]
        w0 = lin.weight.detach().clone()
        tr = Trainer(net)
        loss, parts = tr.train_step(item)
        best = int(np.argmin(crit))
        assert tr.best_head == best == parts['best_head']
        assert sorted(parts) == sorted(['mse', 'best_head'] + ['mse_head%d' % h for h in range(H)])
        for h in range(H):
            assert abs(float(parts['mse_head%d' % h]) - crit[h]) <= 1e-4 * crit[h], (h, float(parts['mse_head%d' % h]), crit[h])
        assert abs(float(loss) - crit[best]) <= 1e-4 * crit[best]
        for h in range(H):
            same = torch.equal(lin.weight.detach()[4 * h:4 * h + 4], w0[4 * h:4 * h + 4])
            assert same == (h != best), h
    finally:
        cfg.train.lossweights = {'lpips': 1.0, 'mse': 0.2, 'l1': 0.0}


def test_training_forward_equals_the_inference_render(case, meta, heads_run):
    """The training forward's per-head rgb / alpha against the inference head_id = -1 render of the same weights, within
    the golden cases' 2e-5 (depth: 1e-4 of far, as the smoke test asks); head_id = h is plane h of head_id = -1 bit for bit."""
    net = make_net(case)
    every = net(**case['data'], head_id=-1, iter_val=meta['iter_val'])
    one = net(**case['data'], head_id=1, iter_val=meta['iter_val'])
    with torch.no_grad():
        inf = net(**case['data'], head_id=-1, iter_val=meta['iter_val'])
    far = float(case['data']['far'].max())
    for h in range(H):
        for k, tol in (('rgb', 2e-5), ('alpha', 2e-5), ('depth', 1e-4 * far)):
            err = float((every[k][h].detach() - inf[k][h]).abs().max())
            assert err <= tol, (k, h, err)
    for k in ('rgb', 'alpha', 'depth'):
        assert torch.equal(one[k].detach(), every[k][1].detach()), k


def test_progress_writes_one_mosaic_per_head_from_one_all_heads_render(case, meta, heads_run, tmp_path):
    """make_progress_fn on a multi-head network: prog_{iter:06}_head{h}.jpg per head, each the mosaic of (render of head h |
    truth) pairs.  Expected files are built here from head h's OWN frames -- the single-head loop after select_head(h), whose
    8-bit images equal the planes of the head_id = -1 render bit for bit -- tiled and written by the same calls: the decoded
    images are equal, and the heads' mosaics differ from each other."""
    from PIL import Image
    from humannerf_amd import render, scene
    from humannerf_amd.train import Trainer, make_progress_fn
    heads_run.train.lossweights = {'lpips': 0.0, 'mse': 0.2, 'l1': 0.0}
    old_iter = heads_run.get('eval_iter', None)
    try:
        net = make_net(case, train=False)
        tr = Trainer(net)
        tr.iter = 7
        frames = [scene.synthetic_frame(H=48, W=40, focal_at_512=1250.0, pose_seed=s) for s in range(4)]
        for f in frames:
            f['target_rgbs'] = np.random.RandomState(1).rand(f['rays'].shape[1], 3).astype(np.float32)
        out = tmp_path / 'progress'
        make_progress_fn(frames, str(out), device=dev())(tr)
        files = sorted(p.name for p in out.iterdir())
        assert files == ['prog_000007_head%d.jpg' % h for h in range(H)]
        mosaics = [np.asarray(Image.open(out / f)) for f in files]
        assert all(m.shape == (48, 4 * 2 * 40, 3) for m in mosaics)
        heads_run.eval_iter = 7
        for h in range(H):
            net.select_head(h)
            pairs = {}
            render.render_frames(net, frames, device=dev(), show_truth=True,
                                 on_image=lambda i, rgb8, a8, t8=None: pairs.__setitem__(i, np.concatenate([rgb8, t8], axis=1)))
            want = tmp_path / ('want_head%d.jpg' % h)
            Image.fromarray(render.tile_images([pairs[i] for i in sorted(pairs)], imgs_per_row=4)).save(want)
            assert np.array_equal(mosaics[h], np.asarray(Image.open(want))), h
        assert all(not np.array_equal(mosaics[a], mosaics[b]) for a in range(H) for b in range(a))
    finally:
        net.select_head(None)
        heads_run.eval_iter = old_iter
        heads_run.train.lossweights = {'lpips': 1.0, 'mse': 0.2, 'l1': 0.0}
