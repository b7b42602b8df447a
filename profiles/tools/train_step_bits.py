"""One step of train.Trainer on a fixed 6-window patch batch with fixed t_rand, below and above the non-rigid kick-in:
writes loss, the three forward outputs and every gradient to OUT.npz (argv[1]).  With more arguments -- PARENT1.npz
PARENT2.npz PARENT3.npz THIS.npz -- it compares instead: tensors bit-equal among the parent's runs must be bit-equal in
THIS; for the others (atomic accumulation order) THIS may differ from a parent run by at most four times the largest
difference among the parent's own three pairs."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

if len(sys.argv) > 2:
    runs = [np.load(p) for p in sys.argv[1:5]]
    par, this = runs[:3], runs[3]
    bad = 0
    for k in par[0].files:
        own = max(float(np.abs(par[a][k].astype(np.float64) - par[b][k]).max()) for a, b in ((0, 1), (0, 2), (1, 2)))
        stable = all(par[0][k].tobytes() == p[k].tobytes() for p in par[1:])
        diff = max(float(np.abs(this[k].astype(np.float64) - p[k]).max()) for p in par)
        ok = this[k].tobytes() == par[0][k].tobytes() if stable else diff <= 4 * own
        bad += not ok
        if not stable or not ok or '/grad/' not in k:
            print('%-72s %s parent pairs max %.3e  this vs parent max %.3e  %s' % (
                k, 'bit-stable' if stable else 'noisy     ', own, diff, 'ok' if ok else 'MISMATCH'))
    n_stable = sum(all(par[0][k].tobytes() == p[k].tobytes() for p in par[1:]) for k in par[0].files)
    print('%d tensors, %d bit-stable in the parent, %d mismatches' % (len(par[0].files), n_stable, bad))
    sys.exit(1 if bad else 0)

import torch
from humannerf_amd import scene
from humannerf_amd.config import cfg
from humannerf_amd.network import Network
from humannerf_amd.seeded import default_shapes, seeded_state
from humannerf_amd.train import Trainer

dev = torch.device('cuda:0')
H = W = 128
S, NP, PS = 32, 6, 16
fr = scene.synthetic_frame(H=H, W=W, focal_at_512=1250.0)
np.random.seed(5)
hit2d = fr['ray_mask'].reshape(H, W)
subject = np.zeros((H, W), dtype=bool); subject[H // 4:3 * H // 4, 3 * W // 8:5 * W // 8] = True
sel, pinfo, div = scene.sample_patch_rays(fr['ray_mask'], subject & hit2d, hit2d, NP, PS, H, W, subject_ratio=0.7)
rs = np.random.RandomState(21)
batch = {k: fr[k] for k in ('dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec', 'cnl_bbox_min_xyz',
                            'cnl_bbox_scale_xyz')}
batch.update(rays=fr['rays'][:, sel], near=fr['near'][sel], far=fr['far'][sel], bgcolor=np.array([30., 90., 200.], dtype=np.float32),
             patch_masks=pinfo['mask'], target_patches=rs.rand(NP, PS, PS, 3).astype(np.float32),
             t_rand=rs.rand(len(sel), S).astype(np.float32))
batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in batch.items()}
batch['patch_div_indices'] = torch.from_numpy(div)
cfg.N_samples, cfg.perturb, cfg.train.lossweights.lpips, cfg.amd.diagnostics = S, 1.0, 0.0, False
res = {}
for it in (500, 30000):
    net = Network(); net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state(default_shapes(), 0).items()}); net = net.to(dev)
    tr = Trainer(net)
    tr.iter = it
    keep = {}
    h = net.register_forward_hook(lambda m, a, out: keep.update(out))
    loss, _ = tr.backward_step(batch)
    h.remove()
    res['iter%d/loss' % it] = loss.cpu().numpy()
    for k in ('rgb', 'alpha', 'depth'):
        res['iter%d/out/%s' % (it, k)] = keep[k].detach().cpu().numpy()
    for k, p in net.named_parameters():
        if p.grad is not None:
            res['iter%d/grad/%s' % (it, k)] = p.grad.cpu().numpy()
    print('iter', it, 'rays', len(sel), 'loss %.9g' % float(loss), 'gradients', sum(p.grad is not None for p in net.parameters()))
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
np.savez(sys.argv[1], **res)
