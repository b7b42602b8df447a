"""Generate tests/golden/multihead_grad_h1.npz and multihead_grad_all.npz: the reference's gradients of a multi-head
canonical MLP (canonical_mlp.multihead.enable, head_depth 1, 3 heads) on seeded weights.

    python tests/make_golden_multihead_train.py <reference checkout>

Needs the reference checkout (imported read-only, on the CPU; only its numerical outputs are stored) and no GPU.
The case is that of grad_s64 (oracle/make_golden.py:203-226): the synthetic frame at ray_stride 73, S = 64, iter_val
30000, training mode, the loss sum(rgb w[:, :3]) + sum(alpha w[:, 3]) + 0.1 sum(depth w[:, 4]) with a seeded weight set
per head (tests/heads_train_cases.head_loss_weights); the weights are heads_train_cases.train_state of
seeded_state(default shapes, seed 0).
  * multihead_grad_h1.npz: the reference's loss.backward() of one pass with head_id = 1;
  * multihead_grad_all.npz: the .grad ACCUMULATED over the three passes head_id = 0, 1, 2, each with its own loss
    weights -- the gradient of the all-heads loss from the reference's own autograd (its own head_id = -1 branch of
    Network.forward raises as committed: it never fills 'offsets').
Stored per parameter as make_golden does -- ``norm/<name>``, then ``grad/<name>`` in full or ``head/<name>`` (the first
4096 elements) -- but tensors are stored in full only up to 32 768 elements (make_golden: 70 000): every tensor smaller
than the twelve 256 x 256 / 256 x 319 weights, which alone are 3 MB, so that each file stays below the project's limit of
1 MiB per committed file (grad_s64.npz, 2.2 MB, predates it).  Both files also carry ``loss`` and ``noise_floor`` / ``noise_floor_cos``: the largest relative norm distance
and the smallest cosine between these fp32 gradients and an fp64 evaluation of the same formulas (torch.autograd through
the oracle), as tests/test_grad_oracle.py::test_reference_gradient_noise_floor measures them for grad_s64 (4.4e-3 and
0.99999 there)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FULL_MAX = 32768


def oracle_head_gradients(state, meta, lw, heads, dtype):
    """Gradients of sum_{h in heads} loss_h by torch.autograd through the oracle in ``dtype``, one render per head on the
    state sliced to that head (shared leaves): name -> ndarray, [loss_h]."""
    import torch
    from tests import multihead_cases as mc
    from tests.test_grad_oracle import grad_frame, reference_loss
    from oracle import oracle
    fr = grad_frame(meta)
    leaves = {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    losses = []
    for h in heads:
        st = dict(leaves)
        st[mc.W_KEY], st[mc.B_KEY] = leaves[mc.W_KEY][4 * h:4 * h + 4], leaves[mc.B_KEY][4 * h:4 * h + 4]
        out = oracle.render(st, fr, iter_val=meta['iter_val'], N_samples=meta['N_samples'], dtype=dtype)
        loss = reference_loss(out, lw[h])
        loss.backward()
        losses.append(float(loss))
    return {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in leaves.items()}, losses


def main(ref):
    import torch
    sys.path.insert(0, REPO)
    from oracle import make_golden
    make_golden.REF = ref
    cfg, create_network = make_golden.import_reference()
    from humannerf_amd.seeded import default_shapes, seeded_state
    from tests import heads_train_cases as hc
    from tests.test_grad_oracle import compare_grads, grad_frame, reference_loss
    torch.set_num_threads(8)
    with open(os.path.join(HERE, 'golden', 'meta.json')) as f:
        meta = json.load(f)['grad_s64']
    state = hc.train_state(seeded_state(default_shapes(), seed=0))
    H = hc.TRAIN_HEADS
    cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions = meta['N_samples'], 0.0, False
    cfg.canonical_mlp.multihead.enable = True
    cfg.canonical_mlp.multihead.head_depth = 1
    cfg.multihead.head_num = H
    net = create_network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    net.train()
    fr = grad_frame(meta)
    assert fr['rays'].shape[1] == meta['n_rays']
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    tens = {k: torch.from_numpy(np.ascontiguousarray(fr[k])) for k in keys}
    lw = hc.head_loss_weights(meta['n_rays'])

    def passes(heads):
        for p in net.parameters():
            p.grad = None
        losses = []
        for h in heads:
            out = net(**tens, head_id=torch.tensor(h), iter_val=meta['iter_val'])
            loss = reference_loss(out, torch.from_numpy(lw[h]))
            loss.backward()                                   # (.grad accumulates over the passes)
            losses.append(float(loss))
        save = {'loss': np.float32(sum(losses)), 'losses': np.array(losses, np.float32), 'heads': np.array(heads)}
        for k, p in net.named_parameters():
            g = p.grad
            save['norm/' + k] = np.float32(0.0 if g is None else g.norm().item())
            if g is not None and g.numel() <= FULL_MAX:
                save['grad/' + k] = g.numpy().copy()
            elif g is not None:
                save['head/' + k] = g.reshape(-1)[:4096].numpy().copy()
        return save

    for name, heads in (('multihead_grad_h1', [1]), ('multihead_grad_all', list(range(H)))):
        save = passes(heads)
        path = os.path.join(HERE, 'golden', name + '.npz')
        np.savez_compressed(path, **save)
        exact, _ = oracle_head_gradients(state, meta, lw, heads, torch.float64)
        stats = compare_grads(exact, np.load(path), rel_norm=1.0, cos_min=0.0)
        save['noise_floor'] = np.float32(stats['worst_rel_norm_err'][0])
        save['noise_floor_cos'] = np.float64(stats['worst_cosine'][0])
        np.savez_compressed(path, **save)
        print(path, os.path.getsize(path), 'bytes; loss', save['loss'], 'fp32 reference vs fp64:', stats)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
