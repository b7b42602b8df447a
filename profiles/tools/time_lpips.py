"""LPIPS-VGG16 (humannerf_amd/lpips.py, hnrf_lpips.hip) against the eager PyTorch-ROCm evaluation of the same arithmetic
(tests/test_lpips_refs.py reference_lpips in fp32: F.conv2d through MIOpen) on the same inputs, in the same run, on the
same GPU: HIP events, profiler off, 3 warm-ups, median of 20.  Seeded trunk (LpipsVGG.seeded): times do not depend on the
weights' values; nothing here says anything about picture quality.  One JSON line per step:

  train   forward + backward of 6 + 6 patches of 32 x 32 (the reference's training shape), both routes;
  metric  forward of one 512 x 512 pair, both routes, and the HIP time over the 2.0 ms that the trunk's 320 GFLOP take
          at the 157 TFLOP/s fp32-MFMA peak;
  step    Trainer.backward_step + optimizer_step on a frame of the synthetic subject, 6 patches of 32 x 32 x 128 samples,
          with lpips_fn and without (bench.py's own `train` leg is the run without: it stays MSE-only).

    python profiles/tools/time_lpips.py --step train|metric|step
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humannerf_amd.lpips import LpipsVGG, seeded_heads, seeded_trunk  # noqa: E402
from tests.test_lpips_refs import reference_lpips  # noqa: E402

WARMUP, REPS = 3, 20


def event_ms(fn):
    for _ in range(WARMUP):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {'median_ms': round(ms[len(ms) // 2], 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4)}


def inputs(N, H, W, dev):
    rs = np.random.RandomState(5)
    in0 = rs.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
    in1 = np.clip(in0 + 0.1 * rs.standard_normal(in0.shape), -1, 1).astype(np.float32)
    # NHWC memory seen as (N,3,H,W), as train.image_loss passes it
    return (torch.from_numpy(a).to(dev).permute(0, 3, 1, 2) for a in (in0, in1))


def eager_setup(dev):
    trunk = {k: v.to(dev) for k, v in seeded_trunk(0).items()}
    lins = [v.reshape(-1).to(dev) for v in seeded_heads(0).values()]
    return lambda a, b: reference_lpips(trunk, lins, a, b, torch.float32)


def step_train(dev):
    lp, eager = LpipsVGG.seeded(0), eager_setup(dev)
    in0, in1 = inputs(6, 32, 32, dev)

    def run(fn):
        a = in0.detach().requires_grad_(True)
        fn(a, in1).mean().backward()
        return a.grad
    res = {'step': 'train', 'shape': '6+6 x 32x32, forward + backward', 'hip': event_ms(lambda: run(lp)),
           'eager': event_ms(lambda: run(eager))}
    g0, g1 = run(lp), run(eager)
    res['grad_rel_diff'] = float((g0 - g1).norm() / g1.norm())
    res['eager_over_hip'] = round(res['eager']['median_ms'] / res['hip']['median_ms'], 3)
    return res


def step_metric(dev):
    lp, eager = LpipsVGG.seeded(0), eager_setup(dev)
    in0, in1 = inputs(1, 512, 512, dev)
    res = {'step': 'metric', 'shape': '1 x 512x512, forward'}
    with torch.no_grad():
        res['hip'] = event_ms(lambda: lp(in0, in1))
        try:
            res['eager'] = event_ms(lambda: eager(in0, in1))
            res['value_rel_diff'] = float(((lp(in0, in1) - eager(in0, in1)).abs() / eager(in0, in1).abs()).max())
            res['hip_over_eager'] = round(res['hip']['median_ms'] / res['eager']['median_ms'], 3)
        except RuntimeError as e:                      # MIOpen cannot run a shape
            res['eager'] = 'failed: %s' % str(e)[:200]
    res['hip_over_fp32_mfma_peak_2.0ms'] = round(res['hip']['median_ms'] / 2.0, 2)
    return res


def step_step(dev):
    from humannerf_amd import dataset
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state
    from humannerf_amd.train import Trainer
    import warnings
    subj = dataset.Subject(os.path.join('tests', 'golden', 'subject_synth'))
    stream = dataset.FrameStream(subj, rank=0, world=1, seed=0, device=dev)
    try:
        batch = next(iter(stream))
    finally:
        stream.close()
    res = {'step': 'step', 'shape': '%d patches of %d, %d samples per ray, %d rays' % (
        cfg.patch.N_patches, cfg.patch.size, cfg.N_samples, batch['rays'].shape[1])}
    state = seeded_state(default_shapes(), seed=0)
    for name, fn in (('mse_only', None), ('lpips_and_mse', LpipsVGG.seeded(0))):
        net = Network()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            tr = Trainer(net.to(dev), lpips_fn=fn)
        res[name] = dict(event_ms(lambda: tr.train_step(batch)), objective=tr.objective)
    res['added_ms'] = round(res['lpips_and_mse']['median_ms'] - res['mse_only']['median_ms'], 4)
    return res


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', required=True, choices=['train', 'metric', 'step'])
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'train': step_train, 'metric': step_metric, 'step': step_step}[args.step](dev)
    out['gpu'] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
