"""Writes tests/golden/lpips_seeded.npz: the reference's own LPIPS class evaluated on the seeded trunk.

    python tests/make_golden_lpips.py <path to a checkout of the reference>

A script, not a test.  The reference's third_parties/lpips imports torchvision only to get ``vgg16().features``; a
stand-in ``torchvision.models`` of this project's own (below) supplies that Sequential, filled by
``humannerf_amd.lpips.seeded_trunk(0)``.  The reference's class, its ScalingLayer, normalize_tensor, NetLinLayer and its
``weights/v0.1/vgg.pth`` do the rest, on the CPU in fp32.  Stored: the five head vectors, and per case
(N, H, W, seed) the inputs, the value and the gradient with respect to in0 of sum(value)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from humannerf_amd.lpips import CONV_IDX, POOL_BEFORE, seeded_trunk  # noqa: E402
from humannerf_amd.ops import LPIPS_CONVS  # noqa: E402

CASES = [(2, 32, 32, 0), (1, 37, 45, 0), (1, 16, 16, 0), (3, 17, 16, 2)]
TRUNK_SEED = 0


def case_inputs(N, H, W, seed):
    """in0 = RandomState(100 + seed).uniform(-1, 1), in1 = clamp(in0 + 0.1 normal): (N,3,H,W) fp32."""
    rs = np.random.RandomState(100 + seed)
    in0 = rs.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
    in1 = np.clip(in0 + 0.1 * rs.standard_normal((N, 3, H, W)), -1, 1).astype(np.float32)
    return in0, in1


def standin_torchvision():
    """``torchvision.models.vgg16(pretrained).features``: the 31-module Sequential with the seeded weights."""
    def vgg16(pretrained=True, **kw):
        mods, state = [], seeded_trunk(TRUNK_SEED)
        for l, (i, (ci, co)) in enumerate(zip(CONV_IDX, LPIPS_CONVS)):
            if l in POOL_BEFORE:
                mods.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
            assert len(mods) == i
            conv = torch.nn.Conv2d(ci, co, 3, padding=1)
            conv.weight.data.copy_(state['features.%d.weight' % i])
            conv.bias.data.copy_(state['features.%d.bias' % i])
            mods += [conv, torch.nn.ReLU(inplace=True)]
        mods.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
        assert len(mods) == 31
        return types.SimpleNamespace(features=torch.nn.Sequential(*mods))

    tv = types.ModuleType('torchvision')
    tv.models = types.ModuleType('torchvision.models')
    tv.models.vgg16 = vgg16
    sys.modules['torchvision'], sys.modules['torchvision.models'] = tv, tv.models


def main(reference):
    standin_torchvision()
    sys.path.insert(0, reference)
    from third_parties.lpips import LPIPS
    model = LPIPS(net='vgg', version='0.1', lpips=True, layers=[0, 1, 2, 3, 4], verbose=False)
    assert not model.training
    out = {'lin%d' % t: getattr(model, 'lin%d' % t).model[1].weight.detach().numpy().reshape(-1).copy() for t in range(5)}
    x = torch.from_numpy(case_inputs(1, 16, 16, 0)[0])
    assert float(model(x, x.clone()).abs().max()) == 0.0
    for N, H, W, seed in CASES:
        in0, in1 = case_inputs(N, H, W, seed)
        a = torch.from_numpy(in0).requires_grad_(True)
        val = model(a, torch.from_numpy(in1))
        assert val.shape == (N, 1, 1, 1)
        grad, = torch.autograd.grad(val.sum(), a)
        key = 'n%d_h%d_w%d_s%d' % (N, H, W, seed)
        out[key + '_in0'], out[key + '_in1'] = in0, in1
        out[key + '_value'] = val.detach().numpy().reshape(N).copy()
        out[key + '_grad'] = grad.numpy().copy()
        print(key, out[key + '_value'])
    path = os.path.join(ROOT, 'tests', 'golden', 'lpips_seeded.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
