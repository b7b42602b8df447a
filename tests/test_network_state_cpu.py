"""Host-side state rules of humannerf_amd.network that need no GPU: the resident-tensor rule of the per-frame caches,
the policy step of the inference f16-range guard, and the table of output keys and shapes."""
import gc
import warnings

import pytest
import torch


def test_resident_tensor_rule():
    """_resident / _still_resident: the same tensor objects, unwritten, hold; a version bump, an equal tensor in
    another object and a collected tensor do not."""
    from humannerf_amd.network import _resident, _still_resident
    a, b = torch.arange(3.), torch.ones(3)
    refs = _resident((a, b))
    assert _still_resident(refs, (a, b))
    assert not _still_resident(refs, (b, a))
    assert not _still_resident(refs, (a, b.clone()))                 # equal by value, another object
    assert not _still_resident(None, (a, b))
    b.add_(0)                                                        # the same values, a later _version
    assert not _still_resident(refs, (a, b))
    refs = _resident((a, b))
    assert _still_resident(refs, (a, b))
    del b
    gc.collect()
    assert refs[1][0]() is None                                      # collected: nothing can be that tensor again
    assert not _still_resident(refs, (a, torch.ones(3)))


@pytest.fixture(scope='module')
def net():
    from humannerf_amd.network import Network
    return Network()                                                 # (a second of initialisation: once for the module)


@pytest.mark.parametrize('flags,names', [((True, False), 'canonical MLP'), ((False, True), 'non-rigid MLP'),
                                         ((True, True), 'canonical and the non-rigid MLP')])
def test_guard_policy_step_without_a_device(net, flags, names):
    """InferenceRangeGuard.act is cfg.amd.on_f16_range applied to a verdict: 'raise' names exactly the MLPs that hit,
    'f32' warns and forces the mode until reset(), 'ignore' only reports; no flag is no hit."""
    from humannerf_amd.config import cfg
    from humannerf_amd.network import ActivationRangeError
    from humannerf_amd.range_guard import InferenceRangeGuard
    guard = net.f16_guard = InferenceRangeGuard()
    old = cfg.amd.get('on_f16_range', 'raise'), cfg.amd.get('mlp_mode', 'f16x3')
    try:
        cfg.amd.mlp_mode = 'f16x3'
        assert guard.act(False, False) is False and net.f16_range_hits == 0
        cfg.amd.on_f16_range = 'raise'
        with pytest.raises(ActivationRangeError) as err:
            guard.act(*flags)
        assert ('of the %s left the range' % names) in str(err.value)
        assert net.f16_range_hits == 1 and net._mlp_mode() == 'f16x3'
        cfg.amd.on_f16_range = 'ignore'
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            assert guard.act(*flags) is True
        assert net.f16_range_hits == 2 and net._mlp_mode() == 'f16x3'
        cfg.amd.on_f16_range = 'f32'
        with pytest.warns(UserWarning, match="switching this network to 'f32'"):
            assert guard.act(*flags) is True
        assert net.f16_range_hits == 3 and net._mlp_mode() == 'f32'
        guard.reset()
        assert net._mlp_mode() == cfg.amd.mlp_mode == 'f16x3'
        assert net.check_f16_range(wait=True) is False and net.f16_range_hits == 3      # nothing watched: no hit
    finally:
        cfg.amd.on_f16_range, cfg.amd.mlp_mode = old


@pytest.mark.parametrize('S,B', [(2, 24), (64, 3)])
def test_output_table(S, B):
    """ops.output_shapes: the 3 lean / 11 diagnostic keys in RenderRays.OUTPUT_KEYS order with the per-ray shapes of
    the reference's return dict (the ones test_gpu_parity asserts for a frame without rays)."""
    from humannerf_amd import ops
    from humannerf_amd.autograd import RenderRays
    assert RenderRays.OUTPUT_KEYS == (
        'rgb', 'alpha', 'depth', 'weights_on_rays', 'rgb_on_rays', 'cnl_xyz', 'cnl_rgb', 'cnl_weight', 'xyz_on_rays',
        'backward_motion_weights', 'offsets')
    lean, full = ops.output_shapes(S, B, False), ops.output_shapes(S, B, True)
    assert tuple(lean) == RenderRays.OUTPUT_KEYS[:3] and tuple(full) == RenderRays.OUTPUT_KEYS
    assert full == {'rgb': (3,), 'alpha': (), 'depth': (), 'weights_on_rays': (S,), 'rgb_on_rays': (S, 3), 'cnl_xyz': (3,),
                    'cnl_rgb': (3,), 'cnl_weight': (), 'xyz_on_rays': (S, 3), 'backward_motion_weights': (S, B),
                    'offsets': (S, 3)}
    assert lean == {k: full[k] for k in lean}
