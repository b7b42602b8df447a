"""Host-side state rules of humannerf_amd.network that need no GPU: the resident-tensor rule of the per-frame caches and
of the weight-keyed ones (identity, data_ptr, _version; weights_changed and what calls it), the policy step of the
inference f16-range guard, and the table of output keys and shapes."""
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


def _alias(p):
    """A new Parameter on ``p``'s memory with ``p``'s version counter value: what a replaced parameter looks like when the
    allocator hands the freed block out again (the ABA case), forced."""
    q = torch.nn.Parameter(p.data)                                   # (the storage used again; a counter of its own, at 0)
    with torch.no_grad():
        while q._version < p._version:
            q.add_(0)
    assert q is not p and (q.data_ptr(), q._version) == (p.data_ptr(), p._version)
    return q


def test_weight_key_rule():
    """The rule of the weight-keyed entries is the resident-tensor rule on parameters: identity, data_ptr, _version."""
    from humannerf_amd.network import _resident, _still_resident
    p, q = torch.nn.Parameter(torch.arange(6.).reshape(2, 3)), torch.nn.Parameter(torch.ones(3))
    refs = _resident([p, q])
    assert _still_resident(refs, [p, q])                             # unchanged: hit
    assert _still_resident(refs, [p, q])
    with torch.no_grad():
        q.copy_(torch.zeros(3))
    assert not _still_resident(refs, [p, q])                         # copy_: miss
    refs = _resident([p, q])
    p.data = torch.zeros(2, 3)                                       # same object, same counter, other memory
    assert p._version == refs[0][2] and not _still_resident(refs, [p, q])
    refs = _resident([p, q])
    assert _still_resident(refs, [p, q])
    p.data.mul_(2.0)                                                 # through .data: NOT seen (Network.weights_changed)
    assert _still_resident(refs, [p, q])
    twin = _alias(q)                                                 # another object at an equal (data_ptr, _version)
    assert not _still_resident(refs, [p, twin])
    assert _still_resident(refs, [p, q])
    del q
    gc.collect()
    assert refs[1][0]() is None                                      # collected: nothing can be that parameter again
    assert not _still_resident(refs, [p, twin])
    assert not _still_resident(refs, [p, _alias(twin)])


def test_weight_keyed_entries_follow_the_rule(net, monkeypatch):
    """Network's packed canonical image and weight volume on the host, with the pack and the decoder counted: which
    histories rebuild (in-place writes, ``.data =``, a replaced Parameter on the same memory, weights_changed,
    load_state_dict, a move or cast of the module) and which do not (nothing, and a write through ``.data`` without
    weights_changed -- the documented blind spot)."""
    from humannerf_amd import ops
    packs, decodes = [], []
    monkeypatch.setattr(ops, 'canonical_pack', lambda ws, bs, mode='f32', out=None: packs.append(out) or torch.zeros(4))
    dec = net.mweight_vol_decoder
    monkeypatch.setattr(dec, 'forward', lambda motion_weights_priors, **_: decodes.append(1) or torch.zeros(1, 25, 2, 2, 2))
    head = net.cnl_mlp.module.output_linear[0]
    priors = torch.ones(25, 2, 2, 2)
    net.eval()

    def rebuilt():
        n = len(packs), len(decodes)
        with torch.no_grad():
            net._canonical_packed()
            net._weight_volume(priors)
        return len(packs) - n[0], len(decodes) - n[1]

    net.weights_changed()
    assert rebuilt() == (1, 1)
    assert rebuilt() == (0, 0) and rebuilt() == (0, 0)               # unchanged: hit
    with torch.no_grad():
        head.weight.copy_(head.weight * 1.5)
        dec.const_embedding.mul_(1.5)
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    assert packs[-1] is not None                                     # (the image's buffer is used again)
    head.bias.data = head.bias.data.clone()
    dec.const_embedding.data = dec.const_embedding.data.clone()
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    head.weight.data.mul_(1.5)                                       # unseen ...
    assert rebuilt() == (0, 0)
    assert net.weights_changed() is net                              # ... until the documented call
    assert net._cnl_pack is None and net._vol_cache is None
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    old_w, old_e = head.weight, dec.const_embedding
    head.weight, dec.const_embedding = _alias(old_w), _alias(old_e)  # replaced Parameters at the old (data_ptr, _version)
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    del old_w, old_e
    gc.collect()
    assert rebuilt() == (0, 0)
    # load_state_dict and Module._apply (every move and cast) drop the entries themselves, at once
    net.load_state_dict(net.state_dict())
    assert net._cnl_pack is None and net._vol_cache is None
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    net.load_state_dict(net.state_dict(), assign=True)
    assert net._cnl_pack is None and net._vol_cache is None
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    net.float()
    assert net._cnl_pack is None and net._vol_cache is None
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    # an injected grid outlives weights_changed, a baked one does not
    net._baked = {'injected': False}
    net._baked_nr = {}
    net.weights_changed()
    assert net._baked is None and net._baked_nr is None
    net._baked = {'injected': True}
    net.weights_changed()
    assert net._baked == {'injected': True}
    net._baked = None
    # the guard's audit schedule restarts with the weights
    net.f16_guard._schedule = ['k', 3]
    net.weights_changed()
    assert net.f16_guard._schedule is None


def test_broadcasts_tell_the_network(tmp_path):
    """dist.GradientSync's broadcasts write through ``.data``: the module is told after broadcast_state (the constructor
    runs one) and after the periodic resync of the decoder, not after an ordinary step; a module without weights_changed
    is left alone.  Over a process group of this process alone (gloo)."""
    import torch.distributed as dist
    from humannerf_amd import dist as hd

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mweight_vol_decoder, self.mlp, self.calls = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), 0

        def weights_changed(self):
            self.calls += 1

    toy = Toy()
    assert not hd.GradientSync(toy, 1).active and toy.calls == 0     # one rank without collectives: nothing is written
    dist.init_process_group('gloo', init_method='file://' + str(tmp_path / 'store'), rank=0, world_size=1)
    try:
        sync = hd.GradientSync(toy, 1, mode='volume', resync_every=2, single_rank_collectives=True)
        assert sync.active and toy.calls == 1
        sync.broadcast_state(toy)
        assert toy.calls == 2
        for p in toy.parameters():
            p.grad = torch.ones_like(p)
        sync.reduce()
        assert toy.calls == 2                                        # step 1: no resync
        sync.reduce()
        assert toy.calls == 3                                        # step 2: the decoder was broadcast again
        sync.finish()
        hd.GradientSync(torch.nn.Linear(2, 2), 1, single_rank_collectives=True)
    finally:
        dist.destroy_process_group()


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
