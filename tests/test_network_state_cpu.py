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
    from humannerf_amd.kept import Kept
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
    assert ('pack', None) not in net._kept and 'vol' not in net._kept
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    old_w, old_e = head.weight, dec.const_embedding
    head.weight, dec.const_embedding = _alias(old_w), _alias(old_e)  # replaced Parameters at the old (data_ptr, _version)
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    del old_w, old_e
    gc.collect()
    assert rebuilt() == (0, 0)
    # load_state_dict and Module._apply (every move and cast) drop the entries themselves, at once
    net.load_state_dict(net.state_dict())
    assert ('pack', None) not in net._kept and 'vol' not in net._kept
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    net.load_state_dict(net.state_dict(), assign=True)
    assert ('pack', None) not in net._kept and 'vol' not in net._kept
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    net.float()
    assert ('pack', None) not in net._kept and 'vol' not in net._kept
    assert rebuilt() == (1, 1) and rebuilt() == (0, 0)
    # an injected grid outlives weights_changed, a baked one does not
    net._kept['baked'], net._kept['baked_nr'] = Kept(), Kept()
    net.weights_changed()
    assert 'baked' not in net._kept and 'baked_nr' not in net._kept
    injected = net._kept['baked'] = Kept(injected=True)
    net.weights_changed()
    assert net._kept['baked'] is injected
    net.set_baked_grid(None, None, None)
    assert 'baked' not in net._kept
    # the guard's audit schedule restarts with the weights
    net.f16_guard._schedule = ['k', 3]
    net.weights_changed()
    assert net.f16_guard._schedule is None


def test_kept_entry_alone():
    """kept.Kept without a Network: the weights test fails on another key, another generation and each of the three ways
    _still_resident fails; the input ladder hits by identity without a comparison, compares fresh tensors once and then
    hits by identity, and without the callable never matches fresh tensors."""
    from humannerf_amd.kept import Kept
    p, q = torch.nn.Parameter(torch.arange(6.)), torch.nn.Parameter(torch.ones(3))
    key = ('f16x3', 1)
    e = Kept(key, 4, [p, q])
    assert e.built_from(key, 4, [p, q])
    assert not e.built_from(('f16x3', 2), 4, [p, q])                 # another key
    assert not e.built_from(key, 5, [p, q])                          # another weights generation
    assert not e.built_from(key, 4, [p, _alias(q)])                  # another object at an equal (data_ptr, _version)
    with torch.no_grad():
        q.add_(0)
    assert not e.built_from(key, 4, [p, q])                          # a later _version
    e = Kept(key, 4, [p, q])
    assert e.built_from(key, 4, [p, q])
    p.data = p.data.clone()
    assert not e.built_from(key, 4, [p, q])                          # another data_ptr
    assert not Kept(key, 4).built_from(key, 4, [])                   # built from no weights (injected): never
    with pytest.raises(TypeError):
        Kept(key, 4, image=torch.zeros(4))                           # (payload has its names)

    def never():
        raise AssertionError('compared by value')

    asked = []
    a, b = torch.arange(3.), torch.ones(3)
    e = Kept(inputs=(a, b), value=7)
    assert e.value == 7 and e.packed is None and not e.injected
    assert e.fed_by((a, b), never)                                   # identity: the callable is not asked
    a2, b2 = a.clone(), b.clone()
    assert not e.fed_by((a2, b2), lambda: asked.append(0) or False) and e.fed_by((a, b), never)     # (unequal: kept as it was)
    assert e.fed_by((a2, b2), lambda: asked.append(1) or True) and asked == [0, 1]                  # asked once ...
    assert e.fed_by((a2, b2), never) and not e.fed_by((a, b))        # ... then these objects hit, the old ones do not
    assert not e.fed_by((a2.clone(), b2.clone())) and not e.fed_by((a2.clone(), b2.clone()))        # no callable: never
    assert e.fed_by((a2, b2), never)
    a2.add_(0)
    assert not e.fed_by((a2, b2))                                    # written in place
    e = Kept()
    assert not e.fed_by((a, b))                                      # nothing remembered
    e.remember((a, b))
    assert e.fed_by((a, b), never)


from test_multihead_cpu import net3                                  # noqa: E402,F401  (the 3-head Network on the CPU)

PRIORS = torch.ones(25, 2, 2, 2)


def _stubbed(net, monkeypatch):
    """The packers and the decoder of ``net`` replaced by counters: (the ``out=`` of every pack, an item per decode)."""
    from humannerf_amd import ops
    packs, decodes = [], []
    monkeypatch.setattr(ops, 'canonical_pack', lambda ws, bs, mode='f32', out=None: packs.append(out) or torch.zeros(4))
    monkeypatch.setattr(ops, 'canonical_heads_pack',
                        lambda ws, bs, n_heads, mode='f32', out=None: packs.append(out) or torch.zeros(4))
    monkeypatch.setattr(net.mweight_vol_decoder, 'forward',
                        lambda motion_weights_priors, **_: decodes.append(1) or torch.zeros(1, 25, 2, 2, 2))
    return packs, decodes


def _fill(net):
    """An entry of every kind ``net`` can hold, none injected: the packed images (every head and the all-heads image of
    a multi-head network) and the weight volume through their sites; the two grids, a head id, another image and one
    of no kind at all planted.  Returns the heads packed."""
    from humannerf_amd.kept import Kept
    heads = list(range(-1, net.head_num)) if net.head_num else [None]
    net.eval()
    with torch.no_grad():
        for h in heads:
            net._head = h
            net._canonical_packed()
        net._head = None
        net._weight_volume(PRIORS)
    gen = net._weights_gen
    net._kept['baked'] = Kept(('f16x3', 16, None), gen, net._cnl_tensors(), grid=torch.zeros(2, 2, 2, 4))
    net._kept['baked_nr'] = Kept(('f16x3', 16), gen, net._nr_tensors(), grid=torch.zeros(2, 2, 2, 4), nr_packed=torch.zeros(4))
    net._kept['head_id'] = Kept(inputs=(PRIORS,), value=1)
    net._kept['another image'] = Kept(('f16x3', 9), gen, net._cnl_tensors(), packed=torch.zeros(4), serial=0)
    net._kept['a seventh'] = Kept()
    return heads


@pytest.mark.parametrize('which', ['net', 'net3'])
def test_no_entry_can_be_forgotten(which, request, monkeypatch):
    """weights_changed() leaves nothing that is not injected, check_f16_range() after a hit no packed canonical image
    and everything else -- whatever the entries are called: the network's own collection is what is looked through."""
    from humannerf_amd.kept import Kept
    net = request.getfixturevalue(which)
    _stubbed(net, monkeypatch)
    net.weights_changed()
    heads = _fill(net)
    assert {('pack', h) for h in heads} | {'vol'} <= set(net._kept) and len(net._kept) == len(heads) + 6
    injected = net._kept['baked'] = Kept(injected=True, grid=torch.zeros(2, 2, 2, 4))
    assert net.weights_changed() is net
    assert all(e.injected for e in net._kept.values()) and list(net._kept.items()) == [('baked', injected)]
    net.set_baked_grid(None, None, None)
    # the canonical-image drop after a hit of the f16-range guard
    _fill(net)
    others = {n: e for n, e in net._kept.items() if e.packed is None}
    assert set(others) == {'vol', 'baked', 'baked_nr', 'head_id', 'a seventh'} and len(net._kept) == len(heads) + 6
    monkeypatch.setattr(net.f16_guard, 'check', lambda wait=True, upto=None: (True, False))
    monkeypatch.setattr(net.f16_guard, 'act', lambda *hit: any(hit))
    monkeypatch.setattr(net.f16_guard, 'plan', lambda mode, n_chunks, weights_key: weights_key)
    assert net._guard_plan('f16x3', 1) == net._kept[('pack', heads[-1])].serial == net._pack_serial   # (the image used last)
    assert net.check_f16_range() is True
    assert all(e.packed is None for e in net._kept.values())        # selected head, other heads, all heads: gone
    assert net._kept == others and net._kept['baked_nr'].nr_packed is not None and net._kept['vol'].vol is not None
    assert net._guard_plan('f16x3', 1) is None                      # (the image used last is gone: no serial)
    net.weights_changed()
    assert net._kept == {}


@pytest.mark.parametrize('which', ['net', 'net3'])
def test_a_generation_step_alone_outdates_every_weight_keyed_entry(which, request, monkeypatch):
    """``_weights_gen += 1``, what a train-path _forward does, and nothing else: every entry built from weights misses
    its weights test, the packed images are packed again into their own buffers, the volume is decoded again."""
    net = request.getfixturevalue(which)
    packs, decodes = _stubbed(net, monkeypatch)
    net.weights_changed()
    heads = _fill(net)
    images = [net._kept[('pack', h)].packed for h in heads]
    assert (len(packs), len(decodes)) == (len(heads), 1) and all(out is None for out in packs)
    _fill(net)
    assert (len(packs), len(decodes)) == (len(heads), 1)             # unchanged: every site hits
    keyed = {n: e for n, e in net._kept.items() if e.weights is not None}
    assert set(keyed) == {('pack', h) for h in heads} | {'vol', 'baked', 'baked_nr', 'another image'}
    params = {n: [ref() for ref, _, _ in e.weights] for n, e in keyed.items()}
    assert all(e.built_from(e.key, net._weights_gen, params[n]) for n, e in keyed.items())
    net._weights_gen += 1
    assert not any(e.built_from(e.key, net._weights_gen, params[n]) for n, e in keyed.items())
    _fill(net)
    assert len(decodes) == 2 and len(packs) == 2 * len(heads)
    assert all(out is image for out, image in zip(packs[len(heads):], images))     # (each image's buffer is used again)
    assert all(net._kept[('pack', h)].gen == net._weights_gen for h in heads) and net._kept['vol'].gen == net._weights_gen
    _fill(net)
    assert (len(packs), len(decodes)) == (2 * len(heads), 2)
    net.weights_changed()


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
