"""What a long-lived ``Network`` keeps from frame to frame -- the packed canonical images (one, per head, all heads), the
decoded weight volume, the baked canonical grid, the frame's baked offset grid, a head id read back from the device, the
workspace and the guard's forced mode -- against the one thing that cannot be stale: a COLD network, a fresh
``Network()`` loaded from the live one's ``state_dict()`` that renders once under the same ``cfg``.

The one assertion, after any scripted history: the live frame equals the cold frame with ``torch.equal``, every output
key.  Around it every test asserts
  * determinism first: two cold networks agree bit for bit (the premise of ``torch.equal``; every configuration here
    is run-to-run identical, profiles/network_state_tests.txt);
  * the mutation mattered: rgb moved by more than 1e-4 max-abs (the threshold of
    test_gpu_train.py::test_render_after_training_steps_uses_the_new_weights), so that a missed invalidation cannot
    pass on a frame that would have been the same anyway;
  * nothing is rebuilt without cause: over the three frames that follow, ``bake_count`` and ``nonrigid_bake_count``
    stand still, ops.canonical_pack / canonical_heads_pack and the decoder's forward are not called.

The frame is the one of that regression test (64 rays) at 32 samples per ray, in three ray chunks of 31, 31 and 2;
grids of 16^3 (24^3 where the resolution changes).  Networks are built on the device from a state kept there."""
import contextlib
import socket

import numpy as np
import pytest
import torch

import multihead_cases as mc
from humannerf_amd import ops, scene
from humannerf_amd.config import cfg

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
S = 32
HEADS = 3
KEYS = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
        'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'cnl_bbox_max_xyz', 'bgcolor']
AMD_KEYS = ('mlp_mode', 'canonical', 'bake_resolution', 'nonrigid', 'nonrigid_bake_resolution', 'diagnostics', 'term_eps',
            'cull_eps', 'on_f16_range', 'f16_range_guard')
MOVED = 1e-4                                    # "the mutation mattered": max |d rgb| above this

CNL = 'cnl_mlp.module.output_linear.0.weight'
NR = 'non_rigid_mlp.module.block_mlps.12.weight'
VOL = 'mweight_vol_decoder.const_embedding'
MLP = dict(canonical='mlp', nonrigid='mlp')
GRID = dict(canonical='baked', bake_resolution=16, nonrigid='mlp')
BOTH = dict(canonical='baked', bake_resolution=16, nonrigid='baked', nonrigid_bake_resolution=16)
CONFIGS = {'mlp': MLP, 'grid': GRID, 'both': BOTH}
# weight-keyed cache -> (state, options that switch it on, the parameter whose change only it can carry, head)
CACHES = {
    'pack': ('single', MLP, CNL, None),
    'head_pack': ('heads', MLP, CNL, 1),
    'all_heads_pack': ('heads', MLP, CNL, -1),
    'volume': ('single', MLP, VOL, None),
    'grid': ('single', GRID, CNL, None),
    'offset_grid': ('single', BOTH, NR, None),
}


# ------------------------------------------------------------------------------------------------------------- fixtures
class _World:
    def __init__(self, seeded_params):
        fr = scene.synthetic_frame(H=512, W=512, focal_at_512=1250.0, ray_stride=61)
        self._batch = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(DEV) for k in KEYS}
        self.rays = self._batch['rays'].shape[1]
        self.chunk = self.rays // 2 - 1
        single = {k: torch.from_numpy(v).to(DEV) for k, v in seeded_params.items()}
        W, b = mc.head_tensors(HEADS)
        heads = dict(single)
        heads[mc.W_KEY], heads[mc.B_KEY] = torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)
        self.states = {'single': single, 'heads': heads}

    def batch(self):
        """The frame's inputs in fresh tensors (tests write into them)."""
        return {k: v.clone() for k, v in self._batch.items()}


@pytest.fixture(scope='module')
def world(seeded_params):
    w = _World(seeded_params)
    n, c = w.rays, w.chunk
    assert 2 * c < n < 3 * c and n % c                               # three chunks, the last one ragged
    return w


@pytest.fixture(scope='module')
def one_rank_group():
    """A process group of this process alone (gloo): its collectives are identities that do run."""
    import torch.distributed as dist
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


@contextlib.contextmanager
def settings(chunk, n_samples=S, **amd):
    """cfg of a test: S samples, no perturbation, ``chunk``, the lean outputs, ``amd``; everything back in finally."""
    keep_amd = {k: cfg.amd.get(k) for k in AMD_KEYS}
    keep = (cfg.N_samples, cfg.perturb, cfg.chunk)
    try:
        cfg.N_samples, cfg.perturb, cfg.chunk = n_samples, 0., chunk
        cfg.amd.diagnostics = False
        for k, v in amd.items():
            cfg.amd[k] = v
        yield
    finally:
        for k, v in keep_amd.items():
            cfg.amd[k] = v
        cfg.N_samples, cfg.perturb, cfg.chunk = keep


@contextlib.contextmanager
def _heads_cfg(n_heads):
    keep = (cfg.get('multihead'), cfg.canonical_mlp.get('multihead'))
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': n_heads, 'split': 'view'}
    try:
        yield
    finally:
        for node, key, val in ((cfg, 'multihead', keep[0]), (cfg.canonical_mlp, 'multihead', keep[1])):
            if val is None:
                node.pop(key)
            else:
                node[key] = val


def new_net(state, head=None):
    """A fresh Network() on the device with ``state`` loaded; ``head`` >= 0 is selected."""
    from humannerf_amd.network import Network
    n_heads = state[mc.W_KEY].shape[0] // 4
    with (_heads_cfg(n_heads) if n_heads > 1 else contextlib.nullcontext()), torch.device(DEV):
        net = Network()
    net.load_state_dict(state, strict=True)
    net.eval()
    if n_heads > 1 and head is not None and head >= 0:
        net.select_head(head)
    return net


def render(net, batch, head=None, iter_val=1e7, head_id=None):
    if head_id is None and head == -1:
        head_id = -1
    with torch.no_grad():
        return net(**batch, iter_val=iter_val, **({} if head_id is None else {'head_id': head_id}))


def cold_frame(live, batch, head=None, **kw):
    """The frame of a cold network: fresh, loaded from the live one's state_dict(), one render under the cfg of now."""
    net = new_net(live.state_dict(), head)
    out = render(net, batch, head, **kw)
    net.f16_guard.reset()
    return out


def cold_pair(live, batch, head=None, **kw):
    """Two cold frames, asserted equal (determinism first); returns one."""
    a, b = cold_frame(live, batch, head, **kw), cold_frame(live, batch, head, **kw)
    assert same(a, b), 'two cold networks differ by %.3e in rgb: not run-to-run identical' % moved(a, b)
    return a


def _pairs(a, b):
    assert set(a) == set(b)
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            yield k, x, y


def same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for _, x, y in _pairs(a, b))


def moved(a, b):
    """max |d rgb| between two frames (over the heads of an all-heads frame)."""
    return max(float((x - y).abs().max()) for k, x, y in _pairs(a, b) if k == 'rgb')


def counted_frame(net, batch, monkeypatch, head=None, **kw):
    """One frame of ``net`` and what it rebuilt: dict(pack, decode, bake, nr_bake)."""
    n = {'pack': 0, 'decode': 0}

    def counting(fn, key):
        def call(*a, **k):
            n[key] += 1
            return fn(*a, **k)
        return call

    bakes = net.bake_count, net.nonrigid_bake_count
    with monkeypatch.context() as m:
        m.setattr(ops, 'canonical_pack', counting(ops.canonical_pack, 'pack'))
        m.setattr(ops, 'canonical_heads_pack', counting(ops.canonical_heads_pack, 'pack'))
        m.setattr(net.mweight_vol_decoder, 'forward', counting(net.mweight_vol_decoder.forward, 'decode'))
        out = render(net, batch, head, **kw)
    n['bake'], n['nr_bake'] = net.bake_count - bakes[0], net.nonrigid_bake_count - bakes[1]
    return out, n


NOTHING = {'pack': 0, 'decode': 0, 'bake': 0, 'nr_bake': 0}


def steady(net, batch, want, monkeypatch, head=None, frames=3, **kw):
    """``frames`` more frames with nothing changed: each is ``want``, none rebuilds anything."""
    for i in range(frames):
        out, n = counted_frame(net, batch, monkeypatch, head, **kw)
        assert n == NOTHING, ('frame %d rebuilt without cause' % i, n)
        assert same(out, want), ('frame %d' % i, moved(out, want))


def twice(net, batch, want, monkeypatch, head=None, first=None, **kw):
    """An input / option route: two frames in a row, both ``want``; the first may rebuild exactly ``first`` (a dict of
    the non-zero counts; None = not looked at), the second nothing."""
    out, n = counted_frame(net, batch, monkeypatch, head, **kw)
    if first is not None:
        assert n == dict(NOTHING, **first), n
    assert same(out, want), moved(out, want)
    steady(net, batch, want, monkeypatch, head, frames=1, **kw)
    return out


# ------------------------------------------------------------------------------------------- weight-mutation routes
def _param(net, name):
    return net.get_parameter(name)


def _owner(net, name):
    mod, _, attr = name.rpartition('.')
    return net.get_submodule(mod), attr


def _train_pass(net, batch):
    """A train-path forward and backward (the gradients stay in .grad)."""
    net.train()
    try:
        with torch.enable_grad():
            net(**batch, iter_val=1e7)['rgb'].square().mean().backward()
    finally:
        net.eval()


def _drop_grads(net):
    for p in net.parameters():
        p.grad = None


class Route:
    """``run(net, name, batch, head)`` changes parameter ``name`` of ``net`` so that the frame moves; ``prepare`` runs in
    front of the frame of before."""
    group = False

    def prepare(self, net):
        pass


class InPlace(Route):                                    # (a)
    def run(self, net, name, batch, head=None):
        with torch.no_grad():
            _param(net, name).mul_(1.5)


class Adam(Route):                                       # (b)
    """One torch.optim.Adam step of half the parameter's mean magnitude per element, in the form asked for, behind a
    train-path forward and backward -- what an optimizer step follows in any training loop, and what tells the network
    that a step is coming.  A multi-head network has no train path (inference only): there the gradient is written by
    hand, and the 'fused' form, which updates through views no version counter sees, is followed by the documented
    weights_changed()."""

    def __init__(self, form):
        self.form = form

    def run(self, net, name, batch, head=None):
        p = _param(net, name)
        opt = torch.optim.Adam([p], lr=0.5 * float(p.detach().abs().mean()), foreach=self.form == 'foreach',
                               fused=self.form == 'fused')
        trained = not net.head_num
        if trained:
            _train_pass(net, batch)
            assert p.grad is not None and bool(p.grad.abs().max() > 0)
        else:
            p.grad = -p.detach().sign()
        opt.step()
        _drop_grads(net)
        if self.form == 'fused' and not trained:
            net.weights_changed()


class Load(Route):                                       # (c)
    def __init__(self, assign):
        self.assign = assign

    def run(self, net, name, batch, head=None):
        sd = dict(net.state_dict())
        sd[name] = sd[name] * 1.5
        net.load_state_dict(sd, strict=True, assign=self.assign)
        net.eval()


class DataAssign(Route):                                 # (d)
    def run(self, net, name, batch, head=None):
        p = _param(net, name)
        p.data = p.data * 1.5


class Replace(Route):                                    # (e)
    """The layer's nn.Parameter object replaced, the old one freed, again and again until a new one lies where the
    parameter of the last frame lay, with the version counter it had (0) -- or 16 times.  Passes either way; says which."""

    def run(self, net, name, batch, head=None):
        mod, attr = _owner(net, name)
        base = getattr(mod, attr).detach().clone()
        setattr(mod, attr, torch.nn.Parameter(base * 1.0))           # a fresh Parameter, counter 0: the keyed one
        render(net, batch, head)
        keyed = getattr(mod, attr).data_ptr()
        setattr(mod, attr, torch.nn.Parameter(base * 1.0))           # (frees the keyed block)
        for tries in range(1, 17):
            setattr(mod, attr, torch.nn.Parameter(base * 1.5))       # (the one before is freed here: nothing else holds it)
            if getattr(mod, attr).data_ptr() == keyed:
                break
        p = getattr(mod, attr)
        print('replace: address %s after %d replacements, _version %d'
              % ('REPEATS' if p.data_ptr() == keyed else 'differs', tries, p._version))


class HostEdit(Route):                                   # (f)
    def run(self, net, name, batch, head=None):
        net.cpu()
        _param(net, name).data.mul_(1.5)
        net.to(DEV)


class Broadcast(Route):                                  # (g)
    group = True

    def prepare(self, net):
        from humannerf_amd.dist import GradientSync
        self.sync = GradientSync(net, 1, single_rank_collectives=True)          # (broadcasts once itself)
        assert self.sync.active

    def run(self, net, name, batch, head=None):
        _param(net, name).data.mul_(1.5)
        self.sync.broadcast_state(net)


class DataEditThenCall(Route):                           # (h)
    def run(self, net, name, batch, head=None):
        _param(net, name).data.mul_(1.5)
        net.weights_changed()


ROUTES = {
    'inplace': InPlace(), 'adam_foreach': Adam('foreach'), 'adam_single': Adam('single'), 'adam_fused': Adam('fused'),
    'load': Load(False), 'load_assign': Load(True), 'data_assign': DataAssign(), 'replace': Replace(),
    'cpu_edit_back': HostEdit(), 'broadcast': Broadcast(), 'data_edit_weights_changed': DataEditThenCall(),
}


@pytest.mark.parametrize('cache', list(CACHES))
@pytest.mark.parametrize('route', list(ROUTES))
def test_weight_route(route, cache, world, monkeypatch, request):
    """Every way of changing a parameter against every weight-keyed entry: frame, change, frame -- and the second frame
    is the cold network's."""
    which, amd, name, head = CACHES[cache]
    r = ROUTES[route]
    if r.group:
        request.getfixturevalue('one_rank_group')
    batch = world.batch()
    with settings(world.chunk, **amd):
        live = new_net(world.states[which], head)
        r.prepare(live)
        before = render(live, batch, head)
        r.run(live, name, batch, head)
        after = render(live, batch, head)
        want = cold_pair(live, batch, head)
        change = moved(after, before)
        print('%s x %s: max |d rgb| of the change %.3e, live vs cold %.3e' % (route, cache, change, moved(after, want)))
        assert change > MOVED, change
        assert same(after, want), moved(after, want)
        steady(live, batch, want, monkeypatch, head)
        assert live.check_f16_range(wait=True) is False


# -------------------------------------------------------------------------------------------- input and option routes
def _new_priors(p):
    """Other priors on the same support: bone b scaled by a factor between 0.5 and 2."""
    return p * torch.linspace(0.5, 2.0, p.shape[0], device=p.device).reshape(-1, 1, 1, 1)


@pytest.mark.parametrize('variant', ['same', 'equal_new', 'new_values', 'in_place'])
def test_priors_route(variant, world, monkeypatch):
    """motion_weights_priors: the same object and equal values in a new object decode nothing, new values decode once,
    in a new object or written into the old one with copy_."""
    batch = world.batch()
    with settings(world.chunk, **MLP):
        live = new_net(world.states['single'])
        before = render(live, batch)
        p = batch['motion_weights_priors']
        if variant == 'equal_new':
            batch['motion_weights_priors'] = p.clone()
        elif variant == 'new_values':
            batch['motion_weights_priors'] = _new_priors(p)
        elif variant == 'in_place':
            p.copy_(_new_priors(p))
        changes = variant in ('new_values', 'in_place')
        want = cold_pair(live, batch)
        after = twice(live, batch, want, monkeypatch, first={'decode': 1} if changes else {})
        print('priors %s: max |d rgb| %.3e' % (variant, moved(after, before)))
        assert (moved(after, before) > MOVED) if changes else same(after, before)


def _new_box(batch):
    lo, hi = batch['cnl_bbox_min_xyz'] - 0.05, batch['cnl_bbox_max_xyz'] + 0.05
    return {'cnl_bbox_min_xyz': lo, 'cnl_bbox_max_xyz': hi, 'cnl_bbox_scale_xyz': 2.0 / (hi - lo)}


@pytest.mark.parametrize('variant', ['same', 'equal_new', 'new_values', 'in_place'])
def test_bbox_route(variant, world, monkeypatch):
    """The bbox tensors of the baked grid, the four cases of the priors: bakes 0, 0, 1, 1 (the offset grid lies over the
    canonical grid's box and follows it)."""
    batch = world.batch()
    with settings(world.chunk, **BOTH):
        live = new_net(world.states['single'])
        before = render(live, batch)
        assert (live.bake_count, live.nonrigid_bake_count) == (1, 1)
        box = ('cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz')
        if variant == 'equal_new':
            batch.update({k: batch[k].clone() for k in box})
        elif variant == 'new_values':
            batch.update(_new_box(batch))
        elif variant == 'in_place':
            for k, v in _new_box(batch).items():
                batch[k].copy_(v)
        changes = variant in ('new_values', 'in_place')
        want = cold_pair(live, batch)
        after = twice(live, batch, want, monkeypatch, first={'bake': 1, 'nr_bake': 1, 'pack': 0} if changes else {})
        print('bbox %s: max |d rgb| %.3e' % (variant, moved(after, before)))
        assert (moved(after, before) > MOVED) if changes else same(after, before)


@pytest.mark.parametrize('variant,bakes', [('same', 0), ('in_place', 1), ('fresh', 1)])
def test_posevec_route(variant, bakes, world, monkeypatch):
    """dst_posevec and the frame's offset grid: the same object holds, the object written in place and a fresh object
    (even of equal values: identity only, nothing is compared) bake once."""
    batch = world.batch()
    with settings(world.chunk, **BOTH):
        live = new_net(world.states['single'])
        before = render(live, batch)
        if variant == 'in_place':
            batch['dst_posevec'] += 0.3
        elif variant == 'fresh':
            batch['dst_posevec'] = batch['dst_posevec'].clone()
        want = cold_pair(live, batch)
        after = twice(live, batch, want, monkeypatch, first={'nr_bake': bakes})
        print('posevec %s: max |d rgb| %.3e' % (variant, moved(after, before)))
        assert (moved(after, before) > MOVED) if variant == 'in_place' else same(after, before)


@pytest.mark.parametrize('config', ['mlp', 'both'])
@pytest.mark.parametrize('where', ['below_kick_in', 'window_half_open'])
def test_iter_val_route(where, config, world, monkeypatch):
    """iter_val across non_rigid_motion_mlp.kick_in_iter (the condition code is zeroed, the window shut) and to a
    half-open Hann window: both are in the offset grid's key."""
    nr = cfg.non_rigid_motion_mlp
    it = float(nr.kick_in_iter - 1) if where == 'below_kick_in' else 0.5 * (nr.kick_in_iter + nr.full_band_iter)
    batch = world.batch()
    with settings(world.chunk, **CONFIGS[config]):
        live = new_net(world.states['single'])
        before = render(live, batch)
        want = cold_pair(live, batch, iter_val=it)
        after = twice(live, batch, want, monkeypatch, iter_val=it, first={'nr_bake': int(config == 'both')})
        print('iter_val %s (%s): max |d rgb| %.3e' % (where, config, moved(after, before)))
        assert moved(after, before) > MOVED
        back = twice(live, batch, before, monkeypatch, first={'nr_bake': int(config == 'both')})
        assert same(back, before)


@pytest.mark.parametrize('config', ['mlp', 'both'])
def test_mlp_mode_toggle(config, world, monkeypatch):
    """cfg.amd.mlp_mode f16x3 -> f32 -> f16x3: the mode is in every key (one pack, or one bake of each grid, per change)."""
    batch = world.batch()
    first = {'pack': 1} if config == 'mlp' else {'pack': 1, 'bake': 1, 'nr_bake': 1}
    with settings(world.chunk, mlp_mode='f16x3', **CONFIGS[config]):
        live = new_net(world.states['single'])
        before = render(live, batch)
        cfg.amd.mlp_mode = 'f32'
        exact = twice(live, batch, cold_frame(live, batch), monkeypatch, first=first)
        print('mlp_mode (%s): max |d rgb| f32 vs f16x3 %.3e' % (config, moved(exact, before)))
        cfg.amd.mlp_mode = 'f16x3'
        back = twice(live, batch, cold_pair(live, batch), monkeypatch, first=first)
        assert same(back, before)
        assert live.check_f16_range(wait=True) is False


def test_baked_options_toggle(world, monkeypatch):
    """cfg.amd.canonical / nonrigid baked -> mlp -> baked: the exact frame in between, and the grids are still there
    on return (nothing is baked again)."""
    batch = world.batch()
    with settings(world.chunk, **BOTH):
        live = new_net(world.states['single'])
        before = render(live, batch)
        cfg.amd.canonical, cfg.amd.nonrigid = 'mlp', 'mlp'
        exact = twice(live, batch, cold_frame(live, batch), monkeypatch, first={})
        print('baked -> mlp: max |d rgb| %.3e' % moved(exact, before))
        assert moved(exact, before) > MOVED                           # (a 16^3 grid is not the MLP)
        cfg.amd.canonical, cfg.amd.nonrigid = 'baked', 'baked'
        back = twice(live, batch, cold_pair(live, batch), monkeypatch, first={})
        assert same(back, before) and (live.bake_count, live.nonrigid_bake_count) == (1, 1)


def test_bake_resolution_change(world, monkeypatch):
    """bake_resolution 16 -> 24 -> 16: one bake each way (one grid is kept)."""
    batch = world.batch()
    with settings(world.chunk, **GRID):
        live = new_net(world.states['single'])
        before = render(live, batch)
        cfg.amd.bake_resolution = 24
        fine = twice(live, batch, cold_frame(live, batch), monkeypatch, first={'bake': 1})
        assert live._kept['baked'].grid.shape[0] == 24 and moved(fine, before) > MOVED
        cfg.amd.bake_resolution = 16
        back = twice(live, batch, cold_pair(live, batch), monkeypatch, first={'bake': 1})
        assert live._kept['baked'].grid.shape[0] == 16 and same(back, before)


def test_select_head_with_a_grid_cached(world, monkeypatch):
    """select_head between frames with a baked grid: the grid holds one head, the head is in its key."""
    batch = world.batch()
    with settings(world.chunk, **GRID):
        live = new_net(world.states['heads'], 0)
        before = render(live, batch)
        live.select_head(1)
        after = twice(live, batch, cold_pair(live, batch, 1), monkeypatch, first={'bake': 1, 'pack': 1})
        assert moved(after, before) > MOVED
        live.select_head(0)
        back = twice(live, batch, before, monkeypatch, first={'bake': 1})          # (head 0's image was kept)
        assert same(back, before)


def test_head_id_device_tensor_edited_in_place(world, monkeypatch):
    """head_id as a device tensor is read back once and remembered by identity and _version: written in place (through
    the tensor itself), it is read again."""
    batch = world.batch()
    with settings(world.chunk, **MLP):
        live = new_net(world.states['heads'])
        hid = torch.tensor(0, device=DEV)
        before = render(live, batch, head_id=hid)
        assert same(render(live, batch, head_id=hid), before) and live._kept['head_id'].inputs[0][0]() is hid
        hid.fill_(2)
        want = cold_pair(live, batch, head_id=2)
        after = twice(live, batch, want, monkeypatch, head_id=hid, first={'pack': 1})
        assert live._kept['head_id'].value == 2 and moved(after, before) > MOVED


def test_injected_grid_is_never_rebaked(world, monkeypatch):
    """set_baked_grid: the injected grid is used whatever happens to the weights; set_baked_grid(None) returns to
    baking, from the weights of then."""
    batch = world.batch()
    with settings(world.chunk, **GRID):
        live = new_net(world.states['single'])
        box = batch['cnl_bbox_min_xyz'], batch['cnl_bbox_max_xyz']
        grid = live.bake_canonical(*box, resolution=24).clone()
        live.set_baked_grid(grid, *box)
        assert live.bake_count == 1
        before = render(live, batch)
        with torch.no_grad():
            _param(live, CNL).mul_(1.5)
        live.weights_changed()
        cold = new_net(live.state_dict())
        cold.set_baked_grid(grid, *box)
        want = render(cold, batch)
        after = twice(live, batch, want, monkeypatch, first={'pack': 1, 'decode': 1})     # (everything but the grid)
        assert same(after, before) and live.bake_count == 1 and live._kept['baked'].injected
        live.set_baked_grid(None, None, None)
        baked = twice(live, batch, cold_pair(live, batch), monkeypatch, first={'bake': 1})
        assert moved(baked, before) > MOVED and live._kept['baked'].grid.shape[0] == 16


def test_samples_and_chunk_change_on_one_workspace(world, monkeypatch):
    """cfg.N_samples and cfg.chunk up (48 samples, one chunk: the workspace grows) and down (16 samples, chunks of 15:
    the grown workspace stays) between frames."""
    batch = world.batch()
    with settings(world.chunk, **MLP):
        live = new_net(world.states['single'])
        render(live, batch)
        small = live._workspace
        cfg.N_samples, cfg.chunk = 48, world.rays
        twice(live, batch, cold_frame(live, batch), monkeypatch, first={})
        grown = live._workspace
        assert grown is not small and grown.numel() > small.numel()
        cfg.N_samples, cfg.chunk = 16, world.chunk // 2
        twice(live, batch, cold_pair(live, batch), monkeypatch, first={})
        assert live._workspace is grown


def test_lean_and_diagnostics_alternate(world, monkeypatch):
    """The lean path (3 outputs) and the diagnostics path (11) alternating on one network."""
    batch = world.batch()
    with settings(world.chunk, **MLP):
        live = new_net(world.states['single'])
        lean = render(live, batch)
        cfg.amd.diagnostics = True
        full = cold_frame(live, batch)
        cfg.amd.diagnostics = False
        want = {False: cold_pair(live, batch), True: full}
        assert len(full) == 11 and len(lean) == 3 and same(lean, want[False])
        for diag in (True, False, True, False):
            cfg.amd.diagnostics = diag
            twice(live, batch, want[diag], monkeypatch, first={})


def test_early_termination_interleaved_with_the_frame_path(world, monkeypatch):
    """cfg.amd.term_eps > 0 takes the chunked path (one workspace for every chunk), 0 the frame path: interleaved."""
    batch = world.batch()
    with settings(world.chunk, **MLP):
        live = new_net(world.states['single'])
        render(live, batch)
        cfg.amd.term_eps = 1e-3
        term = cold_frame(live, batch)
        cfg.amd.term_eps = 0.0
        want = {0.0: cold_pair(live, batch), 1e-3: term}
        for eps in (1e-3, 0.0, 1e-3, 0.0):
            cfg.amd.term_eps = eps
            twice(live, batch, want[eps], monkeypatch, first={})
        assert live.check_f16_range(wait=True) is False


def test_range_guard_hit_forces_f32_until_reset(world, monkeypatch):
    """A hit with on_f16_range = 'f32': the forced mode packs again and the frames are those of an 'f32' network; after
    f16_guard.reset() the f16x3 frame is the cold one again.  The hit is planted: feature 9 of hidden layer 1 is 1e5 at
    every sample, its outgoing column zero (only the guard sees it)."""
    st = dict(world.states['single'])
    for key, edit in (('cnl_mlp.module.pts_linears.2.weight', lambda t: t[9].zero_()),
                      ('cnl_mlp.module.pts_linears.2.bias', lambda t: t[9].fill_(1e5)),
                      ('cnl_mlp.module.pts_linears.4.weight', lambda t: t[:, 9].zero_())):
        st[key] = st[key].clone()
        edit(st[key])
    batch = world.batch()
    with settings(world.chunk, mlp_mode='f16x3', on_f16_range='f32', **MLP):
        live = new_net(st)
        first = render(live, batch)
        with pytest.warns(UserWarning, match="switching this network to 'f32'"):
            assert live.check_f16_range(wait=True) is True
        assert live._mlp_mode() == 'f32' and live.f16_range_hits == 1
        cfg.amd.mlp_mode = 'f32'
        exact = cold_frame(live, batch)
        cfg.amd.mlp_mode = 'f16x3'
        twice(live, batch, exact, monkeypatch, first={'pack': 1})
        live.f16_guard.reset()
        assert live._mlp_mode() == 'f16x3'
        back, n = counted_frame(live, batch, monkeypatch)
        live.f16_guard.reset()                                       # (the frame's own hit: not acted on)
        assert n == dict(NOTHING, pack=1)
        assert same(back, cold_pair(live, batch)) and same(back, first)


def test_train_pass_without_a_step(world, monkeypatch):
    """net.train(), a train-path forward and backward, no optimizer step, net.eval(): the frame is the cold one (and the
    one of before: nothing changed, although everything derived from the weights was rebuilt once)."""
    batch = world.batch()
    with settings(world.chunk, **MLP):
        live = new_net(world.states['single'])
        before = render(live, batch)
        _train_pass(live, batch)
        _drop_grads(live)
        want = cold_pair(live, batch)
        out, n = counted_frame(live, batch, monkeypatch)
        assert n == dict(NOTHING, pack=1, decode=1), n
        assert same(out, want) and same(out, before)
        steady(live, batch, want, monkeypatch)
