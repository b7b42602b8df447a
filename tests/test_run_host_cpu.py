"""The host code that the render loops and the frame entries share, without a GPU: run._sequence (which frames, names
and folder every run_* loop asks for -- the tables below are written out from the loops as they stood before the helper
existed, their drifts included), run._cfg_override, the one statement of the frame workspace size in hnrf_abi.hip, and
the binder of the additive headers in _lib."""
import ctypes

import pytest
import torch

from humannerf_amd import _lib, render, run
from humannerf_amd.config import cfg

DEV = torch.device('cpu')
SIZE = (40, 30)                     # what the stub's image_size() answers
NAMES = ['a-0', 'a-1']              # the first two frame names, '/' replaced


class Stop(Exception):
    """Raised by the first collaborator a loop builds behind its sequence: the test needs no more of the loop."""


class StubSubject:
    framelist = framelist_all = ['a/0', 'a/1', 'a/2']
    dataset_path = 'stub'
    canonical_bbox = {'min_xyz': None, 'max_xyz': None}
    motion_weights_priors = None

    def __init__(self):
        self.calls = []

    def __len__(self):
        return 3

    def image_size(self, name):
        return SIZE

    def movement_frame(self, *a, **kw):
        self.calls.append(('movement', a, kw))
        return {}

    def freeview_frame(self, *a, **kw):
        self.calls.append(('freeview', a, kw))
        return {}

    def tpose_frame(self, *a, **kw):
        self.calls.append(('tpose', a, kw))
        return {}


class StubNetwork:
    head_num = 2
    MESH_LEVEL = 0.

    def extract_canonical_mesh(self, *a, **kw):
        return torch.zeros(1, 3), None, None


@pytest.fixture
def seen(monkeypatch):
    """Spy on run._sequence: what the loop under test got from it; every loop is stopped right behind it."""
    got = {}
    real = run._sequence

    def spy(*a, **kw):
        got['frames'], got['names'], got['folder'] = real(*a, **kw)
        return got['frames'], got['names'], got['folder']

    def stop(*a, **kw):
        raise Stop

    monkeypatch.setattr(run, '_sequence', spy)
    for owner, name in ((run, '_render_loop'), (run, '_VideoOut'), (render, 'ImageWriter'), (render, 'MetricsWriter')):
        monkeypatch.setattr(owner, name, stop)
    return got


def _movement(n=2, **kw):
    return [('movement', (i,), kw) for i in range(n)]


def _cameras(kind, **kw):
    return [(kind, (i, 2), dict(kw, bgcolor=cfg.bgcolor)) for i in range(2)]


IMG = dict(load_image=True, device=DEV)
FREE = dict(train_frame_idx=1, src_type='zju_mocap', image_size=SIZE)
BLANK, NUMBERED = [None, None], ['000000', '000001']

# (caller, its arguments) -> the calls the subject sees, the names, the folder the caller goes on with
CASES = {
    'movement': (lambda n, s: run.run_movement(n, s, device=DEV, test_num=2), _movement(**IMG), NAMES, 'movement'),
    'freeview, world 1': (lambda n, s: run.run_freeview(n, s, frame_idx=1, total_frames=2),
                          _cameras('freeview', **FREE), BLANK, 'freeview_1'),
    'freeview, world 2': (lambda n, s: run.run_freeview(n, s, frame_idx=1, total_frames=2, world=2, rank=1),
                          _cameras('freeview', **FREE), NUMBERED, 'freeview_1'),
    'freeview, its own size and source': (
        lambda n, s: run.run_freeview(n, s, frame_idx=1, total_frames=2, image_size=(8, 6), src_type='wild'),
        _cameras('freeview', train_frame_idx=1, src_type='wild', image_size=(8, 6)), BLANK, 'freeview_1'),
    # the volume loops pass image_size through to the T-pose camera
    'tpose, world 1': (lambda n, s: run.run_tpose(n, s, total_frames=2, image_size=(64, 48)),
                       _cameras('tpose', image_size=(64, 48)), BLANK, 'tpose'),
    'tpose, world 2': (lambda n, s: run.run_tpose(n, s, total_frames=2, world=2), _cameras('tpose', image_size=None),
                       NUMBERED, 'tpose'),
    'heads movement': (lambda n, s: run.run_heads(n, s, 'movement', device=DEV, test_num=2), _movement(**IMG), NAMES,
                       'movement'),
    'heads freeview': (lambda n, s: run.run_heads(n, s, 'freeview', frame_idx=1, total_frames=2, device=DEV),
                       _cameras('freeview', **FREE), BLANK, 'freeview_1'),
    'heads tpose': (lambda n, s: run.run_heads(n, s, 'tpose', total_frames=2, device=DEV, image_size=(64, 48)),
                    _cameras('tpose', image_size=(64, 48)), BLANK, 'tpose'),
    # the mesh loop: movement frames carry image_size= and no image
    'mesh movement': (lambda n, s: run.run_mesh_render(n, s, 'movement', test_num=2), _movement(image_size=SIZE), NAMES,
                      'mesh_movement'),
    'mesh movement, its own size': (lambda n, s: run.run_mesh_render(n, s, 'movement', test_num=2, image_size=(8, 6)),
                                    _movement(image_size=(8, 6)), NAMES, 'mesh_movement'),
    # ... freeview_frame is called without src_type
    'mesh freeview': (lambda n, s: run.run_mesh_render(n, s, 'freeview', frame_idx=1, total_frames=2),
                      _cameras('freeview', train_frame_idx=1, image_size=SIZE), BLANK, 'mesh_freeview_1'),
    # ... the T-pose size is squared: int(np.max(image_size))
    'mesh tpose': (lambda n, s: run.run_mesh_render(n, s, 'tpose', total_frames=2, image_size=(64, 48)),
                   _cameras('tpose', image_size=64), BLANK, 'mesh_tpose'),
    'mesh tpose, no size': (lambda n, s: run.run_mesh_render(n, s, 'tpose', total_frames=2),
                            _cameras('tpose', image_size=None), BLANK, 'mesh_tpose'),
    'surface points': (lambda n, s: run.run_surface_points(n, s, device=DEV, test_num=2), _movement(**IMG), NAMES, 'movement'),
    'surface points, every frame': (lambda n, s: run.run_surface_points(n, s, device=DEV), _movement(3, **IMG),
                                    NAMES + ['a-2'], 'movement'),
    'compare lbs delta': (lambda n, s: run.run_compare_lbs_delta(n, s, device=torch.device('cuda'), test_num=2),
                          _movement(load_image=True, device=torch.device('cuda')), NAMES, 'movement'),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_sequence_of_every_loop(case, seen):
    call, calls, names, folder = CASES[case]
    subject = StubSubject()
    before = cfg.clone()
    show_truth = cfg.get('show_truth', None)
    try:
        with pytest.raises(Stop):
            call(StubNetwork(), subject)
        assert len(seen['frames']) == len(calls)
        subject.calls.clear()
        for i in range(len(seen['frames'])):
            seen['frames'][i]
        assert subject.calls == calls
        assert seen['names'] == names and seen['folder'] == folder
        if case != 'movement':      # an exception in the loop: every override is put back (an absent show_truth as False)
            assert dict(cfg, show_truth=cfg.get('show_truth', False)) == dict(before, show_truth=show_truth or False)
    finally:
        if show_truth is None:                  # run_movement's lasting cfg.show_truth = True
            cfg.pop('show_truth', None)
        else:
            cfg.show_truth = show_truth


def test_sequence_folder_and_frame_count_defaults(seen, monkeypatch):
    """cfg.render_folder_name renames the volume loops' freeview / tpose folders, never a mesh_ folder and never the
    movement folder; cfg.render_frames and cfg.freeview.frame_idx stand in for arguments not given."""
    monkeypatch.setitem(cfg, 'render_folder_name', 'mine')
    monkeypatch.setitem(cfg, 'render_frames', 5)
    monkeypatch.setitem(cfg, 'freeview', {'frame_idx': 2})
    subject = StubSubject()
    with pytest.raises(Stop):
        run.run_freeview(StubNetwork(), subject)
    seen['frames'][4]
    assert seen['folder'] == 'mine' and len(seen['frames']) == 5 and subject.calls[-1][2]['train_frame_idx'] == 2
    with pytest.raises(Stop):
        run.run_tpose(StubNetwork(), subject)
    assert seen['folder'] == 'mine' and len(seen['frames']) == 5
    with pytest.raises(Stop):
        run.run_mesh_render(StubNetwork(), subject, 'freeview')
    assert seen['folder'] == 'mesh_freeview_2'
    with pytest.raises(Stop):
        run.run_mesh_render(StubNetwork(), subject, 'tpose')
    assert seen['folder'] == 'mesh_tpose'
    with pytest.raises(Stop):
        run.run_heads(StubNetwork(), subject, 'movement', device=DEV)
    assert seen['folder'] == 'movement' and len(seen['frames']) == 3


# --------------------------------------------------------------------------------------------- run._cfg_override
@pytest.fixture
def clean_cfg():
    """The four values the manager touches are the tests' to set; the amd node itself is put back, not a copy."""
    keys = ('perturb', 'ignore_non_rigid_motions', 'show_truth', 'amd')
    before = {k: cfg[k] for k in keys if k in cfg}
    yield
    for k in keys:
        cfg.pop(k, None)
    cfg.update(before)


def test_override_restores_after_exit_and_exception(clean_cfg):
    cfg.perturb, cfg.ignore_non_rigid_motions, cfg.show_truth = 1., False, False
    cfg.amd = {'diagnostics': False}
    with run._cfg_override(perturb=0., ignore_non_rigid_motions=True, show_truth=True, diagnostics=True):
        assert (cfg.perturb, cfg.ignore_non_rigid_motions, cfg.show_truth, cfg.amd['diagnostics']) == (0., True, True, True)
    assert (cfg.perturb, cfg.ignore_non_rigid_motions, cfg.show_truth, cfg.amd['diagnostics']) == (1., False, False, False)
    with pytest.raises(KeyError):
        with run._cfg_override(perturb=0., diagnostics=True):
            assert cfg.perturb == 0. and cfg.amd['diagnostics'] is True
            raise KeyError('in the block')
    assert cfg.perturb == 1. and cfg.amd['diagnostics'] is False
    assert cfg.ignore_non_rigid_motions is False            # (a key that was not asked for is not touched)


def test_override_pops_an_absent_diagnostics_key(clean_cfg):
    cfg.amd = {'mlp_mode': 'f16x3'}
    with run._cfg_override(diagnostics=True):
        assert cfg.amd['diagnostics'] is True
    assert 'diagnostics' not in cfg.amd and dict(cfg.amd) == {'mlp_mode': 'f16x3'}
    with pytest.raises(KeyError):
        with run._cfg_override(diagnostics=True):
            raise KeyError('in the block')
    assert 'diagnostics' not in cfg.amd
    cfg.amd['diagnostics'] = None                           # a key that is there keeps its value, None too
    with run._cfg_override(diagnostics=True):
        pass
    assert cfg.amd['diagnostics'] is None


def test_override_leaves_a_cfg_without_amd_node_alone(clean_cfg):
    cfg.pop('amd', None)
    cfg.perturb = 1.
    with run._cfg_override(perturb=0., diagnostics=True):
        assert 'amd' not in cfg and cfg.perturb == 0.
    assert 'amd' not in cfg and cfg.perturb == 1.


def test_override_nests_and_restores_in_order(clean_cfg):
    cfg.perturb, cfg.ignore_non_rigid_motions = 1., False
    cfg.amd = {}
    with run._cfg_override(perturb=.5, diagnostics=False):
        with run._cfg_override(perturb=0., ignore_non_rigid_motions=True, diagnostics=True):
            assert (cfg.perturb, cfg.ignore_non_rigid_motions, cfg.amd['diagnostics']) == (0., True, True)
        assert (cfg.perturb, cfg.ignore_non_rigid_motions, cfg.amd['diagnostics']) == (.5, False, False)
    assert (cfg.perturb, cfg.ignore_non_rigid_motions) == (1., False) and 'diagnostics' not in cfg.amd


def test_override_of_an_absent_show_truth_comes_back_false(clean_cfg):
    cfg.pop('show_truth', None)                 # what the loops did by hand: cfg.show_truth = cfg.get('show_truth', False)
    with run._cfg_override(show_truth=True):
        assert cfg.show_truth is True
    assert cfg.show_truth is False


# --------------------------------------------------------------------------------------------- the frame workspace
# hnrf_render_frame_workspace_bytes(2, 4), hnrf_render_frame_shared_workspace_bytes(2, 4) and
# hnrf_render_frame_heads_workspace_bytes(2, 4, 2) as the library returned them when each entry stated its size itself:
# 2 x 7 parts of 256 bytes | + the representative slot | + 2 planes x 8 samples x 16 bytes
PLAIN_BYTES, SHARED_BYTES, HEADS_BYTES = 3584, 3840, 3840
E_ARG, E_WORKSPACE = -1, -4


def test_frame_workspace_sizes_and_checks_do_not_need_a_gpu():
    lib = _lib.load_heads()
    err = lambda: lib.hnrf_last_error().decode()
    assert lib.hnrf_render_frame_workspace_bytes(2, 4) == PLAIN_BYTES
    assert lib.hnrf_render_frame_shared_workspace_bytes(2, 4) == SHARED_BYTES
    assert lib.hnrf_render_frame_heads_workspace_bytes(2, 4, 2) == HEADS_BYTES
    assert lib.hnrf_render_frame_workspace_bytes(-1, 4) == 0 and lib.hnrf_render_frame_heads_workspace_bytes(2, 4, 9) == 0
    p = 256                                                 # a fake pointer, 256-byte aligned and never followed:
    planes = (ctypes.c_void_p * 2)(p, p)                    # every call below returns at an argument check
    # rays_o .. bbox_scale, hann_w (null: the check behind the workspace's), nr_packed, cnl_packed, bgcolor, mode f16x3,
    # cull_eps, N, S, B, G, chunk
    head = [p] * 10 + [None, p, p, p, 1, 0., 5, 4, 24, 32, 2]
    lean = [p, p, p] + [None] * 8                           # rgb, alpha, depth; no diagnostic outputs
    tail = [None, None, None, None]                         # side stream, events, MLP events, stream
    entries = {
        'hnrf_render_frame_fwd': (PLAIN_BYTES, lambda n: lib.hnrf_render_frame_fwd(*head, p, n, *lean, *tail)),
        'hnrf_render_frame_shared_fwd': (SHARED_BYTES,
                                         lambda n: lib.hnrf_render_frame_shared_fwd(*head, p, n, *lean, p, *tail)),
        'hnrf_render_frame_heads_fwd': (HEADS_BYTES, lambda n: lib.hnrf_render_frame_heads_fwd(
            *head, 2, p, n, planes, planes, planes, *[None] * 8, *tail)),
    }
    for name, (need, call) in entries.items():
        assert call(need - 1) == E_WORKSPACE, name
        assert err() == '%s: workspace %d < %d bytes' % (name, need - 1, need)
        assert call(need) == E_ARG and err() == '%s: hann_w missing' % name


# --------------------------------------------------------------------------------------------- _lib's additive headers
PHRASES = {'cloud': 'the surface-point and frame-distance kernels', 'video': 'the JPEG encoder',
           'segment': 'the body-part segmentation', 'geometry': 'the geometry maps',
           'heads': 'the multi-head canonical MLP'}


def test_header_groups_are_derived_from_one_table():
    assert set(_lib.GROUPS) == set(PHRASES)
    for group, (header, phrase) in _lib.GROUPS.items():
        assert header == 'hnrf_%s.h' % group and phrase == PHRASES[group]
        assert getattr(_lib, group.upper() + '_HEADER_PATH').replace('\\', '/').endswith('/include/' + header)
        assert getattr(_lib, group.upper() + '_SIGNATURES') and callable(getattr(_lib, 'load_' + group))
        assert getattr(_lib, 'load_' + group)() is _lib.load()


@pytest.mark.parametrize('group', sorted(PHRASES))
def test_binder_names_the_group_of_a_missing_symbol(group):
    class Fn:
        restype = argtypes = None

    sigs = getattr(_lib, group.upper() + '_SIGNATURES')
    missing = sorted(sigs)[-1]
    fake = type('FakeLib', (), {name: Fn() for name in sigs if name != missing})()
    with pytest.raises(_lib.HnrfError) as e:
        _lib._bind(group, fake)
    assert str(e.value) == ('%s does not export %s: it was built before %s (include/hnrf_%s.h); rebuild it'
                            % (_lib.LIB_PATH, missing, PHRASES[group], group))
    whole = type('FakeLib', (), {name: Fn() for name in sigs})()
    assert _lib._bind(group, whole) is whole
    assert all((getattr(whole, name).restype, getattr(whole, name).argtypes) == sigs[name] for name in sigs)


def test_build_self_check_binds_every_group(monkeypatch):
    import __graft_entry__ as entry
    import subprocess
    bound = []
    real = _lib._bind
    monkeypatch.setattr(_lib, '_bind', lambda group, lib=None: bound.append(group) or real(group, lib))
    monkeypatch.setattr(subprocess, 'run', lambda *a, **kw: None)          # (the library is built: no make)
    entry.build()
    assert sorted(bound) == sorted(_lib.GROUPS)
