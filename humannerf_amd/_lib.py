"""ctypes binding of libhnrf.so (the C ABI declared in include/hnrf.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C humannerf_amd/csrc``.  There is NO fallback: if the shared object is
missing or a symbol cannot be resolved, importing/using the ops raises.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HNRF_LIB_PATH', os.path.join(_HERE, 'libhnrf.so'))   # override: diagnostic builds only

HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'hnrf.h'))

# The additive headers (each included by hnrf.h): group -> (header file, what a library without its entries was "built
# before").  Their entries are additive to ABI version 13, so a library of that version built before them (HNRF_LIB_PATH)
# still loads; load_<group>() binds them and raises when they are missing.  <GROUP>_HEADER_PATH and <GROUP>_SIGNATURES
# below come from this table, and load_all() -- the self-check of __graft_entry__.build() -- walks it.
GROUPS = {
    'cloud': ('hnrf_cloud.h', 'the surface-point and frame-distance kernels'),
    'video': ('hnrf_video.h', 'the JPEG encoder'),
    'segment': ('hnrf_segment.h', 'the body-part segmentation'),
    'geometry': ('hnrf_geometry.h', 'the geometry maps'),
    'heads': ('hnrf_heads.h', 'the multi-head canonical MLP'),
}

# Headers added after the five above, of the same shape and bound in the same way, but by _bind_late / load_late():
# GROUPS and _bind stay what libraries and callers of ABI version 13 know them as.  build() calls load_late() after
# load_all().
LATE_GROUPS = {
    'skin': ('hnrf_skin.h', 'the skinned glTF export'),
}

# The open table: EVERY LATER HEADER GOES HERE.  The two tables above are pinned to their present keys by the tests that
# came with them; this one is not, and stays so: a test asserts that its group is a member ('x' in OPEN_GROUPS), never
# the full list of keys.  Same shape, bound by _bind_table through load_<group>() / load_open(); build() calls
# load_open() after load_late().
OPEN_GROUPS = {
    'heads_shared': ('hnrf_heads_shared.h', 'the shared evaluation for all heads'),
    'normals': ('hnrf_normals.h', 'the density-gradient normals'),
    'heads_train': ('hnrf_heads_train.h', 'the multi-head training kernels'),
    'view': ('hnrf_view.h', 'view-dependent colour'),
}

_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float,
            'double': ctypes.c_double}
_DECL = re.compile(r'([\w\s]+?[\s*]+)(hnrf_\w+)\s*\(([^()]*)\)\s*;')


class HnrfError(RuntimeError):
    pass


def _ctype(text, decl, ret=False):
    """ctypes type of one C type as the header writes it; anything it does not know raises (it never guesses)."""
    words = text.replace('*', ' * ').split()
    if '*' in words:
        return ctypes.c_char_p if ret and words == ['const', 'char', '*'] else ctypes.c_void_p
    if len(words) == 1 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    raise HnrfError(f'include/hnrf.h: unknown type {text.strip()!r} in `{decl}`')


def parse_header(text):
    """name -> (restype, argtypes) of every function declared in `text` (the C of include/hnrf.h)."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*|^\s*#[^\n]*', ' ', text, flags=re.M)
    sigs = {}
    for m in _DECL.finditer(text):
        decl = ' '.join(m.group(0).split())
        params = [] if m.group(3).strip() in ('', 'void') else m.group(3).split(',')
        # a parameter is its type followed by its name; the name is the last identifier
        args = [_ctype(re.sub(r'\w+\s*$', '', q), decl) for q in params]
        sigs[m.group(2)] = (_ctype(m.group(1), decl, ret=True), args)
    missed = set(re.findall(r'\b(hnrf_\w+)\s*\(', text)) - set(sigs)      # (a parameter list with parentheses, say)
    if missed:
        raise HnrfError(f'include/hnrf.h: cannot parse the declaration of {sorted(missed)}')
    return sigs


def _signatures(path=HEADER_PATH):
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise HnrfError(f'{path}: cannot read the C ABI declarations ({e})') from None


# name -> (restype, argtypes), derived from the declarations of include/hnrf.h
SIGNATURES = _signatures()


def _header(group, table=GROUPS):
    path = os.path.normpath(os.path.join(_HERE, '..', 'include', table[group][0]))
    return path, _signatures(path)


_HEADERS = {group: _header(group) for group in GROUPS}       # group -> (header path, its name -> (restype, argtypes))
CLOUD_HEADER_PATH, CLOUD_SIGNATURES = _HEADERS['cloud']
VIDEO_HEADER_PATH, VIDEO_SIGNATURES = _HEADERS['video']
SEGMENT_HEADER_PATH, SEGMENT_SIGNATURES = _HEADERS['segment']
GEOMETRY_HEADER_PATH, GEOMETRY_SIGNATURES = _HEADERS['geometry']
HEADS_HEADER_PATH, HEADS_SIGNATURES = _HEADERS['heads']
_LATE_HEADERS = {group: _header(group, LATE_GROUPS) for group in LATE_GROUPS}
SKIN_HEADER_PATH, SKIN_SIGNATURES = _LATE_HEADERS['skin']
_OPEN_HEADERS = {group: _header(group, OPEN_GROUPS) for group in OPEN_GROUPS}
HEADS_SHARED_HEADER_PATH, HEADS_SHARED_SIGNATURES = _OPEN_HEADERS['heads_shared']
NORMALS_HEADER_PATH, NORMALS_SIGNATURES = _OPEN_HEADERS['normals']
HEADS_TRAIN_HEADER_PATH, HEADS_TRAIN_SIGNATURES = _OPEN_HEADERS['heads_train']
VIEW_HEADER_PATH, VIEW_SIGNATURES = _OPEN_HEADERS['view']

_lib = None


def load():
    """Load libhnrf.so and type every exported entry point.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HnrfError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `make -C humannerf_amd/csrc`. There is no CPU/PyTorch fallback for the hot path.')
    # One HIP runtime per process: torch bundles its own libamdhip64 (soname
    # libamdhip64.so.7).  Import torch FIRST so that libhnrf's NEEDED entry resolves to
    # that already-loaded copy; loading libhnrf first would pull in /opt/rocm's copy and
    # torch would then load a second runtime whose allocations ours cannot see.
    import torch  # noqa: F401
    tl = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
    if os.path.isfile(tl):
        ctypes.CDLL(tl, mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_bound = set()


def _bind(group, lib=None):
    """load() plus the entries of the group's header, typed.  A library without them raises HnrfError.  ``lib``: a
    library object to bind in the place of the loaded one (every time it is asked for)."""
    return _bind_table(group, lib, GROUPS, _HEADERS)


def _bind_late(group, lib=None):
    """_bind for a group of LATE_GROUPS."""
    return _bind_table(group, lib, LATE_GROUPS, _LATE_HEADERS)


def _bind_table(group, lib, table, headers):
    header, phrase = table[group]
    if lib is None and group in _bound:
        return load()
    target = load() if lib is None else lib
    for name, (res, args) in headers[group][1].items():
        try:
            fn = getattr(target, name)
        except AttributeError:
            raise HnrfError(f'{LIB_PATH} does not export {name}: it was built before {phrase} '
                            f'(include/{header}); rebuild it') from None
        fn.restype = res
        fn.argtypes = args
    if lib is None:
        _bound.add(group)
    return target


def load_cloud():
    return _bind('cloud')


def load_video():
    return _bind('video')


def load_segment():
    return _bind('segment')


def load_geometry():
    return _bind('geometry')


def load_heads():
    return _bind('heads')


def load_skin(lib=None):
    return _bind_late('skin', lib)


def load_heads_shared(lib=None):
    return _bind_table('heads_shared', lib, OPEN_GROUPS, _OPEN_HEADERS)


def load_normals(lib=None):
    return _bind_table('normals', lib, OPEN_GROUPS, _OPEN_HEADERS)


def load_heads_train(lib=None):
    return _bind_table('heads_train', lib, OPEN_GROUPS, _OPEN_HEADERS)


def load_view(lib=None):
    return _bind_table('view', lib, OPEN_GROUPS, _OPEN_HEADERS)


def load_open():
    """load() plus every group of OPEN_GROUPS (the third part of the self-check of __graft_entry__.build())."""
    lib = load()
    for group in OPEN_GROUPS:
        _bind_table(group, None, OPEN_GROUPS, _OPEN_HEADERS)
    return lib


def load_late():
    """load() plus every group of LATE_GROUPS (the second half of the self-check of __graft_entry__.build())."""
    lib = load()
    for group in LATE_GROUPS:
        _bind_late(group)
    return lib


def load_all():
    """load() plus every group of GROUPS (the self-check of __graft_entry__.build())."""
    lib = load()
    for group in GROUPS:
        _bind(group)
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().hnrf_last_error()
        raise HnrfError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')
