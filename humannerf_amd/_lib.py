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
CLOUD_HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'hnrf_cloud.h'))   # included by hnrf.h
VIDEO_HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'hnrf_video.h'))   # included by hnrf.h
SEGMENT_HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'hnrf_segment.h'))   # included by hnrf.h
GEOMETRY_HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'hnrf_geometry.h'))   # included by hnrf.h
HEADS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'hnrf_heads.h'))   # included by hnrf.h

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
# the surface-point / frame-distance entries of include/hnrf_cloud.h: additive to ABI version 13, so a library of that
# version built before them (HNRF_LIB_PATH) still loads; load_cloud() binds them and raises when they are missing
CLOUD_SIGNATURES = _signatures(CLOUD_HEADER_PATH)

# the JPEG encoder's entries of include/hnrf_video.h: additive to ABI version 13 in the same way (load_video)
VIDEO_SIGNATURES = _signatures(VIDEO_HEADER_PATH)

# the body-part segmentation's entries of include/hnrf_segment.h: additive to ABI version 13 in the same way (load_segment)
SEGMENT_SIGNATURES = _signatures(SEGMENT_HEADER_PATH)

# the geometry maps' entries of include/hnrf_geometry.h: additive to ABI version 13 in the same way (load_geometry)
GEOMETRY_SIGNATURES = _signatures(GEOMETRY_HEADER_PATH)

# the multi-head canonical MLP's entries of include/hnrf_heads.h: additive to ABI version 13 in the same way (load_heads)
HEADS_SIGNATURES = _signatures(HEADS_HEADER_PATH)

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


_cloud_bound = False


def load_cloud():
    """load() plus the entries of include/hnrf_cloud.h, typed.  A library without them raises HnrfError."""
    global _cloud_bound
    lib = load()
    if not _cloud_bound:
        for name, (res, args) in CLOUD_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HnrfError(f'{LIB_PATH} does not export {name}: it was built before the surface-point and '
                                f'frame-distance kernels (include/hnrf_cloud.h); rebuild it') from None
            fn.restype = res
            fn.argtypes = args
        _cloud_bound = True
    return lib


_video_bound = False


def load_video():
    """load() plus the entries of include/hnrf_video.h, typed.  A library without them raises HnrfError."""
    global _video_bound
    lib = load()
    if not _video_bound:
        for name, (res, args) in VIDEO_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HnrfError(f'{LIB_PATH} does not export {name}: it was built before the JPEG encoder '
                                f'(include/hnrf_video.h); rebuild it') from None
            fn.restype = res
            fn.argtypes = args
        _video_bound = True
    return lib


_segment_bound = False


def load_segment():
    """load() plus the entries of include/hnrf_segment.h, typed.  A library without them raises HnrfError."""
    global _segment_bound
    lib = load()
    if not _segment_bound:
        for name, (res, args) in SEGMENT_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HnrfError(f'{LIB_PATH} does not export {name}: it was built before the body-part segmentation '
                                f'(include/hnrf_segment.h); rebuild it') from None
            fn.restype = res
            fn.argtypes = args
        _segment_bound = True
    return lib


_geometry_bound = False


def load_geometry():
    """load() plus the entries of include/hnrf_geometry.h, typed.  A library without them raises HnrfError."""
    global _geometry_bound
    lib = load()
    if not _geometry_bound:
        for name, (res, args) in GEOMETRY_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HnrfError(f'{LIB_PATH} does not export {name}: it was built before the geometry maps '
                                f'(include/hnrf_geometry.h); rebuild it') from None
            fn.restype = res
            fn.argtypes = args
        _geometry_bound = True
    return lib


_heads_bound = False


def load_heads():
    """load() plus the entries of include/hnrf_heads.h, typed.  A library without them raises HnrfError."""
    global _heads_bound
    lib = load()
    if not _heads_bound:
        for name, (res, args) in HEADS_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HnrfError(f'{LIB_PATH} does not export {name}: it was built before the multi-head canonical MLP '
                                f'(include/hnrf_heads.h); rebuild it') from None
            fn.restype = res
            fn.argtypes = args
        _heads_bound = True
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().hnrf_last_error()
        raise HnrfError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')
