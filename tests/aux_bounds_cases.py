"""The cases of tests/test_gpu_aux_buffer_bounds.py (GPU) and tests/test_aux_bounds_cases_cpu.py (CPU): the smallest
inputs at which the post-processing entries -- image pre-processing, mesh extraction, skinning, rasteriser, LPIPS, image
metrics, clouds, JPEG, segmentation, geometry maps, density-gradient normals -- can still go wrong in where they write and
read.  numpy only; every builder is deterministic.  The CPU file runs each case through the numpy twin and asserts that
it is not vacuous (a mesh has vertices, a compaction keeps and drops, a status is raised); the GPU file runs it between
guards.  Not a test."""
import numpy as np

from humannerf_amd import cloud, imageproc as ip

F32 = np.float32

# ---------------------------------------------------------------------------------------------- image pre-processing
STRONG_D = np.array([0.31, -0.2, 2e-3, -1e-3, 0.05])
UNDISTORT_CASES = {'5x7x3': ((5, 7, 3), 2.0), '64x80x1': ((64, 80, 1), 25.0), '3x3x4': ((3, 3, 4), 0.8)}


def undistort_case(name):
    """img uint8 (H, W, C), K (3, 3), D (5,) strong enough that taps fall outside the image, and the device constants
    of ops.undistort_image: cam [9] and ir [n_stripes][9] float64, n_stripes, stripe_rows."""
    (H, W, C), focal = UNDISTORT_CASES[name]
    rs = np.random.RandomState(H * 100 + W)
    img = rs.randint(1, 256, (H, W, C)).astype(np.uint8)                      # no zeros: a constant-0 tap shows
    K = np.array([[focal, 0.0, W / 2 + 0.7], [0, focal * 0.99, H / 2 - 0.4], [0, 0, 1.]])
    rows, ir = ip.undistort_stripes(K, H, W)
    cam = np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], ip.distortion_vector(STRONG_D)])
    return dict(img=img, K=K, D=STRONG_D, cam=cam, ir=np.ascontiguousarray(ir), n_stripes=len(ir), rows=rows)


COMPOSITE_SRC = (9, 11)
COMPOSITE_SCALES = [1.0, 0.5, 1.25]


def composite_case(scale, whole=False):
    """orig / alpha uint8 (9, 11, 3), bg float32 [3] in 0..255, the destination size, six 4 x 4 windows that touch all
    four borders of the destination (``whole``: one window of the whole image) and the Lanczos tables (None at scale 1)."""
    Hs, Ws = COMPOSITE_SRC
    rs = np.random.RandomState(17)
    orig = rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    alpha = np.clip(rs.randint(-200, 456, (Hs, Ws, 3)), 0, 255).astype(np.uint8)
    bg = (rs.rand(3) * 255).astype(F32)
    Hd, Wd = (Hs, Ws) if scale == 1.0 else ip.resized_size(Hs, Ws, scale)
    if whole:
        ph, pw, wins = Hd, Wd, [(0, 0)]
    else:
        ph = pw = 4
        wins = [(0, 0), (Wd - 4, 0), (0, Hd - 4), (Wd - 4, Hd - 4), ((Wd - 4) // 2, (Hd - 4) // 2), (Wd - 4, (Hd - 4) // 2)]
    tables = None
    if scale != 1.0:
        xo, xw = ip.resize_tables(Ws, Wd, 1.0 / scale, 'lanczos4')
        yo, yw = ip.resize_tables(Hs, Hd, 1.0 / scale, 'lanczos4')
        tables = tuple(np.ascontiguousarray(a) for a in (xo, xw, yo, yw))
    return dict(orig=orig, alpha=alpha, bg=bg, Hd=Hd, Wd=Wd, ph=ph, pw=pw, wins=np.asarray(wins, np.int32), tables=tables,
                scale=scale)


# (source size, scale, mode): mode 2 = the 2 x 2 box of scale exactly 1/2 where 2 * dst <= src; (9, 11) at 1/2 rounds
# to 4 x 6 and 12 > 11, so it takes the tables; (8, 12) reads the last byte of the last pixel in mode 2
MASK_CASES = [((9, 11), 1.25, 1), ((9, 11), 0.5, 1), ((9, 13), 0.5, 2), ((8, 12), 0.5, 2), ((7, 5), 0.37, 1)]
MASK_CHANNEL = 2


def mask_case(size, scale, mode):
    Hs, Ws = size
    alpha = np.clip(np.random.RandomState(Hs * 31 + Ws).randint(-100, 356, (Hs, Ws, 3)), 0, 255).astype(np.uint8)
    Hd, Wd = ip.resized_size(Hs, Ws, scale)
    assert (mode == 2) == (ip.is_half_scale(scale) and 2 * Hd <= Hs and 2 * Wd <= Ws)
    tables = None
    if mode == 1:
        xo, xw = ip.resize_tables(Ws, Wd, 1.0 / scale, 'linear')
        yo, yw = ip.resize_tables(Hs, Hd, 1.0 / scale, 'linear')
        tables = tuple(np.ascontiguousarray(a) for a in (xo, xw, yo, yw))
    return dict(alpha=alpha, Hd=Hd, Wd=Wd, tables=tables, scale=scale, mode=mode)


# ------------------------------------------------------------------------------------------------- mesh extraction
MESH_CASES = ['sphere-8', 'sphere-9', 'open-8', 'open-9', 'empty-8']
CUBE = (np.array([-1.0, -1.0, -1.0], F32), np.array([1.0, 1.0, 1.0], F32))


def mesh_case(name):
    """density (N, N, N), level, bbox.  sphere: radius 0.8 inside the cube; open: radius 1.2, the surface meets the
    lattice boundary; empty: the level lies above every density (V = F = 0)."""
    from humannerf_amd import mesh
    kind, N = name.split('-')
    N = int(N)
    ax = mesh.lattice_axes(CUBE[0], CUBE[1], N)
    z, y, x = np.meshgrid(ax[2].astype(np.float64), ax[1].astype(np.float64), ax[0].astype(np.float64), indexing='ij')
    r = {'sphere': 0.8, 'open': 1.2, 'empty': 0.8}[kind]
    d = np.ascontiguousarray((r - np.sqrt(x * x + y * y + z * z)).astype(F32))
    return dict(d=d, N=N, level=2.0 if kind == 'empty' else 0.0, bmin=CUBE[0], bmax=CUBE[1], empty=kind == 'empty')


# -------------------------------------------------------------------------------------- skinning and field normals
SKIN_SHAPES = [(77, 24, 5), (77, 7, 2), (1, 1, 2), (0, 24, 5)]                 # (V, B, G)
SKIN_EXTRA = [0, 3]                                                           # channels of vol beyond B
SKIN_KS = [4, 8]


def skin_case(V, B, G, extra, seed=0):
    """verts (V, 3) inside and a little outside the box, with a vertex on the lower corner, one on the upper corner, one
    far outside and one with a NaN coordinate; vol (B + extra, G, G, G); a motion basis, joint matrices with exactly B
    rows, and the inputs of hnrf_field_normals."""
    rs = np.random.RandomState(1000 * V + 10 * B + G + seed)
    bmin, bmax = np.array([-1.0, -1.2, -0.8], F32), np.array([1.1, 1.0, 0.9], F32)
    scale = (F32(2.0) / (bmax - bmin)).astype(F32)
    verts = (bmin + (bmax - bmin) * rs.uniform(-0.1, 1.1, (V, 3))).astype(F32)
    if V >= 1:
        verts[V - 1] = bmax                                                   # on three faces at once (the last vertex)
    if V > 4:
        verts[0] = bmin
        verts[1] = bmax + F32(5.0)
        verts[2, 0] = np.nan
        verts[3] = (bmin[0], 0.0, bmax[2])
    vol = rs.uniform(0.0, 1.0, (B + extra, G, G, G)).astype(F32)
    vol /= vol.sum(0, keepdims=True)
    q, _ = np.linalg.qr(rs.standard_normal((B, 3, 3)))
    Rs = (q + 0.01 * rs.standard_normal((B, 3, 3))).astype(F32)
    Ts = rs.uniform(-0.3, 0.3, (B, 3)).astype(F32)
    mats = rs.uniform(-1, 1, (B, 3, 4)).astype(F32)
    g = (rs.standard_normal((V, 3)) * 100).astype(F32)
    sigma = (rs.standard_normal(V) * 30).astype(F32)
    return dict(verts=verts, vol=vol, bmin=bmin, scale=scale, Rs=Rs, Ts=Ts, mats=mats, g=g, sigma=sigma, V=V, B=B, G=G)


def lbs_inputs(c, K):
    """joints (V, K) uint8 and weights (V, K) of the twin, with a joint index >= B planted in two slots."""
    from humannerf_amd import skin
    j, w, _ = skin.skin_weights_host(c['verts'], c['vol'], c['bmin'], c['scale'], k=K, n_bones=c['B'])
    j, w = j.copy(), w.copy()
    if c['V'] > 6:
        j[5, 1], j[6, K - 1] = c['B'], 255
        w[5, 1], w[6, K - 1] = 0.25, 0.5
    if c['V'] >= 1:
        j[c['V'] - 1, K - 1] = 200                                            # the last slot of the last vertex
        w[c['V'] - 1, K - 1] = 0.125
    return np.ascontiguousarray(j), np.ascontiguousarray(w)


# ------------------------------------------------------------------------------------------------------- rasteriser
RASTER_SIZES = [(1, 1), (5, 7), (17, 33)]
RASTER_SCENES = ['hang', 'cover', 'no_verts', 'no_faces']


def raster_case(scene, H, W):
    """verts, faces, colors, K, E, bgcolor.  'hang': one triangle whose apex lies above the image, whose base lies below
    it and whose sides cross the left and the right border (it leaves the upper corners), and a face with indices
    outside [0, V); 'cover': behind it a triangle that covers the whole image; 'no_verts': V = 0 with two faces;
    'no_faces': F = 0."""
    f, z_hang, z_cover = 40.0, 2.0, 3.0
    px = lambda u, v, z: ((u - W / 2.0) * z / f, (v - H / 2.0) * z / f, z)
    hang = [px(W / 2.0, -0.6 * H - 1, z_hang), px(-0.4 * W - 1, 1.3 * H + 1, z_hang), px(1.4 * W + 1, 1.3 * H + 1, z_hang)]
    cover = [px(-W - 5.0, -5.0, z_cover), px(2 * W + 5.0, -5.0, z_cover), px(W / 2.0, 3 * H + 5.0, z_cover)]
    verts = np.array(hang + cover + [px(1.0, 1.0, 2.5)], F32)
    faces = {'hang': [[0, 1, 2], [0, 7, 2], [-1, 1, 2]], 'cover': [[3, 4, 5], [0, 1, 2], [0, 1, 1 << 30]],
             'no_verts': [[0, 1, 2], [3, 4, 5]], 'no_faces': []}[scene]
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    if scene == 'no_verts':
        verts = np.zeros((0, 3), F32)
    colors = np.random.RandomState(3).uniform(0, 1, verts.shape).astype(F32)
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], F32)
    E = np.eye(4, dtype=F32)
    return dict(verts=verts, faces=faces, colors=colors, K=K, E=E, bg=np.array([0.1, 0.6, 0.3], F32))


# --------------------------------------------------------------------------------------------------- image metrics
METRIC_SIZES = [(7, 7), (8, 9), (33, 70)]
METRIC_MASKS = ['none', 'empty', 'L', 'narrow']


def metrics_case(n_img, H, W, mask_kind):
    """pred, target uint8 (n, H, W, 3) and mask uint8 (n, H, W) or None.  'L': the bounding box exceeds the support;
    'narrow': a crop six columns wide (SSIM is NaN, no error); 'empty': no pixel.  With n = 3 the three images take the
    kinds in turn, starting at ``mask_kind``."""
    rs = np.random.RandomState(H * 100 + W + n_img)
    a = rs.randint(0, 256, (n_img, H, W, 3)).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rs.randint(-12, 13, a.shape), 0, 255).astype(np.uint8)
    if mask_kind == 'none':
        return a, b, None
    kinds = METRIC_MASKS[1:]
    m = np.zeros((n_img, H, W), np.uint8)
    for i in range(n_img):
        kind = kinds[(kinds.index(mask_kind) + i) % 3]
        if kind == 'L':
            m[i, 1:H - 1, 1:3] = 1
            m[i, H - 3:H - 1, 1:W - 1] = 255
        elif kind == 'narrow':
            m[i, 0:H, 0:min(6, W)] = 1
    return a, b, m


# -------------------------------------------------------------------------------------------------- surface points
def rays_case(R, S, B, seed=0):
    rs = np.random.RandomState(seed + 100 * R + 10 * S + B)
    w = (rs.uniform(0, 1, (R, S)) ** 3).astype(F32)
    return w, rs.normal(0, 0.5, (R, S, 3)).astype(F32), (rs.uniform(0, 1, (R, S, B)) ** 4).astype(F32)


NN_SHAPES = [(0, 5), (5, 0), (1, 1), (257, 300)]


def nn_case(Na, Nb):
    rs = np.random.RandomState(Na * 1000 + Nb)
    return rs.uniform(-1, 1, (Na, 3)).astype(F32), rs.uniform(-1, 1, (Nb, 3)).astype(F32)


PAIRS_TAU = 0.02
PAIRS_AXIS = 1


def pairs_case():
    """Four frames packed: 0, 1 and 300 points, and a fourth whose offsets row lies outside ``total`` (it counts as
    empty).  The pairs are (2, 2) (every point finds itself), (2, 1) (one partner at most: frame 1's point lies 0.3 tau
    from point 17 of frame 2), (1, 7) (no such frame) and (3, 2) (the frame outside total).  max_n = 300."""
    rs = np.random.RandomState(5)
    big = rs.uniform(-0.2, 0.2, (300, 3)).astype(F32)
    one = (big[17] + np.array([0.3 * PAIRS_TAU, 0, 0], F32)).astype(F32)[None]
    frames = [dict(xyz=np.zeros((0, 3), F32), rgb=np.zeros((0, 3), F32)), dict(xyz=one, rgb=rs.uniform(0, 1, (1, 3)).astype(F32)),
              dict(xyz=big, rgb=rs.uniform(0, 1, (300, 3)).astype(F32))]
    sorted_frames = [cloud.sort_frame(f['xyz'], f['rgb'], PAIRS_AXIS) for f in frames]
    cat = lambda k, shape, dt: np.ascontiguousarray(np.concatenate([f[k] for f in sorted_frames]).astype(dt).reshape(shape))
    total = 301
    return dict(frames=sorted_frames, xyz=cat('xyz', (total, 3), F32), rgb=cat('rgb', (total, 3), F32),
                orig=cat('orig', (total,), np.int32), offsets=np.array([0, 0, 1, 301, 400], np.int64), total=total, F=4,
                pairs=np.array([[2, 2], [2, 1], [1, 7], [3, 2]], np.int32), max_n=300, tau=PAIRS_TAU, axis=PAIRS_AXIS)


def pairs_twin(c):
    """D (P,) float64 and match (P, max_n) int32 of the twin: an unknown or out-of-range frame counts as empty."""
    empty = dict(xyz=np.zeros((0, 3), F32), rgb=np.zeros((0, 3), F32), orig=np.zeros(0, np.int32))
    frame = lambda f: c['frames'][f] if 0 <= f < 3 else empty
    D, match = np.zeros(len(c['pairs'])), np.full((len(c['pairs']), c['max_n']), -1, np.int32)
    for p, (i, j) in enumerate(c['pairs']):
        m, _, D[p] = cloud.twin_pairs(frame(i), frame(j), c['tau'], c['axis'])
        match[p, :m.size] = m
    return D, match


# ------------------------------------------------------------------------------------------------------------ JPEG
JPEG_SIZES = [(1, 1), (17, 33), (16, 16), (40, 24)]
JPEG_QUALITIES = [1, 100]
JPEG_PADS = [0, 21]                                                           # row_stride = 3 W + pad


def jpeg_image(H, W):
    """Noise of 0 and 255 in every channel: at quality 100 its MCUs are longer than those of uniform noise."""
    return (np.random.RandomState(H * 77 + W).randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)


def jpeg_tight(img, pad):
    """The image as a flat buffer of exactly (H - 1) row_stride + 3 W bytes, row_stride = 3 W + pad: the bytes behind
    the last row's last pixel do not exist."""
    H, W = img.shape[:2]
    stride = 3 * W + pad
    buf = np.random.RandomState(pad + 1).randint(0, 256, (H - 1) * stride + 3 * W).astype(np.uint8)
    for y in range(H):
        buf[y * stride:y * stride + 3 * W] = img[y].reshape(-1)
    return buf, stride


# --------------------------------------------------------------------------------------------------- segmentation
SEG_H, SEG_W = 7, 30
SEG_COUNTS = (150, 190)                                                       # two frames; the boundary lies inside block 0
SEG_RADII = [1, 33]
SEG_PARTS = {1: {'only': [3, 15]}, 32: dict({'p%02d' % p: [p % 24] for p in range(31)}, p31=[23, 5])}
SEG_WEIGHT_MIN = 0.3


def segment_case(bad=False):
    """rec (341, 10) of two frames and one trailing row outside every frame, offsets [0, 150, 340]; two records share
    pixel (3, 4) of frame 0; a NaN weight.  ``bad``: record 160 lies at row 7 = H (status bit 2)."""
    rs = np.random.RandomState(11)
    frames = []
    for n in SEG_COUNTS:
        frames.append(np.concatenate([rs.uniform(0, 1, (n, 6)), rs.uniform(0.05, 1.0, (n, 1)), rs.randint(0, SEG_H, (n, 1)),
                                      rs.randint(0, SEG_W, (n, 1)), rs.randint(0, 24, (n, 1))], axis=1).astype(F32))
    frames[0][10, 7:9] = frames[0][11, 7:9] = (3, 4)
    frames[0][10, 9], frames[0][11, 9] = 3, 23
    frames[0][10, 6] = np.nan                                                 # (a member of the part its own bone seeds)
    if bad:
        frames[1][10, 7] = SEG_H
    extra = frames[1][:1].copy()                                              # a row outside every frame
    rec = np.ascontiguousarray(np.concatenate(frames + [extra]))
    return dict(frames=frames, rec=rec, offsets=np.array([0, 150, 340], np.int64), total=341, F=2)


def segment_twin(c, n_parts, radius, weighted):
    """member (total,) uint32, seg_offsets (P F + 1,) int64, src int32 of the twin; the trailing row is member 0."""
    masks = cloud.bone_masks(SEG_PARTS[n_parts])
    members = [cloud.twin_segment(f, masks, SEG_H, SEG_W, radius) for f in c['frames']]
    seg, src = cloud.twin_compact(members, n_parts, weights=[f[:, 6] for f in c['frames']] if weighted else None,
                                  weight_min=SEG_WEIGHT_MIN if weighted else 0.0)
    return np.concatenate(members + [np.zeros(1, np.uint32)]), seg, src


# --------------------------------------------------------------------------------------------------- geometry maps
SURFACE_R = [0, 1, 5]
SURFACE_S = [1, 64, 65]
MAP_SIZES = [(1, 1), (1, 7), (5, 3)]


def maps_case(H, W, seed=0, bad_index=False):
    """A frame of N rays on H x W pixels: most pixels have a ray, two rays share a pixel (the highest wins); t with
    jumps, both valid bits, alpha, woff, a truth image.  ``bad_index``: one ray index lies outside the image."""
    from tests import geometry_cases as gc
    rs = np.random.RandomState(seed + 100 * H + W)
    HW = H * W
    pix = np.sort(rs.permutation(HW)[:max(1, int(0.9 * HW))]).astype(np.int64)
    if HW > 1:
        pix = np.concatenate([pix, pix[:1]])
    N = pix.size
    o = (np.tile(gc.CAM, (N, 1)) + rs.normal(0, 1e-3, (N, 3))).astype(F32)
    d = gc.camera(H, W)[1][pix].astype(F32)
    y, x = pix // W, pix % W
    t = (3.0 + 0.004 * x - 0.003 * y + 0.08 * (rs.uniform(size=N) < 0.15) * rs.normal(size=N)).astype(F32)
    valid = ((rs.uniform(size=N) > 0.2) * 1 + (rs.uniform(size=N) > 0.2) * 2).astype(np.uint8)
    surf = dict(t_exp=t, t_med=(t + rs.normal(0, 0.01, N)).astype(F32), valid=valid,
                woff=rs.normal(0, 0.015, (N, 3)).astype(F32))
    truth = (rs.randint(0, 256, (H, W, 3)) * (rs.uniform(size=(H, W, 1)) > 0.4)).astype(np.uint8)
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    index = pix.copy()
    if bad_index:
        index[N // 2] = HW + 2
    return dict(o=o, d=d, surf=surf, ray_index=index, N=N, truth=truth, alpha=rs.uniform(0, 1, N).astype(F32),
                M=q.astype(F32), bg=np.array([0.2, 0.5, 1.0], F32), lohi=np.array([2.9, 3.4], F32), edge=0.05)


# ----------------------------------------------------------------------------------------- density-gradient normals
NORMALS_SHAPES = [(R, S, B) for R in (1, 3, 5) for S in (1, 65) for B in (1, 24)]
NORMALS_COUNTS = ['over', 'equal', 'zero']


def ray_normals_case(R, S, B, count_kind):
    """normals_cases.ray_case with an index outside [0, R S) planted (two where there are two kept samples) and the
    count word: 'over' = n_max + 7 (read as n_max), 'equal' = n_max, 'zero' = 0 with idx / g of n_max rows all the same."""
    from tests import normals_cases as nc
    w, bmw, Rs, idx, g, alpha = nc.ray_case(R, S, B, seed=1000 * R + S + B, kept='all' if R == 1 else 'mixed')
    idx = idx.copy()
    if idx.size >= 1:
        idx[-1] = R * S + 3
    if idx.size >= 3:
        idx[1] = -1
    n = idx.size
    count = {'over': n + 7, 'equal': n, 'zero': 0}[count_kind]
    return dict(w=w, bmw=bmw, Rs=Rs, idx=idx, g=g, alpha=alpha, n_max=n, count=np.array([count], np.int32), R=R, S=S, B=B)


def ray_normals_twin(c):
    """(normal, nvalid) of geometry.ray_normals_host on the rows the entry reads: the first min(count, n_max), without
    the indices outside [0, R S)."""
    from humannerf_amd import geometry as geo
    n = min(int(c['count'][0]), c['n_max'])
    idx, g = c['idx'][:n], c['g'][:n]
    keep = (idx >= 0) & (idx < c['R'] * c['S'])
    return geo.ray_normals_host(c['w'], c['bmw'], c['Rs'], idx[keep], g[keep], c['alpha'])
