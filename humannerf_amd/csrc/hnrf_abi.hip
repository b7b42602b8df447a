// Error channel, version, and the inference entry points.  hnrf_render_rays_fwd (one ray chunk, rgb / alpha /
// depth) and hnrf_render_frame_fwd (every chunk of a frame, lean or with the eight diagnostic outputs) run K1 and
// then the same per-chunk body, render_chunk: K2 -> K3 -> K4.  Early ray termination (hnrf_term.hip) walks depth
// slabs instead and shares only the workspace carve (render_carve, hnrf_common.h).  The *_baked_* entries run the
// same two bodies with the baked grid's sampler (hnrf_baked.hip) in K3's place, the *_baked_nr_* entries with the
// fused offset-grid + canonical-grid sampler in the place of K2 and K3.
#include <stdarg.h>
#include <string.h>

#include "hnrf_block_scan.h"

namespace hnrf {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace hnrf

using namespace hnrf;

extern "C" int hnrf_abi_version(void) { return 13; }
extern "C" const char* hnrf_last_error(void) { return g_err; }

extern "C" size_t hnrf_render_workspace_bytes(int64_t R, int S) {
    if (R < 0 || S < 0) return 0;
    return render_carve(nullptr, R, S).bytes;
}

// a failed HIP runtime call (only hnrf_render_frame_fwd makes them, render_chunk in its diagnostic form included)
#define HNRF_HIP(call)                                                          \
    do {                                                                        \
        if ((call) != hipSuccess) {                                             \
            set_error("hnrf_render_frame_fwd / _baked_fwd: %s failed", #call);  \
            return HNRF_E_LAUNCH;                                               \
        }                                                                       \
    } while (0)

namespace {
// Where a chunk's raw comes from: the canonical MLP on `packed`, or -- grid != null -- the baked grid's sampler.
struct CnlSource {
    const void* packed;
    const void* grid;
    int N;
    const float *bmin, *bmax;
};

// no offset grid: xyz comes from K2 (nr_packed) or is x_skel
constexpr BakedGrid kNoOffGrid{nullptr, 0, nullptr, nullptr};

// Shared underflowing inputs (hnrf.h, hnrf_render_frame_shared_fwd): the chunk's ShareOut -- c_off / c_xyz / c_raw in the
// frame's representative slot (x = +0 at floats [0..2], c_off at [4..6], c_xyz at [8..10], c_raw [n][4] from [12]: 44
// floats of the slot's 64 with the 8 planes of hnrf_render_frame_heads_shared_fwd), the chunk's live count and its
// planes.  out null = off.  fused: K1 has already classified (hnrf_sample_warp_share_fwd): idx, the count
// and the fills are written; otherwise hnrf_share_compact runs here.
struct Share {
    const ShareOut* out;
    bool fused;
};

// What K3 writes and K4 composites: the n planes raw [n][P][4] and the outputs o[g] of each.  n == 1: the chunk's own
// raw (c.raw) and FrameOut; n >= 2: all heads of a multi-head canonical image (hnrf_render_frame_heads_fwd), written by
// K3 in one launch.  Every o[g] carries the same xyz / bmw / offsets: those do not depend on the head.
// view_bias: view-dependent colour (hnrf_view.h), the chunk's rows [R][3] added to every plane's raw colour in K4; null =
// none, which is what every entry but hnrf_render_frame_view_fwd passes.
struct Planes {
    int n;
    float* raw;
    const FrameOut* o;
    const float* view_bias = nullptr;
};

// K2 -> K3 -> K4 of one ray chunk whose K1 results are in `c`: the whole of hnrf_render_rays_fwd after K1, and the body
// of every chunk of hnrf_render_frame_fwd.  cull_eps > 0: the MLPs run only on the compacted samples.  ev_start /
// ev_stop (hipEvent_t, nullable) are recorded right before / after the canonical-MLP (or grid sampler) launch.
// off.grid != null (with cnl.grid): xyz and raw both come from the fused sampler of the two grids, which stands for
// K2 and K3; the lean form then writes no xyz at all.
int render_chunk(const RenderCarve& c, const float* rays_d, const float* hann_w, const void* nr_packed,
                 const BakedGrid& off, const CnlSource& cnl, const float* bgcolor, int mode, float cull_eps, int64_t R,
                 int S, const Planes& pl, void* ev_start, void* ev_stop, hipStream_t st,
                 const Share& sh = Share{nullptr, false}) {
    const FrameOut& d = pl.o[0];                                  // (K2's outputs: the same in every plane)
    const size_t P = (size_t)R * (size_t)S;
    const bool cull = cull_eps > 0.f, diag = d.weights != nullptr;
    int rc;
    if (cull && (rc = hnrf_compact_samples(c.mask, cull_eps, (int64_t)P, c.idx, c.count, st))) return rc;
    const int* ci = cull ? c.idx : nullptr;
    const int* cc = cull ? c.count : nullptr;
    float* xyz = diag ? d.xyz : c.xyz;
    if (sh.out) {                                                 // (with K2 and K3 from the MLPs and cull_eps == 0 only)
        if (!sh.fused && (rc = share_compact(c.x_skel, (int64_t)P, *sh.out, st))) return rc;
        ci = c.idx;
        cc = sh.out->count;
    }
    const float* cnl_in = c.x_skel;
    // (d's eight diagnostic pointers are all null in the lean form -- FrameOut::rows, hnrf_render_rays_* -- so d.xyz and
    // d.offsets need no `diag ?` of their own)
    if (off.grid) {
        if (ev_start) (void)hipEventRecord((hipEvent_t)ev_start, st);
        rc = baked_warp_sample(c.x_skel, off, BakedGrid{cnl.grid, cnl.N, cnl.bmin, cnl.bmax}, (int64_t)P, ci, cc, pl.raw,
                               d.xyz, d.offsets, st);
        if (ev_stop) (void)hipEventRecord((hipEvent_t)ev_stop, st);
        if (rc) return rc;
        cnl_in = d.xyz;
    } else {
        if (nr_packed) {
            if ((rc = hnrf_nonrigid_fwd_sparse(c.x_skel, hann_w, nr_packed, mode, (int64_t)P, ci, cc, xyz, d.offsets, st)))
                return rc;
            cnl_in = xyz;
        } else if (diag) {                                        // network.py:276-277: xyz = x_skel, offsets = 0
            HNRF_HIP(hipMemcpyAsync(xyz, c.x_skel, P * 12, hipMemcpyDeviceToDevice, st));
            HNRF_HIP(hipMemsetAsync(d.offsets, 0, P * 12, st));
        }
        if (ev_start) (void)hipEventRecord((hipEvent_t)ev_start, st);
        rc = cnl.grid  ? baked_sample(cnl_in, cnl.grid, cnl.N, cnl.bmin, cnl.bmax, (int64_t)P, ci, cc, pl.raw, st)
             : pl.n > 1 ? hnrf_canonical_heads_fwd_sparse(cnl_in, cnl.packed, mode, (int64_t)P, pl.n, ci, cc, pl.raw, st)
                        : hnrf_canonical_fwd_sparse(cnl_in, cnl.packed, mode, (int64_t)P, ci, cc, pl.raw, st);
        if (ev_stop) (void)hipEventRecord((hipEvent_t)ev_stop, st);
        if (rc) return rc;
    }
    for (int g = 0; g < pl.n; ++g) {
        const FrameOut& o = pl.o[g];
        if ((rc = hnrf_composite_view_fwd(pl.raw + (size_t)g * P * 4, c.mask, c.z_vals, rays_d, diag ? cnl_in : nullptr,
                                          bgcolor, pl.view_bias, R, S, cull ? cull_eps : 0.f, o.rgb, o.alpha, o.depth,
                                          o.weights, o.rgb_on_rays, o.cnl_xyz, o.cnl_rgb, o.cnl_weight, st)))
            return rc;
    }
    return HNRF_OK;
}
// the baked entries' grid arguments (the sampler launches from inside render_chunk without further checks)
int check_source(const char* who, const CnlSource& cnl) {
    if (cnl.grid == nullptr && cnl.N == 0) {
        HNRF_REQUIRE(cnl.packed, HNRF_E_ARG, "%s: null canonical weights", who);
        return HNRF_OK;
    }
    HNRF_REQUIRE(cnl.grid && cnl.bmin && cnl.bmax, HNRF_E_ARG, "%s: null grid / grid bbox pointer", who);
    HNRF_REQUIRE(cnl.N >= 8 && cnl.N <= 512, HNRF_E_ARG, "%s: grid N=%d out of range [8, 512]", who, cnl.N);
    HNRF_REQUIRE(((uintptr_t)cnl.grid & 7) == 0, HNRF_E_ARG, "%s: grid must be 8-byte aligned", who);
    return HNRF_OK;
}

// the *_baked_nr_* entries' offset grid; it goes with a canonical grid only
int check_off_source(const char* who, const BakedGrid& off, const CnlSource& cnl) {
    if (off.grid == nullptr && off.N == 0) return HNRF_OK;
    HNRF_REQUIRE(off.grid && off.bmin && off.bmax, HNRF_E_ARG, "%s: null offset grid / offset grid bbox pointer", who);
    HNRF_REQUIRE(off.N >= 8 && off.N <= 512, HNRF_E_ARG, "%s: offset grid M=%d out of range [8, 512]", who, off.N);
    HNRF_REQUIRE(((uintptr_t)off.grid & 7) == 0, HNRF_E_ARG, "%s: offset grid must be 8-byte aligned", who);
    HNRF_REQUIRE(cnl.grid, HNRF_E_ARG, "%s: an offset grid needs a canonical grid", who);
    return HNRF_OK;
}

int render_rays(const char* who, const Rays& rays, const WarpField& field, const float* hann_w, const void* nr_packed,
                const BakedGrid& off, const CnlSource& cnl, const float* bgcolor, int mode, float cull_eps, int64_t R,
                int S, void* workspace, size_t workspace_bytes, const FrameOut& out, void* ev_mlp_start,
                void* ev_mlp_stop, void* stream) {
    HNRF_REQUIRE(workspace, HNRF_E_ARG, "%s: null workspace / canonical weights", who);
    int src = check_source(who, cnl);
    if (src) return src;
    if ((src = check_off_source(who, off, cnl))) return src;
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "%s: workspace must be 256-byte aligned", who);
    HNRF_REQUIRE(workspace_bytes >= hnrf_render_workspace_bytes(R, S), HNRF_E_WORKSPACE,
                 "%s: workspace %zu < %zu bytes", who, workspace_bytes, hnrf_render_workspace_bytes(R, S));
    HNRF_REQUIRE(nr_packed == nullptr || hann_w != nullptr, HNRF_E_ARG, "%s: hann_w missing", who);
    const RenderCarve c = render_carve(workspace, R, S);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sample_warp(rays, field, R, S, c.z_vals, c.x_skel, c.mask, nullptr, nullptr, st)) return rc;
    return render_chunk(c, rays.d, hann_w, nr_packed, off, cnl, bgcolor, mode, cull_eps, R, S, Planes{1, c.raw, &out},
                        ev_mlp_start, ev_mlp_stop, st);
}
}  // namespace

extern "C" int hnrf_render_rays_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                    const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                    const float* vol, const float* bbox_min, const float* bbox_scale,
                                    const float* hann_w, const void* nr_packed, const void* cnl_packed,
                                    const float* bgcolor, int mode, float cull_eps, int64_t R, int S, int B, int G,
                                    void* workspace, size_t workspace_bytes, float* rgb, float* alpha, float* depth,
                                    void* ev_mlp_start, void* ev_mlp_stop, void* stream) {
    return render_rays("hnrf_render_rays_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                       WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, hann_w, nr_packed, kNoOffGrid,
                       CnlSource{cnl_packed, nullptr, 0, nullptr, nullptr}, bgcolor, mode, cull_eps, R, S, workspace,
                       workspace_bytes, FrameOut{rgb, alpha, depth}, ev_mlp_start, ev_mlp_stop, stream);
}

extern "C" int hnrf_render_rays_baked_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                          const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                          const float* vol, const float* bbox_min, const float* bbox_scale,
                                          const float* hann_w, const void* nr_packed, const void* grid, int grid_N,
                                          const float* grid_bbox_min, const float* grid_bbox_max, const float* bgcolor,
                                          int mode, float cull_eps, int64_t R, int S, int B, int G, void* workspace,
                                          size_t workspace_bytes, float* rgb, float* alpha, float* depth,
                                          void* ev_mlp_start, void* ev_mlp_stop, void* stream) {
    HNRF_REQUIRE(grid, HNRF_E_ARG, "hnrf_render_rays_baked_fwd: null grid");
    return render_rays("hnrf_render_rays_baked_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                       WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, hann_w, nr_packed, kNoOffGrid,
                       CnlSource{nullptr, grid, grid_N, grid_bbox_min, grid_bbox_max}, bgcolor, mode, cull_eps, R, S,
                       workspace, workspace_bytes, FrameOut{rgb, alpha, depth}, ev_mlp_start, ev_mlp_stop, stream);
}

extern "C" int hnrf_render_rays_baked_nr_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                             const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                             const float* vol, const float* bbox_min, const float* bbox_scale,
                                             const void* off_grid, int off_M, const float* off_bbox_min,
                                             const float* off_bbox_max, const void* grid, int grid_N,
                                             const float* grid_bbox_min, const float* grid_bbox_max, const float* bgcolor,
                                             int mode, float cull_eps, int64_t R, int S, int B, int G, void* workspace,
                                             size_t workspace_bytes, float* rgb, float* alpha, float* depth,
                                             void* ev_mlp_start, void* ev_mlp_stop, void* stream) {
    HNRF_REQUIRE(off_grid, HNRF_E_ARG, "hnrf_render_rays_baked_nr_fwd: null offset grid");
    HNRF_REQUIRE(grid, HNRF_E_ARG, "hnrf_render_rays_baked_nr_fwd: null grid");
    return render_rays("hnrf_render_rays_baked_nr_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                       WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, nullptr, nullptr,
                       BakedGrid{off_grid, off_M, off_bbox_min, off_bbox_max},
                       CnlSource{nullptr, grid, grid_N, grid_bbox_min, grid_bbox_max}, bgcolor, mode, cull_eps, R, S,
                       workspace, workspace_bytes, FrameOut{rgb, alpha, depth}, ev_mlp_start, ev_mlp_stop, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Whole frame: Network._batchify_rays (network.py:330-352) over _render_rays -- every ray chunk through K1..K4, the
// per-ray / per-sample results written straight into whole-frame buffers.  With a side stream the LBS warp (K1, an
// L2-gather kernel without LDS) of chunk i+1 runs while the matrix-bound MLP kernels of chunk i own the CUs: K1 leaves
// the critical path (3 % of a 512x512x128 frame).  Two workspaces alternate; the caller provides the events.
//
// The frame workspace for chunks of `rows` rays, the one statement of its size: the two chunk workspaces, behind them --
// share -- the 256 bytes of the representative slot, and -- n_heads >= 2 -- the n_heads raw planes of one chunk.  K3 and
// the K4s of a chunk run on `stream` in order, so one set of planes serves every chunk -- unless the inputs are shared:
// then K1 of chunk i+1 fills the shared rows of its planes on the side stream while the K4s of chunk i still read
// theirs, and two sets alternate like the chunk workspaces (set i & 1; K1 of chunk i+1 waits for ev_done of chunk i-1,
// the last reader of that set).
static size_t plane_set_bytes(int64_t rows, int S, int n_heads) {
    return align256((size_t)n_heads * (size_t)rows * (size_t)S * 16);
}
static size_t frame_ws_bytes(int64_t rows, int S, bool share, int n_heads) {
    return 2 * hnrf_render_workspace_bytes(rows, S) + (share ? 256 : 0) +
           (n_heads ? (share ? 2 : 1) * plane_set_bytes(rows, S, n_heads) : 0);
}
extern "C" size_t hnrf_render_frame_workspace_bytes(int64_t chunk, int S) { return frame_ws_bytes(chunk, S, false, 0); }
extern "C" size_t hnrf_render_frame_shared_workspace_bytes(int64_t chunk, int S) { return frame_ws_bytes(chunk, S, true, 0); }
extern "C" size_t hnrf_render_frame_heads_workspace_bytes(int64_t chunk, int S, int n_heads) {
    if (chunk < 0 || S < 0 || n_heads < 2 || n_heads > 8) return 0;
    return frame_ws_bytes(chunk, S, false, n_heads);
}
extern "C" size_t hnrf_render_frame_heads_shared_workspace_bytes(int64_t chunk, int S, int n_heads) {
    if (chunk < 0 || S < 0 || n_heads < 2 || n_heads > 8) return 0;
    return frame_ws_bytes(chunk, S, true, n_heads);
}

namespace {
// What a frame entry asks for beside the plain frame.  Three types that do not convert into each other: a call site
// that names them in the wrong order does not compile.  Shared inputs and heads go together
// (hnrf_render_frame_heads_shared_fwd): the slot first, the planes -- two sets then, frame_ws_bytes -- behind it.
struct FrameOpts {
    int* live_counts = nullptr;           // shared underflowing inputs: the live count of every chunk (null = off)
    int n_heads = 0;                      // >= 2: every head of a multi-head canonical image, with
    const FrameOut* head_out = nullptr;   // the whole-frame outputs of head g (head_out[0] is `out`)
    const float* view_bias = nullptr;     // view-dependent colour: the per-ray bias [N][3] of K4 (null = none)
};

int render_frame(const char* who, const Rays& rays, const WarpField& field, const float* hann_w, const void* nr_packed,
                 const BakedGrid& off, const CnlSource& cnl, const float* bgcolor, int mode, float cull_eps, int64_t N,
                 int S, int64_t chunk, void* workspace, size_t workspace_bytes, const FrameOut& out, void* side_stream,
                 void* const* events, void* const* mlp_events, void* stream, const FrameOpts& opt = {}) {
    HNRF_REQUIRE(workspace && out.rgb && out.alpha && out.depth, HNRF_E_ARG, "%s: null pointer", who);
    int src = check_source(who, cnl);
    if (src) return src;
    if ((src = check_off_source(who, off, cnl))) return src;
    HNRF_REQUIRE(N >= 0 && chunk >= 1 && S >= 2, HNRF_E_ARG, "%s: bad dims", who);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "%s: workspace must be 256-byte aligned", who);
    const int64_t cr = chunk < N ? chunk : (N > 0 ? N : 1);
    const bool share = opt.live_counts != nullptr;
    const size_t ws_one = hnrf_render_workspace_bytes(cr, S), ws_all = frame_ws_bytes(cr, S, share, opt.n_heads);
    HNRF_REQUIRE(workspace_bytes >= ws_all, HNRF_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, ws_all);
    HNRF_REQUIRE(nr_packed == nullptr || hann_w != nullptr, HNRF_E_ARG, "%s: hann_w missing", who);
    const int n_planes = opt.n_heads ? opt.n_heads : 1;
    // the planes of chunk i (null: the chunk's own raw)
    char* const heads_raw = opt.n_heads ? (char*)workspace + 2 * ws_one + (share ? 256 : 0) : nullptr;
    const size_t heads_set = share ? plane_set_bytes(cr, S, n_planes) : 0;
    HNRF_REQUIRE(!share || ((mode & HNRF_MLP_ARITH_MASK) == HNRF_MLP_F16X3 && nr_packed && cnl.packed && !cnl.grid &&
                            !off.grid && cull_eps == 0.f), HNRF_E_UNSUPPORTED,
                 "%s: shared inputs exist for HNRF_MLP_F16X3 with both MLPs and cull_eps == 0 only", who);
    const bool diag = out.weights != nullptr;
    HNRF_REQUIRE(!diag || (out.rgb_on_rays && out.cnl_xyz && out.cnl_rgb && out.cnl_weight && out.xyz && out.bmw &&
                           out.offsets), HNRF_E_ARG, "%s: the eight diagnostic outputs go together", who);
    HNRF_REQUIRE(!diag || cull_eps == 0.f, HNRF_E_UNSUPPORTED, "%s: sample culling exists in the lean form only", who);
    HNRF_REQUIRE(side_stream == nullptr || events != nullptr, HNRF_E_ARG, "%s: a side stream needs 5 events", who);
    if (N == 0) return HNRF_OK;
    hipStream_t st = (hipStream_t)stream, sd = side_stream ? (hipStream_t)side_stream : st;
    const bool two = side_stream != nullptr && side_stream != stream;
    const int64_t nchunk = (N + chunk - 1) / chunk;
    float* rep = share ? (float*)((char*)workspace + 2 * ws_one) : nullptr;
    const bool fused = share && field.B == 24;                    // K1 classifies; any other bone count: hnrf_share_compact
    // chunk i: its rays, its workspace slot, its rows of the outputs and -- with shared inputs -- its ShareOut
    struct Chunk {
        int64_t R;
        Rays rays;
        RenderCarve c;
        FrameOut o;
        ShareOut sh;
        float* raw;                                               // its n_planes raw planes, R S float4s apart
    };
    auto chunk_at = [&](int64_t i) {
        const int64_t r0 = i * chunk, R = (N - r0 < chunk) ? N - r0 : chunk;
        Chunk k{R, rays.rows(r0, S), render_carve((char*)workspace + (size_t)(i & 1) * ws_one, R, S),
                out.rows(r0, S, field.B), ShareOut{}, nullptr};
        k.raw = heads_raw ? (float*)(heads_raw + (size_t)(i & 1) * heads_set) : k.c.raw;
        if (share)
            k.sh = ShareOut{rep + 4, rep + 8, rep + 12, k.c.idx, opt.live_counts + i, (float4*)k.raw, k.o.offsets, k.o.xyz,
                            n_planes, R * (int64_t)S};
        return k;
    };
    auto warp = [&](int64_t i) {                                  // K1 of chunk i on the side stream
        const Chunk k = chunk_at(i);
        return sample_warp(k.rays, field, k.R, S, k.c.z_vals, k.c.x_skel, k.c.mask, k.o.bmw, fused ? &k.sh : nullptr, sd);
    };
    hipEvent_t ev_in = nullptr, ev_k1[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    int rc;
    if (share) {
        // the representative x = (+0, +0, +0) through the chunks' kernel instances (guarded unless no chunk is: the
        // guard sees the shared class through it), once per frame; no mlp_events around it.  In front of K1 of chunk 0
        // and of ev_in: the fused K1 reads c_off / c_xyz / c_raw and counts into live_counts, on either stream.  (K1 of
        // chunk i+1 writes idx and the raw fills of the workspace -- with heads: of the plane set -- chunk i-1 used: it
        // waits for ev_done of chunk i-1, recorded behind that chunk's last K4, the last reader of both.)  With heads K3
        // writes the representative's P = 1 planes 4 floats apart: c_raw [n][4].
        const int rmode = mode & (HNRF_MLP_ARITH_MASK | HNRF_MLP_NO_RANGE_GUARD);
        HNRF_HIP(hipMemsetAsync(rep, 0, 64, st));
        HNRF_HIP(hipMemsetAsync(opt.live_counts, 0, (size_t)nchunk * sizeof(int), st));
        if ((rc = hnrf_nonrigid_fwd_sparse(rep, hann_w, nr_packed, rmode, 1, nullptr, nullptr, rep + 8, rep + 4, st))) return rc;
        if ((rc = opt.n_heads ? hnrf_canonical_heads_fwd_sparse(rep + 8, cnl.packed, rmode, 1, opt.n_heads, nullptr, nullptr,
                                                                rep + 12, st)
                              : hnrf_canonical_fwd_sparse(rep + 8, cnl.packed, rmode, 1, nullptr, nullptr, rep + 12, st)))
            return rc;
    }
    if (two) {
        ev_in = (hipEvent_t)events[0];
        ev_k1[0] = (hipEvent_t)events[1]; ev_k1[1] = (hipEvent_t)events[2];
        ev_done[0] = (hipEvent_t)events[3]; ev_done[1] = (hipEvent_t)events[4];
        HNRF_HIP(hipEventRecord(ev_in, st));                      // the side stream starts behind everything queued so far
        HNRF_HIP(hipStreamWaitEvent(sd, ev_in, 0));
    }
    if ((rc = warp(0))) return rc;
    if (two) HNRF_HIP(hipEventRecord(ev_k1[0], sd));
    for (int64_t i = 0; i < nchunk; ++i) {
        if (i + 1 < nchunk) {                                     // next chunk's K1: its workspace was last read by chunk i-1
            if (two && i >= 1) HNRF_HIP(hipStreamWaitEvent(sd, ev_done[(i + 1) & 1], 0));
            if (two) {
                if ((rc = warp(i + 1))) return rc;
                HNRF_HIP(hipEventRecord(ev_k1[(i + 1) & 1], sd));
            }
        }
        if (two) HNRF_HIP(hipStreamWaitEvent(st, ev_k1[i & 1], 0));
        // f16-range guard (hnrf.h): every chunk, none, or the one chunk the caller's rotating index names
        int cmode = mode & (HNRF_MLP_ARITH_MASK | HNRF_MLP_NO_RANGE_GUARD);
        if ((mode & HNRF_MLP_GUARD_ONE_CHUNK) && (int64_t)((unsigned)mode >> 16) % nchunk != i) cmode |= HNRF_MLP_NO_RANGE_GUARD;
        const Chunk k = chunk_at(i);
        FrameOut po[8] = {k.o};                                   // the planes' rows of this chunk
        for (int g = 1; g < n_planes; ++g) po[g] = opt.head_out[g].rows(i * chunk, S, field.B);
        if ((rc = render_chunk(k.c, k.rays.d, hann_w, nr_packed, off, cnl, bgcolor, cmode, cull_eps, k.R, S,
                               Planes{n_planes, k.raw, po, opt.view_bias ? opt.view_bias + 3 * i * chunk : nullptr},
                               mlp_events ? mlp_events[2 * i] : nullptr, mlp_events ? mlp_events[2 * i + 1] : nullptr, st,
                               Share{share ? &k.sh : nullptr, fused}))) return rc;
        if (two) HNRF_HIP(hipEventRecord(ev_done[i & 1], st));
        if (!two && i + 1 < nchunk && (rc = warp(i + 1))) return rc;   // single stream: plain sequence
    }
#undef HNRF_HIP
    return HNRF_OK;
}
}  // namespace

extern "C" int hnrf_render_frame_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                     const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                     const float* vol, const float* bbox_min, const float* bbox_scale,
                                     const float* hann_w, const void* nr_packed, const void* cnl_packed,
                                     const float* bgcolor, int mode, float cull_eps, int64_t N, int S, int B, int G,
                                     int64_t chunk, void* workspace, size_t workspace_bytes, float* rgb, float* alpha,
                                     float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz,
                                     float* cnl_rgb, float* cnl_weight, float* xyz_on_rays, float* bmw, float* offsets,
                                     void* side_stream, void* const* events, void* const* mlp_events, void* stream) {
    return render_frame("hnrf_render_frame_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                        WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, hann_w, nr_packed, kNoOffGrid,
                        CnlSource{cnl_packed, nullptr, 0, nullptr, nullptr}, bgcolor, mode, cull_eps, N, S, chunk,
                        workspace, workspace_bytes,
                        FrameOut{rgb, alpha, depth, weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight, xyz_on_rays,
                                 bmw, offsets},
                        side_stream, events, mlp_events, stream);
}

// hnrf_render_frame_heads_fwd and -- live_counts -- hnrf_render_frame_heads_shared_fwd: the per-head planes checked and
// bundled, then the frame
static int frame_heads(const char* who, const Rays& rays, const WarpField& field, const float* hann_w, const void* nr_packed,
                       const void* cnl_packed, const float* bgcolor, int mode, float cull_eps, int64_t N, int S,
                       int64_t chunk, int n_heads, void* workspace, size_t workspace_bytes, float* const* rgb,
                       float* const* alpha, float* const* depth, float* const* weights_on_rays, float* const* rgb_on_rays,
                       float* const* cnl_xyz, float* const* cnl_rgb, float* const* cnl_weight, float* xyz_on_rays, float* bmw,
                       float* offsets, int* live_counts, void* side_stream, void* const* events, void* const* mlp_events,
                       void* stream) {
    HNRF_REQUIRE(n_heads >= 2 && n_heads <= 8, HNRF_E_ARG, "%s: n_heads=%d outside 2..8", who, n_heads);
    HNRF_REQUIRE(rgb && alpha && depth, HNRF_E_ARG, "%s: null output array", who);
    const bool diag = weights_on_rays != nullptr;
    HNRF_REQUIRE(!diag || (rgb_on_rays && cnl_xyz && cnl_rgb && cnl_weight && xyz_on_rays && bmw && offsets), HNRF_E_ARG,
                 "%s: the eight diagnostic outputs go together", who);
    FrameOut ho[8];
    for (int g = 0; g < n_heads; ++g) {
        HNRF_REQUIRE(rgb[g] && alpha[g] && depth[g], HNRF_E_ARG, "%s: null rgb / alpha / depth plane of head %d", who, g);
        HNRF_REQUIRE(!diag || (weights_on_rays[g] && rgb_on_rays[g] && cnl_xyz[g] && cnl_rgb[g] && cnl_weight[g]), HNRF_E_ARG,
                     "%s: null diagnostic plane of head %d", who, g);
        ho[g] = diag ? FrameOut{rgb[g], alpha[g], depth[g], weights_on_rays[g], rgb_on_rays[g], cnl_xyz[g], cnl_rgb[g],
                                cnl_weight[g], xyz_on_rays, bmw, offsets}
                     : FrameOut{rgb[g], alpha[g], depth[g], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bmw, nullptr};
    }
    return render_frame(who, rays, field, hann_w, nr_packed, kNoOffGrid, CnlSource{cnl_packed, nullptr, 0, nullptr, nullptr},
                        bgcolor, mode, cull_eps, N, S, chunk, workspace, workspace_bytes, ho[0], side_stream, events,
                        mlp_events, stream, FrameOpts{live_counts, n_heads, ho});
}

extern "C" int hnrf_render_frame_heads_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                           const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                           const float* vol, const float* bbox_min, const float* bbox_scale,
                                           const float* hann_w, const void* nr_packed, const void* cnl_packed,
                                           const float* bgcolor, int mode, float cull_eps, int64_t N, int S, int B, int G,
                                           int64_t chunk, int n_heads, void* workspace, size_t workspace_bytes,
                                           float* const* rgb, float* const* alpha, float* const* depth,
                                           float* const* weights_on_rays, float* const* rgb_on_rays, float* const* cnl_xyz,
                                           float* const* cnl_rgb, float* const* cnl_weight, float* xyz_on_rays, float* bmw,
                                           float* offsets, void* side_stream, void* const* events,
                                           void* const* mlp_events, void* stream) {
    return frame_heads("hnrf_render_frame_heads_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                       WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, hann_w, nr_packed, cnl_packed,
                       bgcolor, mode, cull_eps, N, S, chunk, n_heads, workspace, workspace_bytes, rgb, alpha, depth,
                       weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight, xyz_on_rays, bmw, offsets, nullptr,
                       side_stream, events, mlp_events, stream);
}

extern "C" int hnrf_render_frame_heads_shared_fwd(
    const float* rays_o, const float* rays_d, const float* near, const float* far, const float* t_rand,
    const float* motion_Rs, const float* motion_Ts, const float* vol, const float* bbox_min, const float* bbox_scale,
    const float* hann_w, const void* nr_packed, const void* cnl_packed, const float* bgcolor, int mode, float cull_eps,
    int64_t N, int S, int B, int G, int64_t chunk, int n_heads, void* workspace, size_t workspace_bytes, float* const* rgb,
    float* const* alpha, float* const* depth, float* const* weights_on_rays, float* const* rgb_on_rays,
    float* const* cnl_xyz, float* const* cnl_rgb, float* const* cnl_weight, float* xyz_on_rays, float* bmw, float* offsets,
    int* live_counts, void* side_stream, void* const* events, void* const* mlp_events, void* stream) {
    HNRF_REQUIRE(live_counts, HNRF_E_ARG, "hnrf_render_frame_heads_shared_fwd: null live_counts");
    return frame_heads("hnrf_render_frame_heads_shared_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                       WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, hann_w, nr_packed, cnl_packed,
                       bgcolor, mode, cull_eps, N, S, chunk, n_heads, workspace, workspace_bytes, rgb, alpha, depth,
                       weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight, xyz_on_rays, bmw, offsets, live_counts,
                       side_stream, events, mlp_events, stream);
}

extern "C" int hnrf_render_frame_shared_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                            const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                            const float* vol, const float* bbox_min, const float* bbox_scale,
                                            const float* hann_w, const void* nr_packed, const void* cnl_packed,
                                            const float* bgcolor, int mode, float cull_eps, int64_t N, int S, int B, int G,
                                            int64_t chunk, void* workspace, size_t workspace_bytes, float* rgb, float* alpha,
                                            float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz,
                                            float* cnl_rgb, float* cnl_weight, float* xyz_on_rays, float* bmw, float* offsets,
                                            int* live_counts, void* side_stream, void* const* events,
                                            void* const* mlp_events, void* stream) {
    HNRF_REQUIRE(live_counts, HNRF_E_ARG, "hnrf_render_frame_shared_fwd: null live_counts");
    return render_frame("hnrf_render_frame_shared_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                        WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, hann_w, nr_packed, kNoOffGrid,
                        CnlSource{cnl_packed, nullptr, 0, nullptr, nullptr}, bgcolor, mode, cull_eps, N, S, chunk,
                        workspace, workspace_bytes,
                        FrameOut{rgb, alpha, depth, weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight, xyz_on_rays,
                                 bmw, offsets},
                        side_stream, events, mlp_events, stream, FrameOpts{live_counts});
}

extern "C" int hnrf_render_frame_baked_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                           const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                           const float* vol, const float* bbox_min, const float* bbox_scale,
                                           const float* hann_w, const void* nr_packed, const void* grid, int grid_N,
                                           const float* grid_bbox_min, const float* grid_bbox_max, const float* bgcolor,
                                           int mode, float cull_eps, int64_t N, int S, int B, int G, int64_t chunk,
                                           void* workspace, size_t workspace_bytes, float* rgb, float* alpha,
                                           float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz,
                                           float* cnl_rgb, float* cnl_weight, float* xyz_on_rays, float* bmw,
                                           float* offsets, void* side_stream, void* const* events,
                                           void* const* mlp_events, void* stream) {
    HNRF_REQUIRE(grid, HNRF_E_ARG, "hnrf_render_frame_baked_fwd: null grid");
    return render_frame("hnrf_render_frame_baked_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                        WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, hann_w, nr_packed, kNoOffGrid,
                        CnlSource{nullptr, grid, grid_N, grid_bbox_min, grid_bbox_max}, bgcolor, mode, cull_eps, N, S,
                        chunk, workspace, workspace_bytes,
                        FrameOut{rgb, alpha, depth, weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight, xyz_on_rays,
                                 bmw, offsets},
                        side_stream, events, mlp_events, stream);
}

extern "C" int hnrf_render_frame_baked_nr_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                              const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                              const float* vol, const float* bbox_min, const float* bbox_scale,
                                              const void* off_grid, int off_M, const float* off_bbox_min,
                                              const float* off_bbox_max, const void* grid, int grid_N,
                                              const float* grid_bbox_min, const float* grid_bbox_max, const float* bgcolor,
                                              int mode, float cull_eps, int64_t N, int S, int B, int G, int64_t chunk,
                                              void* workspace, size_t workspace_bytes, float* rgb, float* alpha,
                                              float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz,
                                              float* cnl_rgb, float* cnl_weight, float* xyz_on_rays, float* bmw,
                                              float* offsets, void* side_stream, void* const* events,
                                              void* const* mlp_events, void* stream) {
    HNRF_REQUIRE(off_grid, HNRF_E_ARG, "hnrf_render_frame_baked_nr_fwd: null offset grid");
    HNRF_REQUIRE(grid, HNRF_E_ARG, "hnrf_render_frame_baked_nr_fwd: null grid");
    return render_frame("hnrf_render_frame_baked_nr_fwd", Rays{rays_o, rays_d, near, far, t_rand},
                        WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, nullptr, nullptr,
                        BakedGrid{off_grid, off_M, off_bbox_min, off_bbox_max},
                        CnlSource{nullptr, grid, grid_N, grid_bbox_min, grid_bbox_max}, bgcolor, mode, cull_eps, N, S,
                        chunk, workspace, workspace_bytes,
                        FrameOut{rgb, alpha, depth, weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight, xyz_on_rays,
                                 bmw, offsets},
                        side_stream, events, mlp_events, stream);
}

// The view path's one frame entry (hnrf_view.h): the frame of whichever of the four single-head entries above its nullable
// arguments select, with the per-ray colour bias in every chunk's K4.
extern "C" int hnrf_render_frame_view_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                          const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                          const float* vol, const float* bbox_min, const float* bbox_scale,
                                          const float* hann_w, const void* nr_packed, const void* cnl_packed,
                                          const void* off_grid, int off_M, const float* off_bbox_min,
                                          const float* off_bbox_max, const void* grid, int grid_N,
                                          const float* grid_bbox_min, const float* grid_bbox_max, const float* view_bias,
                                          const float* bgcolor, int mode, float cull_eps, int64_t N, int S, int B, int G,
                                          int64_t chunk, void* workspace, size_t workspace_bytes, float* rgb, float* alpha,
                                          float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz,
                                          float* cnl_rgb, float* cnl_weight, float* xyz_on_rays, float* bmw, float* offsets,
                                          int* live_counts, void* side_stream, void* const* events,
                                          void* const* mlp_events, void* stream) {
    const char* who = "hnrf_render_frame_view_fwd";
    HNRF_REQUIRE(!off_grid || grid, HNRF_E_ARG, "%s: an offset grid needs a canonical grid", who);
    FrameOpts opt;
    opt.live_counts = live_counts;
    opt.view_bias = view_bias;
    return render_frame(who, Rays{rays_o, rays_d, near, far, t_rand},
                        WarpField{motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, B, G}, off_grid ? nullptr : hann_w,
                        off_grid ? nullptr : nr_packed,
                        off_grid ? BakedGrid{off_grid, off_M, off_bbox_min, off_bbox_max} : kNoOffGrid,
                        grid ? CnlSource{nullptr, grid, grid_N, grid_bbox_min, grid_bbox_max}
                             : CnlSource{cnl_packed, nullptr, 0, nullptr, nullptr},
                        bgcolor, mode, cull_eps, N, S, chunk, workspace, workspace_bytes,
                        FrameOut{rgb, alpha, depth, weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight, xyz_on_rays,
                                 bmw, offsets},
                        side_stream, events, mlp_events, stream, opt);
}
