// Shared helpers for libhnrf (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/hnrf.h"

namespace hnrf {

void set_error(const char* fmt, ...);

#define HNRF_REQUIRE(cond, code, ...)            \
    do {                                         \
        if (!(cond)) {                           \
            hnrf::set_error(__VA_ARGS__);        \
            return (code);                       \
        }                                        \
    } while (0)

static inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return HNRF_E_LAUNCH;
    }
    return HNRF_OK;
}

constexpr int kWave = 64;

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Workspace of one ray chunk of R rays x S samples (P = R S), every part 256-byte aligned:
// z_vals[P] | mask[P] | x_skel[3P] | xyz[3P] | raw[4P] | idx[P] | count.  hnrf_render_rays_fwd, each of the two
// slots of hnrf_render_frame_fwd and hnrf_render_rays_term_fwd carve it; `bytes` is its size
// (hnrf_render_workspace_bytes carves from a null base).
struct RenderCarve {
    float *z_vals, *mask, *x_skel, *xyz, *raw;
    int *idx, *count;
    size_t bytes;
};
static inline RenderCarve render_carve(void* base, int64_t R, int S) {
    const size_t P = (size_t)R * (size_t)S;
    size_t o = 0;
    auto take = [&](size_t n) {
        void* p = (void*)((uintptr_t)base + o);
        o += align256(n);
        return p;
    };
    RenderCarve c;
    c.z_vals = (float*)take(P * 4);
    c.mask = (float*)take(P * 4);
    c.x_skel = (float*)take(P * 12);
    c.xyz = (float*)take(P * 12);
    c.raw = (float*)take(P * 16);
    c.idx = (int*)take(P * 4);
    c.count = (int*)take(sizeof(int));
    c.bytes = o;
    return c;
}

// The argument bundles of the render entries: what the C ABI passes as runs of loose pointers, named once.
// A chunk of a frame is rows [r0, r0 + R) of the frame's rays and outputs.
struct Rays {                 // o [N,3], d [N,3], near [N], far [N], t_rand [N,S] or null
    const float *o, *d, *near, *far, *t_rand;
    Rays rows(int64_t r0, int S) const {
        return Rays{o + 3 * r0, d + 3 * r0, near + r0, far + r0, t_rand ? t_rand + r0 * S : nullptr};
    }
};
struct WarpField {            // K1's motion field: B bones, their G^3 weight volume and its bbox
    const float *Rs, *Ts, *vol, *bbox_min, *bbox_scale;
    int B, G;
};
// rgb / alpha / depth and hnrf_render_frame_fwd's eight diagnostic outputs.  weights == null = the lean form: the six
// that follow, xyz and offsets then count as null; bmw is K1's and goes by itself.
struct FrameOut {
    float *rgb, *alpha, *depth;
    float *weights, *rgb_on_rays, *cnl_xyz, *cnl_rgb, *cnl_weight, *xyz, *bmw, *offsets;
    FrameOut rows(int64_t r0, int S, int B) const {
        const bool diag = weights != nullptr;
        auto at = [](float* p, bool on, int64_t off) { return on ? p + off : nullptr; };
        return FrameOut{rgb + 3 * r0, alpha + r0, depth + r0, at(weights, diag, r0 * S), at(rgb_on_rays, diag, r0 * S * 3),
                        at(cnl_xyz, diag, 3 * r0), at(cnl_rgb, diag, 3 * r0), at(cnl_weight, diag, r0),
                        at(xyz, diag, r0 * S * 3), at(bmw, bmw != nullptr, r0 * S * B), at(offsets, diag, r0 * S * 3)};
    }
};

// hnrf_sample_warp_fwd (hnrf_sample_warp.hip) on the bundles, R rays of S samples.  sh != null: the fused
// classification, hnrf_sample_warp_share_fwd without the argument checks of the share part and without zeroing
// *sh->count (f.B must be 24: the caller's to check).
struct ShareOut;              // hnrf_block_scan.h
int sample_warp(const Rays& rays, const WarpField& f, int64_t R, int S, float* z_vals, float* x_skel, float* fg_mask,
                float* bmw, const ShareOut* sh, hipStream_t st);

// hnrf_share_compact (hnrf_sample_warp.hip) without the argument checks and without zeroing *sh.count: the frame entry
// zeroes its per-chunk counts once.
int share_compact(const float* x_skel, int64_t P, const ShareOut& sh, hipStream_t st);

// Opt a kernel into > 64 KiB of dynamic LDS, once per device of this process (`done`: one bit per device id;
// the attribute is per device, and a process may drive more than one).
static inline int reserve_lds(const void* fn, int bytes, unsigned long long& done, const char* what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done & bit) return HNRF_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        set_error("%s: cannot reserve %d bytes of LDS", what, bytes);
        return HNRF_E_LAUNCH;
    }
    done |= bit;
    return HNRF_OK;
}

// Launch of kernel K with `lds` bytes of dynamic LDS, > 64 KiB allowed: owns K's per-device mask for reserve_lds (one per
// kernel instance: a function-local static of the template).  LDS_MAX: the size reserved where launches differ in size.
template <auto K, int LDS_MAX = 0, typename... Args>
static inline int launch_lds(const char* what, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    static unsigned long long done = 0;
    if (int rc = reserve_lds((const void*)K, LDS_MAX ? LDS_MAX : (int)lds, done, what)) return rc;
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    return check_launch(what);
}
// A kernel instance as a value, for a generic lambda that states one launch's arguments once and is called with the
// instance chosen at run time: launch_lds<decltype(k)::value>(...).
template <auto K>
struct Kernel {
    static constexpr auto value = K;
};

// The N^3 lattice of hnrf_density_grid and hnrf_bake_canonical (hnrf_mesh.hip): positions of the lattice points
// p0 .. p0 + cnt - 1 ([z][y][x], x fastest) -> xyz [cnt,3]; both walk it in chunks of kLatticeChunk points per
// canonical-MLP launch (56 MiB of workspace).
constexpr int64_t kLatticeChunk = 1 << 21;
int lattice_points(const float* bmin, const float* bmax, int N, int64_t p0, int64_t cnt, float* xyz, hipStream_t st);

// Baked canonical grid (hnrf_baked.hip): raw[p] = the grid sampled at xyz[p]; idx / count null = every p < P, else
// the samples idx[0 .. *count).  Arguments are the caller's to check.
int baked_sample(const float* xyz, const void* grid, int N, const float* bmin, const float* bmax, int64_t P,
                 const int* idx, const int* count, float* raw, hipStream_t st);

// Baked offset field + baked canonical grid in one kernel (hnrf_baked.hip): raw[p] = cnl sampled at x_skel[p] + the
// offset grid sampled at x_skel[p]; xyz / offsets nullable; idx / count as above.  Arguments are the caller's to check.
struct BakedGrid {
    const void* grid;
    int N;
    const float *bmin, *bmax;
};
int baked_warp_sample(const float* x_skel, const BakedGrid& off, const BakedGrid& cnl, int64_t P, const int* idx,
                      const int* count, float* raw, float* xyz, float* offsets, hipStream_t st);

// HNRF_MLP_F16X3 back end (hnrf_mlp_f16.hip)
size_t canonical16_bytes();
size_t nonrigid16_bytes();
size_t canonical16_status_offset();
size_t nonrigid16_status_offset();
int canonical16_pack(const float* const* w, const float* const* b, void* packed, hipStream_t st, int n_heads = 1);
int nonrigid16_pack(const float* const* w, const float* const* b, const float* cond, void* packed, hipStream_t st);
// n_heads >= 2: the all-heads instances on a multi-head image, raw / d_raw [n_heads][P][4]
int canonical16_fwd(const float* xyz, const void* packed, int64_t P, float* raw, const int* idx, const int* count,
                    bool guard, hipStream_t st, int n_heads = 1);
int canonical16_fwd_train(const float* xyz, const void* packed, int64_t P, float* raw, float* pe_out, float* acts,
                          uint32_t* relu_bits, int half, hipStream_t st, int n_heads = 1);
int nonrigid16_fwd(const float* x_skel, const float* hann_w, const void* packed, int64_t P, float* xyz,
                   float* offsets, const int* idx, const int* count, bool guard, hipStream_t st);

int nonrigid16_fwd_train(const float* x_skel, const float* hann_w, const void* packed, int64_t P, float* xyz,
                         float* offsets, float* pe_out, float* acts, uint32_t* relu_bits, int half, hipStream_t st);

size_t canonical16_bwd_bytes(int n_heads = 1);
int canonical16_bwd_pack(const float* const* w, void* packed, hipStream_t st, int n_heads = 1);
int canonical16_bwd(const float* xyz, const float* d_raw, const uint32_t* relu_bits, const void* packed, int64_t P,
                    const float* d_raw_amax, float* dZ, float* d_xyz, float* dz_amax, int half, hipStream_t st,
                    int n_heads = 1);

size_t nonrigid16_bwd_bytes();
int nonrigid16_bwd_pack(const float* const* w, void* packed, hipStream_t st);
int nonrigid16_bwd(const float* x_skel, const float* hann_w, const float* d_xyz, const uint32_t* relu_bits,
                   const void* packed, int64_t P, const float* d_xyz_amax, float* dZ, float* d_x_skel, float* dz_amax,
                   int half, hipStream_t st);

}  // namespace hnrf
