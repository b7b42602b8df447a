// PSNR and SSIM of 8-bit image pairs on the device (hnrf.h "Image metrics"): what MetricsWriter.append does per frame
// on the host through compute_psnr / compute_ssim (core/utils/metrics_util.py:78-106; humannerf_amd/render.py psnr,
// ssim), on the uint8 images that render.unpack_to_image leaves on the device.
//
// The inputs are 8-bit, so everything up to the closed-form expression is exact integer arithmetic: a 7x7 window sum
// of x, y, x^2, y^2 or xy is at most 49 * 255^2 = 3 186 225 (int32), the squared error of a whole 8192^2 x 3 image at
// most 1.3e13 (uint64).  Floating point enters per window, in fp64, in the operand order of render.ssim, with
// contraction OFF (the Makefile compiles this file with -ffp-contract=off): render.metrics_u8 is the numpy statement
// of the same arithmetic, and a window's value has the same bits on both sides.  Only the order in which the window
// values are added differs (here: 4 rows per lane, a tree over the 256 lanes, the tiles in index order; numpy: pairwise).
// No atomics, every sum in a fixed order: two runs give the same bits, and image n's values do not depend on the batch.
//
// Four launches on the caller's stream, nothing read back:
//   1 metrics_sse_kernel   per image <= 256 workgroups stride over the pixels: squared error (uint64), number of pixels
//                          inside the mask and their bounding box, one partial per workgroup
//   2 metrics_box_kernel   one workgroup per image folds the box partials: x0 y0 x1 y1 (exclusive) count -> workspace
//   3 metrics_ssim_kernel  one workgroup per 32x32 tile of window positions and image; tiles outside the crop exit
//   4 metrics_final_kernel one workgroup per image adds the partials and writes psnr, ssim
// Memory-trivial (1.5 MB read per 512^2 pair, twice): the point is that the pixels stay on the device.
#include "hnrf_common.h"

namespace hnrf {

constexpr int kMetricsMaxSide = 8192;
constexpr int kRedBlocks = 256;          // first-level partials per image
constexpr int kWin = 7;
constexpr int kTile = 32;                // window positions per tile side
constexpr int kHalo = kTile + kWin - 1;  // 38 pixel rows / columns under a tile
constexpr int kPitch = 40;               // bytes per pixel row in LDS

// Workspace, every part 256-byte aligned: sse_part [n][256] u64 | box_part [n][256][8] i32 | box [n][8] i32 |
// ssim_part [n][3][gy][gx] f64, gx x gy = the tiles of the window positions of the WHOLE image.
struct MetricsCarve {
    unsigned long long* sse_part;
    int *box_part, *box;
    double* ssim_part;
    int gx, gy;
    size_t bytes;
};
static inline MetricsCarve metrics_carve(void* base, int n, int H, int W) {
    size_t o = 0;
    auto take = [&](size_t bytes) {
        void* p = (void*)((uintptr_t)base + o);
        o += align256(bytes);
        return p;
    };
    MetricsCarve c;
    c.gx = W >= kWin ? (W - kWin + 1 + kTile - 1) / kTile : 0;
    c.gy = H >= kWin ? (H - kWin + 1 + kTile - 1) / kTile : 0;
    c.sse_part = (unsigned long long*)take((size_t)n * kRedBlocks * 8);
    c.box_part = (int*)take((size_t)n * kRedBlocks * 8 * 4);
    c.box = (int*)take((size_t)n * 8 * 4);
    c.ssim_part = (double*)take((size_t)n * 3 * c.gx * c.gy * 8);
    c.bytes = o;
    return c;
}

// ---- 1: squared error, mask count and bounding box; mask null = every pixel is inside
__global__ __launch_bounds__(256) void metrics_sse_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, int H, int W,
                                                          unsigned long long* __restrict__ sse_part,
                                                          int* __restrict__ box_part) {
    __shared__ unsigned long long s_sse[256];
    __shared__ int s_box[5][256];
    const int img = blockIdx.y, tid = threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* p = pred + (int64_t)img * HW * 3;
    const uint8_t* t = target + (int64_t)img * HW * 3;
    const uint8_t* m = mask ? mask + (int64_t)img * HW : nullptr;
    unsigned long long sse = 0;
    int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < HW; i += (int64_t)gridDim.x * 256) {
        if (m && !m[i]) continue;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        const int d0 = (int)p[i * 3] - (int)t[i * 3], d1 = (int)p[i * 3 + 1] - (int)t[i * 3 + 1];
        const int d2 = (int)p[i * 3 + 2] - (int)t[i * 3 + 2];
        sse += (unsigned)(d0 * d0 + d1 * d1 + d2 * d2);
        ++cnt;
        x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
    }
    s_sse[tid] = sse;
    s_box[0][tid] = x0; s_box[1][tid] = y0; s_box[2][tid] = x1; s_box[3][tid] = y1; s_box[4][tid] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            s_sse[tid] += s_sse[tid + s];
            s_box[0][tid] = min(s_box[0][tid], s_box[0][tid + s]);
            s_box[1][tid] = min(s_box[1][tid], s_box[1][tid + s]);
            s_box[2][tid] = max(s_box[2][tid], s_box[2][tid + s]);
            s_box[3][tid] = max(s_box[3][tid], s_box[3][tid + s]);
            s_box[4][tid] += s_box[4][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o = (int64_t)img * kRedBlocks + blockIdx.x;
        sse_part[o] = s_sse[0];
        for (int k = 0; k < 5; ++k) box_part[o * 8 + k] = s_box[k][0];
    }
}

// ---- 2: the crop of the image = cv2.boundingRect of the mask's non-zero pixels; empty mask -> an empty box
__global__ __launch_bounds__(256) void metrics_box_kernel(const int* __restrict__ box_part, int nb, int* __restrict__ box) {
    __shared__ int s_box[5][256];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int* q = box_part + ((int64_t)img * kRedBlocks + tid) * 8;
    const bool in = tid < nb;
    s_box[0][tid] = in ? q[0] : 0x7fffffff; s_box[1][tid] = in ? q[1] : 0x7fffffff;
    s_box[2][tid] = in ? q[2] : -1; s_box[3][tid] = in ? q[3] : -1; s_box[4][tid] = in ? q[4] : 0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            s_box[0][tid] = min(s_box[0][tid], s_box[0][tid + s]);
            s_box[1][tid] = min(s_box[1][tid], s_box[1][tid + s]);
            s_box[2][tid] = max(s_box[2][tid], s_box[2][tid + s]);
            s_box[3][tid] = max(s_box[3][tid], s_box[3][tid + s]);
            s_box[4][tid] += s_box[4][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool any = s_box[4][0] > 0;
        int* b = box + img * 8;
        b[0] = any ? s_box[0][0] : 0; b[1] = any ? s_box[1][0] : 0;
        b[2] = any ? s_box[2][0] + 1 : 0; b[3] = any ? s_box[3][0] + 1 : 0;
        b[4] = s_box[4][0];
    }
}

// One window from its integer moments: render.ssim's lines for ux .. s, operand for operand.  The means are the sums
// over 49 * 255 (pixels k / 255), the second moments over 49 * 255^2; one rounding each.
__device__ __forceinline__ double ssim_window(int sx, int sy, int sxx, int syy, int sxy, double c1, double c2) {
    const double ux = (double)sx / 12495.0, uy = (double)sy / 12495.0;
    const double uxx = (double)sxx / 3186225.0, uyy = (double)syy / 3186225.0, uxy = (double)sxy / 3186225.0;
    const double cov_norm = 49.0 / 48.0;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    return ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
}

// ---- 3: a 32x32 tile of window positions of the crop: 38x38 haloed pixels of both images and all three channels into
// LDS, then per channel the horizontal 7-sums of x, y, x^2, y^2, xy (int32, LDS), the vertical 7-sums from there (each
// lane slides down 4 rows of one column: lanes of a wave read consecutive dwords), the fp64 expression, and one partial.
__global__ __launch_bounds__(256) void metrics_ssim_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target,
                                                           int H, int W, const int* __restrict__ box, double c1, double c2,
                                                           double* __restrict__ ssim_part) {
    __shared__ uint8_t pix[2][3][kHalo * kPitch];
    __shared__ int hs[5][kHalo][kTile];
    __shared__ double red[256];
    const int img = blockIdx.z, tid = threadIdx.x;
    const int* b = box + img * 8;
    const int bx0 = b[0], by0 = b[1];
    const int npx = b[2] - bx0 - (kWin - 1), npy = b[3] - by0 - (kWin - 1);   // window positions of the crop
    const int px0 = blockIdx.x * kTile, py0 = blockIdx.y * kTile;
    if (npx < 1 || npy < 1 || px0 >= npx || py0 >= npy) return;
    const int tw = min(kTile, npx - px0), th = min(kTile, npy - py0);
    const int rows = th + kWin - 1, rowbytes = (tw + kWin - 1) * 3;           // all inside the crop, hence the image
    const int64_t HW3 = (int64_t)H * W * 3;
    const uint8_t* p = pred + (int64_t)img * HW3 + ((int64_t)(by0 + py0) * W + bx0 + px0) * 3;
    const uint8_t* t = target + (int64_t)img * HW3 + ((int64_t)(by0 + py0) * W + bx0 + px0) * 3;
    for (int k = tid; k < rows * rowbytes; k += 256) {
        const int r = k / rowbytes, j = k - r * rowbytes;
        const int col = j / 3, c = j - col * 3;
        const int64_t g = (int64_t)r * W * 3 + j;
        pix[0][c][r * kPitch + col] = p[g];
        pix[1][c][r * kPitch + col] = t[g];
    }
    __syncthreads();
    const int tx = tid & (kTile - 1), r0 = (tid >> 5) * 4;
    for (int c = 0; c < 3; ++c) {
        for (int k = tid; k < rows * kTile; k += 256) {
            const int r = k >> 5, x = k & (kTile - 1);
            if (x >= tw) continue;
            const uint8_t* px = &pix[0][c][r * kPitch + x];
            const uint8_t* py = &pix[1][c][r * kPitch + x];
            int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int i = 0; i < kWin; ++i) {
                const int a = px[i], d = py[i];
                sx += a; sy += d; sxx += a * a; syy += d * d; sxy += a * d;
            }
            hs[0][r][x] = sx; hs[1][r][x] = sy; hs[2][r][x] = sxx; hs[3][r][x] = syy; hs[4][r][x] = sxy;
        }
        __syncthreads();
        double acc = 0.0;
        if (tx < tw && r0 < th) {
            int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
            for (int i = 0; i < kWin; ++i) {
                s0 += hs[0][r0 + i][tx]; s1 += hs[1][r0 + i][tx]; s2 += hs[2][r0 + i][tx];
                s3 += hs[3][r0 + i][tx]; s4 += hs[4][r0 + i][tx];
            }
            acc = ssim_window(s0, s1, s2, s3, s4, c1, c2);
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                if (r0 + q < th) {
                    const int lo = r0 + q - 1, hi = r0 + q + kWin - 1;
                    s0 += hs[0][hi][tx] - hs[0][lo][tx]; s1 += hs[1][hi][tx] - hs[1][lo][tx];
                    s2 += hs[2][hi][tx] - hs[2][lo][tx]; s3 += hs[3][hi][tx] - hs[3][lo][tx];
                    s4 += hs[4][hi][tx] - hs[4][lo][tx];
                    acc = acc + ssim_window(s0, s1, s2, s3, s4, c1, c2);
                }
            }
        }
        red[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] = red[tid] + red[tid + s];
            __syncthreads();
        }
        if (tid == 0)
            ssim_part[(((int64_t)img * 3 + c) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
        __syncthreads();                                                     // hs and red are written again
    }
}

// ---- 4: psnr = -10 log10(SSE / (255^2 count)), ssim = mean over the channels of the mean over the window positions
__global__ __launch_bounds__(256) void metrics_final_kernel(const unsigned long long* __restrict__ sse_part, int nb,
                                                            const int* __restrict__ box, const double* __restrict__ ssim_part,
                                                            int gx, int gy, double* __restrict__ out) {
    __shared__ unsigned long long s_sse[256];
    __shared__ double red[256];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int* b = box + img * 8;
    const int npx = b[2] - b[0] - (kWin - 1), npy = b[3] - b[1] - (kWin - 1);
    s_sse[tid] = tid < nb ? sse_part[(int64_t)img * kRedBlocks + tid] : 0ull;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) s_sse[tid] += s_sse[tid + s];
        __syncthreads();
    }
    double mean[3] = {0.0, 0.0, 0.0};
    const bool has = npx >= 1 && npy >= 1;
    if (has) {
        const int ntx = (npx + kTile - 1) / kTile, nty = (npy + kTile - 1) / kTile;   // the tiles that wrote a partial
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double* part = ssim_part + ((int64_t)img * 3 + c) * gy * gx;
            double acc = 0.0;
            for (int k = tid; k < ntx * nty; k += 256) {
                const int ty = k / ntx, tx = k - ty * ntx;
                acc = acc + part[(int64_t)ty * gx + tx];
            }
            red[tid] = acc;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (tid < s) red[tid] = red[tid] + red[tid + s];
                __syncthreads();
            }
            mean[c] = red[0] / (double)((int64_t)npx * npy);
            __syncthreads();
        }
    }
    if (tid == 0) {
        const double mse = (double)s_sse[0] / (65025.0 * (double)(3 * (int64_t)b[4]));   // 0 / 0 = NaN on an empty mask
        out[img * 2] = -10.0 * log10(mse);                                             // equal images: +inf
        out[img * 2 + 1] = has ? ((mean[0] + mean[1]) + mean[2]) / 3.0 : __builtin_nan("");
    }
}

}  // namespace hnrf

using namespace hnrf;

static bool metrics_sizes_ok(int n_img, int H, int W) {
    return n_img >= 1 && n_img <= 65535 && H >= 1 && W >= 1 && H <= kMetricsMaxSide && W <= kMetricsMaxSide;
}

extern "C" size_t hnrf_image_metrics_workspace_bytes(int n_img, int H, int W) {
    if (!metrics_sizes_ok(n_img, H, W)) return 0;
    return metrics_carve(nullptr, n_img, H, W).bytes;
}

extern "C" int hnrf_image_metrics(const uint8_t* pred, const uint8_t* target, const uint8_t* mask, int n_img, int H, int W,
                                  double data_range, void* workspace, size_t workspace_bytes, double* out, void* stream) {
    HNRF_REQUIRE(pred && target && workspace && out, HNRF_E_ARG, "hnrf_image_metrics: null pointer");
    HNRF_REQUIRE(metrics_sizes_ok(n_img, H, W), HNRF_E_UNSUPPORTED,
                 "hnrf_image_metrics: %d images of %dx%d (1 <= n_img <= 65535, 1 <= H, W <= %d)", n_img, H, W, kMetricsMaxSide);
    HNRF_REQUIRE(data_range > 0.0 && data_range <= 1e150, HNRF_E_UNSUPPORTED, "hnrf_image_metrics: data_range %g", data_range);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out & 7) == 0, HNRF_E_ARG,
                 "hnrf_image_metrics: workspace must be 256-byte aligned, out 8-byte aligned");
    const MetricsCarve c = metrics_carve(workspace, n_img, H, W);
    HNRF_REQUIRE(workspace_bytes >= c.bytes, HNRF_E_WORKSPACE, "hnrf_image_metrics: workspace of %zu bytes, %zu needed",
                 workspace_bytes, c.bytes);
    hipStream_t st = (hipStream_t)stream;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    const int64_t HW = (int64_t)H * W;
    const int nb = (int)((HW + 255) / 256 < kRedBlocks ? (HW + 255) / 256 : kRedBlocks);
    hipLaunchKernelGGL(metrics_sse_kernel, dim3(nb, n_img), dim3(256), 0, st, pred, target, mask, H, W, c.sse_part, c.box_part);
    hipLaunchKernelGGL(metrics_box_kernel, dim3(n_img), dim3(256), 0, st, c.box_part, nb, c.box);
    if (c.gx > 0 && c.gy > 0)
        hipLaunchKernelGGL(metrics_ssim_kernel, dim3(c.gx, c.gy, n_img), dim3(256), 0, st, pred, target, H, W, c.box, c1, c2,
                           c.ssim_part);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(n_img), dim3(256), 0, st, c.sse_part, nb, c.box, c.ssim_part, c.gx, c.gy, out);
    return check_launch("hnrf_image_metrics");
}
