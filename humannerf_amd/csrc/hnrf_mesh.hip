// Mesh extraction of the canonical body: density lattice, marching tetrahedra, forward skinning.
//
// Density lattice (hnrf_density_grid): N^3 points over the canonical bbox, [z][y][x] with x fastest; point (x,y,z) at
// bmin + (float)i * step, step = (bmax - bmin) / (N - 1), every operation rounded on its own (this file is compiled
// with -ffp-contract=off: humannerf_amd/mesh.py restates the positions bit for bit).  Chunk by chunk: a kernel writes
// the points, the canonical MLP launcher (hnrf_canonical_fwd, unchanged) evaluates them, an epilogue writes
// density = relu(sigma) * fg, fg = the sum of the B bone channels of the weight volume, trilinear with the
// grid_sample semantics of K1 (align_corners, zero padding) under the identity motion -- the gate rendering applies
// to alpha (alpha = (1 - exp(-relu(sigma) delta)) * fg_mask, hnrf_composite.hip).
//
// Isosurface (hnrf_mesh_count / hnrf_mesh_emit): marching tetrahedra on the Kuhn decomposition of every cell (six
// tetrahedra around the cell's main diagonal), which needs no case table beyond the 6 x 16 one below and gives a
// watertight, edge-manifold surface wherever it does not meet the lattice boundary (there it stays open).  Every
// lattice point owns the 7 lattice edges to its +x, +y, +z, +xy, +xz, +yz, +xyz neighbours (slots 0..6); a vertex
// sits on each edge whose ends are on different sides of `level` (inside: density > level), vertices ordered by
// (point, slot), triangles by (cell, tetrahedron, triangle).  Counts come from integer block scans, so the output is
// bit-reproducible (no atomics anywhere).
//
// Forward skinning (hnrf_forward_skin): x_o = sum_b w_b(x_c) A_b^-1(x_c) / max(sum_b w_b, 1e-4), the forward
// counterpart of K1's inverse warp on the same volume.
#include <math.h>

#include "hnrf_block_scan.h"
#include "hnrf_trilinear.h"

namespace hnrf {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kDensityChunk = kLatticeChunk;
constexpr int kMaxSkinBones = 128;

// Cell corner c: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Slot s of a point is the edge to its corner kSlotCorner[s].
__constant__ unsigned char c_slot_corner[7] = {1, 2, 4, 3, 5, 6, 7};
// Kuhn tetrahedra: (0, e_a, e_a + e_b, 7) for the permutations (a, b, c) of the axes in lexicographic order.
__constant__ unsigned char c_tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// [tet][inside mask of its 4 corners]: triangle count, and per triangle 3 edges as owner corner * 8 + slot, wound
// counter-clockwise seen from outside (humannerf_amd/mesh.py:tet_table generates both and checks this copy).
__constant__ unsigned char c_tri_count[6][16] = {
    {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0}, {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0},
    {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0}, {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0},
    {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0}, {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0}};
__constant__ unsigned char c_tri_edges[6][16][2][3] = {
    {{{0, 0, 0}, {0, 0, 0}}, {{0, 3, 6}, {0, 0, 0}}, {{0, 13, 9}, {0, 0, 0}}, {{3, 6, 13}, {3, 13, 9}}, {{3, 9, 26}, {0, 0, 0}}, {{0, 26, 6}, {0, 9, 26}}, {{0, 13, 26}, {0, 26, 3}}, {{6, 13, 26}, {0, 0, 0}}, {{6, 26, 13}, {0, 0, 0}}, {{0, 3, 26}, {0, 26, 13}}, {{0, 26, 9}, {0, 6, 26}}, {{3, 26, 9}, {0, 0, 0}}, {{3, 9, 13}, {3, 13, 6}}, {{0, 9, 13}, {0, 0, 0}}, {{0, 6, 3}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}},
    {{{0, 0, 0}, {0, 0, 0}}, {{0, 6, 4}, {0, 0, 0}}, {{0, 10, 13}, {0, 0, 0}}, {{4, 13, 6}, {4, 10, 13}}, {{4, 41, 10}, {0, 0, 0}}, {{0, 6, 41}, {0, 41, 10}}, {{0, 41, 13}, {0, 4, 41}}, {{6, 41, 13}, {0, 0, 0}}, {{6, 13, 41}, {0, 0, 0}}, {{0, 41, 4}, {0, 13, 41}}, {{0, 10, 41}, {0, 41, 6}}, {{4, 10, 41}, {0, 0, 0}}, {{4, 13, 10}, {4, 6, 13}}, {{0, 13, 10}, {0, 0, 0}}, {{0, 4, 6}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}},
    {{{0, 0, 0}, {0, 0, 0}}, {{1, 6, 3}, {0, 0, 0}}, {{1, 16, 20}, {0, 0, 0}}, {{3, 20, 6}, {3, 16, 20}}, {{3, 26, 16}, {0, 0, 0}}, {{1, 6, 26}, {1, 26, 16}}, {{1, 26, 20}, {1, 3, 26}}, {{6, 26, 20}, {0, 0, 0}}, {{6, 20, 26}, {0, 0, 0}}, {{1, 26, 3}, {1, 20, 26}}, {{1, 16, 26}, {1, 26, 6}}, {{3, 16, 26}, {0, 0, 0}}, {{3, 20, 16}, {3, 6, 20}}, {{1, 20, 16}, {0, 0, 0}}, {{1, 3, 6}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}},
    {{{0, 0, 0}, {0, 0, 0}}, {{1, 5, 6}, {0, 0, 0}}, {{1, 20, 18}, {0, 0, 0}}, {{5, 6, 20}, {5, 20, 18}}, {{5, 18, 48}, {0, 0, 0}}, {{1, 48, 6}, {1, 18, 48}}, {{1, 20, 48}, {1, 48, 5}}, {{6, 20, 48}, {0, 0, 0}}, {{6, 48, 20}, {0, 0, 0}}, {{1, 5, 48}, {1, 48, 20}}, {{1, 48, 18}, {1, 6, 48}}, {{5, 48, 18}, {0, 0, 0}}, {{5, 18, 20}, {5, 20, 6}}, {{1, 18, 20}, {0, 0, 0}}, {{1, 6, 5}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}},
    {{{0, 0, 0}, {0, 0, 0}}, {{2, 4, 6}, {0, 0, 0}}, {{2, 35, 32}, {0, 0, 0}}, {{4, 6, 35}, {4, 35, 32}}, {{4, 32, 41}, {0, 0, 0}}, {{2, 41, 6}, {2, 32, 41}}, {{2, 35, 41}, {2, 41, 4}}, {{6, 35, 41}, {0, 0, 0}}, {{6, 41, 35}, {0, 0, 0}}, {{2, 4, 41}, {2, 41, 35}}, {{2, 41, 32}, {2, 6, 41}}, {{4, 41, 32}, {0, 0, 0}}, {{4, 32, 35}, {4, 35, 6}}, {{2, 32, 35}, {0, 0, 0}}, {{2, 6, 4}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}},
    {{{0, 0, 0}, {0, 0, 0}}, {{2, 6, 5}, {0, 0, 0}}, {{2, 33, 35}, {0, 0, 0}}, {{5, 35, 6}, {5, 33, 35}}, {{5, 48, 33}, {0, 0, 0}}, {{2, 6, 48}, {2, 48, 33}}, {{2, 48, 35}, {2, 5, 48}}, {{6, 48, 35}, {0, 0, 0}}, {{6, 35, 48}, {0, 0, 0}}, {{2, 48, 5}, {2, 35, 48}}, {{2, 33, 48}, {2, 48, 6}}, {{5, 33, 48}, {0, 0, 0}}, {{5, 35, 33}, {5, 6, 35}}, {{2, 35, 33}, {0, 0, 0}}, {{2, 5, 6}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}}};

__device__ __forceinline__ float lattice_step(float lo, float hi, int N) { return (hi - lo) / (float)(N - 1); }

// ---- density lattice -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void lattice_points_kernel(const float* __restrict__ bmin,
                                                                  const float* __restrict__ bmax, int N, int64_t p0,
                                                                  int64_t cnt, float* __restrict__ xyz) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= cnt) return;
    const int64_t p = p0 + i;
    const int x = (int)(p % N), y = (int)((p / N) % N), z = (int)(p / ((int64_t)N * N));
    xyz[3 * i + 0] = bmin[0] + (float)x * lattice_step(bmin[0], bmax[0], N);
    xyz[3 * i + 1] = bmin[1] + (float)y * lattice_step(bmin[1], bmax[1], N);
    xyz[3 * i + 2] = bmin[2] + (float)z * lattice_step(bmin[2], bmax[2], N);
}

__global__ __launch_bounds__(kThreads) void density_epilogue_kernel(
    const float4* __restrict__ raw, const float* __restrict__ xyz, const float* __restrict__ vol, int B, int G,
    const float* __restrict__ bbox_min, const float* __restrict__ bbox_scale, int64_t p0, int64_t cnt,
    float* __restrict__ density, float* __restrict__ sigma_out, float* __restrict__ fg_out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= cnt) return;
    const Trilinear t = trilinear_at(xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], bbox_min, bbox_scale, G);
    const size_t chan = (size_t)G * G * G;
    float fg = 0.f;
    for (int b = 0; b < B; ++b) fg += trilinear_channel(t, vol + b * chan);
    const float sigma = raw[i].w;
    density[p0 + i] = (sigma > 0.f ? sigma : 0.f) * fg;
    if (sigma_out) sigma_out[p0 + i] = sigma;
    if (fg_out) fg_out[p0 + i] = fg;
}

// ---- marching tetrahedra -------------------------------------------------------------------------------------------
struct Cell {
    unsigned inside;    // bit c: corner c of the cell at p is inside (corners outside the lattice: 0)
    unsigned valid;     // bit c: corner c exists
};

__device__ __forceinline__ Cell load_cell(const float* __restrict__ d, float level, int N, int64_t p, int x, int y, int z) {
    Cell c = {0u, 0u};
    const int64_t NN = (int64_t)N * N;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = (k >> 2) & 1;
        if (x + dx < N && y + dy < N && z + dz < N) {
            c.valid |= 1u << k;
            if (d[p + dz * NN + dy * N + dx] > level) c.inside |= 1u << k;
        }
    }
    return c;
}

__device__ __forceinline__ unsigned edge_flags(const Cell& c) {
    unsigned f = 0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int k = c_slot_corner[s];
        if (((c.valid >> k) & 1u) && (((c.inside >> k) ^ c.inside) & 1u)) f |= 1u << s;
    }
    return f;
}

__device__ __forceinline__ int cell_triangles(const Cell& c) {
    if (c.valid != 0xffu) return 0;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned m = ((c.inside >> c_tet[k][0]) & 1u) | (((c.inside >> c_tet[k][1]) & 1u) << 1) |
                           (((c.inside >> c_tet[k][2]) & 1u) << 2) | (((c.inside >> c_tet[k][3]) & 1u) << 3);
        n += c_tri_count[k][m];
    }
    return n;
}

// word[p] = (exclusive prefix of the block's vertex counts at p) << 8 | edge flags of p; per block: vertex and
// triangle totals.
__global__ __launch_bounds__(kThreads) void mesh_count_kernel(const float* __restrict__ d, float level, int N, int64_t M,
                                                              uint32_t* __restrict__ word, int* __restrict__ blk_v,
                                                              int* __restrict__ blk_t) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned flags = 0;
    int nt = 0;
    if (p < M) {
        const int x = (int)(p % N), y = (int)((p / N) % N), z = (int)(p / ((int64_t)N * N));
        const Cell c = load_cell(d, level, N, p, x, y, z);
        flags = edge_flags(c);
        nt = cell_triangles(c);
    }
    int tot_v, tot_t;
    const int before = block_exclusive_scan(__popc(flags), &tot_v);
    (void)block_exclusive_scan(nt, &tot_t);
    if (p < M) word[p] = ((uint32_t)before << 8) | flags;
    if (threadIdx.x == 0) {
        blk_v[blockIdx.x] = tot_v;
        blk_t[blockIdx.x] = tot_t;
    }
}

// One block: exclusive scan of the per-block totals -> per-block bases (int64), counts = {V, F}.
__global__ __launch_bounds__(1024) void mesh_scan_blocks_kernel(const int* __restrict__ blk_v, const int* __restrict__ blk_t,
                                                                int64_t nblk, int64_t* __restrict__ base_v,
                                                                int64_t* __restrict__ base_t, int64_t* __restrict__ counts) {
    __shared__ int64_t part[2][1024 / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int64_t run_v = 0, run_t = 0;
    for (int64_t off = 0; off < nblk; off += 1024) {
        const int64_t i = off + threadIdx.x;
        const int64_t v = i < nblk ? blk_v[i] : 0, t = i < nblk ? blk_t[i] : 0;
        int64_t iv = v, it = t;
#pragma unroll
        for (int dd = 1; dd < kWave; dd <<= 1) {
            const int64_t uv = __shfl_up(iv, dd, kWave), ut = __shfl_up(it, dd, kWave);
            if (lane >= dd) { iv += uv; it += ut; }
        }
        if (lane == kWave - 1) { part[0][wave] = iv; part[1][wave] = it; }
        __syncthreads();
        int64_t bv = 0, bt = 0, sv = 0, st = 0;
        for (int w = 0; w < 1024 / kWave; ++w) {
            if (w < wave) { bv += part[0][w]; bt += part[1][w]; }
            sv += part[0][w];
            st += part[1][w];
        }
        __syncthreads();
        if (i < nblk) {
            base_v[i] = run_v + bv + iv - v;
            base_t[i] = run_t + bt + it - t;
        }
        run_v += sv;
        run_t += st;
    }
    if (threadIdx.x == 0) {
        counts[0] = run_v;
        counts[1] = run_t;
    }
}

__global__ __launch_bounds__(kThreads) void mesh_emit_kernel(
    const float* __restrict__ d, float level, const float* __restrict__ bmin, const float* __restrict__ bmax, int N,
    int64_t M, const uint32_t* __restrict__ word, const int64_t* __restrict__ base_v, const int64_t* __restrict__ base_t,
    int64_t V, int64_t F, float* __restrict__ verts, int* __restrict__ faces) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t NN = (int64_t)N * N;
    int x = 0, y = 0, z = 0, nt = 0;
    Cell c = {0u, 0u};
    if (p < M) {
        x = (int)(p % N); y = (int)((p / N) % N); z = (int)(p / NN);
        c = load_cell(d, level, N, p, x, y, z);
        nt = cell_triangles(c);
    }
    int tot_t;
    const int tri_before = block_exclusive_scan(nt, &tot_t);
    if (p >= M) return;
    const uint32_t w = word[p];
    const unsigned flags = w & 0x7fu;
    if (flags) {
        const float sx = lattice_step(bmin[0], bmax[0], N), sy = lattice_step(bmin[1], bmax[1], N),
                    sz = lattice_step(bmin[2], bmax[2], N);
        const float ax = bmin[0] + (float)x * sx, ay = bmin[1] + (float)y * sy, az = bmin[2] + (float)z * sz;
        const float da = d[p];
        int64_t vid = base_v[blockIdx.x] + (int64_t)(w >> 8);
        for (int s = 0; s < 7; ++s) {
            if (!((flags >> s) & 1u)) continue;
            const int k = c_slot_corner[s];
            const int dx = k & 1, dy = (k >> 1) & 1, dz = (k >> 2) & 1;
            const float db = d[p + dz * NN + dy * N + dx];
            const float t = (level - da) / (db - da);
            const float bx = bmin[0] + (float)(x + dx) * sx, by = bmin[1] + (float)(y + dy) * sy,
                        bz = bmin[2] + (float)(z + dz) * sz;
            if (vid < V) {
                verts[3 * vid + 0] = ax + t * (bx - ax);
                verts[3 * vid + 1] = ay + t * (by - ay);
                verts[3 * vid + 2] = az + t * (bz - az);
            }
            ++vid;
        }
    }
    if (nt == 0) return;
    int64_t fid = base_t[blockIdx.x] + tri_before;
    for (int k = 0; k < 6; ++k) {
        const unsigned m = ((c.inside >> c_tet[k][0]) & 1u) | (((c.inside >> c_tet[k][1]) & 1u) << 1) |
                           (((c.inside >> c_tet[k][2]) & 1u) << 2) | (((c.inside >> c_tet[k][3]) & 1u) << 3);
        for (int j = 0; j < c_tri_count[k][m]; ++j, ++fid) {
            int ids[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const unsigned code = c_tri_edges[k][m][j][e];
                const unsigned u = code >> 3, s = code & 7u;
                const int64_t q = p + (int64_t)((u >> 2) & 1u) * NN + ((u >> 1) & 1u) * N + (u & 1u);
                const uint32_t wq = word[q];
                ids[e] = (int)(base_v[q / kThreads] + (int64_t)(wq >> 8) + __popc((wq & 0x7fu) & ((1u << s) - 1u)));
            }
            if (fid < F) {
                faces[3 * fid + 0] = ids[0];
                faces[3 * fid + 1] = ids[1];
                faces[3 * fid + 2] = ids[2];
            }
        }
    }
}

// ---- forward skinning ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void forward_skin_kernel(
    const float* __restrict__ verts, int64_t V, const float* __restrict__ Rs, const float* __restrict__ Ts,
    const float* __restrict__ vol, int B, int G, const float* __restrict__ bbox_min,
    const float* __restrict__ bbox_scale, float* __restrict__ out) {
    __shared__ float inv[kMaxSkinBones * 12];          // per bone: R_b^-1 (row-major 3x3) | T_b
    for (int b = threadIdx.x; b < B; b += kThreads) {
        const float* R = Rs + 9 * b;
        const float c00 = R[4] * R[8] - R[5] * R[7], c01 = R[5] * R[6] - R[3] * R[8], c02 = R[3] * R[7] - R[4] * R[6];
        const float det = R[0] * c00 + R[1] * c01 + R[2] * c02;
        const float r = 1.0f / det;
        float* o = inv + 12 * b;
        o[0] = c00 * r; o[1] = (R[2] * R[7] - R[1] * R[8]) * r; o[2] = (R[1] * R[5] - R[2] * R[4]) * r;
        o[3] = c01 * r; o[4] = (R[0] * R[8] - R[2] * R[6]) * r; o[5] = (R[2] * R[3] - R[0] * R[5]) * r;
        o[6] = c02 * r; o[7] = (R[1] * R[6] - R[0] * R[7]) * r; o[8] = (R[0] * R[4] - R[1] * R[3]) * r;
        o[9] = Ts[3 * b + 0]; o[10] = Ts[3 * b + 1]; o[11] = Ts[3 * b + 2];
    }
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const float px = verts[3 * v + 0], py = verts[3 * v + 1], pz = verts[3 * v + 2];
    const Trilinear t = trilinear_at(px, py, pz, bbox_min, bbox_scale, G);
    const size_t chan = (size_t)G * G * G;
    float wsum = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    for (int b = 0; b < B; ++b) {
        const float w = trilinear_channel(t, vol + b * chan);
        const float* o = inv + 12 * b;
        const float ex = px - o[9], ey = py - o[10], ez = pz - o[11];
        const float qx = fmaf(o[2], ez, fmaf(o[1], ey, o[0] * ex));
        const float qy = fmaf(o[5], ez, fmaf(o[4], ey, o[3] * ex));
        const float qz = fmaf(o[8], ez, fmaf(o[7], ey, o[6] * ex));
        wsum += w;
        ax += w * qx;
        ay += w * qy;
        az += w * qz;
    }
    const float den = fmaxf(wsum, 0.0001f);
    out[3 * v + 0] = ax / den;
    out[3 * v + 1] = ay / den;
    out[3 * v + 2] = az / den;
}

// mesh workspace carve: word[M] u32 | blk_v[nblk] i32 | blk_t[nblk] i32 | base_v[nblk] i64 | base_t[nblk] i64
struct MeshCarve {
    uint32_t* word;
    int *blk_v, *blk_t;
    int64_t *base_v, *base_t;
};

MeshCarve carve_mesh(void* ws, int64_t M) {
    const size_t nblk = (size_t)((M + kThreads - 1) / kThreads);
    char* w = (char*)ws;
    MeshCarve c;
    c.word = (uint32_t*)w;  w += align256((size_t)M * 4);
    c.blk_v = (int*)w;      w += align256(nblk * 4);
    c.blk_t = (int*)w;      w += align256(nblk * 4);
    c.base_v = (int64_t*)w; w += align256(nblk * 8);
    c.base_t = (int64_t*)w;
    return c;
}

}  // namespace

int lattice_points(const float* bmin, const float* bmax, int N, int64_t p0, int64_t cnt, float* xyz, hipStream_t st) {
    hipLaunchKernelGGL(lattice_points_kernel, dim3((unsigned)((cnt + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       bmin, bmax, N, p0, cnt, xyz);
    return check_launch("lattice_points");
}
}  // namespace hnrf

using namespace hnrf;

extern "C" size_t hnrf_density_grid_workspace_bytes(int N) {
    if (N < 8 || N > 512) return 0;
    const int64_t M = (int64_t)N * N * N, C = M < kDensityChunk ? M : kDensityChunk;
    return align256((size_t)C * 12) + align256((size_t)C * 16);
}

extern "C" int hnrf_density_grid(const void* cnl_packed, int mode, const float* vol, int B, int G, const float* bbox_min,
                                 const float* bbox_max, const float* bbox_scale, int N, void* workspace,
                                 size_t workspace_bytes, float* density, float* sigma, float* fg, void* stream) {
    HNRF_REQUIRE(cnl_packed && vol && bbox_min && bbox_max && bbox_scale && workspace && density, HNRF_E_ARG,
                 "hnrf_density_grid: null pointer");
    HNRF_REQUIRE(N >= 8 && N <= 512, HNRF_E_ARG, "hnrf_density_grid: N=%d out of range [8, 512]", N);
    HNRF_REQUIRE(B >= 1 && G >= 2 && G <= 1024, HNRF_E_ARG, "hnrf_density_grid: bad dims B=%d G=%d", B, G);
    const int arith = mode & HNRF_MLP_ARITH_MASK;
    HNRF_REQUIRE(arith == HNRF_MLP_F32 || arith == HNRF_MLP_F16X3, HNRF_E_UNSUPPORTED,
                 "hnrf_density_grid: mode %d not built", arith);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_density_grid: workspace must be 256-byte aligned");
    HNRF_REQUIRE(workspace_bytes >= hnrf_density_grid_workspace_bytes(N), HNRF_E_WORKSPACE,
                 "hnrf_density_grid: workspace %zu < %zu bytes", workspace_bytes, hnrf_density_grid_workspace_bytes(N));
    const int64_t M = (int64_t)N * N * N, C = M < kDensityChunk ? M : kDensityChunk;
    float* xyz = (float*)workspace;
    float* raw = (float*)((char*)workspace + align256((size_t)C * 12));
    hipStream_t st = (hipStream_t)stream;
    for (int64_t p0 = 0; p0 < M; p0 += C) {
        const int64_t cnt = (M - p0 < C) ? M - p0 : C;
        const unsigned blocks = (unsigned)((cnt + kThreads - 1) / kThreads);
        int rc = lattice_points(bbox_min, bbox_max, N, p0, cnt, xyz, st);
        if (rc) return rc;
        // every chunk guarded: a hit ORs HNRF_STATUS_F16_RANGE into the packed image's status word
        if ((rc = hnrf_canonical_fwd(xyz, cnl_packed, arith, cnt, raw, stream))) return rc;
        hipLaunchKernelGGL(density_epilogue_kernel, dim3(blocks), dim3(kThreads), 0, st, (const float4*)raw, xyz, vol, B,
                           G, bbox_min, bbox_scale, p0, cnt, density, sigma, fg);
        if ((rc = check_launch("hnrf_density_grid"))) return rc;
    }
    return HNRF_OK;
}

extern "C" size_t hnrf_mesh_workspace_bytes(int N) {
    if (N < 8 || N > 512) return 0;
    const int64_t M = (int64_t)N * N * N;
    const size_t nblk = (size_t)((M + kThreads - 1) / kThreads);
    return align256((size_t)M * 4) + 2 * align256(nblk * 4) + 2 * align256(nblk * 8);
}

extern "C" int hnrf_mesh_count(const float* density, int N, float level, void* workspace, size_t workspace_bytes,
                               int64_t* counts, void* stream) {
    HNRF_REQUIRE(density && workspace && counts, HNRF_E_ARG, "hnrf_mesh_count: null pointer");
    HNRF_REQUIRE(N >= 8 && N <= 512, HNRF_E_ARG, "hnrf_mesh_count: N=%d out of range [8, 512]", N);
    HNRF_REQUIRE(isfinite(level), HNRF_E_ARG, "hnrf_mesh_count: level must be finite");
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_mesh_count: workspace must be 256-byte aligned");
    HNRF_REQUIRE(workspace_bytes >= hnrf_mesh_workspace_bytes(N), HNRF_E_WORKSPACE,
                 "hnrf_mesh_count: workspace %zu < %zu bytes", workspace_bytes, hnrf_mesh_workspace_bytes(N));
    const int64_t M = (int64_t)N * N * N, nblk = (M + kThreads - 1) / kThreads;
    const MeshCarve c = carve_mesh(workspace, M);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, density, level, N, M, c.word,
                       c.blk_v, c.blk_t);
    int rc = check_launch("hnrf_mesh_count");
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, c.blk_v, c.blk_t, nblk, c.base_v, c.base_t,
                       counts);
    return check_launch("hnrf_mesh_count");
}

extern "C" int hnrf_mesh_emit(const float* density, int N, float level, const float* bbox_min, const float* bbox_max,
                              const void* workspace, size_t workspace_bytes, int64_t V, int64_t F, float* verts,
                              int* faces, void* stream) {
    HNRF_REQUIRE(density && bbox_min && bbox_max && workspace, HNRF_E_ARG, "hnrf_mesh_emit: null pointer");
    HNRF_REQUIRE((V == 0 || verts) && (F == 0 || faces), HNRF_E_ARG, "hnrf_mesh_emit: null output pointer");
    HNRF_REQUIRE(N >= 8 && N <= 512, HNRF_E_ARG, "hnrf_mesh_emit: N=%d out of range [8, 512]", N);
    HNRF_REQUIRE(isfinite(level), HNRF_E_ARG, "hnrf_mesh_emit: level must be finite");
    HNRF_REQUIRE(V >= 0 && V <= 2147483647LL && F >= 0, HNRF_E_ARG, "hnrf_mesh_emit: bad counts V=%lld F=%lld",
                 (long long)V, (long long)F);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_mesh_emit: workspace must be 256-byte aligned");
    HNRF_REQUIRE(workspace_bytes >= hnrf_mesh_workspace_bytes(N), HNRF_E_WORKSPACE,
                 "hnrf_mesh_emit: workspace %zu < %zu bytes", workspace_bytes, hnrf_mesh_workspace_bytes(N));
    const int64_t M = (int64_t)N * N * N, nblk = (M + kThreads - 1) / kThreads;
    const MeshCarve c = carve_mesh(const_cast<void*>(workspace), M);
    hipLaunchKernelGGL(mesh_emit_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, (hipStream_t)stream, density, level,
                       bbox_min, bbox_max, N, M, c.word, c.base_v, c.base_t, V, F, verts, faces);
    return check_launch("hnrf_mesh_emit");
}

extern "C" int hnrf_forward_skin(const float* verts, int64_t V, const float* motion_Rs, const float* motion_Ts,
                                 const float* vol, int B, int G, const float* bbox_min, const float* bbox_scale,
                                 float* out, void* stream) {
    HNRF_REQUIRE(V >= 0 && (V + kThreads - 1) / kThreads < 2147483647LL, HNRF_E_ARG, "hnrf_forward_skin: bad V=%lld",
                 (long long)V);
    HNRF_REQUIRE(B >= 1 && B <= kMaxSkinBones && G >= 2 && G <= 1024, HNRF_E_ARG,
                 "hnrf_forward_skin: bad dims B=%d G=%d (B <= %d)", B, G, kMaxSkinBones);
    if (V == 0) return HNRF_OK;        // (no vertices: the pointers are not looked at, as in hnrf_skin.h)
    HNRF_REQUIRE(verts && motion_Rs && motion_Ts && vol && bbox_min && bbox_scale && out, HNRF_E_ARG,
                 "hnrf_forward_skin: null pointer");
    hipLaunchKernelGGL(forward_skin_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, verts, V, motion_Rs, motion_Ts, vol, B, G, bbox_min, bbox_scale, out);
    return check_launch("hnrf_forward_skin");
}
