// The trilinear look-up of the weight volume at a canonical point, shared by the density lattice's gate and forward
// skinning (hnrf_mesh.hip) and by the bone weights of the skinned export (hnrf_skin.hip): one statement, so that the
// weights the export writes are the weights hnrf_forward_skin blends with, bit for bit.  Both files are compiled with
// -ffp-contract=off: every operation below is rounded on its own.
#pragma once
#include <math.h>

#include "hnrf_common.h"

namespace hnrf {

// The trilinear (align_corners, zero padding) value of a channel at canonical point (x,y,z), written like K1
// (hnrf_sample_warp.hip) for the identity motion; the corner weights do not depend on the channel.  A NaN coordinate
// clamps to a node outside the volume on that axis: every corner weight is 0.
struct Trilinear {
    unsigned o[8];      // element offsets of the 8 corners in one channel (clamped into the volume)
    float c[8];         // corner weights, 0 for corners outside the volume
};

__device__ __forceinline__ Trilinear trilinear_at(float qx, float qy, float qz, const float* bbox_min,
                                                  const float* bbox_scale, int G) {
    const float gm1 = (float)(G - 1);
    const float ix = (((qx - bbox_min[0]) * bbox_scale[0] - 1.0f) + 1.0f) * 0.5f * gm1;
    const float iy = (((qy - bbox_min[1]) * bbox_scale[1] - 1.0f) + 1.0f) * 0.5f * gm1;
    const float iz = (((qz - bbox_min[2]) * bbox_scale[2] - 1.0f) + 1.0f) * 0.5f * gm1;
    const float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
    const float wx1 = ix - fx0, wy1 = iy - fy0, wz1 = iz - fz0;
    const float wx0 = (fx0 + 1.0f) - ix, wy0 = (fy0 + 1.0f) - iy, wz0 = (fz0 + 1.0f) - iz;
    const int x0 = (int)fminf(fmaxf(fx0, -2.0f), gm1 + 1.0f);
    const int y0 = (int)fminf(fmaxf(fy0, -2.0f), gm1 + 1.0f);
    const int z0 = (int)fminf(fmaxf(fz0, -2.0f), gm1 + 1.0f);
    const float ux0 = (x0 >= 0 && x0 < G) ? wx0 : 0.f, ux1 = (x0 + 1 >= 0 && x0 + 1 < G) ? wx1 : 0.f;
    const float uy0 = (y0 >= 0 && y0 < G) ? wy0 : 0.f, uy1 = (y0 + 1 >= 0 && y0 + 1 < G) ? wy1 : 0.f;
    const float uz0 = (z0 >= 0 && z0 < G) ? wz0 : 0.f, uz1 = (z0 + 1 >= 0 && z0 + 1 < G) ? wz1 : 0.f;
    const unsigned cx0 = min(max(x0, 0), G - 1), cx1 = min(max(x0 + 1, 0), G - 1);
    const unsigned cy0 = min(max(y0, 0), G - 1), cy1 = min(max(y0 + 1, 0), G - 1);
    const unsigned cz0 = min(max(z0, 0), G - 1), cz1 = min(max(z0 + 1, 0), G - 1);
    Trilinear t;
    const unsigned GG = (unsigned)G * (unsigned)G;
    t.o[0] = cz0 * GG + cy0 * G + cx0;  t.c[0] = ux0 * uy0 * uz0;
    t.o[1] = cz0 * GG + cy0 * G + cx1;  t.c[1] = ux1 * uy0 * uz0;
    t.o[2] = cz0 * GG + cy1 * G + cx0;  t.c[2] = ux0 * uy1 * uz0;
    t.o[3] = cz0 * GG + cy1 * G + cx1;  t.c[3] = ux1 * uy1 * uz0;
    t.o[4] = cz1 * GG + cy0 * G + cx0;  t.c[4] = ux0 * uy0 * uz1;
    t.o[5] = cz1 * GG + cy0 * G + cx1;  t.c[5] = ux1 * uy0 * uz1;
    t.o[6] = cz1 * GG + cy1 * G + cx0;  t.c[6] = ux0 * uy1 * uz1;
    t.o[7] = cz1 * GG + cy1 * G + cx1;  t.c[7] = ux1 * uy1 * uz1;
    return t;
}

__device__ __forceinline__ float trilinear_channel(const Trilinear& t, const float* __restrict__ ch) {
    float w = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) w += ch[t.o[k]] * t.c[k];
    return w;
}

}  // namespace hnrf
