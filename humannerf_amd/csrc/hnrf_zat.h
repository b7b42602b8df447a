// The depth of sample s of S along a ray: the one statement K1 (hnrf_sample_warp.hip) and the surface distance of the
// geometry maps (hnrf_geometry.hip) share.
#pragma once
#include <hip/hip_runtime.h>

namespace hnrf {

// torch.linspace(0, 1, S)[s] in fp32 (start + step*i below the midpoint,
// end - step*(S-1-i) from it on; torch's own kernels differ from these two forms
// by an ulp on some elements), then the reference's lerp (network.py:457-458).
__device__ __forceinline__ float z_at(float nr, float fr, int s, int S) {
#pragma clang fp contract(off)
    const float step = 1.0f / (float)(S - 1);
    const float t = (s < S / 2) ? step * (float)s : 1.0f - step * (float)(S - 1 - s);
    return nr * (1.0f - t) + fr * t;
}

}  // namespace hnrf
