// Stand-alone caller of the host-side argument checks of include/hnrf_geometry.h, for a sanitizer build of that host
// code: every call below must be refused BEFORE any launch, so the program needs no GPU.  It is compiled together with
// csrc/hnrf_geometry.hip (not against libhnrf.so: the code under test carries the instrumentation) and brings the two
// functions of hnrf_abi.hip that file needs.  From the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/cabi/geometry_args_host.cpp humannerf_amd/csrc/hnrf_geometry.hip -o /tmp/geometry_args_host \
//     && /tmp/geometry_args_host
//
// Prints one line per refusal and "geometry_args_host: N refusals, ok"; exits 1 when a call is not refused or its
// message does not name the argument.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/hnrf.h"

namespace hnrf {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace hnrf

static int g_fail = 0, g_count = 0;

static void refused(int rc, const char* needle, const char* what) {
    ++g_count;
    const bool ok = rc != 0 && strstr(hnrf::g_err, needle) != nullptr;
    printf("%-44s rc %2d  %s%s\n", what, rc, hnrf::g_err, ok ? "" : "   <-- NOT REFUSED AS EXPECTED");
    if (!ok) g_fail = 1;
    hnrf::g_err[0] = 0;
}

int main() {
    alignas(256) static float buf[1024];
    float* f = buf;
    uint8_t* u8 = (uint8_t*)buf;
    int* i32 = (int*)buf;
    int64_t* i64 = (int64_t*)buf;
    const float nan = __builtin_nanf("");

    // ---- hnrf_ray_surface
    refused(hnrf_ray_surface(f, f, f, f, f, f, 4, 0, .5f, f, f, f, u8, nullptr), "S 0", "ray_surface: S = 0");
    refused(hnrf_ray_surface(f, f, f, f, f, f, 4, 65537, .5f, f, f, f, u8, nullptr), "S 65537", "ray_surface: S too large");
    refused(hnrf_ray_surface(f, f, f, f, f, f, -1, 4, .5f, f, f, f, u8, nullptr), "R -1", "ray_surface: R < 0");
    refused(hnrf_ray_surface(f, f, f, f, f, f, (int64_t)1 << 31, 4, .5f, f, f, f, u8, nullptr), "R ", "ray_surface: R = 2^31");
    refused(hnrf_ray_surface(f, f, f, f, f, f, (int64_t)1 << 30, 65536, .5f, f, f, f, u8, nullptr), "R ", "ray_surface: R S >= 2^40");
    refused(hnrf_ray_surface(f, f, f, f, f, f, 4, 4, nan, f, f, f, u8, nullptr), "alpha_min", "ray_surface: alpha_min NaN");
    refused(hnrf_ray_surface(f, f, f, f, nullptr, nullptr, 4, 4, .5f, f, f, nullptr, u8, nullptr), "t_med needs weights",
            "ray_surface: t_med, lean");
    refused(hnrf_ray_surface(f, f, f, f, nullptr, nullptr, 4, 4, .5f, f, nullptr, f, u8, nullptr), "woff needs weights",
            "ray_surface: woff, lean");
    refused(hnrf_ray_surface(f, f, f, f, f, nullptr, 4, 4, .5f, f, nullptr, f, u8, nullptr), "woff needs weights and offsets",
            "ray_surface: woff without offsets");
    refused(hnrf_ray_surface(nullptr, f, f, f, f, f, 4, 4, .5f, f, f, f, u8, nullptr), "near", "ray_surface: near null");
    refused(hnrf_ray_surface(f, f, nullptr, f, f, f, 4, 4, .5f, f, f, f, u8, nullptr), "null pointer", "ray_surface: alpha null");
    refused(hnrf_ray_surface(f, f, f, f, f, f, 4, 4, .5f, f, f, f, nullptr, nullptr), "null pointer", "ray_surface: valid null");

    // ---- hnrf_pixel_rays
    refused(hnrf_pixel_rays(i64, 1, 0, 2, i32, i32, nullptr), "H 0", "pixel_rays: H = 0");
    refused(hnrf_pixel_rays(i64, 1, 2, 16385, i32, i32, nullptr), "W 16385", "pixel_rays: W too large");
    refused(hnrf_pixel_rays(i64, -1, 2, 2, i32, i32, nullptr), "N -1", "pixel_rays: N < 0");
    refused(hnrf_pixel_rays(i64, (int64_t)1 << 31, 2, 2, i32, i32, nullptr), "N ", "pixel_rays: N = 2^31");
    refused(hnrf_pixel_rays(nullptr, 1, 2, 2, i32, i32, nullptr), "null pointer", "pixel_rays: ray_index null");
    refused(hnrf_pixel_rays(i64, 1, 2, 2, nullptr, i32, nullptr), "null pointer", "pixel_rays: pix2ray null");
    refused(hnrf_pixel_rays(i64, 1, 2, 2, i32, nullptr, nullptr), "null pointer", "pixel_rays: status null");
    refused(hnrf_pixel_rays(i64, 1, 2, 2, (int*)((char*)buf + 2), i32, nullptr), "aligned", "pixel_rays: pix2ray misaligned");
    refused(hnrf_pixel_rays((int64_t*)((char*)buf + 4), 1, 2, 2, i32, i32, nullptr), "aligned", "pixel_rays: ray_index misaligned");

    // ---- hnrf_geometry_maps
    auto maps = [&](const float* t_exp, const float* t_med, int surface, const float* alpha, const float* woff, const int* pix,
                    int64_t N, int H, int W, float edge, const float* M, const float* bg, const float* lohi) {
        return hnrf_geometry_maps(f, f, t_exp, t_med, u8, surface, alpha, woff, pix, N, H, W, edge, M, bg, lohi, .25f, .8f,
                                  nullptr, nullptr, f, u8, u8, u8, u8, u8, nullptr);
    };
    refused(maps(f, f, 2, f, f, i32, 4, 2, 2, .05f, f, f, f), "surface 2", "geometry_maps: surface = 2");
    refused(maps(f, f, 0, f, f, i32, 4, 0, 2, .05f, f, f, f), "H 0", "geometry_maps: H = 0");
    refused(maps(f, f, 0, f, f, i32, 4, 2, 20000, .05f, f, f, f), "W 20000", "geometry_maps: W too large");
    refused(maps(f, f, 0, f, f, i32, -3, 2, 2, .05f, f, f, f), "N -3", "geometry_maps: N < 0");
    refused(maps(f, f, 0, f, f, i32, 4, 2, 2, nan, f, f, f), "edge", "geometry_maps: edge NaN");
    refused(maps(f, f, 0, f, f, i32, 4, 2, 2, -1.f, f, f, f), "edge", "geometry_maps: edge < 0");
    refused(maps(f, nullptr, 1, f, f, i32, 4, 2, 2, .05f, f, f, f), "t_med", "geometry_maps: median without t_med");
    refused(maps(nullptr, f, 0, f, f, i32, 4, 2, 2, .05f, f, f, f), "t_exp", "geometry_maps: expected without t_exp");
    refused(maps(f, f, 0, f, f, nullptr, 4, 2, 2, .05f, f, f, f), "null pointer", "geometry_maps: pix2ray null");
    refused(maps(f, f, 0, f, f, i32, 4, 2, 2, .05f, f, nullptr, f), "null pointer", "geometry_maps: bgcolor null");
    refused(maps(f, f, 0, f, f, i32, 4, 2, 2, .05f, nullptr, f, f), "normal8 needs M", "geometry_maps: M null");
    refused(maps(f, f, 0, f, f, i32, 4, 2, 2, .05f, f, f, nullptr), "depth8 needs lohi", "geometry_maps: lohi null");
    refused(maps(f, f, 0, nullptr, f, i32, 4, 2, 2, .05f, f, f, f), "shaded8 needs alpha", "geometry_maps: alpha null");
    refused(maps(f, f, 0, f, nullptr, i32, 4, 2, 2, .05f, f, f, f), "offset8 needs woff", "geometry_maps: woff null");
    refused(maps(f, f, 0, f, f, (int*)((char*)buf + 1), 4, 2, 2, .05f, f, f, f), "aligned", "geometry_maps: pix2ray misaligned");

    printf("geometry_args_host: %d refusals, %s\n", g_count, g_fail ? "FAILED" : "ok");
    return g_fail;
}
