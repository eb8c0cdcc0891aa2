// export.hip -- the export side of soft_renderer: texture-atlas creation (save_obj with surface textures) and mesh voxelisation.
// Cold paths (one call per saved model); float and double, as the reference dispatches both.  Built with -ffp-contract=off:
// every atlas texel and every surface voxel is decided by the reference's own expressions in the reference's order.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"
#include "voxel_fill.h"

namespace lasr {

// ===========================================================================
// Texture atlas, third_party/softras/soft_renderer/cuda/create_texture_image_cuda_kernel.cu:10-70.  The image is a grid of
// tile_width x tile_height tiles of R_out x R_out pixels; pixel (x, y) belongs to face x / R_out + (y / R_out) * tile_width.
// Its barycentric coordinates in the face's triangle faces_uv[fn] (pixel units) pick texel (w_x, w_y) of the face's R_in x R_in
// folded-triangle texture, or the mirrored upper one.  One thread per pixel; pixels of tiles past the last face are 1.
// ===========================================================================
template <typename T>
__global__ __launch_bounds__(256) void texture_atlas_kernel(const T* __restrict__ faces_uv, const T* __restrict__ textures,
                                                            T* __restrict__ image, int F, int R, int R_out, int tile_width, int H,
                                                            int W, T eps)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int x = i % W, y = i / W;
    const int fn = x / R_out + (y / R_out) * tile_width;
    T* px = image + (size_t)i * 3;
    if (fn >= F) {
        px[0] = px[1] = px[2] = T(1);
        return;
    }
    const T* p = faces_uv + (size_t)fn * 6;
    const T p0x = p[0], p0y = p[1], p1x = p[2], p1y = p[3], p2x = p[4], p2y = p[5];
    T fi[9] = {p1y - p2y, p2x - p1x, p1x * p2y - p2x * p1y,
               p2y - p0y, p0x - p2x, p2x * p0y - p0x * p2y,
               p0y - p1y, p1x - p0x, p0x * p1y - p1x * p0y};
    const T den = p2x * (p0y - p1y) + p0x * (p1y - p2y) + p1x * (p2y - p0y);
#pragma unroll
    for (int k = 0; k < 9; k++) fi[k] /= (den + eps);
    const T xf = (T)x, yf = (T)y;
    T w[3], w_sum = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        w[k] = fi[3 * k + 0] * xf + fi[3 * k + 1] * yf + fi[3 * k + 2];
        w[k] = fmax(fmin(w[k], T(1)), T(0));                 // fmin / fmax: a NaN becomes 1, as the reference's min / max
        w_sum += w[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] /= (w_sum + eps);
    const int w_x = (int)(w[0] * (T)R), w_y = (int)(w[1] * (T)R);  // w in [0, 1): 0 <= w_x, w_y <= R - 1 (clamped below)
    int t;
    if ((w[0] + w[1]) * (T)R - (T)w_x - (T)w_y <= T(1)) t = min(w_y, R - 1) * R + min(w_x, R - 1);
    else t = max(R - 1 - w_y, 0) * R + max(R - 1 - w_x, 0);
    const T* tex = textures + ((size_t)fn * R * R + t) * 3;
    px[0] = tex[0];
    px[1] = tex[1];
    px[2] = tex[2];
}

// ===========================================================================
// Voxelisation, third_party/softras/soft_renderer/functional/voxelization.py:41-57 with cuda/voxelization_cuda_kernel.cu:30-190.
// Occupancy is a bit grid [B][S (c0)][S (c1)][Wd words along c2], Wd = ceil(S / 64), bit c2 & 63 of word c2 >> 6.
// ===========================================================================
__device__ __forceinline__ void set_voxel(unsigned long long* occ, int S, int Wd, int b, int c0, int c1, int c2)
{
    atomicOr(occ + (((size_t)b * S + c0) * S + c1) * Wd + (c2 >> 6), 1ull << (c2 & 63));
}

// The surface: the union of voxelize_sub1 along the three axes and voxelize_sub2.  One wave per (mesh, face).  voxelize_sub1 with
// dim d scans columns at integer (y, x) of the permuted coordinates (Y, X, Z) = (c2, c1, c0) for d = 0, (c0, c2, c1) for d = 1 and
// (c0, c1, c2) for d = 2, and the transpose of voxelization.py:17 puts its voxel (y, x, z) back at (z, x, y), (y, z, x) and
// (y, x, z).  Instead of every face per column, a face visits the columns of its bounding box widened by one on each side (the
// float test alone decides every one of them); marks are idempotent ORs, so the order does not matter.
template <typename T>
__global__ __launch_bounds__(256) void voxel_surface_kernel(const T* __restrict__ faces, unsigned long long* __restrict__ occ, int B,
                                                            int F, int S, int Wd)
{
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)B * F) return;
    const int b = (int)(wid / F);
    const T* f = faces + (size_t)wid * 9;
    const T Sf = (T)S;
    if (lane < 3) {                                            // voxelize_sub2: the voxel of each vertex
        const T a = floor(f[3 * lane + 0]), c = floor(f[3 * lane + 1]), e = floor(f[3 * lane + 2]);
        if (a >= T(0) && a < Sf && c >= T(0) && c < Sf && e >= T(0) && e < Sf) set_voxel(occ, S, Wd, b, (int)a, (int)c, (int)e);
    }
    for (int d = 0; d < 3; d++) {
        const int iy = d == 0 ? 2 : 0, ix = d == 1 ? 2 : 1, iz = d == 0 ? 0 : (d == 1 ? 1 : 2);
        const T Y0 = f[iy], X0 = f[ix], Z0 = f[iz], Y1 = f[3 + iy], X1 = f[3 + ix], Z1 = f[3 + iz];
        const T Y2 = f[6 + iy], X2 = f[6 + ix], Z2 = f[6 + iz];
        const T ylo = floor(fmin(fmin(Y0, Y1), Y2)) - T(1), yhi = ceil(fmax(fmax(Y0, Y1), Y2)) + T(1);
        const T xlo = floor(fmin(fmin(X0, X1), X2)) - T(1), xhi = ceil(fmax(fmax(X0, X1), X2)) + T(1);
        if (!(ylo < Sf && yhi >= T(0) && xlo < Sf && xhi >= T(0))) continue;     // outside the grid, or not finite
        const int y0 = ylo > T(0) ? (int)ylo : 0, y1 = yhi < Sf - T(1) ? (int)yhi : S - 1;
        const int x0 = xlo > T(0) ? (int)xlo : 0, x1 = xhi < Sf - T(1) ? (int)xhi : S - 1;
        const int nx = x1 - x0 + 1, n = (y1 - y0 + 1) * nx;
        const T y1d = Y1 - Y0, x1d = X1 - X0, z1d = Z1 - Z0;
        const T y2d = Y2 - Y0, x2d = X2 - X0, z2d = Z2 - Z0;
        const T det = x1d * y2d - x2d * y1d;
        if (det == T(0)) continue;
        for (int k = lane; k < n; k += 64) {
            const int y = y0 + k / nx, x = x0 + k % nx;
            const T ypd = (T)y - Y0, xpd = (T)x - X0;
            const T t1 = (y2d * xpd - x2d * ypd) / det;
            const T t2 = (-y1d * xpd + x1d * ypd) / det;
            if (t1 < T(0) || t2 < T(0) || T(1) < t1 + t2) continue;
            const T zf = floor(t1 * z1d + t2 * z2d + Z0);
            if (!(zf >= T(0) && zf < Sf)) continue;
            const int z = (int)zf;
            for (int m = 0; m < 4; m++) {                      // (y, x), (y-1, x), (y, x-1), (y-1, x-1)
                const int yi = y - (m & 1), xi = x - (m >> 1);
                if (yi < 0 || xi < 0) continue;
                if (d == 0) set_voxel(occ, S, Wd, b, z, xi, yi);
                else if (d == 1) set_voxel(occ, S, Wd, b, yi, z, xi);
                else set_voxel(occ, S, Wd, b, yi, xi, z);
            }
        }
    }
}

template <typename T>
int create_texture_image(const T* faces_uv, const T* textures, T* image, int F, int R_in, int R_out, float eps, void* hip_stream)
{
    if (F < 0 || R_in < 1 || R_out < 1) return LASR_E_BADARG;
    if (F == 0) return LASR_OK;
    if (!faces_uv || !textures || !image) return LASR_E_BADARG;
    const int tile_width = (int)sqrt((double)(F - 1)) + 1, tile_height = (F - 1) / tile_width + 1;
    const long long H = (long long)tile_height * R_out, W = (long long)tile_width * R_out;
    if (H * W * 3 > 0x7fffffffLL || (long long)F * R_in * R_in * 3 > 0x7fffffffLL) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    LASR_LAUNCH(K_TEXTURE_ATLAS, texture_atlas_kernel<T>, dim3((unsigned)((H * W + 255) / 256)), dim3(256), 0, faces_uv, textures,
                image, F, R_in, R_out, tile_width, (int)H, (int)W, (T)eps);
    return launch_ok();
}

static size_t voxel_words(int B, int S) { return (size_t)B * S * S * ((S + 63) / 64); }

template <typename T>
int voxelize(const T* faces, int* voxels, int* sweeps, void* workspace, size_t workspace_bytes, int B, int F, int S, void* hip_stream)
{
    if (B < 0 || F < 0 || S < 1 || S > LASR_VOXEL_MAX_SIZE) return LASR_E_BADARG;
    if ((long long)B * F * 9 > 0x7fffffffLL) return LASR_E_BADARG;
    if (B == 0) return LASR_OK;
    if (!voxels || (F > 0 && !faces)) return LASR_E_BADARG;
    const size_t need = lasr_voxelize_workspace_bytes(B, S);
    if (!workspace || workspace_bytes < need) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    const int Wd = (S + 63) / 64;
    unsigned long long* occ = (unsigned long long*)workspace;
    if (hipMemsetAsync(occ, 0, voxel_words(B, S) * 8, st) != hipSuccess) return launch_ok();
    if (F > 0)
        LASR_LAUNCH(K_VOXEL_SURFACE, voxel_surface_kernel<T>, dim3((unsigned)(((long long)B * F + 3) / 4)), dim3(256), 0, faces, occ,
                    B, F, S, Wd);
    if (S <= kLdsMaxS)
        LASR_LAUNCH(K_VOXEL_FILL, voxel_fill_kernel<true>, dim3(B), dim3(kFillThreads), 0, occ, nullptr, voxels, sweeps, S, Wd);
    else
        LASR_LAUNCH(K_VOXEL_FILL, voxel_fill_kernel<false>, dim3(B), dim3(kFillThreads), 0, occ, occ + voxel_words(B, S), voxels,
                    sweeps, S, Wd);
    return launch_ok();
}

}  // namespace lasr

extern "C" int lasr_create_texture_image(const float* faces_uv, const float* textures, float* image, int F, int R_in, int R_out,
                                         float eps, void* hip_stream)
{
    return lasr::create_texture_image<float>(faces_uv, textures, image, F, R_in, R_out, eps, hip_stream);
}

extern "C" int lasr_create_texture_image_f64(const double* faces_uv, const double* textures, double* image, int F, int R_in,
                                             int R_out, float eps, void* hip_stream)
{
    return lasr::create_texture_image<double>(faces_uv, textures, image, F, R_in, R_out, eps, hip_stream);
}

extern "C" size_t lasr_voxelize_workspace_bytes(int B, int S)
{
    if (B < 0 || S < 1 || S > LASR_VOXEL_MAX_SIZE) return 0;
    return lasr::voxel_words(B, S) * 8 * (S <= lasr::kLdsMaxS ? 1 : 3);
}

extern "C" int lasr_voxelize(const float* faces, int* voxels, int* sweeps, void* workspace, size_t workspace_bytes, int B, int F, int S,
                             void* hip_stream)
{
    return lasr::voxelize<float>(faces, voxels, sweeps, workspace, workspace_bytes, B, F, S, hip_stream);
}

extern "C" int lasr_voxelize_f64(const double* faces, int* voxels, int* sweeps, void* workspace, size_t workspace_bytes, int B, int F,
                                 int S, void* hip_stream)
{
    return lasr::voxelize<double>(faces, voxels, sweeps, workspace, workspace_bytes, B, F, S, hip_stream);
}
