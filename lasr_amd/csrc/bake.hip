// bake.hip -- texture baking of scripts/bake_texture.py (lasr_amd/nnutils/bake.py assembles the frames): fills the per-face surface
// textures [F, R*R, 3] the rasteriser samples (sr_device.h: surface_texel) from the video.  This is the project's own addition;
// the reference has no counterpart, and the definition is the one of include/lasr_ops.h and DESIGN.md section 4.11.
// Visibility comes from the hard-mode rasteriser (lasr_sr_forward_bg, func_id_rgb = func_id_alpha = 0): plane 1 of its aggrs_info
// names the nearest face of every pixel, read here exactly as vis.hip reads raster0.  One thread per texel owns its accumulator
// and visits the frames of a launch in increasing order: no atomics, the same bits whatever the chunking of the frames.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"

namespace lasr {

// Barycentric centroid (c0, c1) of the region surface_texel(c0, c1, R) maps to texel j = iy * R + ix: the lower triangle of cell
// (ix, iy) when ix + iy <= R - 1, else the upper triangle of cell (R-1-ix, R-1-iy).
__device__ __forceinline__ void bake_centroid(int j, int R, float& c0, float& c1)
{
    const int iy = j / R, ix = j - iy * R;
    const float inv = 1.f / (float)R;
    if (ix + iy <= R - 1) {
        c0 = ((float)ix + (1.f / 3.f)) * inv;
        c1 = ((float)iy + (1.f / 3.f)) * inv;
    } else {
        c0 = ((float)(R - 1 - ix) + (2.f / 3.f)) * inv;
        c1 = ((float)(R - 1 - iy) + (2.f / 3.f)) * inv;
    }
}

__device__ __forceinline__ int bake_clamp(int x, int hi) { return min(max(x, 0), hi); }

// One thread per texel i = f * R*R + j; frames 0 .. T-1 of this launch in order.
__global__ __launch_bounds__(256) void bake_accumulate_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                              const float4* __restrict__ K, const float* __restrict__ raster,
                                                              const unsigned char* __restrict__ frames,
                                                              const unsigned char* __restrict__ masks, float4* __restrict__ accum,
                                                              int T, int V, int F, int R, int IS, int H, int W, int power)
{
    const int RR = R * R;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F * RR) return;
    const int f = i / RR, j = i - f * RR;
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return;
    float c0, c1;
    bake_centroid(j, R, c0, c1);
    const float c2 = 1.f - c0 - c1;
    const size_t P = (size_t)IS * IS, HW = (size_t)H * W;
    float4 acc = accum[i];
    for (int t = 0; t < T; t++) {
        const float* v = verts + (size_t)t * V * 3;
        const float ax = v[i0 * 3], ay = v[i0 * 3 + 1], az = v[i0 * 3 + 2];
        const float bx = v[i1 * 3], by = v[i1 * 3 + 1], bz = v[i1 * 3 + 2];
        const float cx = v[i2 * 3], cy = v[i2 * 3 + 1], cz = v[i2 * 3 + 2];
        const float px = c0 * ax + c1 * bx + c2 * cx;
        const float py = c0 * ay + c1 * by + c2 * cy;
        const float pz = c0 * az + c1 * bz + c2 * cz;
        if (!(pz > 0.f)) continue;
        const float4 k = K[t];                                       // fx fy px py
        const float u = k.x * px / pz + k.z, w = k.y * py / pz + k.w;
        if (!(u >= 0.f && u < (float)W && w >= 0.f && w < (float)H)) continue;
        const int col = (int)u, row = (int)w;                        // the pixel that holds (u, v): u in [col, col + 1)
        const float fo = raster[((size_t)t * 2 + 1) * P + (size_t)row * IS + col];   // row 0 is the top row (NDC y = +1)
        if (!(fo == (float)f)) continue;
        // bilinear taps around (u - 0.5, v - 0.5): pixel centres sit at half-integers
        const float su = u - 0.5f, sv = w - 0.5f;
        const float fu = floorf(su), fv = floorf(sv);
        const float tx = su - fu, ty = sv - fv;
        const int x0 = bake_clamp((int)fu, W - 1), x1 = bake_clamp((int)fu + 1, W - 1);
        const int y0 = bake_clamp((int)fv, H - 1), y1 = bake_clamp((int)fv + 1, H - 1);
        const size_t o00 = (size_t)y0 * W + x0, o01 = (size_t)y0 * W + x1, o10 = (size_t)y1 * W + x0, o11 = (size_t)y1 * W + x1;
        if (masks) {                                                 // the silhouette holds all four taps: no background bleeds in
            const unsigned char* m = masks + (size_t)t * HW;
            if (!(m[o00] > 0 && m[o01] > 0 && m[o10] > 0 && m[o11] > 0)) continue;
        }
        // |n . d|^power: unit face normal against the unit viewing ray, by repeated multiplication
        float wgt = 1.f;
        if (power > 0) {
            const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
            const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
            const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const float nn = sqrtf(nx * nx + ny * ny + nz * nz), pn = sqrtf(px * px + py * py + pz * pz);
            const float den = nn * pn;
            const float cs = den > 0.f ? fabsf(nx * px + ny * py + nz * pz) / den : 0.f;
            for (int q = 0; q < power; q++) wgt *= cs;
        }
        const unsigned char* fr = frames + (size_t)t * HW * 3;
        const float w00 = (1.f - tx) * (1.f - ty), w01 = tx * (1.f - ty), w10 = (1.f - tx) * ty, w11 = tx * ty;
        float rgb[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            rgb[ch] = (w00 * (float)fr[o00 * 3 + ch] + w01 * (float)fr[o01 * 3 + ch] + w10 * (float)fr[o10 * 3 + ch] +
                       w11 * (float)fr[o11 * 3 + ch]) * (1.f / 255.f);
        acc.x += wgt * rgb[0];
        acc.y += wgt * rgb[1];
        acc.z += wgt * rgb[2];
        acc.w += wgt;
    }
    accum[i] = acc;
}

// textures = accum.rgb / accum.w where a frame saw the texel, else the fallback vertex colour at the texel's centroid (0.5 grey
// without one); weight = accum.w.
__global__ __launch_bounds__(256) void bake_resolve_kernel(const float4* __restrict__ accum, const int* __restrict__ faces,
                                                           const float* __restrict__ fallback, float* __restrict__ textures,
                                                           float* __restrict__ weight, int V, int F, int R)
{
    const int RR = R * R;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F * RR) return;
    const float4 a = accum[i];
    float r = 0.5f, g = 0.5f, b = 0.5f;
    if (a.w > 0.f) {
        r = a.x / a.w;
        g = a.y / a.w;
        b = a.z / a.w;
    } else if (fallback) {
        const int f = i / RR, j = i - f * RR;
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            float c0, c1;
            bake_centroid(j, R, c0, c1);
            const float c2 = 1.f - c0 - c1;
            r = c0 * fallback[i0 * 3] + c1 * fallback[i1 * 3] + c2 * fallback[i2 * 3];
            g = c0 * fallback[i0 * 3 + 1] + c1 * fallback[i1 * 3 + 1] + c2 * fallback[i2 * 3 + 1];
            b = c0 * fallback[i0 * 3 + 2] + c1 * fallback[i1 * 3 + 2] + c2 * fallback[i2 * 3 + 2];
        }
    }
    textures[(size_t)i * 3] = r;
    textures[(size_t)i * 3 + 1] = g;
    textures[(size_t)i * 3 + 2] = b;
    weight[i] = a.w;
}

static bool bake_sizes_ok(int V, int F, int R)
{
    return V >= 1 && F >= 0 && R >= 1 && R <= LASR_BAKE_MAX_RES && (long long)F * R * R * 4 <= 0x7fffffffLL &&
           (long long)V * 3 <= 0x7fffffffLL;
}

}  // namespace lasr

extern "C" int lasr_bake_accumulate(const float* verts, const int* faces, const float* K, const float* raster,
                                    const unsigned char* frames, const unsigned char* masks, float* accum, int T, int V, int F, int R,
                                    int IS, int H, int W, int power, void* hip_stream)
{
    if (T < 0 || !lasr::bake_sizes_ok(V, F, R)) return LASR_E_BADARG;
    if (H < 1 || W < 1 || H > IS || W > IS || IS > LASR_BAKE_MAX_SIZE) return LASR_E_BADARG;
    if (power < 0 || power > LASR_BAKE_MAX_POWER) return LASR_E_BADARG;
    if (T == 0 || F == 0) return LASR_OK;
    if (!verts || !faces || !K || !raster || !frames || !accum) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const long long n = (long long)F * R * R;
    LASR_LAUNCH(K_BAKE_ACCUMULATE, lasr::bake_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, verts, faces,
                (const float4*)K, raster, frames, masks, (float4*)accum, T, V, F, R, IS, H, W, power);
    return launch_ok();
}

extern "C" int lasr_bake_resolve(const float* accum, const int* faces, const float* fallback, float* textures, float* weight, int V,
                                 int F, int R, void* hip_stream)
{
    if (!lasr::bake_sizes_ok(V, F, R)) return LASR_E_BADARG;
    if (F == 0) return LASR_OK;
    if (!accum || !faces || !textures || !weight) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const long long n = (long long)F * R * R;
    LASR_LAUNCH(K_BAKE_RESOLVE, lasr::bake_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const float4*)accum,
                faces, fallback, textures, weight, V, F, R);
    return launch_ok();
}
