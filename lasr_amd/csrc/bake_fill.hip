// bake_fill.hip -- completes the atlas of bake.hip where no frame looked (scripts/bake_texture.py --fill, lasr_amd/nnutils/bake.py):
// a texel with weight == 0 takes the colour of its mirror image on the bilaterally symmetric rest shape, and what is still unfilled
// is smoothed from its neighbours across the texel adjacency.  This is the project's own addition; the reference has no
// counterpart, and the definition is the one of include/lasr_ops.h and DESIGN.md section 4.11.
// bake_mirror_kernel: one listed texel per lane, 256 per block; the faces of the rest mesh pass through LDS in tiles of
// LASR_BAKE_FILL_TILE records of three float4 (as chamfer.hip passes its targets), every lane reads the same record (a broadcast),
// and each lane keeps a running (d2, face, barycentrics).  Ascending face index and a strict `<`: the lowest index among equal
// distances.  bake_blend_kernel: one Jacobi iteration, one thread per texel.  No atomics, no waits across blocks.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"
#include "point_triangle.h"
#include "sr_device.h"

namespace lasr {

constexpr int BF_TILE = LASR_BAKE_FILL_TILE;

// as bake.hip: bake_centroid
__device__ __forceinline__ void fill_centroid(int j, int R, float& c0, float& c1)
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

__device__ __forceinline__ bool fill_face(const int* __restrict__ faces, int f, int V, int& i0, int& i1, int& i2)
{
    i0 = faces[f * 3]; i1 = faces[f * 3 + 1]; i2 = faces[f * 3 + 2];
    return (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
}

// unnormalised normal (V1 - V0) x (V2 - V0)
__device__ __forceinline__ void fill_normal(const float* __restrict__ v, int i0, int i1, int i2, float* n)
{
    const float e1x = v[i1 * 3] - v[i0 * 3], e1y = v[i1 * 3 + 1] - v[i0 * 3 + 1], e1z = v[i1 * 3 + 2] - v[i0 * 3 + 2];
    const float e2x = v[i2 * 3] - v[i0 * 3], e2y = v[i2 * 3 + 1] - v[i0 * 3 + 1], e2z = v[i2 * 3 + 2] - v[i0 * 3 + 2];
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
}

// coordinate `axis` negated, without indexing the registers at run time
__device__ __forceinline__ void fill_mirror(float* x, int axis)
{
    x[0] = axis == 0 ? -x[0] : x[0];
    x[1] = axis == 1 ? -x[1] : x[1];
    x[2] = axis == 2 ? -x[2] : x[2];
}

__global__ __launch_bounds__(256) void bake_mirror_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const int* __restrict__ texels, const float* __restrict__ textures,
                                                          const float* __restrict__ weight, float* __restrict__ out_textures,
                                                          int* __restrict__ src, float* __restrict__ d2, int V, int F, int R, int M,
                                                          int axis, float max_d2)
{
    __shared__ float4 tile[BF_TILE * 3];
    const int RR = R * R;
    const int m = blockIdx.x * 256 + threadIdx.x;
    int f = 0, j = 0, f0 = 0, f1 = 0, f2 = 0;
    bool live = false;
    float p[3] = {0.f, 0.f, 0.f};
    if (m < M) {
        const int i = texels[m];
        if (i >= 0 && i < F * RR) {
            f = i / RR;
            j = i - f * RR;
            live = fill_face(faces, f, V, f0, f1, f2);
        }
    }
    if (live) {
        float c0, c1;
        fill_centroid(j, R, c0, c1);
        const float c2 = 1.f - c0 - c1;
#pragma unroll
        for (int d = 0; d < 3; d++) p[d] = c0 * verts[f0 * 3 + d] + c1 * verts[f1 * 3 + d] + c2 * verts[f2 * 3 + d];
        fill_mirror(p, axis);
    }
    float best = INFINITY, b0 = 0.f, b1 = 0.f;
    int g = -1;
    for (int q0 = 0; q0 < F; q0 += BF_TILE) {
        const int cnt = min(BF_TILE, F - q0);
        __syncthreads();                                       // the previous tile has been read by every wave
        for (int t = threadIdx.x; t < cnt; t += 256) {
            int i0, i1, i2;
            const bool ok = fill_face(faces, q0 + t, V, i0, i1, i2);
            if (!ok) i0 = i1 = i2 = 0;                         // V >= 1: a readable vertex; the flag keeps the face out
            tile[t * 3] = make_float4(verts[i0 * 3], verts[i0 * 3 + 1], verts[i0 * 3 + 2], ok ? 1.f : 0.f);
            tile[t * 3 + 1] = make_float4(verts[i1 * 3], verts[i1 * 3 + 1], verts[i1 * 3 + 2], 0.f);
            tile[t * 3 + 2] = make_float4(verts[i2 * 3], verts[i2 * 3 + 1], verts[i2 * 3 + 2], 0.f);
        }
        __syncthreads();
        if (!live) continue;
        for (int t = 0; t < cnt; t++) {
            const float4 A = tile[t * 3], B = tile[t * 3 + 1], C = tile[t * 3 + 2];
            if (A.w == 0.f) continue;                          // the same for every lane
            const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z}, c[3] = {C.x, C.y, C.z};
            const Closest cl = point_triangle(p, a, b, c);
            if (cl.d2 < best) { best = cl.d2; g = q0 + t; b0 = cl.w[0]; b1 = cl.w[1]; }
        }
    }
    if (m >= M) return;
    int result;
    if (g < 0) {
        result = -1 - LASR_BAKE_MIRROR_NO_FACE;
    } else if (!(best <= max_d2)) {
        result = -1 - LASR_BAKE_MIRROR_FAR;
    } else {
        int g0, g1, g2;
        (void)fill_face(faces, g, V, g0, g1, g2);              // valid: it went through the tile with its flag set
        float nf[3], ng[3];
        fill_normal(verts, f0, f1, f2, nf);
        fill_normal(verts, g0, g1, g2, ng);
        fill_mirror(nf, axis);
        if (!(nf[0] * ng[0] + nf[1] * ng[1] + nf[2] * ng[2] > 0.f)) {
            result = -1 - LASR_BAKE_MIRROR_NORMAL;
        } else {
            const float keep = 1.f - 0x1p-20f, pull = 0x1p-20f / 3.f;
            const int jm = min(max(surface_texel(b0 * keep + pull, b1 * keep + pull, R), 0), RR - 1);
            const size_t s = (size_t)g * RR + jm;
            if (!(weight[s] > 0.f)) {
                result = -1 - LASR_BAKE_MIRROR_UNSEEN;
            } else {
                const size_t o = (size_t)f * RR + j;
                out_textures[o * 3] = textures[s * 3];
                out_textures[o * 3 + 1] = textures[s * 3 + 1];
                out_textures[o * 3 + 2] = textures[s * 3 + 2];
                result = (int)s;
            }
        }
    }
    src[m] = result;
    d2[m] = best;
}

// texel index of the lower triangle L(ix, iy) / the upper triangle U(cx, cy) of a face
__device__ __forceinline__ int fill_lower(int ix, int iy, int R) { return iy * R + ix; }
__device__ __forceinline__ int fill_upper(int cx, int cy, int R) { return (R - 1 - cy) * R + (R - 1 - cx); }

// The texel across face edge k at slot s (counted from the edge's end p), or -1.
__device__ __forceinline__ int fill_across(const int* __restrict__ nbr, int f, int k, int s, int F, int R)
{
    const int code = nbr[f * 3 + k];
    if (code < 0) return -1;
    const int g = code / 6, k2 = (code >> 1) % 3;
    if (g >= F) return -1;
    const int s2 = (code & 1) ? s : R - 1 - s;
    const int ix = k2 == 0 ? 0 : (k2 == 1 ? s2 : R - 1 - s2);
    const int iy = k2 == 0 ? R - 1 - s2 : (k2 == 1 ? 0 : s2);
    return g * R * R + fill_lower(ix, iy, R);
}

__global__ __launch_bounds__(256) void bake_blend_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         const unsigned char* __restrict__ fixed, const int* __restrict__ nbr, int F,
                                                         int R)
{
    const int RR = R * R;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F * RR) return;
    float r = in[(size_t)i * 3], gch = in[(size_t)i * 3 + 1], b = in[(size_t)i * 3 + 2];
    if (!fixed[i]) {
        const int f = i / RR, j = i - f * RR;
        const int iy = j / R, ix = j - iy * R;
        int n[3];
        if (ix + iy <= R - 1) {
            n[0] = ix >= 1 ? f * RR + fill_upper(ix - 1, iy, R) : fill_across(nbr, f, 0, R - 1 - iy, F, R);
            n[1] = iy >= 1 ? f * RR + fill_upper(ix, iy - 1, R) : fill_across(nbr, f, 1, ix, F, R);
            n[2] = ix + iy <= R - 2 ? f * RR + fill_upper(ix, iy, R) : fill_across(nbr, f, 2, iy, F, R);
        } else {
            const int cx = R - 1 - ix, cy = R - 1 - iy;
            n[0] = f * RR + fill_lower(cx + 1, cy, R);
            n[1] = f * RR + fill_lower(cx, cy + 1, R);
            n[2] = f * RR + fill_lower(cx, cy, R);
        }
        float sr = 0.f, sg = 0.f, sb = 0.f;
        int count = 0;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (n[k] >= 0) {
                sr = sr + in[(size_t)n[k] * 3];
                sg = sg + in[(size_t)n[k] * 3 + 1];
                sb = sb + in[(size_t)n[k] * 3 + 2];
                count++;
            }
        if (count > 0) {
            const float cf = (float)count;
            r = sr / cf;
            gch = sg / cf;
            b = sb / cf;
        }
    }
    out[(size_t)i * 3] = r;
    out[(size_t)i * 3 + 1] = gch;
    out[(size_t)i * 3 + 2] = b;
}

// as bake.hip: bake_sizes_ok
static bool fill_sizes_ok(int V, int F, int R)
{
    return V >= 1 && F >= 0 && R >= 1 && R <= LASR_BAKE_MAX_RES && (long long)F * R * R * 4 <= 0x7fffffffLL &&
           (long long)V * 3 <= 0x7fffffffLL;
}

}  // namespace lasr

extern "C" int lasr_bake_mirror(const float* rest_verts, const int* faces, const int* texels, const float* textures,
                                const float* weight, float* out_textures, int* src, float* d2, int V, int F, int R, int M, int axis,
                                float max_d2, void* hip_stream)
{
    if (!lasr::fill_sizes_ok(V, F, R) || M < 0 || axis < 0 || axis > 2) return LASR_E_BADARG;
    if (!(max_d2 >= 0.f && max_d2 <= 3.4028235e38f)) return LASR_E_BADARG;               // false for NaN
    if (M == 0 || F == 0) return LASR_OK;
    if (!rest_verts || !faces || !texels || !textures || !weight || !out_textures || !src || !d2) return LASR_E_BADARG;
    if (out_textures == textures) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::bake_mirror_kernel, dim3((unsigned)(((long long)M + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       rest_verts, faces, texels, textures, weight, out_textures, src, d2, V, F, R, M, axis, max_d2);
    return launch_ok();
}

extern "C" int lasr_bake_blend(const float* in, float* out, const unsigned char* fixed, const int* nbr, int F, int R, void* hip_stream)
{
    if (!lasr::fill_sizes_ok(1, F, R) || (long long)F * 6 + 5 > 0x7fffffffLL) return LASR_E_BADARG;
    if (F == 0) return LASR_OK;
    if (!in || !out || !fixed || !nbr || in == out) return LASR_E_BADARG;
    const long long n = (long long)F * R * R;
    hipLaunchKernelGGL(lasr::bake_blend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, in, out,
                       fixed, nbr, F, R);
    return launch_ok();
}
