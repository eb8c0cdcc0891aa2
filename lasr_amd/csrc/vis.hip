// vis.hip -- the shading and compositing pass of render_vis.py (lasr_amd/vis.py assembles the scene).
// Visibility comes from the hard-mode rasteriser (lasr_sr_forward_bg, func_id_rgb = func_id_alpha = 0): one raster per layer
// from the camera and one orthographic raster of the whole scene from the light, each leaving the face index of every pixel in
// aggrs_info[:, 1].  This pass turns those maps into the final frame: one thread per output pixel.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"

namespace lasr {

struct VisShade {
    float rgb[3];
    float z;                                  // camera-space depth of the shaded point
};

// Vertex record [12 floats]: camera-space position x y z, NDC x | normal x y z, NDC y | colour r g b, 0.
// Face record [8 floats]: unit face normal x y z, 0 | light-space plane a b c, 0 with w = a u + b v + c.
// The kernel reads, per shaded pixel, the face's vertex indices, its record and three vertex records; the shadow test reads a
// face index and a face record per PCF tap.  All of them are gathered from buffers that stay in L2.

// Fraction of the 3x3 PCF taps around light-space point (pu, pv) that reach depth pw unoccluded.  Tap k sits one texel
// (h = 2 half / S) away per step and names the texel it falls in.  The depths are compared at that texel's centre, which the face
// the light raster stored there is known to cover: the occluder's exact plane depth there against the receiver's own face plane
// extended to it (on a convex surface that tangent plane lies outside the body: no self-shadow).  A face never shadows itself.
__device__ __forceinline__ float vis_shadow(const float* __restrict__ smap, const float4* __restrict__ face_rec, float4 xf, int S,
                                            int F, int g, float pu, float pv, float pw, float ar, float br, float bias)
{
    const float h = 2.f / (xf.z * (float)S);
    const float halfS = 0.5f * (float)S, invS = 1.f / (float)S;
    int lit = 0;
#pragma unroll
    for (int j = -1; j <= 1; j++) {
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const float qu = pu + (float)i * h, qv = pv + (float)j * h;
            const float tx = ((qu - xf.x) * xf.z + 1.f) * halfS;
            const float ty = ((qv - xf.y) * xf.z + 1.f) * halfS;
            if (!(tx >= 0.f && tx < (float)S && ty >= 0.f && ty < (float)S)) {
                lit++;
                continue;
            }
            const int col = (int)tx, yi = (int)ty;
            const float fo = smap[(size_t)(S - 1 - yi) * S + col];   // the rasteriser's row flip: row 0 is NDC y = +1
            if (!(fo >= 0.f && fo < (float)F) || (int)fo == g) {
                lit++;
                continue;
            }
            const float uc = xf.x + (float)(2 * col + 1 - S) * invS / xf.z;   // the texel centre in light space
            const float vc = xf.y + (float)(2 * yi + 1 - S) * invS / xf.z;
            const float4 pl = face_rec[(size_t)(int)fo * 2 + 1];
            const float w_occ = pl.x * uc + pl.y * vc + pl.z;
            const float w_rec = pw + ar * (uc - pu) + br * (vc - pv);
            if (!(w_rec > w_occ + bias)) lit++;
        }
    }
    return (float)lit * (1.f / 9.f);
}

// Shades global face g at NDC point (xp, yp) of frame n; false when g names no usable face.
__device__ __forceinline__ bool vis_shade_face(const float4* __restrict__ vrec, const int4* __restrict__ faces,
                                               const float4* __restrict__ frec, const float* __restrict__ smap, float4 xf, int V,
                                               int F, int S, int g, float xp, float yp, const lasr_vis_params& p, VisShade& o)
{
    const int4 fi = faces[g];
    if ((unsigned)fi.x >= (unsigned)V || (unsigned)fi.y >= (unsigned)V || (unsigned)fi.z >= (unsigned)V) return false;
    const float4* r0 = vrec + (size_t)fi.x * 3;
    const float4* r1 = vrec + (size_t)fi.y * 3;
    const float4* r2 = vrec + (size_t)fi.z * 3;
    const float4 a0 = r0[0], b0 = r0[1], c0 = r0[2];
    const float4 a1 = r1[0], b1 = r1[1], c1 = r1[2];
    const float4 a2 = r2[0], b2 = r2[1], c2 = r2[2];
    // screen-space barycentrics of the pixel centre (vertex NDC: x in .w of the first float4, y in .w of the second)
    const float x0 = a0.w, y0 = b0.w, x1 = a1.w, y1 = b1.w, x2 = a2.w, y2 = b2.w;
    const float den = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    if (!(den != 0.f)) return false;
    float w0 = ((x1 - xp) * (y2 - yp) - (x2 - xp) * (y1 - yp)) / den;
    float w1 = ((x2 - xp) * (y0 - yp) - (x0 - xp) * (y2 - yp)) / den;
    float w2 = ((x0 - xp) * (y1 - yp) - (x1 - xp) * (y0 - yp)) / den;
    w0 = fminf(fmaxf(w0, 0.f), 1.f);
    w1 = fminf(fmaxf(w1, 0.f), 1.f);
    w2 = fminf(fmaxf(w2, 0.f), 1.f);
    // perspective-correct weights: screen barycentrics over camera depth, normalised
    float l0 = w0 / a0.z, l1 = w1 / a1.z, l2 = w2 / a2.z;
    const float ls = l0 + l1 + l2;
    if (!(ls > 0.f)) return false;
    l0 /= ls;
    l1 /= ls;
    l2 /= ls;
    const float px = l0 * a0.x + l1 * a1.x + l2 * a2.x;
    const float py = l0 * a0.y + l1 * a1.y + l2 * a2.y;
    const float pz = l0 * a0.z + l1 * a1.z + l2 * a2.z;
    const float4 fr = frec[(size_t)g * 2], fp = frec[(size_t)g * 2 + 1];
    float nx, ny, nz;
    if (p.smooth) {
        nx = l0 * b0.x + l1 * b1.x + l2 * b2.x;
        ny = l0 * b0.y + l1 * b1.y + l2 * b2.y;
        nz = l0 * b0.z + l1 * b1.z + l2 * b2.z;
        const float nn = sqrtf(nx * nx + ny * ny + nz * nz);
        if (nn > 1e-12f) {
            nx /= nn;
            ny /= nn;
            nz /= nn;
        } else {
            nx = fr.x;
            ny = fr.y;
            nz = fr.z;
        }
    } else {
        nx = fr.x;
        ny = fr.y;
        nz = fr.z;
    }
    if (nx * px + ny * py + nz * pz > 0.f) {        // two-sided: a normal turned away from the camera (at the origin) flips
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    const float ndl = fmaxf(0.f, -(nx * p.light_d[0] + ny * p.light_d[1] + nz * p.light_d[2]));
    float s = 1.f;
    if (ndl > 0.f) {
        const float pu = px * p.light_u[0] + py * p.light_u[1] + pz * p.light_u[2];
        const float pv = px * p.light_v[0] + py * p.light_v[1] + pz * p.light_v[2];
        const float pw = px * p.light_d[0] + py * p.light_d[1] + pz * p.light_d[2];
        s = vis_shadow(smap, frec, xf, S, F, g, pu, pv, pw, fp.x, fp.y, p.shadow_bias);
    }
    const float k = p.k_ambient + p.k_diffuse * ndl * s;
    o.rgb[0] = fminf(fmaxf(0.6f * (l0 * c0.x + l1 * c1.x + l2 * c2.x) * k, 0.f), 1.f);
    o.rgb[1] = fminf(fmaxf(0.6f * (l0 * c0.y + l1 * c1.y + l2 * c2.y) * k, 0.f), 1.f);
    o.rgb[2] = fminf(fmaxf(0.6f * (l0 * c0.z + l1 * c1.z + l2 * c2.z) * k, 0.f), 1.f);
    o.z = pz;
    return true;
}

__device__ __forceinline__ unsigned vis_u8(float c) { return (unsigned)__float2int_rn(c * 255.f); }   // c in [0, 1]

// One thread per pixel of the cropped H x W output of frame blockIdx.y.  Output: packed RGBA8 (r in the low byte, alpha 255).
__global__ __launch_bounds__(256) void vis_shade_kernel(const float4* __restrict__ vert_rec, const int4* __restrict__ faces,
                                                        const float4* __restrict__ face_rec, const float* __restrict__ raster0,
                                                        const float* __restrict__ raster1, const float* __restrict__ shadow,
                                                        const float4* __restrict__ shadow_xf, const unsigned* __restrict__ frames,
                                                        unsigned* __restrict__ out, int V, int F, int F0, int IS, int S, int H, int W,
                                                        lasr_vis_params p)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int n = blockIdx.y;
    const int r = i / W, c = i - r * W;
    const size_t P = (size_t)IS * IS, pix = (size_t)r * IS + c;
    const float yp = (float)(2 * (IS - 1 - r) + 1 - IS) / (float)IS;   // the rasteriser's pixel centres and row flip
    const float xp = (float)(2 * c + 1 - IS) / (float)IS;
    const float4* vrec = vert_rec + (size_t)n * V * 3;
    const float4* frec = face_rec + (size_t)n * F * 2;
    const float* smap = shadow + ((size_t)n * 2 + 1) * S * S;
    const float4 xf = shadow_xf[n];

    float rgb[3] = {p.background[0], p.background[1], p.background[2]};
    VisShade op, sf;
    const float f0 = raster0[((size_t)n * 2 + 1) * P + pix];
    const bool has0 = f0 >= 0.f && f0 < (float)F0 &&
                      vis_shade_face(vrec, faces, frec, smap, xf, V, F, S, (int)f0, xp, yp, p, op);
    if (has0) {
        rgb[0] = op.rgb[0];
        rgb[1] = op.rgb[1];
        rgb[2] = op.rgb[2];
    }
    if (raster1) {                                   // the translucent surface over the opaque layer
        const float f1 = raster1[((size_t)n * 2 + 1) * P + pix];
        if (f1 >= 0.f && f1 < (float)(F - F0) &&
            vis_shade_face(vrec, faces, frec, smap, xf, V, F, S, F0 + (int)f1, xp, yp, p, sf) && !(has0 && op.z < sf.z)) {
            const float a = p.surface_alpha;
            rgb[0] = a * sf.rgb[0] + (1.f - a) * rgb[0];
            rgb[1] = a * sf.rgb[1] + (1.f - a) * rgb[1];
            rgb[2] = a * sf.rgb[2] + (1.f - a) * rgb[2];
        }
    }
    unsigned u[3] = {vis_u8(fminf(fmaxf(rgb[0], 0.f), 1.f)), vis_u8(fminf(fmaxf(rgb[1], 0.f), 1.f)),
                     vis_u8(fminf(fmaxf(rgb[2], 0.f), 1.f))};
    const size_t o = (size_t)n * H * W + i;
    if (frames) {                                    // cv2.addWeighted(render, 0.5, frame, 0.5, 0): round half to even
        const unsigned fr = frames[o];
#pragma unroll
        for (int k = 0; k < 3; k++) u[k] = (unsigned)__float2int_rn(0.5f * (float)u[k] + 0.5f * (float)((fr >> (8 * k)) & 255u));
    }
    out[o] = u[0] | (u[1] << 8) | (u[2] << 16) | 0xff000000u;
}

}  // namespace lasr

extern "C" int lasr_vis_shade(const float* vert_rec, const int* faces, const float* face_rec, const float* raster0,
                              const float* raster1, const float* shadow, const float* shadow_xf, const unsigned* frames,
                              unsigned* out, int N, int V, int F, int F0, int IS, int S, int H, int W, const lasr_vis_params* params,
                              void* hip_stream)
{
    if (N < 0 || V < 1 || F < 1 || F0 < 1 || F0 > F || (!raster1 && F0 != F) || (raster1 && F0 == F)) return LASR_E_BADARG;
    if (IS < 1 || IS > LASR_VIS_MAX_SIZE || S < 1 || S > LASR_VIS_MAX_SIZE || H < 1 || H > IS || W < 1 || W > IS)
        return LASR_E_BADARG;
    if ((long long)V * 12 > 0x7fffffffLL || (long long)F * 8 > 0x7fffffffLL || N > 65535) return LASR_E_BADARG;
    if (!params) return LASR_E_BADARG;
    if (params->overlay && !frames) return LASR_E_BADARG;
    if (N == 0) return LASR_OK;
    if (!vert_rec || !faces || !face_rec || !raster0 || !shadow || !shadow_xf || !out) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const long long HW = (long long)H * W;
    LASR_LAUNCH(K_VIS_SHADE, lasr::vis_shade_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)N), dim3(256), 0,
                (const float4*)vert_rec, (const int4*)faces, (const float4*)face_rec, raster0, raster1, shadow,
                (const float4*)shadow_xf, params->overlay ? frames : nullptr, out, V, F, F0, IS, S, H, W, *params);
    return launch_ok();
}
