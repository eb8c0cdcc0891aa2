// tracks.hip -- dense long-range point tracks of scripts/export_tracks.py (lasr_amd/nnutils/tracks.py walks the frames): query
// pixels are anchored on the surface of the frame they name (face + barycentrics) and carried through every frame with a
// visibility decision.  This is the project's own addition; the reference has no counterpart, and the definition is the one of
// include/lasr_ops.h and DESIGN.md section 4.14.  Conventions are those of bake.hip: camera-space verts with OpenCV axes, shared
// faces, K = fx fy px py in pixels, and plane 1 of the hard-mode raster's aggrs_info naming the nearest face of every pixel.
// One thread per query (anchor) or per (frame, query) with the query index fastest (project): no atomics, the same bits for any
// split of the frames into windows.  The preview's key pass uses an integer atomicMax, which is order-independent.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"
#include "track_anchor.h"

namespace lasr {

// One thread per query.  verts / K / raster hold the n frames t0 .. t0 + n - 1.
__global__ __launch_bounds__(256) void track_anchor_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                           const float4* __restrict__ K, const float* __restrict__ raster,
                                                           const float* __restrict__ queries, float4* __restrict__ anchors,
                                                           float2* __restrict__ snapped, int t0, int n, int Q, int V, int F, int IS,
                                                           int H, int W, int snap)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const float tq = queries[(size_t)q * 3];
    if (!(tq >= (float)t0 && tq < (float)(t0 + n))) return;         // another window's query (or not a number): left untouched
    const int t = (int)tq - t0;
    float v = queries[(size_t)q * 3 + 1], u = queries[(size_t)q * 3 + 2];
    float4 rec = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
    int face = -1;
    const float* plane = raster + ((size_t)t * 2 + 1) * IS * IS;
    if (u >= 0.f && u < (float)W && v >= 0.f && v < (float)H) {
        const int col = (int)u, row = (int)v;
        face = track_named(plane, IS, row, col, F);
        if (face < 0 && snap > 0) {
            float best = 3.4e38f;
            int br = -1, bc = -1;
            const int r0 = max(row - snap, 0), r1 = min(row + snap, H - 1);
            const int c0 = max(col - snap, 0), c1 = min(col + snap, W - 1);
            for (int r = r0; r <= r1; r++)                           // increasing flat index: a strict < keeps the lowest on ties
                for (int c = c0; c <= c1; c++) {
                    const int g = track_named(plane, IS, r, c, F);
                    const float du = ((float)c + 0.5f) - u, dv = ((float)r + 0.5f) - v;
                    const float d = du * du + dv * dv;
                    if (g >= 0 && d < best) { best = d; br = r; bc = c; face = g; }
                }
            if (face >= 0) { u = (float)bc + 0.5f; v = (float)br + 0.5f; }
        }
    }
    snapped[q] = make_float2(v, u);
    if (face >= 0) {
        const int i0 = faces[face * 3], i1 = faces[face * 3 + 1], i2 = faces[face * 3 + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            const TrackFace tf = track_face(verts + (size_t)t * V * 3, i0, i1, i2);
            const float4 k = K[t];
            float c1, c2;
            if (track_barycentrics(tf, k, u, v, c1, c2)) {           // step 3 (track_anchor.h, shared with reproj.hip)
                float px, py, pz;
                track_point(tf, c1, c2, px, py, pz);
                const float np = tf.nx * px + tf.ny * py + tf.nz * pz;
                rec = make_float4(__int_as_float(face), c1, c2, np >= 0.f ? 1.f : -1.f);
            }
        }
    }
    anchors[q] = rec;
}

// One thread per (frame, query): blockIdx.y is the frame of the window, so K and the frame's base pointers are wave-uniform.
__global__ __launch_bounds__(256) void track_project_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                            const float4* __restrict__ K, const float* __restrict__ raster,
                                                            const float4* __restrict__ anchors, float2* __restrict__ tracks,
                                                            unsigned char* __restrict__ state, int Q, int V, int F, int IS, int H,
                                                            int W, int win)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int t = blockIdx.y;
    const float4 rec = anchors[q];                                   // one 16-byte load
    const int face = __float_as_int(rec.x);
    const float nanv = __int_as_float(0x7fc00000);
    float2 out = make_float2(nanv, nanv);
    unsigned char st = 0;
    int i0 = 0, i1 = 0, i2 = 0;
    bool ok = face >= 0 && face < F;
    if (ok) {
        i0 = faces[face * 3]; i1 = faces[face * 3 + 1]; i2 = faces[face * 3 + 2];
        ok = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
    }
    if (ok) {
        const TrackFace tf = track_face(verts + (size_t)t * V * 3, i0, i1, i2);
        float px, py, pz;
        track_point(tf, rec.y, rec.z, px, py, pz);
        if (!(pz > 0.f)) {
            st = 4;
        } else {
            const float4 k = K[t];
            float u, v;
            track_pinhole(k, px, py, pz, u, v);
            out = make_float2(u, v);
            if (!(u >= 0.f && u < (float)W && v >= 0.f && v < (float)H)) {
                st = 3;
            } else {
                const float np = tf.nx * px + tf.ny * py + tf.nz * pz;
                bool vis = ((np >= 0.f) ? 1.f : -1.f) == rec.w;      // (a) the same side of the face as at the anchor
                if (vis) {                                           // (b) the face or a vertex-neighbour of it owns a window pixel
                    const float* plane = raster + ((size_t)t * 2 + 1) * IS * IS;
                    const int col = (int)u, row = (int)v;
                    const int r0 = max(row - win, 0), r1 = min(row + win, H - 1);
                    const int c0 = max(col - win, 0), c1 = min(col + win, W - 1);
                    bool hit = false;
                    for (int r = r0; r <= r1 && !hit; r++)
                        for (int c = c0; c <= c1 && !hit; c++) {
                            const int g = track_named(plane, IS, r, c, F);
                            if (g < 0) continue;
                            if (g == face) { hit = true; break; }
                            const int j0 = faces[g * 3], j1 = faces[g * 3 + 1], j2 = faces[g * 3 + 2];
                            hit = j0 == i0 || j0 == i1 || j0 == i2 || j1 == i0 || j1 == i1 || j1 == i2 || j2 == i0 || j2 == i1 ||
                                  j2 == i2;
                        }
                    vis = hit;
                }
                st = vis ? 1 : 2;
            }
        }
    }
    const size_t o = (size_t)t * Q + q;
    tracks[o] = out;
    state[o] = st;
}

// Preview, pass 1: one thread per (frame, query); a visible point raises the keys of its disc to q + 1.
__global__ __launch_bounds__(256) void track_splat_keys_kernel(const float2* __restrict__ tracks, const unsigned char* __restrict__ state,
                                                               unsigned* __restrict__ keys, int Q, int H, int W, int radius)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int t = blockIdx.y;
    const size_t o = (size_t)t * Q + q;
    if (state[o] != 1) return;
    const float2 p = tracks[o];
    if (!(p.x >= 0.f && p.x < (float)W && p.y >= 0.f && p.y < (float)H)) return;   // state 1 implies it; a foreign array may not
    const int col = (int)p.x, row = (int)p.y;
    unsigned* plane = keys + (size_t)t * H * W;
    for (int dy = -radius; dy <= radius; dy++) {
        const int r = row + dy;
        if (r < 0 || r >= H) continue;
        for (int dx = -radius; dx <= radius; dx++) {
            const int c = col + dx;
            if (c < 0 || c >= W || dx * dx + dy * dy > radius * radius) continue;
            atomicMax(plane + (size_t)r * W + c, (unsigned)q + 1u);
        }
    }
}

// Preview, pass 2: one thread per pixel of the n frames.
__global__ __launch_bounds__(256) void track_splat_resolve_kernel(const unsigned* __restrict__ keys, const unsigned char* __restrict__ colors,
                                                                  const unsigned char* __restrict__ frames, unsigned char* __restrict__ out,
                                                                  long long pixels, int Q)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= pixels) return;
    const unsigned key = keys[i];
    const bool on = key > 0u && key <= (unsigned)Q;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const unsigned f = frames[i * 3 + ch];
        unsigned o = f;
        if (on) {
            const unsigned c = colors[(size_t)(key - 1u) * 3 + ch];
            o = (LASR_TRACK_SPLAT_ALPHA * c + (255u - LASR_TRACK_SPLAT_ALPHA) * f + 127u) / 255u;
        }
        out[i * 3 + ch] = (unsigned char)o;
    }
}

static bool track_sizes_ok(int n, int Q, int V, int F, int IS, int H, int W)
{
    return n >= 0 && Q >= 0 && V >= 1 && F >= 0 && H >= 1 && W >= 1 && H <= IS && W <= IS && IS <= LASR_TRACK_MAX_SIZE &&
           (long long)V * 3 <= 0x7fffffffLL && (long long)F * 3 <= 0x7fffffffLL && F <= (1 << 24);
}

static bool track_image_ok(int n, int Q, int H, int W)
{
    return n >= 0 && Q >= 0 && H >= 1 && W >= 1 && H <= LASR_TRACK_MAX_SIZE && W <= LASR_TRACK_MAX_SIZE;
}

static const int TRACK_GRID_Y = 65535;                               // frames per launch of the kernels that put the frame in blockIdx.y

}  // namespace lasr

extern "C" int lasr_track_anchor(const float* verts, const int* faces, const float* K, const float* raster, const float* queries,
                                 void* anchors, float* snapped, int t0, int n, int Q, int V, int F, int IS, int H, int W,
                                 int snap_radius, void* hip_stream)
{
    if (!lasr::track_sizes_ok(n, Q, V, F, IS, H, W)) return LASR_E_BADARG;
    if (t0 < 0 || (long long)t0 + n > (1 << 24)) return LASR_E_BADARG;    // frame positions are exact in fp32
    if (snap_radius < 0 || snap_radius > LASR_TRACK_MAX_SNAP) return LASR_E_BADARG;
    if (n == 0 || Q == 0) return LASR_OK;
    if (!verts || (!faces && F > 0) || !K || !raster || !queries || !anchors || !snapped) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(lasr::track_anchor_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, verts, faces, (const float4*)K,
                       raster, queries, (float4*)anchors, (float2*)snapped, t0, n, Q, V, F, IS, H, W, snap_radius);
    return launch_ok();
}

extern "C" int lasr_track_project(const float* verts, const int* faces, const float* K, const float* raster, const void* anchors,
                                  float* tracks, unsigned char* state, int n, int Q, int V, int F, int IS, int H, int W, int window,
                                  void* hip_stream)
{
    if (!lasr::track_sizes_ok(n, Q, V, F, IS, H, W)) return LASR_E_BADARG;
    if (window < 0 || window > LASR_TRACK_MAX_WINDOW) return LASR_E_BADARG;
    if (n == 0 || Q == 0) return LASR_OK;
    if (!verts || (!faces && F > 0) || !K || !raster || !anchors || !tracks || !state) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t P = (size_t)IS * IS;
    for (int f0 = 0; f0 < n; f0 += lasr::TRACK_GRID_Y) {
        const int m = n - f0 < lasr::TRACK_GRID_Y ? n - f0 : lasr::TRACK_GRID_Y;
        hipLaunchKernelGGL(lasr::track_project_kernel, dim3((unsigned)((Q + 255) / 256), (unsigned)m), dim3(256), 0, st,
                           verts + (size_t)f0 * V * 3, faces, (const float4*)K + f0, raster + (size_t)f0 * 2 * P,
                           (const float4*)anchors, (float2*)tracks + (size_t)f0 * Q, state + (size_t)f0 * Q, Q, V, F, IS, H, W, window);
    }
    return launch_ok();
}

extern "C" int lasr_track_splat_keys(const float* tracks, const unsigned char* state, unsigned* keys, int n, int Q, int H, int W,
                                     int radius, void* hip_stream)
{
    if (!lasr::track_image_ok(n, Q, H, W)) return LASR_E_BADARG;
    if (radius < 0 || radius > LASR_TRACK_MAX_RADIUS) return LASR_E_BADARG;
    if (n == 0 || Q == 0) return LASR_OK;
    if (!tracks || !state || !keys) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    for (int f0 = 0; f0 < n; f0 += lasr::TRACK_GRID_Y) {
        const int m = n - f0 < lasr::TRACK_GRID_Y ? n - f0 : lasr::TRACK_GRID_Y;
        hipLaunchKernelGGL(lasr::track_splat_keys_kernel, dim3((unsigned)((Q + 255) / 256), (unsigned)m), dim3(256), 0, st,
                           (const float2*)tracks + (size_t)f0 * Q, state + (size_t)f0 * Q, keys + (size_t)f0 * H * W, Q, H, W, radius);
    }
    return launch_ok();
}

extern "C" int lasr_track_splat_resolve(const unsigned* keys, const unsigned char* colors, const unsigned char* frames,
                                        unsigned char* out, int n, int Q, int H, int W, void* hip_stream)
{
    if (!lasr::track_image_ok(n, Q, H, W)) return LASR_E_BADARG;
    const long long pixels = (long long)n * H * W;
    if (pixels > 0x7fffffffLL * 256) return LASR_E_BADARG;
    if (n == 0) return LASR_OK;
    if (!keys || (!colors && Q > 0) || !frames || !out) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(lasr::track_splat_resolve_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, st, keys, colors,
                       frames, out, pixels, Q);
    return launch_ok();
}
