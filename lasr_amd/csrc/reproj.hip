// reproj.hip -- reprojection scores of scripts/eval_reproj.py (lasr_amd/nnutils/reproj.py walks the frames): per frame the
// hard-mode raster of the predicted mesh against the annotation (region similarity J and boundary measure F of DAVIS), the
// rendered flow to the next frame against the observed one (end-point error) and the vertex colours against the frame.  This is
// the project's own addition; the reference has no counterpart, and the definition is the one of include/lasr_ops.h and DESIGN.md
// section 4.15.  Conventions are those of tracks.hip, and the anchoring of a pixel centre is the very code of lasr_track_anchor
// (track_anchor.h).  A wave owns 64 consecutive columns of one row, so a ballot is a word of the bit map and the integer counts
// are popcounts, gathered over the sixteen waves of a workgroup before one atomic per counter (one per wave made the pixel pass
// wait on its own atomics: 1.6 ms a chunk of 1080p frames); the two floating-point sums go through per-workgroup partials in
// double and a second launch.  Integer atomics only: the same bits on every run and for any split of the frames into chunks.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"
#include "track_anchor.h"

namespace lasr {

typedef unsigned long long u64;

enum { RP_INTER, RP_UNION, RP_NPRED, RP_NGT, RP_NPB, RP_NGB, RP_PM, RP_GM, RP_NFLOW, RP_NLE1, RP_NLE3, RP_NRGB, RP_COUNTS };
static_assert(RP_COUNTS == 12, "counts is [n,12] in include/lasr_ops.h");

static const int RP_ROWS = 16;                                       // rows (waves) of a workgroup of the pixel pass
// the counters of the pixel pass in the order the workgroup gathers them
__device__ static const int RP_PIXEL_SLOTS[8] = {RP_INTER, RP_UNION, RP_NPRED, RP_NGT, RP_NFLOW, RP_NLE1, RP_NLE3, RP_NRGB};

__device__ __forceinline__ double rp_wave_sum(double v)              // a fixed tree: lane 0 holds the sum of the 64 lanes
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// Block (64, RP_ROWS): wave y owns the columns 64 blockIdx.x .. + 63 of row RP_ROWS blockIdx.y + y of frame blockIdx.z.
__global__ __launch_bounds__(64 * RP_ROWS) void reproj_pixel_kernel(const float* __restrict__ verts, const float* __restrict__ verts_next,
                                                           const int* __restrict__ faces, const float4* __restrict__ K,
                                                           const float4* __restrict__ K_next, const float* __restrict__ raster,
                                                           const unsigned char* __restrict__ gt, const float* __restrict__ flow,
                                                           const float* __restrict__ occ, const unsigned char* __restrict__ frames,
                                                           const unsigned char* __restrict__ colors, u64* __restrict__ bits,
                                                           u64* __restrict__ counts, double* __restrict__ partials, int V, int F,
                                                           int IS, int H, int W, int WW)
{
    __shared__ double red[RP_ROWS][2];
    __shared__ unsigned tally[RP_ROWS][8];                           // popcounts of the wave's ballots, RP_PIXEL_SLOTS order
    const int t = blockIdx.z, lane = threadIdx.x;
    const int row = blockIdx.y * RP_ROWS + threadIdx.y, col = blockIdx.x * 64 + lane;
    const bool in = row < H && col < W;
    const size_t pix = ((size_t)t * H + (in ? row : 0)) * W + (in ? col : 0);
    const float* plane = raster + ((size_t)t * 2 + 1) * IS * IS;
    const int face = in ? track_named(plane, IS, row, col, F) : -1;
    const bool pred = face >= 0;
    const bool ann = in && gt[pix] != 0;
    const u64 bp = __ballot(pred), bg = __ballot(ann);
    if (lane == 0 && row < H) {
        bits[(((size_t)t * 2) * H + row) * WW + blockIdx.x] = bp;
        bits[(((size_t)t * 2 + 1) * H + row) * WW + blockIdx.x] = bg;
    }
    u64 b_flow = 0ull, b_le1 = 0ull, b_le3 = 0ull, b_rgb = 0ull;
    double epe_sum = 0., sq_sum = 0.;
    if ((bp & bg) && (verts_next || frames)) {                       // wave-uniform
        bool anchored = false;
        int i0 = 0, i1 = 0, i2 = 0;
        float c1 = 0.f, c2 = 0.f;
        if (pred && ann) {
            i0 = faces[face * 3]; i1 = faces[face * 3 + 1]; i2 = faces[face * 3 + 2];
            if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
                const TrackFace tf = track_face(verts + (size_t)t * V * 3, i0, i1, i2);
                anchored = track_barycentrics(tf, K[t], (float)col + 0.5f, (float)row + 0.5f, c1, c2);
            }
        }
        if (frames) {
            float sq = 0.f;
            if (anchored) {
                const unsigned char* C = colors + (size_t)t * V * 3;
                const unsigned char* fr = frames + pix * 3;
                const float c0 = 1.f - c1 - c2;
                float d[3];
#pragma unroll
                for (int k = 0; k < 3; k++)
                    d[k] = (c0 * (float)C[i0 * 3 + k] + c1 * (float)C[i1 * 3 + k] + c2 * (float)C[i2 * 3 + k]) - (float)fr[k];
                sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            }
            b_rgb = __ballot(anchored);
            sq_sum = (double)sq;
        }
        if (verts_next) {
            bool ok = false;
            float epe = 0.f;
            if (anchored) {
                const float* fl = flow + pix * 3;
                const float fu = fl[0], fv = fl[1];
                ok = fl[2] != 0.f && fabsf(fu) <= 3.4028235e38f && fabsf(fv) <= 3.4028235e38f;
                if (ok && occ) ok = occ[pix] < 10.f;
                if (ok) {
                    const TrackFace tn = track_face(verts_next + (size_t)t * V * 3, i0, i1, i2);
                    float px, py, pz;
                    track_point(tn, c1, c2, px, py, pz);
                    ok = pz > 0.f;
                    if (ok) {
                        float u, v;
                        track_pinhole(K_next[t], px, py, pz, u, v);
                        const float du = (u - ((float)col + 0.5f)) - fu, dv = (v - ((float)row + 0.5f)) - fv;
                        epe = sqrtf(du * du + dv * dv);
                        ok = epe == epe;                             // a prediction that is not a number scores nothing
                        if (!ok) epe = 0.f;
                    }
                }
            }
            b_flow = __ballot(ok);
            b_le1 = __ballot(ok && epe <= 1.f);
            b_le3 = __ballot(ok && epe <= 3.f);
            epe_sum = (double)epe;
        }
        epe_sum = rp_wave_sum(epe_sum);
        sq_sum = rp_wave_sum(sq_sum);
    }
    if (lane == 0) {
        red[threadIdx.y][0] = epe_sum; red[threadIdx.y][1] = sq_sum;
        const u64 b[8] = {bp & bg, bp | bg, bp, bg, b_flow, b_le1, b_le3, b_rgb};
#pragma unroll
        for (int k = 0; k < 8; k++) tally[threadIdx.y][k] = (unsigned)__popcll(b[k]);
    }
    __syncthreads();
    if (threadIdx.y == 0 && lane < 8) {                              // one integer atomic per workgroup and counter
        unsigned c = 0;
        for (int y = 0; y < RP_ROWS; y++) c += tally[y][lane];
        if (c) atomicAdd(counts + (size_t)t * RP_COUNTS + RP_PIXEL_SLOTS[lane], (u64)c);
    } else if (threadIdx.y == 1 && lane < 2) {                       // the waves' sums in row order
        double a = 0.;
        for (int y = 0; y < RP_ROWS; y++) a += red[y][lane];
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.y;
        partials[((size_t)t * nblk + blk) * 2 + lane] = a;
    }
}

// One workgroup per frame: thread i folds the partials i, i + 256, ... in order, then the 256 results fold across halves.
__global__ __launch_bounds__(256) void reproj_reduce_kernel(const double* __restrict__ partials, double* __restrict__ sums, int nblk)
{
    __shared__ double acc[2][256];
    const int t = blockIdx.x, i = threadIdx.x;
    const double* p = partials + (size_t)t * nblk * 2;
    double a = 0., b = 0.;
    for (int j = i; j < nblk; j += 256) { a += p[(size_t)j * 2]; b += p[(size_t)j * 2 + 1]; }
    acc[0][i] = a; acc[1][i] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (i < s) { acc[0][i] += acc[0][i + s]; acc[1][i] += acc[1][i + s]; }
        __syncthreads();
    }
    if (i < 2) sums[(size_t)t * 2 + i] = acc[i][0];
}

// Boundary map of include/lasr_ops.h on the words of one map: one thread per (map, row, word) of frame blockIdx.y.
__global__ __launch_bounds__(256) void reproj_boundary_map_kernel(const u64* __restrict__ bits, u64* __restrict__ out, int H, int W,
                                                                  int WW)
{
    const long long per = (long long)2 * H * WW;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= per) return;
    const int w = (int)(idx % WW), row = (int)((idx / WW) % H);
    const size_t o = (size_t)blockIdx.y * per + idx;                 // (frame, map, row, word)
    const u64 seg = bits[o];
    const u64 segn = w + 1 < WW ? bits[o + 1] : 0ull;
    const u64 e = (seg >> 1) | (segn << 63);                         // e(r, c) = seg(r, c + 1); bits at or beyond W are 0
    u64 b;
    const int lastw = (W - 1) >> 6;
    const u64 lastbit = 1ull << ((W - 1) & 63);
    if (row + 1 < H) {
        const u64 s = bits[o + WW];
        const u64 sn = w + 1 < WW ? bits[o + WW + 1] : 0ull;
        const u64 se = (s >> 1) | (sn << 63);
        b = (seg ^ e) | (seg ^ s) | (seg ^ se);
        if (w == lastw) b = (b & ~lastbit) | ((seg ^ s) & lastbit);  // the last column is seg xor s
    } else {
        b = seg ^ e;                                                 // the last row is seg xor e
        if (w == lastw) b &= ~lastbit;                               // the last pixel is 0
    }
    out[o] = b;
}

__device__ __forceinline__ u64 rp_smear_up(u64 m, int h)            // OR of m << d, d = 0 .. min(h, 63), by doubling
{
    h = min(h, 63);
    for (int cur = 1; cur <= h;) {
        const int step = min(cur, h + 1 - cur);
        m |= m << step;
        cur += step;
    }
    return m;
}

__device__ __forceinline__ u64 rp_smear_down(u64 m, int h)
{
    h = min(h, 63);
    for (int cur = 1; cur <= h;) {
        const int step = min(cur, h + 1 - cur);
        m |= m >> step;
        cur += step;
    }
    return m;
}

// Word w of the row `p` (WW words) dilated along the row by |dx| <= h.  The own word is smeared both ways; of a word o places to
// the left only its highest bit matters (it reaches the columns up to hi + h - 64 o of this word), of one to the right its lowest.
__device__ __forceinline__ u64 rp_dilate_row(const u64* __restrict__ p, int w, int WW, int h)
{
    const u64 own = p[w];
    u64 d = rp_smear_up(own, h) | rp_smear_down(own, h);
    const int reach = (h + 63) >> 6;
    for (int o = 1; o <= reach; o++) {
        if (w - o >= 0) {
            const u64 m = p[w - o];
            if (m) {
                const int top = (63 - __clzll((long long)m)) + h - 64 * o;
                if (top >= 63) d = ~0ull;
                else if (top >= 0) d |= (2ull << top) - 1ull;
            }
        }
        if (w + o < WW) {
            const u64 m = p[w + o];
            if (m) {
                const int low = 64 * o + (__ffsll((unsigned long long)m) - 1) - h;
                if (low <= 0) d = ~0ull;
                else if (low < 64) d |= ~0ull << low;
            }
        }
    }
    return d;
}

// One thread per (row, word) of frame blockIdx.y: its boundary words against the disk dilation of the other map's.
__global__ __launch_bounds__(256) void reproj_boundary_match_kernel(const u64* __restrict__ bmap, u64* __restrict__ counts, int H,
                                                                    int WW, int radius)
{
    const long long per = (long long)H * WW;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < per;
    const int w = live ? (int)(idx % WW) : 0, row = live ? (int)(idx / WW) : 0;
    const u64* P = bmap + (size_t)blockIdx.y * 2 * per;              // boundary of pred
    const u64* G = P + per;                                          // boundary of gt
    const u64 bp = live ? P[idx] : 0ull, bg = live ? G[idx] : 0ull;
    u64 dil_g = 0ull, dil_p = 0ull;
    if (bp | bg) {
        const int r2 = radius * radius;
        for (int dy = -radius; dy <= radius; dy++) {
            const int y = row + dy;
            if (y < 0 || y >= H) continue;
            const int v = r2 - dy * dy;
            int h = (int)sqrtf((float)v);                            // floor(sqrt(v)) in integers
            while (h * h > v) h--;
            while ((h + 1) * (h + 1) <= v) h++;
            if (bp) dil_g |= rp_dilate_row(G + (size_t)y * WW, w, WW, h);
            if (bg) dil_p |= rp_dilate_row(P + (size_t)y * WW, w, WW, h);
        }
    }
    unsigned c[4] = {(unsigned)__popcll(bp), (unsigned)__popcll(bg), (unsigned)__popcll(bp & dil_g), (unsigned)__popcll(bg & dil_p)};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_down(c[k], o, 64);
        if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd(counts + (size_t)blockIdx.y * RP_COUNTS + RP_NPB + k, (u64)c[k]);
    }
}

static bool reproj_image_ok(int n, int H, int W)
{
    return n >= 0 && H >= 1 && W >= 1 && H <= LASR_TRACK_MAX_SIZE && W <= LASR_TRACK_MAX_SIZE;
}

static const int REPROJ_GRID_FRAMES = 65535;                         // frames per launch of the kernels that put the frame in the grid

}  // namespace lasr

extern "C" size_t lasr_reproj_workspace_bytes(int n, int H, int W)
{
    if (!lasr::reproj_image_ok(n, H, W)) return 0;
    const size_t WW = (size_t)(W + 63) / 64, HB = (size_t)(H + lasr::RP_ROWS - 1) / lasr::RP_ROWS;
    return (size_t)n * WW * HB * 2 * sizeof(double);
}

extern "C" int lasr_reproj_pixels(const float* verts, const float* verts_next, const int* faces, const float* K, const float* K_next,
                                  const float* raster, const unsigned char* gt, const float* flow, const float* occ,
                                  const unsigned char* frames, const unsigned char* colors, unsigned long long* bits,
                                  unsigned long long* counts, double* sums, void* workspace, int n, int V, int F, int IS, int H, int W,
                                  void* hip_stream)
{
    if (!lasr::reproj_image_ok(n, H, W)) return LASR_E_BADARG;
    if (V < 1 || F < 0 || H > IS || W > IS || IS > LASR_TRACK_MAX_SIZE || (long long)V * 3 > 0x7fffffffLL ||
        (long long)F * 3 > 0x7fffffffLL || F > (1 << 24))
        return LASR_E_BADARG;
    const bool any_flow = verts_next || K_next || flow || occ, all_flow = verts_next && K_next && flow;
    const bool any_rgb = frames || colors, all_rgb = frames && colors;
    if ((any_flow && !all_flow) || (any_rgb && !all_rgb)) return LASR_E_BADARG;    // an optional group comes whole or not at all
    if (n == 0) return LASR_OK;
    if (!verts || (!faces && F > 0) || !K || !raster || !gt || !bits || !counts || !sums || !workspace) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const int WW = (W + 63) / 64, HB = (H + lasr::RP_ROWS - 1) / lasr::RP_ROWS;
    const size_t P = (size_t)IS * IS, HW = (size_t)H * W, nblk = (size_t)WW * HB;
    double* partials = (double*)workspace;
    for (int f0 = 0; f0 < n; f0 += lasr::REPROJ_GRID_FRAMES) {
        const int m = n - f0 < lasr::REPROJ_GRID_FRAMES ? n - f0 : lasr::REPROJ_GRID_FRAMES;
        const size_t f = (size_t)f0;
        hipLaunchKernelGGL(lasr::reproj_pixel_kernel, dim3((unsigned)WW, (unsigned)HB, (unsigned)m), dim3(64, lasr::RP_ROWS), 0, st,
                           verts + f * V * 3, verts_next ? verts_next + f * V * 3 : nullptr, faces, (const float4*)K + f,
                           K_next ? (const float4*)K_next + f : nullptr, raster + f * 2 * P, gt + f * HW,
                           flow ? flow + f * HW * 3 : nullptr, occ ? occ + f * HW : nullptr, frames ? frames + f * HW * 3 : nullptr,
                           colors ? colors + f * V * 3 : nullptr, bits + f * 2 * H * WW, counts + f * lasr::RP_COUNTS,
                           partials + f * nblk * 2, V, F, IS, H, W, WW);
        hipLaunchKernelGGL(lasr::reproj_reduce_kernel, dim3((unsigned)m), dim3(256), 0, st, partials + f * nblk * 2, sums + f * 2,
                           (int)nblk);
    }
    return launch_ok();
}

extern "C" int lasr_reproj_boundary(const unsigned long long* bits, unsigned long long* scratch_bits, unsigned long long* counts, int n,
                                    int H, int W, int radius, void* hip_stream)
{
    if (!lasr::reproj_image_ok(n, H, W)) return LASR_E_BADARG;
    if (radius < 0 || radius > LASR_REPROJ_MAX_RADIUS) return LASR_E_BADARG;
    if (n == 0) return LASR_OK;
    if (!bits || !scratch_bits || !counts) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const int WW = (W + 63) / 64;
    const size_t per = (size_t)H * WW;
    for (int f0 = 0; f0 < n; f0 += lasr::REPROJ_GRID_FRAMES) {
        const int m = n - f0 < lasr::REPROJ_GRID_FRAMES ? n - f0 : lasr::REPROJ_GRID_FRAMES;
        const size_t f = (size_t)f0;
        hipLaunchKernelGGL(lasr::reproj_boundary_map_kernel, dim3((unsigned)((2 * per + 255) / 256), (unsigned)m), dim3(256), 0, st,
                           bits + f * 2 * per, scratch_bits + f * 2 * per, H, W, WW);
        hipLaunchKernelGGL(lasr::reproj_boundary_match_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)m), dim3(256), 0, st,
                           scratch_bits + f * 2 * per, counts + f * lasr::RP_COUNTS, H, WW, radius);
    }
    return launch_ok();
}
