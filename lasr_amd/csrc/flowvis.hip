// flowvis.hip -- the training monitor's device side (lasr_amd/nnutils/monitor.py, lasr_amd/ext_utils/flowlib.py; DESIGN.md
// section 4.10): Middlebury colour coding of flow fields, the 3 x 3 contact sheet of an epoch and the ring of per-step scalars.
// Nothing here is on the optimisation's critical path; the point is that watching a run costs no host synchronisation per step.
//
// Reductions are order-independent by construction: maxima and minima go through integer atomicMax on an order-preserving bit
// pattern (one per block and statistic), sums are taken in a fixed order without atomics.  The statistics words live in
// caller-owned scratch that is zero before a call and zero again after it: the last block of the second launch (found by a
// ticket counter in the same scratch) clears them, so no memset launch precedes a call.
#include <stdint.h>

#include <algorithm>

#include "../../include/lasr_ops.h"
#include "ops_common.h"

namespace lasr {

constexpr int FV_NCOLS = 55;                  // RY 15 + YG 6 + GC 4 + CB 11 + BM 13 + MR 6
constexpr float FV_UNKNOWN = 1e7f;            // flowlib's UNKNOWN_FLOW_THRESH
constexpr float FV_EPS = 2.220446049250313e-16f;   // numpy's finfo(float).eps, the reference's guard of the division
constexpr float FV_PI = 3.14159265358979323846f;

// The Middlebury colour wheel (make_color_wheel): six linear ramps, floor(255 i / n) along each.
struct FvWheel { unsigned char c[FV_NCOLS][3]; };

static FvWheel fv_make_wheel()
{
    FvWheel w;
    const int seg[6] = {15, 6, 4, 11, 13, 6};
    int col = 0;
    for (int s = 0; s < 6; s++) {
        for (int i = 0; i < seg[s]; i++, col++) {
            const int up = (255 * i) / seg[s], down = 255 - up;
            int r = 0, g = 0, b = 0;
            switch (s) {
                case 0: r = 255; g = up; break;       // red -> yellow
                case 1: r = down; g = 255; break;     // yellow -> green
                case 2: g = 255; b = up; break;       // green -> cyan
                case 3: g = down; b = 255; break;     // cyan -> blue
                case 4: b = 255; r = up; break;       // blue -> magenta
                default: b = down; r = 255; break;    // magenta -> red
            }
            w.c[col][0] = (unsigned char)r; w.c[col][1] = (unsigned char)g; w.c[col][2] = (unsigned char)b;
        }
    }
    return w;
}

// A flow sample as the colour coding sees it: masked, unknown (|u| or |v| > 1e7) and NaN samples count as (0, 0).
struct FvSample { float u, v; bool dark; };

__device__ __forceinline__ FvSample fv_sample(float u, float v, bool masked_out)
{
    FvSample s;
    if (masked_out) { u = 0.f; v = 0.f; }
    s.dark = (fabsf(u) > FV_UNKNOWN) || (fabsf(v) > FV_UNKNOWN) || (u != u) || (v != v);
    s.u = s.dark ? 0.f : u;
    s.v = s.dark ? 0.f : v;
    return s;
}

__device__ __forceinline__ float fv_radius(const FvSample& s) { return sqrtf(s.u * s.u + s.v * s.v); }

__device__ __forceinline__ unsigned fv_level(float x)      // uint8(floor(x)) for x in [0, 255]
{
    return (unsigned)fminf(fmaxf(floorf(x), 0.f), 255.f);
}

// compute_color for one sample normalised by the image's maximum radius -> r | g << 8 | b << 16
__device__ __forceinline__ unsigned fv_colour(const FvSample& s, float maxrad, const unsigned char (*wheel)[4])
{
    if (s.dark) return 0u;
    const float den = maxrad + FV_EPS;
    const float u = s.u / den, v = s.v / den;
    const float rad = sqrtf(u * u + v * v);
    const float a = atan2f(-v, -u) / FV_PI;
    const float fk = (a + 1.f) / 2.f * (float)(FV_NCOLS - 1) + 1.f;
    int k0 = (int)floorf(fk);
    k0 = min(max(k0, 1), FV_NCOLS);
    const int k1 = (k0 == FV_NCOLS) ? 1 : k0 + 1;
    const float f = fk - (float)k0;
    unsigned out = 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float col0 = (float)wheel[k0 - 1][c] / 255.f, col1 = (float)wheel[k1 - 1][c] / 255.f;
        float col = (1.f - f) * col0 + f * col1;
        col = (rad <= 1.f) ? 1.f - rad * (1.f - col) : col * 0.75f;
        out |= fv_level(255.f * col) << (8 * c);
    }
    return out;
}

__device__ __forceinline__ void fv_load_wheel(unsigned char (*wheel)[4], const FvWheel& w)
{
    for (int i = threadIdx.x; i < FV_NCOLS; i += blockDim.x) {
        wheel[i][0] = w.c[i][0]; wheel[i][1] = w.c[i][1]; wheel[i][2] = w.c[i][2]; wheel[i][3] = 0;
    }
    __syncthreads();
}

// order-preserving map float -> uint32 (NaN never reaches it), so that atomicMax on words that start at 0 gives the float maximum
__device__ __forceinline__ unsigned fv_ordered(float x)
{
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float fv_unordered(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// Maximum over a 256-thread block of NSTAT words per thread; thread s < NSTAT of wave 0 issues the one atomicMax of statistic s.
template <int NSTAT>
__device__ __forceinline__ void block_max_to_global(unsigned (&v)[NSTAT], unsigned* dst, unsigned (*red)[NSTAT])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NSTAT; s++) {
        const unsigned m = wave_max_u32(v[s]);
        if (lane == 0) red[wave][s] = m;
    }
    __syncthreads();
    if (threadIdx.x < NSTAT) {
        const int s = threadIdx.x;
        const unsigned m = max(max(red[0][s], red[1][s]), max(red[2][s], red[3][s]));
        if (m != 0u) atomicMax(dst + s, m);
    }
}

// The last block of a launch to get here clears the statistics words and the ticket itself.  Every block has consumed the
// statistics it needs before it draws its ticket.
__device__ __forceinline__ void fv_release_stats(unsigned* stats, int n_stats, unsigned n_blocks)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned t = atomicAdd(stats + n_stats, 1u);
        if (t == n_blocks - 1u) {
            for (int i = 0; i <= n_stats; i++) stats[i] = 0u;
            __threadfence();
        }
    }
}

// ---- lasr_flow_to_image ------------------------------------------------------------------------------------------------------
// pass 1: stats[b] = bit pattern of the maximum radius of image b (radii are >= 0: integer order = float order)
template <int C>
__global__ __launch_bounds__(256) void flow_maxrad_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                          unsigned* __restrict__ stats, long long HW)
{
    __shared__ unsigned red[4][1];
    const int b = blockIdx.y;
    const float* f = flow + (size_t)b * HW * C;
    const float* m = mask ? mask + (size_t)b * HW : nullptr;
    unsigned best[1] = {0u};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
        const FvSample s = fv_sample(f[i * C], f[i * C + 1], m && m[i] == 0.f);
        best[0] = max(best[0], __float_as_uint(fv_radius(s)));
    }
    block_max_to_global<1>(best, stats + b, red);
}

// pass 2: every lane owns 4 consecutive pixels of the flattened batch, whose 12 bytes leave as three dword stores
template <int C>
__global__ __launch_bounds__(256) void flow_colour_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                          unsigned char* __restrict__ out, unsigned* __restrict__ stats,
                                                          long long HW, long long P, int B, FvWheel w, int vec)
{
    __shared__ unsigned char wheel[FV_NCOLS][4];
    fv_load_wheel(wheel, w);
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long p0 = g * 4;
    if (p0 < P) {
        float in[4 * C];
        float mk[4] = {1.f, 1.f, 1.f, 1.f};
        const int n = (int)min(4LL, P - p0);
        if (n == 4 && vec) {
            const float4* q = reinterpret_cast<const float4*>(flow + p0 * C);
#pragma unroll
            for (int j = 0; j < C; j++) {
                const float4 t = q[j];
                in[4 * j] = t.x; in[4 * j + 1] = t.y; in[4 * j + 2] = t.z; in[4 * j + 3] = t.w;
            }
            if (mask) {
                const float4 t = *reinterpret_cast<const float4*>(mask + p0);
                mk[0] = t.x; mk[1] = t.y; mk[2] = t.z; mk[3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool live = j < n;
                in[j * C] = live ? flow[(p0 + j) * C] : 0.f;
                in[j * C + 1] = live ? flow[(p0 + j) * C + 1] : 0.f;
                if (mask) mk[j] = live ? mask[p0 + j] : 1.f;
            }
        }
        unsigned rgb[4];
        long long b = p0 / HW;
        long long next = (b + 1) * HW;                     // first pixel of the next image
        float maxrad = __uint_as_float(stats[b]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (p0 + j >= next && b + 1 < B) {
                b++;
                next += HW;
                maxrad = __uint_as_float(stats[b]);
            }
            rgb[j] = fv_colour(fv_sample(in[j * C], in[j * C + 1], mk[j] == 0.f), maxrad, wheel);
        }
        unsigned char* o = out + p0 * 3;
        if (n == 4) {
            unsigned* o4 = reinterpret_cast<unsigned*>(o);      // 12 g bytes past a 4-byte aligned base
            o4[0] = rgb[0] | (rgb[1] << 24);
            o4[1] = (rgb[1] >> 8) | (rgb[2] << 16);
            o4[2] = (rgb[2] >> 16) | (rgb[3] << 8);
        } else {
            for (int j = 0; j < n; j++) {
                o[3 * j] = (unsigned char)(rgb[j] & 255u);
                o[3 * j + 1] = (unsigned char)((rgb[j] >> 8) & 255u);
                o[3 * j + 2] = (unsigned char)(rgb[j] >> 16);
            }
        }
    }
    fv_release_stats(stats, B, gridDim.x);
}

// ---- lasr_monitor_sheet ------------------------------------------------------------------------------------------------------
enum { SH_RAD_OBS = 0, SH_RAD_RD, SH_ERR_MAX, SH_ERR_NMIN, SH_PRED_MAX, SH_PRED_NMIN, SH_GT_MAX, SH_GT_NMIN, SH_NSTAT };

__device__ __forceinline__ float sh_at(const lasr_sheet_plane& p, int c, long long i)
{
    return p.ptr[c * p.chan_stride + i * p.pix_stride];
}

// maximum and (as the maximum of the complemented key) minimum of a min-max panel; NaN samples take no part
__device__ __forceinline__ void sh_minmax(float x, unsigned& mx, unsigned& nmin)
{
    if (x != x) return;
    const unsigned k = fv_ordered(x);
    mx = max(mx, k);
    nmin = max(nmin, ~k);
}

__global__ __launch_bounds__(256) void sheet_stats_kernel(lasr_sheet_inputs in, unsigned* __restrict__ stats, int IS)
{
    __shared__ unsigned red[4][SH_NSTAT];
    unsigned v[SH_NSTAT];
#pragma unroll
    for (int s = 0; s < SH_NSTAT; s++) v[s] = 0u;
    const long long HW = (long long)IS * IS;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
        const float m = sh_at(in.vis_mask, 0, i);
        const bool off = m == 0.f;
        v[SH_RAD_OBS] = max(v[SH_RAD_OBS], __float_as_uint(fv_radius(fv_sample(sh_at(in.flow_obs, 0, i), sh_at(in.flow_obs, 1, i), off))));
        v[SH_RAD_RD] = max(v[SH_RAD_RD], __float_as_uint(fv_radius(fv_sample(sh_at(in.flow_rd, 0, i), sh_at(in.flow_rd, 1, i), off))));
        sh_minmax(sh_at(in.flow_err, 0, i) * m, v[SH_ERR_MAX], v[SH_ERR_NMIN]);
        sh_minmax(sh_at(in.mask_pred, 0, i), v[SH_PRED_MAX], v[SH_PRED_NMIN]);
        sh_minmax(sh_at(in.mask_gt, 0, i), v[SH_GT_MAX], v[SH_GT_NMIN]);
    }
    block_max_to_global<SH_NSTAT>(v, stats, red);
}

// floor(255 (x - min) / (max - min)) clipped to 0..255; a constant or empty panel and NaN samples come out 0
__device__ __forceinline__ unsigned sh_scaled(float x, unsigned kmax, unsigned knmin)
{
    if (kmax == 0u || x != x) return 0u;
    const float hi = fv_unordered(kmax), lo = fv_unordered(~knmin);
    if (!(hi > lo)) return 0u;
    const unsigned l = fv_level(255.f * (x - lo) / (hi - lo));
    return l | (l << 8) | (l << 16);
}

__device__ __forceinline__ unsigned sh_rgb(const lasr_sheet_plane& p, long long i)     // floor(255 x) clipped, per channel
{
    unsigned out = 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float x = 255.f * sh_at(p, c, i);
        out |= (x != x ? 0u : fv_level(x)) << (8 * c);
    }
    return out;
}

__global__ __launch_bounds__(256) void sheet_compose_kernel(lasr_sheet_inputs in, unsigned char* __restrict__ out,
                                                            unsigned* __restrict__ stats, int IS, FvWheel w)
{
    __shared__ unsigned char wheel[FV_NCOLS][4];
    __shared__ unsigned st[SH_NSTAT];
    if (threadIdx.x < SH_NSTAT) st[threadIdx.x] = stats[threadIdx.x];
    fv_load_wheel(wheel, w);                               // ends with the barrier that also publishes st
    const int W3 = 3 * IS;
    const long long P = (long long)W3 * W3;
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 < P) {
        const int n = (int)min(4LL, P - p0);
        const float half = 0.5f * (float)IS;
        unsigned rgb[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < n; j++) {
            const long long p = p0 + j;
            const int R = (int)(p / W3), Cc = (int)(p - (long long)R * W3);
            const int tr = R / IS, tc = Cc / IS;
            const int r = R - tr * IS, c = Cc - tc * IS;
            const long long i = (long long)r * IS + c;
            unsigned px = 0u;
            switch (tr * 3 + tc) {
                case 0:
                    px = fv_colour(fv_sample(sh_at(in.flow_obs, 0, i), sh_at(in.flow_obs, 1, i), sh_at(in.vis_mask, 0, i) == 0.f),
                                   __uint_as_float(st[SH_RAD_OBS]), wheel);
                    break;
                case 1:
                    px = fv_colour(fv_sample(sh_at(in.flow_rd, 0, i), sh_at(in.flow_rd, 1, i), sh_at(in.vis_mask, 0, i) == 0.f),
                                   __uint_as_float(st[SH_RAD_RD]), wheel);
                    break;
                case 2: px = sh_scaled(sh_at(in.flow_err, 0, i) * sh_at(in.vis_mask, 0, i), st[SH_ERR_MAX], st[SH_ERR_NMIN]); break;
                case 3: px = sh_scaled(sh_at(in.mask_pred, 0, i), st[SH_PRED_MAX], st[SH_PRED_NMIN]); break;
                case 4: px = sh_scaled(sh_at(in.mask_gt, 0, i), st[SH_GT_MAX], st[SH_GT_NMIN]); break;
                case 5: px = in.part.ptr ? sh_rgb(in.part, i) : 0u; break;
                case 6: px = sh_rgb(in.img1, i); break;
                case 7: px = sh_rgb(in.img2, i); break;
                default: {
                    px = sh_rgb(in.texture, i);
                    // bone marks: a ring of radii 1.5 .. 4.5 (pixel centres on the integer grid) around IS/2 + IS/2 (x, y), later
                    // bones over earlier ones; a NaN centre marks nothing
                    for (int k = 0; k < in.n_ctl; k++) {
                        const float cx = half + half * in.ctl[(long long)k * in.ctl_stride];
                        const float cy = half + half * in.ctl[(long long)k * in.ctl_stride + 1];
                        const float dx = (float)c - cx, dy = (float)r - cy;
                        const float d2 = dx * dx + dy * dy;
                        if (d2 >= 2.25f && d2 <= 20.25f)
                            px = fv_level(in.palette[3 * k]) | (fv_level(in.palette[3 * k + 1]) << 8) | (fv_level(in.palette[3 * k + 2]) << 16);
                    }
                }
            }
            rgb[j] = px;
        }
        unsigned char* o = out + p0 * 3;
        if (n == 4) {
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
            o4[0] = rgb[0] | (rgb[1] << 24);
            o4[1] = (rgb[1] >> 8) | (rgb[2] << 16);
            o4[2] = (rgb[2] >> 16) | (rgb[3] << 8);
        } else {
            for (int j = 0; j < n; j++) {
                o[3 * j] = (unsigned char)(rgb[j] & 255u);
                o[3 * j + 1] = (unsigned char)((rgb[j] >> 8) & 255u);
                o[3 * j + 2] = (unsigned char)(rgb[j] >> 16);
            }
        }
    }
    fv_release_stats(stats, SH_NSTAT, gridDim.x);
}

// ---- lasr_scalar_ring_push ---------------------------------------------------------------------------------------------------
// One block.  Wave w takes scalars w, w + 4, ...: lane l adds elements l, l + 64, ... in that order, the 64 partial sums fold
// through a fixed butterfly.  The head counter advances after every wave has used it.
__global__ __launch_bounds__(256) void scalar_ring_push_kernel(const long long* __restrict__ table, int K, float* __restrict__ ring,
                                                               unsigned* __restrict__ head, int capacity)
{
    const unsigned h = *head;
    float* row = ring + (size_t)(h % (unsigned)capacity) * K;
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < K; k += 4) {
        const float* src = reinterpret_cast<const float*>(table[2 * k]);
        const long long count = table[2 * k + 1];
        float s = 0.f;
        if (src)
            for (long long i = lane; i < count; i += 64) s += src[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) row[k] = (src && count > 0) ? s / (float)count : __uint_as_float(0x7fc00000u);
    }
    __syncthreads();
    if (threadIdx.x == 0) *head = h + 1u;
}

}  // namespace lasr

static bool fv_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int lasr_flow_to_image(const float* flow, const float* mask, unsigned char* out, void* stats_scratch, int B, int H, int W,
                                  int C, void* hip_stream)
{
    if (B < 0 || H < 0 || W < 0 || (C != 2 && C != 3) || B > 65535) return LASR_E_BADARG;
    const long long HW = (long long)H * W, P = HW * B;
    if (P == 0) return LASR_OK;
    if (P > 0x7fffffffLL / 4) return LASR_E_BADARG;
    if (!flow || !out || !stats_scratch || !fv_aligned(out, 4) || !fv_aligned(flow, 4) || !fv_aligned(mask, 4)) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    unsigned* stats = (unsigned*)stats_scratch;
    static const lasr::FvWheel wheel = lasr::fv_make_wheel();
    const unsigned gx1 = (unsigned)std::min<long long>((HW + 1023) / 1024, 64);
    const unsigned gx2 = (unsigned)((P + 1023) / 1024);
    const int vec = fv_aligned(flow, 16) && fv_aligned(mask, 16);
    if (C == 2) {
        LASR_LAUNCH(K_FLOW_MAXRAD, lasr::flow_maxrad_kernel<2>, dim3(gx1, (unsigned)B), dim3(256), 0, flow, mask, stats, HW);
        LASR_LAUNCH(K_FLOW_COLOUR, lasr::flow_colour_kernel<2>, dim3(gx2), dim3(256), 0, flow, mask, out, stats, HW, P, B, wheel, vec);
    } else {
        LASR_LAUNCH(K_FLOW_MAXRAD, lasr::flow_maxrad_kernel<3>, dim3(gx1, (unsigned)B), dim3(256), 0, flow, mask, stats, HW);
        LASR_LAUNCH(K_FLOW_COLOUR, lasr::flow_colour_kernel<3>, dim3(gx2), dim3(256), 0, flow, mask, out, stats, HW, P, B, wheel, vec);
    }
    return launch_ok();
}

extern "C" size_t lasr_flow_to_image_scratch_bytes(int B) { return B < 0 ? 0 : ((size_t)B + 1) * sizeof(unsigned); }

extern "C" size_t lasr_monitor_sheet_scratch_bytes(void) { return (lasr::SH_NSTAT + 1) * sizeof(unsigned); }

extern "C" int lasr_monitor_sheet(const lasr_sheet_inputs* in, unsigned char* out, void* stats_scratch, int IS, void* hip_stream)
{
    if (IS < 0 || IS > LASR_SHEET_MAX_SIZE) return LASR_E_BADARG;
    if (IS == 0) return LASR_OK;
    if (!in || !out || !stats_scratch || !fv_aligned(out, 4)) return LASR_E_BADARG;
    const lasr_sheet_plane* need[] = {&in->flow_obs, &in->flow_rd, &in->vis_mask, &in->flow_err, &in->mask_pred, &in->mask_gt,
                                      &in->img1, &in->img2, &in->texture};
    for (const lasr_sheet_plane* p : need)
        if (!p->ptr) return LASR_E_BADARG;
    if (in->n_ctl < 0 || (in->n_ctl > 0 && (!in->ctl || !in->palette || in->ctl_stride < 2))) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    unsigned* stats = (unsigned*)stats_scratch;
    static const lasr::FvWheel wheel = lasr::fv_make_wheel();
    const long long HW = (long long)IS * IS;
    const unsigned gs = (unsigned)std::min<long long>((HW + 255) / 256, 64);
    const unsigned gc = (unsigned)((9 * HW + 1023) / 1024);
    LASR_LAUNCH(K_SHEET_STATS, lasr::sheet_stats_kernel, dim3(gs), dim3(256), 0, *in, stats, IS);
    LASR_LAUNCH(K_SHEET_COMPOSE, lasr::sheet_compose_kernel, dim3(gc), dim3(256), 0, *in, out, stats, IS, wheel);
    return launch_ok();
}

extern "C" size_t lasr_scalar_ring_bytes(int capacity, int K)
{
    if (capacity < 1 || K < 1 || K > LASR_RING_MAX_SCALARS) return 0;
    return (size_t)capacity * K * sizeof(float);
}

extern "C" int lasr_scalar_ring_push(const void* table, int K, float* ring, unsigned* head, int capacity, void* hip_stream)
{
    if (K < 0 || K > LASR_RING_MAX_SCALARS || capacity < 1) return LASR_E_BADARG;
    if (K == 0) return LASR_OK;
    if (!table || !ring || !head) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    LASR_LAUNCH(K_SCALAR_RING_PUSH, lasr::scalar_ring_push_kernel, dim3(1), dim3(256), 0, (const long long*)table, K, ring, head, capacity);
    return launch_ok();
}
