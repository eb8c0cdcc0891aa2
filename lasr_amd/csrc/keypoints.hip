// keypoints.hip -- keypoint transfer of scripts/eval_badja.py (BADJA PCK; reference: scripts/eval_badja.py:225-242).
// For each of B pairs, the flow of the reference frame comes from the hard-mode raster of its geometry with the target frame's
// projected vertices as vertex colours ([B,4,S,S], render_flow_soft_3).  Every keypoint moves with the flow of the nearest
// VALID pixel of the H x W crop: one pass over the pixels tests all J keypoints against each of them, so the reference's dense
// [J, H*W] distance tensor never exists.  DESIGN.md section 4.5 states the arithmetic and the reduction.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"

namespace lasr {

constexpr int KP_THREADS = 256;
constexpr int KP_WAVES = KP_THREADS / 64;

// The flow of pixel (r, c) of pair b from the raster's colour planes, in the reference's fp32 operations
// (nnutils/geom_utils.py:73-95 then eval_badja.py:227): background (blue < 1e-9) -> 0; else colour.xy - grid with
// grid = (p * 2) * (1 / (S - 1)) - 1 -- torch's division of a device tensor by a scalar multiplies by the fp32 reciprocal.
__device__ __forceinline__ void kp_flow(float c0, float c1, float c2, int r, int c, float inv, float& fx, float& fy)
{
    if (c2 < 1e-9f) {
        fx = 0.f;
        fy = 0.f;
    } else {
        fx = c0 - ((float)c * 2.f * inv - 1.f);
        fy = c1 - ((float)r * 2.f * inv - 1.f);
    }
}

// torch's norm(2, -1) over two elements: sqrt(x*x + y*y), no contraction (built -ffp-contract=off), correctly rounded sqrt.
__device__ __forceinline__ bool kp_invalid(float fx, float fy) { return sqrtf(fx * fx + fy * fy) < 1e-6f; }

__device__ __forceinline__ unsigned long long kp_wave_min(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// Per pair (blockIdx.y) a band of `rows` rows (blockIdx.x).  Per keypoint k the search key of flat pixel i = r*W + c is
//   key = (invalid * 1e6 + (row_k - r)^2) + (col_k - c)^2        (fp32, eval_badja.py:238's operation order)
// a non-negative float whose bits order as uint32; (bits << 32) | i ordered as uint64 is torch's argmin, first index on ties.
// Each lane visits its pixels in increasing i, so a strict < keeps the first; then wave, LDS, one atomicMin per block and k.
template <int JMAX>
__global__ __launch_bounds__(KP_THREADS) void kp_transfer_kernel(const float* __restrict__ colors, const float* __restrict__ kp,
                                                                 unsigned long long* __restrict__ keys, int J, int S, int H, int W,
                                                                 int rows, int vec)
{
    __shared__ float s_kp[2 * JMAX];
    __shared__ unsigned long long s_min[KP_WAVES][JMAX];
    const int b = blockIdx.y;
    for (int t = threadIdx.x; t < 2 * J; t += KP_THREADS) s_kp[t] = kp[(size_t)b * J * 2 + t];
    __syncthreads();

    unsigned best[JMAX], bidx[JMAX];
#pragma unroll
    for (int k = 0; k < JMAX; k++) {
        best[k] = 0xffffffffu;                            // above every non-NaN key (+inf is 0x7f800000)
        bidx[k] = 0xffffffffu;
    }
    const size_t P = (size_t)S * S;
    const float* p0 = colors ? colors + (size_t)b * 4 * P : nullptr;
    const float inv = 1.f / (float)(S - 1);
    const int r0 = blockIdx.x * rows, r1 = min(H, r0 + rows);
    for (int r = r0; r < r1; r++) {
        const size_t row = (size_t)r * S;
        float dr2[JMAX];                                  // (row_k - r)^2 is constant along the row
#pragma unroll
        for (int k = 0; k < JMAX; k++) {
            const float dr = k < J ? s_kp[2 * k] - (float)r : 0.f;
            dr2[k] = dr * dr;
        }
        for (int cb = threadIdx.x * 4; cb < W; cb += KP_THREADS * 4) {
            float c0[4], c1[4], c2[4];
            if (!p0) {
#pragma unroll
                for (int q = 0; q < 4; q++) c0[q] = c1[q] = c2[q] = 0.f;   // the zero flow: every pixel invalid
            } else if (vec && cb + 3 < W) {
                const float4 a = *(const float4*)(p0 + row + cb);
                const float4 g = *(const float4*)(p0 + P + row + cb);
                const float4 z = *(const float4*)(p0 + 2 * P + row + cb);
                c0[0] = a.x; c0[1] = a.y; c0[2] = a.z; c0[3] = a.w;
                c1[0] = g.x; c1[1] = g.y; c1[2] = g.z; c1[3] = g.w;
                c2[0] = z.x; c2[1] = z.y; c2[2] = z.z; c2[3] = z.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool in = cb + q < W;
                    c0[q] = in ? p0[row + cb + q] : 0.f;
                    c1[q] = in ? p0[P + row + cb + q] : 0.f;
                    c2[q] = in ? p0[2 * P + row + cb + q] : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int c = cb + q;
                if (c >= W) break;
                float fx = 0.f, fy = 0.f;
                if (p0) kp_flow(c0[q], c1[q], c2[q], r, c, inv, fx, fy);
                const float pen = kp_invalid(fx, fy) ? 1e6f : 0.f;
                const unsigned i = (unsigned)(r * W + c);
#pragma unroll
                for (int k = 0; k < JMAX; k++) {
                    if (k < J) {
                        const float dc = s_kp[2 * k + 1] - (float)c;
                        const unsigned kb = __float_as_uint((pen + dr2[k]) + dc * dc);
                        if (kb < best[k]) {
                            best[k] = kb;
                            bidx[k] = i;
                        }
                    }
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < JMAX; k++) {
        if (k < J) {
            const unsigned long long m = kp_wave_min(((unsigned long long)best[k] << 32) | bidx[k]);
            if (lane == 0) s_min[wave][k] = m;
        }
    }
    __syncthreads();
    if (threadIdx.x < J) {
        unsigned long long m = s_min[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < KP_WAVES; w++) m = s_min[w][threadIdx.x] < m ? s_min[w][threadIdx.x] : m;
        if (m != ~0ull) atomicMin(&keys[(size_t)b * J + threadIdx.x], m);
    }
}

// One thread per (pair, keypoint): the winning flat index, the flow there, and kp + flow scaled as the reference scales it:
// row + flow_y * H / 2, col + flow_x * W / 2 (eval_badja.py:239-242).  idx shares its storage with the keys.
__global__ __launch_bounds__(256) void kp_sample_kernel(const float* __restrict__ colors, const float* __restrict__ kp,
                                                        unsigned long long* __restrict__ keys, float* __restrict__ pred, int B,
                                                        int J, int S, int H, int W)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * J) return;
    const int b = t / J;
    const unsigned long long key = keys[t];
    const unsigned i = (unsigned)(key & 0xffffffffull);
    const float kr = kp[2 * (size_t)t], kc = kp[2 * (size_t)t + 1];
    long long* idx = (long long*)keys;
    if (key == ~0ull || i >= (unsigned)(H * W)) {         // only a NaN keypoint leaves its key unset
        idx[t] = -1;
        pred[2 * (size_t)t] = __int_as_float(0x7fc00000);
        pred[2 * (size_t)t + 1] = __int_as_float(0x7fc00000);
        return;
    }
    const int r = (int)(i / (unsigned)W), c = (int)(i - (unsigned)r * (unsigned)W);
    float fx = 0.f, fy = 0.f;
    if (colors) {
        const size_t P = (size_t)S * S, o = (size_t)b * 4 * P + (size_t)r * S + c;
        kp_flow(colors[o], colors[o + P], colors[o + 2 * P], r, c, 1.f / (float)(S - 1), fx, fy);
    }
    idx[t] = (long long)i;
    pred[2 * (size_t)t] = kr + fy * (float)H * 0.5f;
    pred[2 * (size_t)t + 1] = kc + fx * (float)W * 0.5f;
}

}  // namespace lasr

extern "C" int lasr_kp_transfer(const float* colors, const float* kp, long long* idx, float* pred, int B, int J, int S, int H, int W,
                                void* hip_stream)
{
    if (B < 0 || J < 1 || J > LASR_KP_MAX_JOINTS || S < 2 || S > LASR_KP_MAX_SIZE || H < 1 || H > S || W < 1 || W > S)
        return LASR_E_BADARG;
    if (B > 65535 || (long long)B * J > 0x7fffffffLL) return LASR_E_BADARG;
    if (B == 0) return LASR_OK;
    if (!kp || !idx || !pred) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    if (hipMemsetAsync(idx, 0xff, (size_t)B * J * sizeof(long long), st) != hipSuccess) return launch_ok();
    // rows per workgroup: about 2048 workgroups over the launch (8 per CU), at least one row each
    const long long rows_total = (long long)B * H;
    const int rows = (int)(rows_total / 2048 > 1 ? (rows_total / 2048 < H ? rows_total / 2048 : H) : 1);
    const int vec = colors && (S % 4 == 0) && ((uintptr_t)colors % 16 == 0);
    const dim3 grid((unsigned)((H + rows - 1) / rows), (unsigned)B);
    unsigned long long* keys = (unsigned long long*)idx;
    if (J <= 24)                                          // BADJA annotates 20 joints: fewer registers, more waves per SIMD
        LASR_LAUNCH(K_KP_TRANSFER, lasr::kp_transfer_kernel<24>, grid, dim3(lasr::KP_THREADS), 0, colors, kp, keys, J, S, H, W, rows,
                    vec);
    else
        LASR_LAUNCH(K_KP_TRANSFER, lasr::kp_transfer_kernel<64>, grid, dim3(lasr::KP_THREADS), 0, colors, kp, keys, J, S, H, W, rows,
                    vec);
    const int n = B * J;
    LASR_LAUNCH(K_KP_SAMPLE, lasr::kp_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, colors, kp, keys, pred, B, J, S,
                H, W);
    return launch_ok();
}
