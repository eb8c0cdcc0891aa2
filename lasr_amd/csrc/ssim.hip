// ssim.hip -- the structural-similarity texture term of optimize.py --ptex_method ssim (lasr_amd/nnutils/fused_ops.py:
// ssim_distance, lasr_amd/nnutils/mesh_net.py: StructuralDistance).  This is the project's own addition; the reference has no
// counterpart, and the definition is the one of include/lasr_ops.h, tests/ssim_restated.py and DESIGN.md section 4.19.
// ssim_forward_kernel: one block of 256 threads per 32 x 16 tile of the output map of one (image, channel).  a and b of the tile
// and its halo of 10 are staged in LDS, the five planes a, b, a a, b b, a b go through the horizontal pass of the 11-tap window into
// LDS and through the vertical pass into registers, the map s (and, when asked for, its three partial planes) is evaluated and the
// block's sum is written; ssim_fold_kernel adds the block sums of an image in index order in fp64.
// ssim_backward_kernel: one block per 32 x 16 tile of grad_b.  The three partial planes of the 42 x 26 output pixels that reach the
// tile are read back (SAVED) or recomputed from a 52 x 36 patch of a and b, go through the transposed window in two passes and are
// combined with a(q) and b(q).
// LDS addressing: every ds_read / ds_write of the passes has, within a group of 32 lanes, addresses that are 32 consecutive dwords
// plus a multiple of 32, so each lane has its own bank (bank = dword address mod 32 for ds_read_b32 / ds_write_b32): the 32-wide
// passes keep a 32-lane group inside one row; the 42-wide passes of the recompute walk a linear index and the staged patch has
// a pitch of 42 + 32, which makes the address the linear index plus a multiple of 32.
// No floating-point atomics: the same input gives the same bits on every run.  Built with -ffp-contract=off; `/` is IEEE.
#include <math.h>
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"

namespace lasr {

constexpr int SS_TW = LASR_SSIM_TILE_W, SS_TH = LASR_SSIM_TILE_H;     // the tile: of the output map (forward), of grad_b (backward)
constexpr int SS_K = 11, SS_HALO = SS_K - 1;
constexpr int SS_IW = SS_TW + SS_HALO, SS_IH = SS_TH + SS_HALO;       // 42 x 26: the forward's input patch, the backward's plane patch
constexpr int SS_RW = SS_IW + SS_HALO, SS_RH = SS_IH + SS_HALO;       // 52 x 36: the input patch of the recomputing backward
constexpr int SS_RP = SS_IW + 32;                                     // its pitch in LDS (see the head of the file)

static_assert(SS_TW == 32 && SS_TH == 16, "a 32-lane group is one row of a tile; a thread owns rows t / 32 and t / 32 + 8");
static_assert(SS_RP >= SS_RW, "the padded pitch holds the patch");

// g[k] = exp(-(k - 5)^2 / (2 1.5^2)) / sum, formed in fp64 and rounded once to fp32 (tests/test_ssim_cpu.py compares these
// literals with the restatement's window)
struct SsWindow {
    float g[SS_K];
};
static const SsWindow SS_WINDOW = {{0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,
                                    0.213005543f, 0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f}};

// s and (P) its derivatives by mu_b, E[bb] and E[ab] from the five blurred planes, in the order include/lasr_ops.h states
template <bool P> __device__ __forceinline__ float ss_map(const float (&m)[5], float C1, float C2, float& p1, float& p2, float& p3)
{
    const float mua = m[0], mub = m[1];
    const float saa = m[2] - mua * mua, sbb = m[3] - mub * mub, sab = m[4] - mua * mub;
    const float A1 = 2.f * mua * mub + C1, A2 = 2.f * sab + C2;
    const float B1 = (mua * mua + mub * mub) + C1, B2 = (saa + sbb) + C2;
    const float den = B1 * B2;
    const float s = (A1 * A2) / den;
    if (P) {
        const float u = (2.f * mub) * s;
        p1 = ((2.f * mua) * (A2 - A1)) / den - (u / B1 - u / B2);
        p2 = -(s / B2);
        p3 = (2.f * A1) / den;
    }
    return s;
}

// rows x 32 outputs of the horizontal pass over the five planes of a patch with `pitch`: out[j][r 32 + x]
__device__ __forceinline__ void ss_moments_h32(const float* sa, const float* sb, float* hb, int rows, int pitch, const SsWindow& w)
{
    for (int idx = threadIdx.x; idx < rows * 32; idx += 256) {
        const int r = idx >> 5, x = idx & 31;
        float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const float av = sa[r * pitch + x + k], bv = sb[r * pitch + x + k];
            acc[0] = acc[0] + w.g[k] * av;
            acc[1] = acc[1] + w.g[k] * bv;
            acc[2] = acc[2] + w.g[k] * (av * av);
            acc[3] = acc[3] + w.g[k] * (bv * bv);
            acc[4] = acc[4] + w.g[k] * (av * bv);
        }
#pragma unroll
        for (int j = 0; j < 5; j++) hb[j * rows * 32 + idx] = acc[j];
    }
}

__global__ __launch_bounds__(256) void ssim_fold_kernel(const float* __restrict__ scratch, float* __restrict__ d, int N, int NB,
                                                         double count)
{
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    double s = 0.;
    for (int b = 0; b < NB; b++) s += (double)scratch[(size_t)n * NB + b];
    d[n] = (float)(1. - s / count);
}

template <bool SAVE>
__global__ __launch_bounds__(256) void ssim_forward_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ partials, float* __restrict__ scratch, int rep, int H,
                                                            int W, float C1, float C2, SsWindow w)
{
    __shared__ float sa[SS_IH * SS_IW], sb[SS_IH * SS_IW], hb[5 * SS_IH * SS_TW];
    __shared__ float red[4];
    const int tid = threadIdx.x, Ho = H - SS_HALO, Wo = W - SS_HALO;
    const int x0 = blockIdx.x * SS_TW, y0 = blockIdx.y * SS_TH;
    const int n = blockIdx.z / 3, c = blockIdx.z - 3 * n;
    const float* pa = a + ((size_t)(n / rep) * 3 + c) * H * W;
    const float* pb = b + ((size_t)n * 3 + c) * H * W;
    for (int idx = tid; idx < SS_IH * SS_IW; idx += 256) {
        const int r = idx / SS_IW, col = idx - r * SS_IW;
        const int gy = y0 + r, gx = x0 + col;
        const bool in = gy < H && gx < W;
        sa[idx] = in ? pa[(size_t)gy * W + gx] : 0.f;
        sb[idx] = in ? pb[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    ss_moments_h32(sa, sb, hb, SS_IH, SS_IW, w);
    __syncthreads();
    const int x = tid & 31;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int y = (tid >> 5) + 8 * i;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SS_K; k++)
#pragma unroll
            for (int j = 0; j < 5; j++) m[j] = m[j] + w.g[k] * hb[j * SS_IH * SS_TW + (y + k) * SS_TW + x];
        float p1 = 0.f, p2 = 0.f, p3 = 0.f;
        float s = ss_map<SAVE>(m, C1, C2, p1, p2, p3);
        const bool in = y0 + y < Ho && x0 + x < Wo;
        if (!in) s = 0.f;
        sum = sum + s;
        if (SAVE && in) {
            float* pp = partials + ((size_t)blockIdx.z * 3 * Ho + (y0 + y)) * Wo + (x0 + x);
            pp[0] = p1;
            pp[(size_t)Ho * Wo] = p2;
            pp[(size_t)2 * Ho * Wo] = p3;
        }
    }
    // the block's sum in a fixed order: lane l += lane l + o for o = 32 ... 1, then the four waves in order
    for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_down(sum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        const size_t nb = (size_t)gridDim.x * gridDim.y;
        scratch[((size_t)blockIdx.z * nb) + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

template <bool SAVED> struct SsBwdLds {
    // recompute: the patch of a and b (then the planes, which are formed once the patch is spent) | the five blurred planes
    // (then the planes after the transposed horizontal pass)
    static constexpr int A = SAVED ? 3 * SS_IH * SS_IW : 2 * SS_RH * SS_RP;
    static constexpr int B = SAVED ? 3 * SS_IH * SS_TW : 5 * SS_RH * SS_IW;
};
static_assert(2 * SS_RH * SS_RP >= 3 * SS_IH * SS_IW && 5 * SS_RH * SS_IW >= 3 * SS_IH * SS_TW, "the buffers are reused");

template <bool SAVED>
__global__ __launch_bounds__(256) void ssim_backward_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ partials, const float* __restrict__ grad_d,
                                                             float* __restrict__ grad_b, int rep, int H, int W, float C1, float C2,
                                                             double count, SsWindow w)
{
    __shared__ float bufA[SsBwdLds<SAVED>::A], bufB[SsBwdLds<SAVED>::B];
    const int tid = threadIdx.x, Ho = H - SS_HALO, Wo = W - SS_HALO;
    const int qx0 = blockIdx.x * SS_TW, qy0 = blockIdx.y * SS_TH;
    const int px0 = qx0 - SS_HALO, py0 = qy0 - SS_HALO;               // the first output pixel that reaches the tile
    const int n = blockIdx.z / 3, c = blockIdx.z - 3 * n;
    const float* pa = a + ((size_t)(n / rep) * 3 + c) * H * W;
    const float* pb = b + ((size_t)n * 3 + c) * H * W;
    float* sp = bufA;                                                 // sp[j][r 42 + col]: plane j at output pixel (py0 + r, px0 + col)
    if (SAVED) {
        const float* pp = partials + (size_t)blockIdx.z * 3 * Ho * Wo;
        for (int idx = tid; idx < SS_IH * SS_IW; idx += 256) {
            const int r = idx / SS_IW, col = idx - r * SS_IW;
            const int py = py0 + r, px = px0 + col;
            const bool in = py >= 0 && py < Ho && px >= 0 && px < Wo;
#pragma unroll
            for (int j = 0; j < 3; j++) sp[j * SS_IH * SS_IW + idx] = in ? pp[((size_t)j * Ho + py) * Wo + px] : 0.f;
        }
    } else {
        float* sa = bufA;
        float* sb = bufA + SS_RH * SS_RP;
        float* hb = bufB;
        for (int idx = tid; idx < SS_RH * SS_RW; idx += 256) {
            const int r = idx / SS_RW, col = idx - r * SS_RW;
            const int gy = py0 + r, gx = px0 + col;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            sa[r * SS_RP + col] = in ? pa[(size_t)gy * W + gx] : 0.f;
            sb[r * SS_RP + col] = in ? pb[(size_t)gy * W + gx] : 0.f;
        }
        __syncthreads();
        // the horizontal pass, 36 rows x 42 columns on a linear index: the address is idx + 32 r + k
        for (int idx = tid; idx < SS_RH * SS_IW; idx += 256) {
            const int r = idx / SS_IW, x = idx - r * SS_IW;
            float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SS_K; k++) {
                const float av = sa[r * SS_RP + x + k], bv = sb[r * SS_RP + x + k];
                acc[0] = acc[0] + w.g[k] * av;
                acc[1] = acc[1] + w.g[k] * bv;
                acc[2] = acc[2] + w.g[k] * (av * av);
                acc[3] = acc[3] + w.g[k] * (bv * bv);
                acc[4] = acc[4] + w.g[k] * (av * bv);
            }
#pragma unroll
            for (int j = 0; j < 5; j++) hb[j * SS_RH * SS_IW + idx] = acc[j];
        }
        __syncthreads();
        // the vertical pass and the planes, 26 x 42 on a linear index: the address is idx + 42 k
        for (int idx = tid; idx < SS_IH * SS_IW; idx += 256) {
            const int r = idx / SS_IW, col = idx - r * SS_IW;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SS_K; k++)
#pragma unroll
                for (int j = 0; j < 5; j++) m[j] = m[j] + w.g[k] * hb[j * SS_RH * SS_IW + idx + k * SS_IW];
            float p1, p2, p3;
            ss_map<true>(m, C1, C2, p1, p2, p3);
            const int py = py0 + r, px = px0 + col;
            const bool in = py >= 0 && py < Ho && px >= 0 && px < Wo;
            sp[idx] = in ? p1 : 0.f;
            sp[SS_IH * SS_IW + idx] = in ? p2 : 0.f;
            sp[2 * SS_IH * SS_IW + idx] = in ? p3 : 0.f;
        }
    }
    __syncthreads();
    // the transposed window, horizontally: u[j][r 32 + x] = sum_k g[10 - k] plane j (py0 + r, qx0 + x - 10 + k)
    float* su = bufB;
    for (int idx = tid; idx < SS_IH * SS_TW; idx += 256) {
        const int r = idx >> 5, x = idx & 31;
        float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SS_K; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) acc[j] = acc[j] + w.g[SS_HALO - k] * sp[j * SS_IH * SS_IW + r * SS_IW + x + k];
#pragma unroll
        for (int j = 0; j < 3; j++) su[j * SS_IH * SS_TW + idx] = acc[j];
    }
    __syncthreads();
    const float coef = (float)(-(double)grad_d[n] / count);
    const int x = tid & 31;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int y = (tid >> 5) + 8 * i;
        float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SS_K; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) t[j] = t[j] + w.g[SS_HALO - k] * su[j * SS_IH * SS_TW + (y + k) * SS_TW + x];
        const int qy = qy0 + y, qx = qx0 + x;
        if (qy < H && qx < W) {
            const size_t at = (size_t)qy * W + qx;
            const float av = pa[at], bv = pb[at];
            float v = t[0] + (2.f * bv) * t[1];
            v = v + av * t[2];
            grad_b[((size_t)blockIdx.z * H) * W + at] = coef * v;
        }
    }
}

static bool ss_sizes_ok(int M, int rep, int H, int W, float L)
{
    if (M < 1 || rep < 1 || (long long)M * rep * 3 > 65535) return false;          // grid z = 3 N
    if (H < LASR_SSIM_MIN_SIZE || H > LASR_SSIM_MAX_SIZE || W < LASR_SSIM_MIN_SIZE || W > LASR_SSIM_MAX_SIZE) return false;
    return isfinite(L) && L > 0.f;
}

static int ss_tiles(int n, int tile) { return (n + tile - 1) / tile; }

}  // namespace lasr

extern "C" size_t lasr_ssim_scratch_floats(int M, int rep, int H, int W)
{
    if (!lasr::ss_sizes_ok(M, rep, H, W, 1.f)) return 0;
    return (size_t)M * rep * 3 * lasr::ss_tiles(W - lasr::SS_HALO, lasr::SS_TW) * lasr::ss_tiles(H - lasr::SS_HALO, lasr::SS_TH);
}

extern "C" int lasr_ssim_forward(const float* a, const float* b, float* d, float* partials, float* scratch, int M, int rep, int H,
                                 int W, float L, void* hip_stream)
{
    using namespace lasr;
    if (!ss_sizes_ok(M, rep, H, W, L)) return LASR_E_BADARG;
    if (!a || !b || !d || !scratch) return LASR_E_BADARG;
    if ((const void*)d == (const void*)a || (const void*)d == (const void*)b || d == scratch || partials == d
        || (partials && (partials == scratch || (const void*)partials == (const void*)a || (const void*)partials == (const void*)b))
        || (const void*)scratch == (const void*)a || (const void*)scratch == (const void*)b)
        return LASR_E_BADARG;
    const int N = M * rep, Ho = H - SS_HALO, Wo = W - SS_HALO;
    const float C1 = (0.01f * L) * (0.01f * L), C2 = (0.03f * L) * (0.03f * L);
    const dim3 grid((unsigned)ss_tiles(Wo, SS_TW), (unsigned)ss_tiles(Ho, SS_TH), (unsigned)(3 * N));
    hipStream_t st = (hipStream_t)hip_stream;
    if (partials)
        hipLaunchKernelGGL(ssim_forward_kernel<true>, grid, dim3(256), 0, st, a, b, partials, scratch, rep, H, W, C1, C2, SS_WINDOW);
    else
        hipLaunchKernelGGL(ssim_forward_kernel<false>, grid, dim3(256), 0, st, a, b, partials, scratch, rep, H, W, C1, C2, SS_WINDOW);
    hipLaunchKernelGGL(ssim_fold_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, (const float*)scratch, d, N,
                       (int)(3 * grid.x * grid.y), 3. * (double)Ho * (double)Wo);
    return launch_ok();
}

extern "C" int lasr_ssim_backward(const float* a, const float* b, const float* partials, const float* grad_d, float* grad_b, int M,
                                  int rep, int H, int W, float L, void* hip_stream)
{
    using namespace lasr;
    if (!ss_sizes_ok(M, rep, H, W, L)) return LASR_E_BADARG;
    if (!a || !b || !grad_d || !grad_b) return LASR_E_BADARG;
    if ((const void*)grad_b == (const void*)a || (const void*)grad_b == (const void*)b || (const void*)grad_b == (const void*)grad_d
        || (const void*)grad_b == (const void*)partials)
        return LASR_E_BADARG;
    const int N = M * rep, Ho = H - SS_HALO, Wo = W - SS_HALO;
    const float C1 = (0.01f * L) * (0.01f * L), C2 = (0.03f * L) * (0.03f * L);
    const dim3 grid((unsigned)ss_tiles(W, SS_TW), (unsigned)ss_tiles(H, SS_TH), (unsigned)(3 * N));
    const double count = 3. * (double)Ho * (double)Wo;
    hipStream_t st = (hipStream_t)hip_stream;
    if (partials)
        hipLaunchKernelGGL(ssim_backward_kernel<true>, grid, dim3(256), 0, st, a, b, partials, grad_d, grad_b, rep, H, W, C1, C2, count,
                           SS_WINDOW);
    else
        hipLaunchKernelGGL(ssim_backward_kernel<false>, grid, dim3(256), 0, st, a, b, partials, grad_d, grad_b, rep, H, W, C1, C2, count,
                           SS_WINDOW);
    return launch_ok();
}
