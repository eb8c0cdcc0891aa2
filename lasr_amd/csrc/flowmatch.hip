// flowmatch.hip -- large-displacement matching for the variational optical flow (preprocess/flow_match.py runs the passes; --vf_match
// of preprocess/auto_gen.py, propagate_mask.py and auto_mask.py): a factor-2 pyramid loses a structure that is smaller than its own
// motion, so at one pyramid level an integer block-matching stage finds, per pixel, the displacement of least SAD over 8-bit pixels,
// and the forward-backward-consistent matches that explain the images clearly better than the upsampled flow replace it there; the
// unchanged warps refine them (the "extended coarse-to-fine" idea of Xu, Jia & Matsushita 2012, reduced to a greedy per-pixel choice).
// The definition is the one of include/lasr_ops.h, DESIGN.md section 4.16 and tests/flowmatch_restated.py.  Everything here is
// integer arithmetic: a kernel gives the restatement's very numbers in whatever order it sums.  No atomics, no inline assembly, plain
// vector stores; every global read is clamped in index space.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"

namespace lasr {

constexpr int FM_TX = 32, FM_TY = 8;                                  // pixels of one workgroup of the search
static_assert(FM_TX * FM_TY == 256, "thread mapping of fm_search_kernel");

__device__ __forceinline__ int fm_clamp(int v, int hi) { return min(max(v, 0), hi); }

// One pixel is r | g << 8 | b << 16 with a zero top byte: one v_sad_u8 sums the three channel differences of a pixel pair.
__device__ __forceinline__ uint32_t fm_sad(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }

// ---- quantise ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fm_quantise_kernel(const uint8_t* __restrict__ img, const float* __restrict__ level,
                                                          uint32_t* __restrict__ out, int H, int W)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    uint32_t c[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
        c[k] = img ? (uint32_t)img[i * 3 + k] : (uint32_t)fminf(fmaxf(rintf(255.f * level[i * 3 + k]), 0.f), 255.f);
    out[i] = c[0] | (c[1] << 8) | (c[2] << 16);
}

// ---- search ------------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads owns 32 x 8 pixels, one thread a pixel.  LDS holds B's window, the tile with a halo of r + R, and A's
// tile with a halo of r, both already clamped to the frame: (32 + 2 (r + R)) x (8 + 2 (r + R)) + (32 + 2 r) x (8 + 2 r) words, 33952
// bytes at R = 32, r = 3, so four workgroups share a CU's LDS.  A lane reads the word of its own column: the 32 lanes of a tile row
// read 32 consecutive words, one per bank.
// A's (2r+1)^2 patch stays in registers for the whole search.  For one dy the patch of B slides along dx: a window of (2r+1) x (2r+1)
// registers is kept as a ring over its columns, so one step reads 2r+1 new words from LDS, not (2r+1)^2; the dx loop is unrolled by
// 2r+1 so that every ring slot is a compile-time register.  Per pixel and displacement that is (2r+1)^2 v_sad_u8, 2r+1 LDS reads and
// one 64-bit key comparison.  The key is C << 32 | (dx^2 + dy^2) << 14 | (dy + 32) << 7 | (dx + 32): its unsigned minimum is the
// lexicographic minimum of (C, dx^2 + dy^2, dy, dx), whatever the visiting order.  Tiles of 32 x 4 and 32 x 2 were measured beside
// 32 x 8: the same time at R = 24, r = 2 and up to 1.9 x slower at R = 32, r = 3.
template <int r>
__global__ __launch_bounds__(256) void fm_search_kernel(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                        int32_t* __restrict__ d, int32_t* __restrict__ c1, int H, int W, int R)
{
    constexpr int P = 2 * r + 1;
    extern __shared__ uint32_t fm_smem[];
    const int SBW = FM_TX + 2 * (r + R), SBH = FM_TY + 2 * (r + R);
    constexpr int SAW = FM_TX + 2 * r, SAH = FM_TY + 2 * r;
    uint32_t* sB = fm_smem;
    uint32_t* sA = fm_smem + SBW * SBH;
    const int bx = (int)blockIdx.x * FM_TX, by = (int)blockIdx.y * FM_TY;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < SBW * SBH; i += 256) {
        const int ly = i / SBW, lx = i - ly * SBW;
        sB[i] = B[(size_t)fm_clamp(by + ly - (r + R), H - 1) * W + fm_clamp(bx + lx - (r + R), W - 1)];
    }
    for (int i = tid; i < SAW * SAH; i += 256) {
        const int ly = i / SAW, lx = i - ly * SAW;
        sA[i] = A[(size_t)fm_clamp(by + ly - r, H - 1) * W + fm_clamp(bx + lx - r, W - 1)];
    }
    __syncthreads();
    const int tx = tid & (FM_TX - 1), ty = tid / FM_TX;
    const int x = bx + tx, y = by + ty;
    if (x >= W || y >= H) return;                                     // (no barrier below)
    uint32_t a[P][P];
#pragma unroll
    for (int qy = 0; qy < P; qy++)
#pragma unroll
        for (int qx = 0; qx < P; qx++) a[qy][qx] = sA[(ty + qy) * SAW + tx + qx];
    unsigned long long best = ~0ull;
    for (int dy = -R; dy <= R; dy++) {
        // the tap (qy, qx) of displacement (dx, dy) is the word (ty + qy + dy + R, tx + qx + dx + R) of sB; with dxr = dx + R in
        // 0 .. 2R the largest column is 31 + 2r + 2R = SBW - 1, the largest row 7 + 2r + 2R = SBH - 1
        const uint32_t* row = sB + (ty + dy + R) * SBW + tx;
        const bool yok = (unsigned)(y + dy) < (unsigned)H;
        const int dy2 = dy * dy;
        uint32_t w[P][P];                                             // w[qy][c % P] = column c of the window
#pragma unroll
        for (int qy = 0; qy < P; qy++)
#pragma unroll
            for (int c = 0; c < P - 1; c++) w[qy][c] = row[qy * SBW + c];
        for (int dxr0 = 0; dxr0 <= 2 * R; dxr0 += P) {
#pragma unroll
            for (int k = 0; k < P; k++) {
                const int dxr = dxr0 + k;
                if (dxr <= 2 * R) {                                   // (uniform)
#pragma unroll
                    for (int qy = 0; qy < P; qy++) w[qy][(k + P - 1) % P] = row[qy * SBW + dxr + P - 1];
                    uint32_t c = 0;
#pragma unroll
                    for (int qy = 0; qy < P; qy++)
#pragma unroll
                        for (int qx = 0; qx < P; qx++) c = fm_sad(a[qy][qx], w[qy][(k + qx) % P], c);
                    const int dx = dxr - R;
                    const unsigned long long key = ((unsigned long long)c << 32) |
                                                   (unsigned long long)(((uint32_t)(dx * dx + dy2) << 14) | ((uint32_t)(dy + 32) << 7) | (uint32_t)(dx + 32));
                    const bool ok = yok && (unsigned)(x + dx) < (unsigned)W;
                    best = (ok && key < best) ? key : best;
                }
            }
        }
    }
    const size_t i = (size_t)y * W + x;
    const uint32_t lo = (uint32_t)best;
    reinterpret_cast<int2*>(d)[i] = make_int2((int)(lo & 127u) - 32, (int)((lo >> 7) & 127u) - 32);
    c1[i] = (int32_t)(best >> 32);
}

// ---- select and propagate ----------------------------------------------------------------------------------------------------------

// C(p, d) from global memory, every tap clamped into the frame in both images.
__device__ __forceinline__ int fm_cost(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, int H, int W, int x, int y,
                                       int dx, int dy, int r)
{
    uint32_t c = 0;
    for (int qy = -r; qy <= r; qy++) {
        const size_t ra = (size_t)fm_clamp(y + qy, H - 1) * W, rb = (size_t)fm_clamp(y + qy + dy, H - 1) * W;
        for (int qx = -r; qx <= r; qx++) c = fm_sad(A[ra + fm_clamp(x + qx, W - 1)], B[rb + fm_clamp(x + qx + dx, W - 1)], c);
    }
    return (int)c;
}

__device__ __forceinline__ bool fm_inside(int x, int y, int H, int W) { return (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H; }

__device__ __forceinline__ int fm_norm(int a, int b) { return max(abs(a), abs(b)); }

__global__ __launch_bounds__(256) void fm_select_kernel(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                        const int32_t* __restrict__ d_ab, const int32_t* __restrict__ c1,
                                                        const int32_t* __restrict__ d_ba, const float* __restrict__ uv,
                                                        uint8_t* __restrict__ seeded, int32_t* __restrict__ cand, int32_t* __restrict__ ccur,
                                                        int H, int W, int R, int r, int K)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)H * W;
    if (i >= n) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const int cux = (int)fminf(fmaxf(rintf(uv[i]), (float)-R), (float)R);            // rintf: half to even
    const int cuy = (int)fminf(fmaxf(rintf(uv[n + i]), (float)-R), (float)R);
    const int P = 2 * r + 1;
    const int cc = fm_inside(x + cux, y + cuy, H, W) ? fm_cost(A, B, H, W, x, y, cux, cuy, r) : P * P * 765;
    const int2 f = reinterpret_cast<const int2*>(d_ab)[i];
    const int2 b = reinterpret_cast<const int2*>(d_ba)[(size_t)fm_clamp(y + f.y, H - 1) * W + fm_clamp(x + f.x, W - 1)];
    const bool s = fm_norm(f.x + b.x, f.y + b.y) <= 1 && 256ll * c1[i] < (long long)K * cc && fm_norm(f.x - cux, f.y - cuy) > 1;
    seeded[i] = s ? 1 : 0;
    reinterpret_cast<int2*>(cand)[i] = s ? f : make_int2(cux, cuy);
    ccur[i] = cc;
}

// One Jacobi iteration, buffer to buffer: at most four patch evaluations per pixel.
__global__ __launch_bounds__(256) void fm_propagate_kernel(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                           const uint8_t* __restrict__ s_in, const int32_t* __restrict__ c_in,
                                                           const int32_t* __restrict__ ccur, uint8_t* __restrict__ s_out,
                                                           int32_t* __restrict__ c_out, int H, int W, int r, int K)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    int2 take = reinterpret_cast<const int2*>(c_in)[i];
    uint8_t s = s_in[i];
    if (!s) {
        const int cc = ccur[i];
        int best = cc;
        const int ox[4] = {-1, 1, 0, 0}, oy[4] = {0, 0, -1, 1};                      // left, right, upper, lower
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int nx = x + ox[k], ny = y + oy[k];
            if (!fm_inside(nx, ny, H, W)) continue;
            const size_t j = (size_t)ny * W + nx;
            if (!s_in[j]) continue;
            const int2 dd = reinterpret_cast<const int2*>(c_in)[j];
            if (!fm_inside(x + dd.x, y + dd.y, H, W)) continue;
            const int c = fm_cost(A, B, H, W, x, y, dd.x, dd.y, r);
            if (256ll * c < (long long)K * cc && c < best) {
                best = c;
                take = dd;
                s = 1;
            }
        }
    }
    s_out[i] = s;
    reinterpret_cast<int2*>(c_out)[i] = take;
}

static bool fm_size_ok(int H, int W)
{
    return H >= LASR_VARFLOW_MIN_SIZE && W >= LASR_VARFLOW_MIN_SIZE && H <= LASR_VARFLOW_MAX_SIZE && W <= LASR_VARFLOW_MAX_SIZE;
}

static bool fm_patch_ok(int r) { return r >= 1 && r <= LASR_FLOWMATCH_MAX_PATCH; }

static bool fm_radius_ok(int R) { return R >= 1 && R <= LASR_FLOWMATCH_MAX_R; }

static bool fm_k_ok(int K) { return K >= 1 && K <= 256; }

static unsigned fm_blocks(int H, int W) { return (unsigned)(((size_t)H * W + 255) / 256); }

template <int r>
static void fm_launch_search(const uint32_t* qA, const uint32_t* qB, int32_t* d, int32_t* c1, int H, int W, int R, hipStream_t st)
{
    const dim3 grid((unsigned)((W + FM_TX - 1) / FM_TX), (unsigned)((H + FM_TY - 1) / FM_TY));
    const size_t words = (size_t)(FM_TX + 2 * (r + R)) * (FM_TY + 2 * (r + R)) + (size_t)(FM_TX + 2 * r) * (FM_TY + 2 * r);
    hipLaunchKernelGGL(fm_search_kernel<r>, grid, dim3(256), words * sizeof(uint32_t), st, qA, qB, d, c1, H, W, R);
}

}  // namespace lasr

extern "C" int lasr_flowmatch_quantise(const unsigned char* img, const float* level, unsigned int* out, int H, int W, void* hip_stream)
{
    if (!lasr::fm_size_ok(H, W)) return LASR_E_BADARG;
    if (!out || (img == nullptr) == (level == nullptr)) return LASR_E_BADARG;     // exactly one of the two sources
    if ((const void*)img == (const void*)out || (const void*)level == (const void*)out) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::fm_quantise_kernel, dim3(lasr::fm_blocks(H, W)), dim3(256), 0, (hipStream_t)hip_stream, img, level, out, H, W);
    return launch_ok();
}

extern "C" int lasr_flowmatch_search(const unsigned int* qA, const unsigned int* qB, int* d, int* c1, int H, int W, int R, int r,
                                     void* hip_stream)
{
    if (!lasr::fm_size_ok(H, W) || !lasr::fm_radius_ok(R) || !lasr::fm_patch_ok(r)) return LASR_E_BADARG;
    if (!qA || !qB || !d || !c1 || d == c1) return LASR_E_BADARG;
    if ((const void*)d == (const void*)qA || (const void*)d == (const void*)qB || (const void*)c1 == (const void*)qA ||
        (const void*)c1 == (const void*)qB)
        return LASR_E_BADARG;
    const hipStream_t st = (hipStream_t)hip_stream;
    if (r == 1) lasr::fm_launch_search<1>(qA, qB, d, c1, H, W, R, st);
    else if (r == 2) lasr::fm_launch_search<2>(qA, qB, d, c1, H, W, R, st);
    else lasr::fm_launch_search<3>(qA, qB, d, c1, H, W, R, st);
    return launch_ok();
}

extern "C" int lasr_flowmatch_select(const unsigned int* qA, const unsigned int* qB, const int* d_ab, const int* c1, const int* d_ba,
                                     const float* uv, unsigned char* seeded, int* cand, int* ccur, int H, int W, int R, int r, int K,
                                     void* hip_stream)
{
    if (!lasr::fm_size_ok(H, W) || !lasr::fm_radius_ok(R) || !lasr::fm_patch_ok(r) || !lasr::fm_k_ok(K)) return LASR_E_BADARG;
    if (!qA || !qB || !d_ab || !c1 || !d_ba || !uv || !seeded || !cand || !ccur) return LASR_E_BADARG;
    if (cand == ccur || cand == d_ab || cand == d_ba || cand == c1 || ccur == d_ab || ccur == d_ba || ccur == c1) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::fm_select_kernel, dim3(lasr::fm_blocks(H, W)), dim3(256), 0, (hipStream_t)hip_stream, qA, qB, d_ab, c1, d_ba,
                       uv, seeded, cand, ccur, H, W, R, r, K);
    return launch_ok();
}

extern "C" int lasr_flowmatch_propagate(const unsigned int* qA, const unsigned int* qB, const unsigned char* seeded_in, const int* cand_in,
                                        const int* ccur, unsigned char* seeded_out, int* cand_out, int H, int W, int r, int K,
                                        void* hip_stream)
{
    if (!lasr::fm_size_ok(H, W) || !lasr::fm_patch_ok(r) || !lasr::fm_k_ok(K)) return LASR_E_BADARG;
    if (!qA || !qB || !seeded_in || !cand_in || !ccur || !seeded_out || !cand_out) return LASR_E_BADARG;
    if (seeded_out == seeded_in || cand_out == cand_in || cand_out == ccur) return LASR_E_BADARG;      // a Jacobi step: buffer to buffer
    hipLaunchKernelGGL(lasr::fm_propagate_kernel, dim3(lasr::fm_blocks(H, W)), dim3(256), 0, (hipStream_t)hip_stream, qA, qB, seeded_in,
                       cand_in, ccur, seeded_out, cand_out, H, W, r, K);
    return launch_ok();
}
