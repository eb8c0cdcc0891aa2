// robustflow.hip -- the gradient-constancy term of the variational optical flow (preprocess/robust_flow.py runs the passes;
// --vf_gamma of preprocess/auto_gen.py, propagate_mask.py and auto_mask.py): Brox et al. 2004 ask that the image gradient, not only
// the brightness, is kept along the flow, which an additive change of the lighting leaves untouched; Bruhn & Weickert 2005 give the
// two data terms their own robust penalties.  The definition is the one of include/lasr_ops.h, DESIGN.md section 4.16 and
// tests/robustflow_restated.py, whose operation order every kernel here follows (built with -ffp-contract=off, as varflow.hip).
// Pyramid, expansion, solver and consistency map stay those of varflow.hip: the weights pass here hands lasr_varflow_sor the combined
// tensor J = (beta psi_b) Jb + (gamma psi_g) Jg with psi_d = 1.  No floating-point atomics anywhere: the same input gives the same
// bits on every run.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"

namespace lasr {

// ---- derivative record -------------------------------------------------------------------------------------------------------------
// A level's record holds, per pixel, I, Ix, Iy, Ixx, Ixy, Iyy of channel 0, then of channel 1, then of channel 2: 18 floats = 72
// bytes, so that one bilinear corner of the warp reads one contiguous piece.  It is constant over a level's warps and written once
// per level and frame.  One workgroup of 256 threads owns RF_TX x RF_TY = 32 x 8 pixels and stages them and a halo of 2 (the central
// difference applied twice) in LDS, channels interleaved as in the image: lanes one pixel apart read words 3 apart, free of bank
// conflicts.  The results go through LDS too, so that a tile row's 32 x 72 = 2304 bytes leave as consecutive words.
constexpr int RF_REC = LASR_RFLOW_RECORD;
constexpr int RF_TX = 32, RF_TY = 8, RF_HALO = 2;
constexpr int RF_SW = RF_TX + 2 * RF_HALO, RF_SH = RF_TY + 2 * RF_HALO;
static_assert(RF_TX * RF_TY == 256 && RF_REC == 18, "thread mapping and record layout of rflow_derivs_kernel");

struct RfTile {                                                       // the staged tile and its place in the image
    const float* s;
    int bx, by, H, W;
    __device__ __forceinline__ float at(int y, int x, int c) const { return s[((y - by + RF_HALO) * RF_SW + (x - bx + RF_HALO)) * 3 + c]; }
    __device__ __forceinline__ float gx(int y, int x, int c) const { return 0.5f * (at(y, min(x + 1, W - 1), c) - at(y, max(x - 1, 0), c)); }
    __device__ __forceinline__ float gy(int y, int x, int c) const { return 0.5f * (at(min(y + 1, H - 1), x, c) - at(max(y - 1, 0), x, c)); }
};

__global__ __launch_bounds__(256) void rflow_derivs_kernel(const float* __restrict__ I, float* __restrict__ R, int H, int W)
{
    __shared__ float s_in[RF_SW * RF_SH * 3];
    __shared__ float s_out[RF_TX * RF_TY * RF_REC];
    const int bx = (int)blockIdx.x * RF_TX, by = (int)blockIdx.y * RF_TY;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < RF_SW * RF_SH * 3; i += 256) {
        const int cell = i / 3, c = i - cell * 3;
        const int ly = cell / RF_SW, lx = cell - ly * RF_SW;
        const int gx = bx + lx - RF_HALO, gy = by + ly - RF_HALO;
        s_in[i] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? I[((size_t)gy * W + gx) * 3 + c] : 0.f;
    }
    __syncthreads();
    const int tx = tid & (RF_TX - 1), ty = tid / RF_TX;
    const int x = bx + tx, y = by + ty;
    if (x < W && y < H) {
        // every position read below is clamped into the frame and lies within 2 of (y, x): inside the staged region
        const RfTile t = {s_in, bx, by, H, W};
        const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yu = max(y - 1, 0), yd = min(y + 1, H - 1);
        float* o = s_out + (ty * RF_TX + tx) * RF_REC;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            o[c * 6 + 0] = t.at(y, x, c);
            o[c * 6 + 1] = t.gx(y, x, c);
            o[c * 6 + 2] = t.gy(y, x, c);
            o[c * 6 + 3] = 0.5f * (t.gx(y, xr, c) - t.gx(y, xl, c));
            o[c * 6 + 4] = 0.5f * (t.gx(yd, x, c) - t.gx(yu, x, c));
            o[c * 6 + 5] = 0.5f * (t.gy(yd, x, c) - t.gy(yu, x, c));
        }
    }
    __syncthreads();
    const int row_words = min(RF_TX, W - bx) * RF_REC;                // the part of a tile row that lies inside the frame
    for (int i = tid; i < RF_TX * RF_TY * RF_REC; i += 256) {
        const int r = i / (RF_TX * RF_REC), k = i - r * (RF_TX * RF_REC);
        if (by + r < H && k < row_words) R[((size_t)(by + r) * W + bx) * RF_REC + k] = s_out[i];
    }
}

// ---- linearisation -----------------------------------------------------------------------------------------------------------------

struct RfChannel {                                                    // one channel of one pixel's record
    float i, x, y, xx, xy, yy;
};

__device__ __forceinline__ RfChannel rf_load(const float* __restrict__ p)
{
    RfChannel r;
    r.i = p[0];
    r.x = p[1];
    r.y = p[2];
    r.xx = p[3];
    r.xy = p[4];
    r.yy = p[5];
    return r;
}

__device__ __forceinline__ float rf_lerp4(float v00, float v01, float v10, float v11, float tx, float ty)
{
    return (v00 * (1.f - tx) + v01 * tx) * (1.f - ty) + (v10 * (1.f - tx) + v11 * tx) * ty;
}

__device__ __forceinline__ void rf_acc(float& j, float t, int c) { j = c == 0 ? t : j + t; }

// One thread per pixel: the six planes of the brightness tensor (the very values of varflow_tensor_kernel) and of the gradient
// tensor, zero where the warped position leaves the frame.  The four corners of I2's record are read channel by channel, 24
// contiguous bytes each; the twelve sums live in named registers.
__global__ __launch_bounds__(256) void rflow_tensor_kernel(const float* __restrict__ R1, const float* __restrict__ R2,
                                                           const float* __restrict__ uv, float* __restrict__ Jb, float* __restrict__ Jg,
                                                           int H, int W)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)H * W;
    if (i >= n) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const float X = (float)x + uv[i], Y = (float)y + uv[n + i];
    const bool valid = X >= 0.f && X <= (float)(W - 1) && Y >= 0.f && Y <= (float)(H - 1);         // false for a NaN flow too
    const float Xc = fminf(fmaxf(X, 0.f), (float)(W - 1)), Yc = fminf(fmaxf(Y, 0.f), (float)(H - 1));
    const float flx = floorf(Xc), fly = floorf(Yc);
    const int x0 = (int)flx, y0 = (int)fly;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float tx = Xc - flx, ty = Yc - fly;
    const float* p00 = R2 + ((size_t)y0 * W + x0) * RF_REC;
    const float* p01 = R2 + ((size_t)y0 * W + x1) * RF_REC;
    const float* p10 = R2 + ((size_t)y1 * W + x0) * RF_REC;
    const float* p11 = R2 + ((size_t)y1 * W + x1) * RF_REC;
    const float* p1 = R1 + i * RF_REC;
    float b11 = 0.f, b12 = 0.f, b22 = 0.f, b13 = 0.f, b23 = 0.f, b33 = 0.f;
    float g11 = 0.f, g12 = 0.f, g22 = 0.f, g13 = 0.f, g23 = 0.f, g33 = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const RfChannel a = rf_load(p00 + c * 6), b = rf_load(p01 + c * 6), e = rf_load(p10 + c * 6), f = rf_load(p11 + c * 6);
        const RfChannel m = rf_load(p1 + c * 6);
        const float s2 = rf_lerp4(a.i, b.i, e.i, f.i, tx, ty);
        const float s2x = rf_lerp4(a.x, b.x, e.x, f.x, tx, ty), s2y = rf_lerp4(a.y, b.y, e.y, f.y, tx, ty);
        const float Ix = 0.5f * (s2x + m.x), Iy = 0.5f * (s2y + m.y), It = s2 - m.i;
        rf_acc(b11, Ix * Ix, c);
        rf_acc(b12, Ix * Iy, c);
        rf_acc(b22, Iy * Iy, c);
        rf_acc(b13, Ix * It, c);
        rf_acc(b23, Iy * It, c);
        rf_acc(b33, It * It, c);
        const float Ixx = 0.5f * (rf_lerp4(a.xx, b.xx, e.xx, f.xx, tx, ty) + m.xx);
        const float Ixy = 0.5f * (rf_lerp4(a.xy, b.xy, e.xy, f.xy, tx, ty) + m.xy);
        const float Iyy = 0.5f * (rf_lerp4(a.yy, b.yy, e.yy, f.yy, tx, ty) + m.yy);
        const float Ixt = s2x - m.x, Iyt = s2y - m.y;
        rf_acc(g11, Ixx * Ixx + Ixy * Ixy, c);
        rf_acc(g12, Ixx * Ixy + Ixy * Iyy, c);
        rf_acc(g22, Ixy * Ixy + Iyy * Iyy, c);
        rf_acc(g13, Ixx * Ixt + Ixy * Iyt, c);
        rf_acc(g23, Ixy * Ixt + Iyy * Iyt, c);
        rf_acc(g33, Ixt * Ixt + Iyt * Iyt, c);
    }
    Jb[i] = valid ? b11 : 0.f;
    Jb[n + i] = valid ? b12 : 0.f;
    Jb[2 * n + i] = valid ? b22 : 0.f;
    Jb[3 * n + i] = valid ? b13 : 0.f;
    Jb[4 * n + i] = valid ? b23 : 0.f;
    Jb[5 * n + i] = valid ? b33 : 0.f;
    Jg[i] = valid ? g11 : 0.f;
    Jg[n + i] = valid ? g12 : 0.f;
    Jg[2 * n + i] = valid ? g22 : 0.f;
    Jg[3 * n + i] = valid ? g13 : 0.f;
    Jg[4 * n + i] = valid ? g23 : 0.f;
    Jg[5 * n + i] = valid ? g33 : 0.f;
}

// ---- weights -----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float rf_psi(const float* __restrict__ J, size_t n, size_t i, float du, float dv, float e2)
{
    const float r2 = (du * du) * J[i] + ((2.f * du) * dv) * J[n + i] + (dv * dv) * J[2 * n + i] + (2.f * du) * J[3 * n + i] +
                     (2.f * dv) * J[4 * n + i] + J[5 * n + i];
    return 0.5f / sqrtf(fmaxf(r2, 0.f) + e2);
}

// One thread per pixel, one pass: psi_b and psi_g from the two linearised residuals, the combined tensor the solver sees, psi_d = 1,
// and psi_s from the gradients of the updated flow (the neighbour reads of varflow_weights_kernel).
__global__ __launch_bounds__(256) void rflow_weights_kernel(const float* __restrict__ Jb, const float* __restrict__ Jg,
                                                            const float* __restrict__ uv, const float* __restrict__ d,
                                                            float* __restrict__ J, float* __restrict__ psi, int H, int W, float eps,
                                                            float beta, float gamma)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)H * W;
    if (i >= n) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const float e2 = eps * eps;
    const float du = d[i], dv = d[n + i];
    const float wb = beta * rf_psi(Jb, n, i, du, dv, e2), wg = gamma * rf_psi(Jg, n, i, du, dv, e2);
#pragma unroll
    for (int q = 0; q < 6; q++) J[q * n + i] = wb * Jb[q * n + i] + wg * Jg[q * n + i];
    psi[i] = 1.f;
    const size_t l = i - (x > 0), r = i + (x < W - 1), up = i - (y > 0 ? (size_t)W : 0), dn = i + (y < H - 1 ? (size_t)W : 0);
    const float ux = 0.5f * ((uv[r] + d[r]) - (uv[l] + d[l])), uy = 0.5f * ((uv[dn] + d[dn]) - (uv[up] + d[up]));
    const float vx = 0.5f * ((uv[n + r] + d[n + r]) - (uv[n + l] + d[n + l])), vy = 0.5f * ((uv[n + dn] + d[n + dn]) - (uv[n + up] + d[n + up]));
    psi[n + i] = 0.5f / sqrtf(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + e2);
}

static bool rf_size_ok(int H, int W)
{
    return H >= LASR_VARFLOW_MIN_SIZE && W >= LASR_VARFLOW_MIN_SIZE && H <= LASR_VARFLOW_MAX_SIZE && W <= LASR_VARFLOW_MAX_SIZE;
}

static bool rf_pos(float v) { return v > 0.f && v <= 3.0e38f; }       // finite and positive (false for NaN)

static bool rf_nonneg(float v) { return v >= 0.f && v <= 3.0e38f; }   // finite and not negative (false for NaN)

}  // namespace lasr

extern "C" int lasr_rflow_derivs(const float* level, float* record, int H, int W, void* hip_stream)
{
    if (!lasr::rf_size_ok(H, W)) return LASR_E_BADARG;
    if (!level || !record || level == record) return LASR_E_BADARG;
    const dim3 grid((unsigned)((W + lasr::RF_TX - 1) / lasr::RF_TX), (unsigned)((H + lasr::RF_TY - 1) / lasr::RF_TY));
    hipLaunchKernelGGL(lasr::rflow_derivs_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, level, record, H, W);
    return launch_ok();
}

extern "C" int lasr_rflow_tensor(const float* R1, const float* R2, const float* uv, float* Jb, float* Jg, int H, int W, void* hip_stream)
{
    if (!lasr::rf_size_ok(H, W)) return LASR_E_BADARG;
    if (!R1 || !R2 || !uv || !Jb || !Jg || Jb == Jg) return LASR_E_BADARG;
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(lasr::rflow_tensor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, R1, R2, uv, Jb,
                       Jg, H, W);
    return launch_ok();
}

extern "C" int lasr_rflow_weights(const float* Jb, const float* Jg, const float* uv, const float* d, float* J, float* psi, int H, int W,
                                  float eps, float beta, float gamma, void* hip_stream)
{
    if (!lasr::rf_size_ok(H, W) || !lasr::rf_pos(eps)) return LASR_E_BADARG;
    if (!lasr::rf_nonneg(beta) || !lasr::rf_nonneg(gamma) || !(beta > 0.f || gamma > 0.f)) return LASR_E_BADARG;
    if (!Jb || !Jg || !uv || !d || !J || !psi || J == Jb || J == Jg || J == psi) return LASR_E_BADARG;
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(lasr::rflow_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, Jb, Jg, uv, d,
                       J, psi, H, W, eps, beta, gamma);
    return launch_ok();
}
