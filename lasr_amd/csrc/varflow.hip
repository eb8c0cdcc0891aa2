// varflow.hip -- classical variational optical flow of preprocess/auto_gen.py --flow_method variational and of
// preprocess/propagate_mask.py (lasr_amd/nnutils/varflow.py runs the passes): coarse-to-fine, warping, robust data and smoothness
// terms (Brox et al. 2004, simplified), solved by red-black SOR.  This is the project's own addition; the reference estimates flow
// with a network and has no counterpart, and the definition is the one of include/lasr_ops.h, DESIGN.md section 4.16 and
// tests/varflow_restated.py, whose operation order every kernel here follows (built with -ffp-contract=off, as bake.hip).
// Flow fields inside the solver are planar [2,H,W] = (u, v); images are [H,W,3] fp32 in 0..1.  No floating-point atomics anywhere:
// the same input gives the same bits on every run.
#include <float.h>
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"

namespace lasr {

// ---- solver tile -------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads owns VF_TX x VF_TY = 64 x 8 pixels: a tile row is 256 bytes = two whole 128-byte lines of every
// plane (when W is a multiple of 32; otherwise no tile shape is line-aligned).  A thread owns a horizontal pair (2k, 2k + 1) of one
// row, one red and one black pixel, so every lane works in both half-sweeps.  du, dv, u, v and psi_s of the tile and a halo of 2
// are staged in 5 x 68 x 12 x 4 = 16320 bytes of LDS (9 workgroups fit in the 160 KiB of a CU, more than the 8 that 32 waves allow).
// A staged row keeps its even columns first and its odd columns behind them (VF_HALF apart): the 32 lanes of a half-wave, which
// read pixels two columns apart, read consecutive words, so every ds_read_b32 of the sweeps is free of bank conflicts.
constexpr int VF_TX = 64, VF_TY = 8, VF_HALO = 2;
constexpr int VF_SW = VF_TX + 2 * VF_HALO, VF_SH = VF_TY + 2 * VF_HALO, VF_HALF = VF_SW / 2;
constexpr int VF_RING = 2 * (VF_TX + 2) + 2 * VF_TY;                 // pixels of the ring at distance 1 around the tile
static_assert(VF_TX == 64 && VF_TY * (VF_TX / 2) == 256 && VF_RING <= 256, "thread mapping of varflow_sor_kernel");

__device__ __forceinline__ int vf_sidx(int lx, int ly) { return ly * VF_SW + (lx & 1) * VF_HALF + (lx >> 1); }

struct VfPixel {                                                      // the per-pixel constants of one sweep
    float J11, J12, J22, J13, J23, psid;
};

__device__ __forceinline__ VfPixel vf_load_pixel(const float* __restrict__ J, const float* __restrict__ psi, size_t n, size_t g)
{
    VfPixel p;
    p.J11 = J[g];
    p.J12 = J[n + g];
    p.J22 = J[2 * n + g];
    p.J13 = J[3 * n + g];
    p.J23 = J[4 * n + g];
    p.psid = psi[g];
    return p;
}

// One SOR update of the staged pixel (lx, ly) = image pixel (gx, gy); reads its four neighbours of the other colour.
__device__ __forceinline__ void vf_update(float* s_du, float* s_dv, const float* s_u, const float* s_v, const float* s_ps, int lx, int ly,
                                          int gx, int gy, int H, int W, const VfPixel& p, float ah, float om, float om1, float& o_du,
                                          float& o_dv)
{
    const int c = vf_sidx(lx, ly), l = vf_sidx(lx - 1, ly), r = vf_sidx(lx + 1, ly), up = vf_sidx(lx, ly - 1), dn = vf_sidx(lx, ly + 1);
    const float ps = s_ps[c];
    const float wl = gx > 0 ? ah * (ps + s_ps[l]) : 0.f, wr = gx < W - 1 ? ah * (ps + s_ps[r]) : 0.f;
    const float wu = gy > 0 ? ah * (ps + s_ps[up]) : 0.f, wd = gy < H - 1 ? ah * (ps + s_ps[dn]) : 0.f;
    const float ws = ((wl + wr) + wu) + wd;
    const float u = s_u[c], v = s_v[c], du = s_du[c], dv = s_dv[c];
    const float su = ((wl * (s_u[l] + s_du[l]) + wr * (s_u[r] + s_du[r])) + wu * (s_u[up] + s_du[up])) + wd * (s_u[dn] + s_du[dn]);
    const float ndu = om1 * du + om * (((su - ws * u) - p.psid * (p.J13 + p.J12 * dv)) / (p.psid * p.J11 + ws));
    const float sv = ((wl * (s_v[l] + s_dv[l]) + wr * (s_v[r] + s_dv[r])) + wu * (s_v[up] + s_dv[up])) + wd * (s_v[dn] + s_dv[dn]);
    const float ndv = om1 * dv + om * (((sv - ws * v) - p.psid * (p.J23 + p.J12 * ndu)) / (p.psid * p.J22 + ws));
    s_du[c] = ndu;
    s_dv[c] = ndv;
    o_du = ndu;
    o_dv = ndv;
}

// One full red-black iteration, d_in -> d_out (two buffers: a neighbouring workgroup reads this tile's old values as its halo).
// The red half-sweep runs on the tile and on the ring at distance 1, whose red pixels the black half-sweep of the tile reads; the
// ring's values are recomputed here from the same inputs by the same code as in the workgroup that owns them, so they carry the
// same bits, and are not stored.
__global__ __launch_bounds__(256) void varflow_sor_kernel(const float* __restrict__ J, const float* __restrict__ psi,
                                                          const float* __restrict__ uv, const float* __restrict__ d_in,
                                                          float* __restrict__ d_out, int H, int W, float ah, float om, float om1)
{
    __shared__ float s_du[VF_SW * VF_SH], s_dv[VF_SW * VF_SH], s_u[VF_SW * VF_SH], s_v[VF_SW * VF_SH], s_ps[VF_SW * VF_SH];
    const size_t n = (size_t)H * W;
    const int bx = (int)blockIdx.x * VF_TX, by = (int)blockIdx.y * VF_TY;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < VF_SW * VF_SH; i += 256) {
        const int ly = i / VF_SW, lx = i - ly * VF_SW;
        const int gx = bx + lx - VF_HALO, gy = by + ly - VF_HALO;
        float a = 0.f, b = 0.f, c = 0.f, e = 0.f, f = 0.f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            a = d_in[g];
            b = d_in[n + g];
            c = uv[g];
            e = uv[n + g];
            f = psi[n + g];
        }
        const int s = vf_sidx(lx, ly);
        s_du[s] = a;
        s_dv[s] = b;
        s_u[s] = c;
        s_v[s] = e;
        s_ps[s] = f;
    }
    // the thread's pair: columns bx + 2k and bx + 2k + 1 of row by + ty; bx is even, so the red one, (x + y) even, is at offset y & 1
    const int k = tid & 31, ty = tid >> 5;
    const int gy = by + ty, ly = ty + VF_HALO;
    const int off_r = gy & 1, off_b = off_r ^ 1;
    const int gx_r = bx + 2 * k + off_r, gx_b = bx + 2 * k + off_b;
    const bool in_r = gy < H && gx_r < W, in_b = gy < H && gx_b < W;
    const size_t g_r = (size_t)gy * W + gx_r, g_b = (size_t)gy * W + gx_b;
    VfPixel p_r = {}, p_b = {};
    if (in_r) p_r = vf_load_pixel(J, psi, n, g_r);
    if (in_b) p_b = vf_load_pixel(J, psi, n, g_b);
    // the thread's ring pixel, if it has one: top row, bottom row, left column, right column of the 66 x 10 region
    int rx = 0, ry = 0;
    bool ring = false;
    if (tid < VF_RING) {
        if (tid < VF_TX + 2) { rx = 1 + tid; ry = 1; }
        else if (tid < 2 * (VF_TX + 2)) { rx = 1 + tid - (VF_TX + 2); ry = VF_TY + VF_HALO; }
        else if (tid < 2 * (VF_TX + 2) + VF_TY) { rx = 1; ry = VF_HALO + tid - 2 * (VF_TX + 2); }
        else { rx = VF_TX + VF_HALO; ry = VF_HALO + tid - 2 * (VF_TX + 2) - VF_TY; }
        const int x = bx + rx - VF_HALO, y = by + ry - VF_HALO;
        ring = x >= 0 && x < W && y >= 0 && y < H && ((x + y) & 1) == 0;
    }
    VfPixel p_ring = {};
    if (ring) p_ring = vf_load_pixel(J, psi, n, (size_t)(by + ry - VF_HALO) * W + (bx + rx - VF_HALO));
    __syncthreads();
    float du_r = 0.f, dv_r = 0.f, du_b = 0.f, dv_b = 0.f, t0, t1;
    if (in_r) vf_update(s_du, s_dv, s_u, s_v, s_ps, 2 * k + off_r + VF_HALO, ly, gx_r, gy, H, W, p_r, ah, om, om1, du_r, dv_r);
    if (ring) vf_update(s_du, s_dv, s_u, s_v, s_ps, rx, ry, bx + rx - VF_HALO, by + ry - VF_HALO, H, W, p_ring, ah, om, om1, t0, t1);
    __syncthreads();
    if (in_b) vf_update(s_du, s_dv, s_u, s_v, s_ps, 2 * k + off_b + VF_HALO, ly, gx_b, gy, H, W, p_b, ah, om, om1, du_b, dv_b);
    if (in_r) {
        d_out[g_r] = du_r;
        d_out[n + g_r] = dv_r;
    }
    if (in_b) {
        d_out[g_b] = du_b;
        d_out[n + g_b] = dv_b;
    }
}

// ---- pyramid -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void varflow_unit_kernel(const unsigned char* __restrict__ img, float* __restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)img[i] / 255.f;
}

__device__ __forceinline__ float vf_at(const float* __restrict__ I, int W, int y, int x, int c) { return I[((size_t)y * W + x) * 3 + c]; }

// One thread per output element (y, x, c) of the [h,w,3] level.
__global__ __launch_bounds__(256) void varflow_reduce_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int h,
                                                             int w)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)h * w * 3) return;
    const int c = (int)(i % 3);
    const size_t px = i / 3;
    const int y = (int)(px / w), x = (int)(px - (size_t)y * w);
    const float kern[5] = {1.f / 16.f, 4.f / 16.f, 6.f / 16.f, 4.f / 16.f, 1.f / 16.f};
    float acc = 0.f;
    for (int a = 0; a < 5; a++) {
        const int yy = min(max(2 * y + a - 2, 0), H - 1);
        float row = 0.f;
        for (int b = 0; b < 5; b++) {
            const int xx = min(max(2 * x + b - 2, 0), W - 1);
            const float t = kern[b] * vf_at(in, W, yy, xx, c);
            row = b == 0 ? t : row + t;
        }
        const float t = kern[a] * row;
        acc = a == 0 ? t : acc + t;
    }
    out[i] = acc;
}

__device__ __forceinline__ float vf_lerp4(float v00, float v01, float v10, float v11, float tx, float ty)
{
    return (v00 * (1.f - tx) + v01 * tx) * (1.f - ty) + (v10 * (1.f - tx) + v11 * tx) * ty;
}

// One thread per pixel of the finer level, both planes.
__global__ __launch_bounds__(256) void varflow_expand_kernel(const float* __restrict__ in, float* __restrict__ out, int hc, int wc, int h,
                                                             int w)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)h * w, nc = (size_t)hc * wc;
    if (i >= n) return;
    const int y = (int)(i / w), x = (int)(i - (size_t)y * w);
    const float sy = (float)y * 0.5f, sx = (float)x * 0.5f;
    const float fy = floorf(sy), fx = floorf(sx);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = min(y0 + 1, hc - 1), x1 = min(x0 + 1, wc - 1);
    const float ty = sy - fy, tx = sx - fx;
    for (int p = 0; p < 2; p++) {
        const float* f = in + p * nc;
        out[p * n + i] = 2.f * vf_lerp4(f[(size_t)y0 * wc + x0], f[(size_t)y0 * wc + x1], f[(size_t)y1 * wc + x0], f[(size_t)y1 * wc + x1],
                                        tx, ty);
    }
}

// ---- linearisation -----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float vf_gx(const float* __restrict__ I, int W, int y, int x, int c)
{
    return 0.5f * (vf_at(I, W, y, min(x + 1, W - 1), c) - vf_at(I, W, y, max(x - 1, 0), c));
}

__device__ __forceinline__ float vf_gy(const float* __restrict__ I, int H, int W, int y, int x, int c)
{
    return 0.5f * (vf_at(I, W, min(y + 1, H - 1), x, c) - vf_at(I, W, max(y - 1, 0), x, c));
}

// One thread per pixel: the six planes of the motion tensor, zero where the warped position leaves the frame.
__global__ __launch_bounds__(256) void varflow_tensor_kernel(const float* __restrict__ I1, const float* __restrict__ I2,
                                                             const float* __restrict__ uv, float* __restrict__ J, int H, int W)
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
    float j[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 3; c++) {
        const float g2x = vf_lerp4(vf_gx(I2, W, y0, x0, c), vf_gx(I2, W, y0, x1, c), vf_gx(I2, W, y1, x0, c), vf_gx(I2, W, y1, x1, c), tx, ty);
        const float g2y = vf_lerp4(vf_gy(I2, H, W, y0, x0, c), vf_gy(I2, H, W, y0, x1, c), vf_gy(I2, H, W, y1, x0, c),
                                   vf_gy(I2, H, W, y1, x1, c), tx, ty);
        const float i2 = vf_lerp4(vf_at(I2, W, y0, x0, c), vf_at(I2, W, y0, x1, c), vf_at(I2, W, y1, x0, c), vf_at(I2, W, y1, x1, c), tx, ty);
        const float Ix = 0.5f * (g2x + vf_gx(I1, W, y, x, c));
        const float Iy = 0.5f * (g2y + vf_gy(I1, H, W, y, x, c));
        const float It = i2 - vf_at(I1, W, y, x, c);
        const float t[6] = {Ix * Ix, Ix * Iy, Iy * Iy, Ix * It, Iy * It, It * It};
        for (int q = 0; q < 6; q++) j[q] = c == 0 ? t[q] : j[q] + t[q];
    }
    for (int q = 0; q < 6; q++) J[q * n + i] = valid ? j[q] : 0.f;
}

// One thread per pixel: psi_d from the linearised residual, psi_s from the gradients of the updated flow.
__global__ __launch_bounds__(256) void varflow_weights_kernel(const float* __restrict__ J, const float* __restrict__ uv,
                                                              const float* __restrict__ d, float* __restrict__ psi, int H, int W, float eps)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)H * W;
    if (i >= n) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const float e2 = eps * eps;
    const float du = d[i], dv = d[n + i];
    const float r2 = (du * du) * J[i] + ((2.f * du) * dv) * J[n + i] + (dv * dv) * J[2 * n + i] + (2.f * du) * J[3 * n + i] +
                     (2.f * dv) * J[4 * n + i] + J[5 * n + i];
    psi[i] = 0.5f / sqrtf(fmaxf(r2, 0.f) + e2);
    const size_t l = i - (x > 0), r = i + (x < W - 1), up = i - (y > 0 ? (size_t)W : 0), dn = i + (y < H - 1 ? (size_t)W : 0);
    const float ux = 0.5f * ((uv[r] + d[r]) - (uv[l] + d[l])), uy = 0.5f * ((uv[dn] + d[dn]) - (uv[up] + d[up]));
    const float vx = 0.5f * ((uv[n + r] + d[n + r]) - (uv[n + l] + d[n + l])), vy = 0.5f * ((uv[n + dn] + d[n + dn]) - (uv[n + up] + d[n + up]));
    psi[n + i] = 0.5f / sqrtf(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + e2);
}

// ---- occlusion ---------------------------------------------------------------------------------------------------------------------

// One thread per pixel: forward-backward disagreement, as a logit-like score clamped to +-6; never exactly 0.
__global__ __launch_bounds__(256) void varflow_occ_kernel(const float* __restrict__ f_ab, const float* __restrict__ f_ba,
                                                          float* __restrict__ occ, int H, int W, float tau, float s)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const float fx = f_ab[i * 2], fy = f_ab[i * 2 + 1];
    const float X = (float)x + fx, Y = (float)y + fy;
    float o = 6.f;
    if (X >= 0.f && X <= (float)(W - 1) && Y >= 0.f && Y <= (float)(H - 1)) {                      // false for a NaN flow too
        const float flx = floorf(X), fly = floorf(Y);
        const int x0 = (int)flx, y0 = (int)fly;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float tx = X - flx, ty = Y - fly;
        const size_t a = ((size_t)y0 * W + x0) * 2, b = ((size_t)y0 * W + x1) * 2, c = ((size_t)y1 * W + x0) * 2, e = ((size_t)y1 * W + x1) * 2;
        const float ex = fx + vf_lerp4(f_ba[a], f_ba[b], f_ba[c], f_ba[e], tx, ty);
        const float ey = fy + vf_lerp4(f_ba[a + 1], f_ba[b + 1], f_ba[c + 1], f_ba[e + 1], tx, ty);
        o = fminf(fmaxf((sqrtf(ex * ex + ey * ey) - tau) / s, -6.f), 6.f);
        if (!(o == o)) o = 6.f;                                                                     // a NaN in f_ba
        if (o == 0.f) o = FLT_MIN;                                                                  // the loader reads 0 as padding
    }
    occ[i] = o;
}

static bool vf_size_ok(int H, int W)
{
    return H >= LASR_VARFLOW_MIN_SIZE && W >= LASR_VARFLOW_MIN_SIZE && H <= LASR_VARFLOW_MAX_SIZE && W <= LASR_VARFLOW_MAX_SIZE;
}

static bool vf_pos(float v) { return v > 0.f && v <= 3.0e38f; }       // finite and positive (false for NaN)

static unsigned vf_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace lasr

extern "C" int lasr_varflow_reduce(const unsigned char* img_u8, const float* in, float* level0, float* out, int H, int W, void* hip_stream)
{
    if (!lasr::vf_size_ok(H, W)) return LASR_E_BADARG;
    if ((img_u8 != nullptr) == (in != nullptr)) return LASR_E_BADARG;                  // exactly one input form
    if (img_u8 ? (!level0 || out == level0) : (level0 != nullptr || !out || out == in)) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t n = (size_t)H * W * 3;
    if (img_u8) {
        hipLaunchKernelGGL(lasr::varflow_unit_kernel, dim3(lasr::vf_blocks(n)), dim3(256), 0, st, img_u8, level0, n);
        in = level0;
    }
    if (out) {
        const int h = (H + 1) / 2, w = (W + 1) / 2;
        hipLaunchKernelGGL(lasr::varflow_reduce_kernel, dim3(lasr::vf_blocks((size_t)h * w * 3)), dim3(256), 0, st, in, out, H, W, h, w);
    }
    return launch_ok();
}

extern "C" int lasr_varflow_expand(const float* uv_coarse, float* uv_fine, int hc, int wc, int h, int w, void* hip_stream)
{
    if (!lasr::vf_size_ok(h, w) || hc < 1 || wc < 1 || hc != (h + 1) / 2 || wc != (w + 1) / 2) return LASR_E_BADARG;
    if (!uv_coarse || !uv_fine || uv_coarse == uv_fine) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::varflow_expand_kernel, dim3(lasr::vf_blocks((size_t)h * w)), dim3(256), 0, (hipStream_t)hip_stream, uv_coarse,
                       uv_fine, hc, wc, h, w);
    return launch_ok();
}

extern "C" int lasr_varflow_tensor(const float* I1, const float* I2, const float* uv, float* J, int H, int W, void* hip_stream)
{
    if (!lasr::vf_size_ok(H, W)) return LASR_E_BADARG;
    if (!I1 || !I2 || !uv || !J) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::varflow_tensor_kernel, dim3(lasr::vf_blocks((size_t)H * W)), dim3(256), 0, (hipStream_t)hip_stream, I1, I2, uv,
                       J, H, W);
    return launch_ok();
}

extern "C" int lasr_varflow_weights(const float* J, const float* uv, const float* d, float* psi, int H, int W, float eps, void* hip_stream)
{
    if (!lasr::vf_size_ok(H, W) || !lasr::vf_pos(eps)) return LASR_E_BADARG;
    if (!J || !uv || !d || !psi) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::varflow_weights_kernel, dim3(lasr::vf_blocks((size_t)H * W)), dim3(256), 0, (hipStream_t)hip_stream, J, uv, d,
                       psi, H, W, eps);
    return launch_ok();
}

extern "C" int lasr_varflow_sor(const float* J, const float* psi, const float* uv, float* d, float* scratch, int H, int W, float alpha,
                                float omega, int iters, void* hip_stream)
{
    if (!lasr::vf_size_ok(H, W) || !lasr::vf_pos(alpha) || !(omega > 0.f && omega < 2.f) || iters < 0) return LASR_E_BADARG;
    if (!J || !psi || !uv || !d || !scratch || d == scratch) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)((W + lasr::VF_TX - 1) / lasr::VF_TX), (unsigned)((H + lasr::VF_TY - 1) / lasr::VF_TY));
    const float ah = alpha * 0.5f, om1 = 1.f - omega;
    float *src = d, *dst = scratch;
    for (int it = 0; it < iters; it++) {
        hipLaunchKernelGGL(lasr::varflow_sor_kernel, grid, dim3(256), 0, st, J, psi, uv, (const float*)src, dst, H, W, ah, omega, om1);
        float* t = src;
        src = dst;
        dst = t;
    }
    if (src != d) (void)hipMemcpyAsync(d, src, (size_t)H * W * 2 * sizeof(float), hipMemcpyDeviceToDevice, st);   // an odd count
    return launch_ok();
}

extern "C" int lasr_varflow_occ(const float* f_ab, const float* f_ba, float* occ, int H, int W, float tau, float s, void* hip_stream)
{
    if (!lasr::vf_size_ok(H, W) || !(tau >= 0.f && tau <= 3.0e38f) || !lasr::vf_pos(s)) return LASR_E_BADARG;
    if (!f_ab || !f_ba || !occ) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::varflow_occ_kernel, dim3(lasr::vf_blocks((size_t)H * W)), dim3(256), 0, (hipStream_t)hip_stream, f_ab, f_ba,
                       occ, H, W, tau, s);
    return launch_ok();
}
