// motionseg.hip -- motion segmentation of preprocess/auto_mask.py (lasr_amd/nnutils/motionseg.py runs the passes): silhouettes
// from motion alone.  This is the project's own addition; the reference has no counterpart (its preprocess/mask.py is a detector),
// and the definition is the one of include/lasr_ops.h and DESIGN.md section 4.17.
// One ordered frame pair: the forward-backward confidence of its flow, `iters` IRLS iterations of an 8-parameter motion model
// (a per-pixel robust reduction to 28 fp64 moments and a residual histogram, then one workgroup that solves and writes the next
// state on the device), and the evidence map.  No floating-point atomics anywhere: the same input gives the same bits on every run.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"

namespace lasr {

constexpr int MS_BLOCKS = LASR_MOTIONSEG_BLOCKS, MS_MOM = LASR_MOTIONSEG_MOMENTS, MS_BINS = LASR_MOTIONSEG_BINS;
constexpr int MS_SIGMA = 8, MS_MED = 9, MS_N = 10, MS_STATUS = 11;

__device__ __forceinline__ bool ms_finite(float v) { return fabsf(v) <= 3.4028235e38f; }      // false for NaN

__device__ __forceinline__ float ms_bilinear(const float* __restrict__ f, int W, int xa, int xb, int ya, int yb, float tx, float ty)
{
    const float v00 = f[((size_t)ya * W + xa) * 2], v01 = f[((size_t)ya * W + xb) * 2];
    const float v10 = f[((size_t)yb * W + xa) * 2], v11 = f[((size_t)yb * W + xb) * 2];
    return (v00 * (1.f - tx) + v01 * tx) * (1.f - ty) + (v10 * (1.f - tx) + v11 * tx) * ty;
}

// One thread per pixel of frame a: the taps and the expression of maskprop_unary_kernel's conf.
__global__ __launch_bounds__(256) void motionseg_conf_kernel(const float* __restrict__ f_ab, const float* __restrict__ f_ba,
                                                             float* __restrict__ conf, int H, int W, float inv2tau2)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const float fx = f_ab[i * 2], fy = f_ab[i * 2 + 1];
    const float qx = (float)x + fx, qy = (float)y + fy;
    float c = 0.f;
    if (qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1)) {       // false for a NaN flow too
        const float flx = floorf(qx), fly = floorf(qy);
        const int xa = (int)flx, ya = (int)fly;
        const int xb = min(xa + 1, W - 1), yb = min(ya + 1, H - 1);
        const float tx = qx - flx, ty = qy - fly;
        const float ex = fx + ms_bilinear(f_ba, W, xa, xb, ya, yb, tx, ty);
        const float ey = fy + ms_bilinear(f_ba + 1, W, xa, xb, ya, yb, tx, ty);
        c = expf(-(ex * ex + ey * ey) * inv2tau2);
        if (!(c >= 0.f)) c = 0.f;                                                      // the flow back is not a number
    }
    conf[i] = c;
}

// The model and the residual of one pixel in fp32, in the operation order of tests/motionseg_restated.py.
struct MsModel {
    float th[8];
    double cx, cy, s;
    __device__ __forceinline__ void load(const double* __restrict__ state, int H, int W)
    {
        for (int k = 0; k < 8; k++) th[k] = (float)state[k];
        cx = 0.5 * (double)(W - 1);
        cy = 0.5 * (double)(H - 1);
        s = 0.5 * (double)(H > W ? H : W);
    }
    __device__ __forceinline__ float r2(int x, int y, float u, float v, double& X, double& Y) const
    {
        X = ((double)x - cx) / s;
        Y = ((double)y - cy) / s;
        const float Xf = (float)X, Yf = (float)Y;
        const float um = th[0] + th[1] * Xf + th[2] * Yf + th[6] * (Xf * Xf) + th[7] * (Xf * Yf);
        const float vm = th[3] + th[4] * Xf + th[5] * Yf + th[6] * (Xf * Yf) + th[7] * (Yf * Yf);
        const float du = u - um, dv = v - vm;
        return du * du + dv * dv;
    }
};

// Workgroup b owns the pixels b * 256 + lane, + gridDim.x * 256, ...: fixed by (H, W).  28 fp64 accumulators per lane, folded
// across the wave by shuffles, across the four waves through LDS in wave order, one row of `partials` per workgroup; workgroup 0
// zeroes the rows of the workgroups that do not exist.  The histogram is LDS-private and merged with integer atomics.
__global__ __launch_bounds__(256) void motionseg_moments_kernel(const float* __restrict__ flow, const float* __restrict__ conf,
                                                                const double* __restrict__ state, double* __restrict__ partials,
                                                                unsigned* __restrict__ hist, int H, int W)
{
    __shared__ unsigned h[MS_BINS];
    __shared__ double red[4][MS_MOM];
    for (int i = threadIdx.x; i < MS_BINS; i += 256) h[i] = 0u;
    __syncthreads();
    MsModel m;
    m.load(state, H, W);
    const double sd = state[MS_SIGMA];
    const bool flat = !(fabs(sd) <= 1.7976931348623157e308);                           // sigma = inf: the first iteration
    const float sig = (float)sd, s2 = sig * sig;
    double a[MS_MOM];
#pragma unroll
    for (int k = 0; k < MS_MOM; k++) a[k] = 0.;
    const long long n = (long long)H * W, stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float c = conf[i], u = flow[i * 2], v = flow[i * 2 + 1];
        if (!(c > 0.f) || !ms_finite(u) || !ms_finite(v)) continue;                    // skipped, never multiplied by 0
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        double X, Y;
        const float r2 = m.r2(x, y, u, v, X, Y);
        float w = c;
        if (!flat) {
            const float t = 1.f + r2 / s2;
            w = c / (t * t);
        }
        if (c >= 0.5f) {
            const float b = floorf(16.f * sqrtf(r2));
            atomicAdd(&h[b < (float)(MS_BINS - 1) ? (int)b : MS_BINS - 1], 1u);
        }
        const double wd = (double)w, ud = (double)u, vd = (double)v;
        const double X2 = X * X, XY = X * Y, Y2 = Y * Y;
        const double mono[15] = {1., X, Y, X2, XY, Y2, X2 * X, X2 * Y, X * Y2, Y2 * Y, X2 * X2, X2 * XY, X2 * Y2, XY * Y2, Y2 * Y2};
#pragma unroll
        for (int k = 0; k < 15; k++) a[k] += wd * mono[k];
        const double wu = wd * ud, wv = wd * vd;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            a[15 + k] += wu * mono[k];
            a[21 + k] += wv * mono[k];
        }
        a[27] += wd * (ud * ud + vd * vd);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MS_MOM; k++) {
        double s = a[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < MS_MOM)
        partials[(size_t)blockIdx.x * MS_MOM + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x])
                                                             + red[3][threadIdx.x];
    if (blockIdx.x == 0)
        for (int i = (int)gridDim.x * MS_MOM + (int)threadIdx.x; i < MS_BLOCKS * MS_MOM; i += 256) partials[i] = 0.;
    for (int i = threadIdx.x; i < MS_BINS; i += 256) {
        const unsigned c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// the model's basis as exponent pairs of X^i Y^j (-1: the entry is 0); slot of a monomial: d (d + 1) / 2 + j with d = i + j
__device__ const signed char MS_BU[8][2] = {{0, 0}, {1, 0}, {0, 1}, {-1, -1}, {-1, -1}, {-1, -1}, {2, 0}, {1, 1}};
__device__ const signed char MS_BV[8][2] = {{-1, -1}, {-1, -1}, {-1, -1}, {0, 0}, {1, 0}, {0, 1}, {1, 1}, {0, 2}};

__device__ __forceinline__ int ms_slot(int i, int j) { return (i + j) * (i + j + 1) / 2 + j; }

// One workgroup.  Threads 0..27 fold the rows of `partials` in index order; all threads scan the histogram (4 bins each, a
// Hillis-Steele scan of the 256 sums in LDS) for its total and the median bin; thread 0 assembles, solves and writes the state.
__global__ __launch_bounds__(256) void motionseg_solve_kernel(const double* __restrict__ partials, const unsigned* __restrict__ hist,
                                                              double* __restrict__ state, int model, double k_sigma, double sigma_min,
                                                              double ridge)
{
    __shared__ double M[MS_MOM], A[8][8], L[8][8], b[8], th[8], rhs[8], yv[8], d[8];
    __shared__ unsigned scan[2][256];
    __shared__ int med_bin;
    const int t = threadIdx.x;
    if (t < MS_MOM) {
        double s = 0.;
        for (int r = 0; r < MS_BLOCKS; r++) s += partials[(size_t)r * MS_MOM + t];
        M[t] = s;
    }
    unsigned own[4], sum = 0u;
    for (int k = 0; k < 4; k++) {
        own[k] = hist[t * 4 + k];
        sum += own[k];
    }
    scan[0][t] = sum;
    if (t == 0) med_bin = 0;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < 256; o <<= 1) {
        scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned n = scan[cur][255], target = (n + 1u) / 2u;
    unsigned below = scan[cur][t] - sum;                                               // the exclusive prefix
    if (n > 0u && below < target && below + sum >= target) {                           // exactly one thread
        int k = 0;
        while (below + own[k] < target) below += own[k++];
        med_bin = t * 4 + k;
    }
    __syncthreads();
    if (t != 0) return;
    const bool on_lin = model >= 1, on_quad = model >= 2;
    for (int i = 0; i < 8; i++) {
        for (int j = 0; j < 8; j++) {
            double s = 0.;
            if (MS_BU[i][0] >= 0 && MS_BU[j][0] >= 0) s += M[ms_slot(MS_BU[i][0] + MS_BU[j][0], MS_BU[i][1] + MS_BU[j][1])];
            if (MS_BV[i][0] >= 0 && MS_BV[j][0] >= 0) s += M[ms_slot(MS_BV[i][0] + MS_BV[j][0], MS_BV[i][1] + MS_BV[j][1])];
            A[i][j] = s;
        }
        double s = 0.;
        if (MS_BU[i][0] >= 0) s += M[15 + ms_slot(MS_BU[i][0], MS_BU[i][1])];
        if (MS_BV[i][0] >= 0) s += M[21 + ms_slot(MS_BV[i][0], MS_BV[i][1])];
        b[i] = s;
        th[i] = state[i];
    }
    for (int k = 0; k < 8; k++) {
        const bool on = k == 0 || k == 3 || (k >= 6 ? on_quad : on_lin);
        if (on) continue;
        for (int j = 0; j < 8; j++) A[k][j] = A[j][k] = 0.;
        A[k][k] = 1.;
        b[k] = th[k] = 0.;
    }
    for (int i = 0; i < 8; i++) {
        double s = 0.;
        for (int j = 0; j < 8; j++) s += A[i][j] * th[j];
        const bool on = i == 0 || i == 3 || (i >= 6 ? on_quad : on_lin);
        rhs[i] = on ? b[i] - s : 0.;
    }
    double tr = 0.;
    for (int k = 0; k < 8; k++) tr += A[k][k];
    const double lam = ridge * tr / 8.;
    for (int k = 0; k < 8; k++) A[k][k] += lam;
    bool ok = n > 0u;
    for (int j = 0; j < 8 && ok; j++) {
        double p = A[j][j];
        for (int k = 0; k < j; k++) p -= L[j][k] * L[j][k];
        if (!(p > 0.)) {
            ok = false;
            break;
        }
        L[j][j] = sqrt(p);
        for (int i = j + 1; i < 8; i++) {
            double s = A[i][j];
            for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    if (ok) {
        for (int i = 0; i < 8; i++) {
            double s = rhs[i];
            for (int k = 0; k < i; k++) s -= L[i][k] * yv[k];
            yv[i] = s / L[i][i];
        }
        for (int i = 7; i >= 0; i--) {
            double s = yv[i];
            for (int k = i + 1; k < 8; k++) s -= L[k][i] * d[k];
            d[i] = s / L[i][i];
            if (!(fabs(d[i]) <= 1.7976931348623157e308)) ok = false;
        }
    }
    state[MS_N] = (double)n;
    if (!ok) {
        state[MS_STATUS] = 1.;
        return;
    }
    const double med = ((double)med_bin + 0.5) / 16.;
    const double sg = k_sigma * med;
    for (int k = 0; k < 8; k++) state[k] = th[k] + d[k];
    state[MS_SIGMA] = sg > sigma_min ? sg : sigma_min;
    state[MS_MED] = med;
    state[MS_STATUS] = 0.;
}

// One thread per pixel.
__global__ __launch_bounds__(256) void motionseg_evidence_kernel(const float* __restrict__ flow, const float* __restrict__ conf,
                                                                 const double* __restrict__ state, float* __restrict__ evid, int H,
                                                                 int W, float kappa, float U, int accumulate)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const float c = conf[i], u = flow[i * 2], v = flow[i * 2 + 1];
    float e = 0.f;
    if (c > 0.f && ms_finite(u) && ms_finite(v)) {
        MsModel m;
        m.load(state, H, W);
        const float sig = (float)state[MS_SIGMA];
        const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        double X, Y;
        const float r2 = m.r2(x, y, u, v, X, Y);
        e = c * fminf(fmaxf(r2 / (sig * sig) - kappa, -U), U);
    }
    evid[i] = accumulate ? evid[i] + e : e;
}

static bool ms_size_ok(int H, int W) { return H >= 0 && W >= 0 && H <= LASR_MOTIONSEG_MAX_SIZE && W <= LASR_MOTIONSEG_MAX_SIZE; }

static bool ms_pos(float v) { return v > 0.f && v <= 3.0e38f; }       // finite and positive (false for NaN)

}  // namespace lasr

extern "C" int lasr_motionseg_conf(const float* f_ab, const float* f_ba, float* conf, int H, int W, float tau, void* hip_stream)
{
    if (!lasr::ms_size_ok(H, W) || !lasr::ms_pos(tau)) return LASR_E_BADARG;
    if (H == 0 || W == 0) return LASR_OK;
    if (!f_ab || !f_ba || !conf || conf == f_ab || conf == f_ba) return LASR_E_BADARG;
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(lasr::motionseg_conf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, f_ab,
                       f_ba, conf, H, W, 1.f / (2.f * tau * tau));
    return launch_ok();
}

extern "C" int lasr_motionseg_moments(const float* flow, const float* conf, const double* state, double* partials, unsigned* hist,
                                      int H, int W, void* hip_stream)
{
    if (!lasr::ms_size_ok(H, W)) return LASR_E_BADARG;
    if (H == 0 || W == 0) return LASR_OK;
    if (!flow || !conf || !state || !partials || !hist) return LASR_E_BADARG;
    const void *in[3] = {flow, conf, state}, *out[2] = {partials, hist};
    for (const void* o : out)
        for (const void* i : in)
            if (o == i) return LASR_E_BADARG;
    if ((const void*)partials == (const void*)hist) return LASR_E_BADARG;
    const long long n = (long long)H * W, blocks = (n + 255) / 256;
    hipLaunchKernelGGL(lasr::motionseg_moments_kernel, dim3((unsigned)(blocks < lasr::MS_BLOCKS ? blocks : lasr::MS_BLOCKS)), dim3(256),
                       0, (hipStream_t)hip_stream, flow, conf, state, partials, hist, H, W);
    return launch_ok();
}

extern "C" int lasr_motionseg_solve(const double* partials, const unsigned* hist, double* state, int H, int W, int model, float k_sigma,
                                    float sigma_min, float ridge, void* hip_stream)
{
    if (!lasr::ms_size_ok(H, W) || model < 0 || model > 2) return LASR_E_BADARG;
    if (!lasr::ms_pos(k_sigma) || !lasr::ms_pos(sigma_min) || !(ridge >= 0.f && ridge <= 3.0e38f)) return LASR_E_BADARG;
    if (H == 0 || W == 0) return LASR_OK;
    if (!partials || !hist || !state || (const void*)state == (const void*)partials || (const void*)state == (const void*)hist)
        return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::motionseg_solve_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, partials, hist, state, model,
                       (double)k_sigma, (double)sigma_min, (double)ridge);
    return launch_ok();
}

extern "C" int lasr_motionseg_evidence(const float* flow, const float* conf, const double* state, float* evid, int H, int W, float kappa,
                                       float U, int accumulate, void* hip_stream)
{
    if (!lasr::ms_size_ok(H, W) || !lasr::ms_pos(kappa) || !lasr::ms_pos(U)) return LASR_E_BADARG;
    if (accumulate != 0 && accumulate != 1) return LASR_E_BADARG;
    if (H == 0 || W == 0) return LASR_OK;
    if (!flow || !conf || !state || !evid || evid == flow || evid == conf || (const void*)evid == (const void*)state)
        return LASR_E_BADARG;
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(lasr::motionseg_evidence_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, flow,
                       conf, state, evid, H, W, kappa, U, accumulate);
    return launch_ok();
}
