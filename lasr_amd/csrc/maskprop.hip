// maskprop.hip -- silhouette propagation of preprocess/propagate_mask.py (lasr_amd/nnutils/maskprop.py runs the passes): carries one
// annotated mask through a video along the VCN flow.  This is the project's own addition; the reference has no counterpart (its
// preprocess/mask.py is a detector), and the definition is the one of include/lasr_ops.h and DESIGN.md section 4.13.
// One step s -> t: colour histograms of frame s (LDS-private per workgroup, merged with integer atomics), a unary field from the
// backward warp, the forward-backward flow consistency and the histograms' log ratio, then K edge-aware mean-field iterations on
// a tile staged with its halo in LDS.  No floating-point atomics anywhere: the same input gives the same bits on every run.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"

namespace lasr {

constexpr int MP_BINS = LASR_MASKPROP_BINS;
constexpr int MP_TX = 32, MP_TY = 8;                                 // mean-field tile: 4 waves of 32 x 2 pixels, one pixel per lane

__device__ __forceinline__ int mp_bin(const unsigned char* px)
{
    return ((int)(px[0] >> 4) << 8) | ((int)(px[1] >> 4) << 4) | (int)(px[2] >> 4);
}

__device__ __forceinline__ float mp_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// hist[1][bin] += #{p in window : P >= hi}, hist[0][bin] += #{p in window : P <= lo}.  Each block owns rows y0 + blockIdx.x,
// + gridDim.x, ... of the window and counts them in its own LDS histogram; only the bins it touched reach global memory.
__global__ __launch_bounds__(256) void maskprop_hist_kernel(const unsigned char* __restrict__ img, const float* __restrict__ P,
                                                            unsigned* __restrict__ hist, int W, int x0, int y0, int x1, int y1,
                                                            float hi, float lo)
{
    __shared__ unsigned h[2 * MP_BINS];
    for (int i = threadIdx.x; i < 2 * MP_BINS; i += 256) h[i] = 0u;
    __syncthreads();
    const int ww = x1 - x0;
    for (int y = y0 + (int)blockIdx.x; y < y1; y += (int)gridDim.x) {
        const size_t row = (size_t)y * W;
        for (int x = x0 + (int)threadIdx.x; x < x0 + ww; x += 256) {
            const float p = P[row + x];
            const int fg = p >= hi, bg = p <= lo;
            if (fg | bg) atomicAdd(&h[(fg ? MP_BINS : 0) + mp_bin(img + (row + x) * 3)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * MP_BINS; i += 256) {
        const unsigned c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// One block: totals of the two histogram rows (integers, so exact), then app[b] = log((hf[b]/Nf + eps) / (hb[b]/Nb + eps)).
__global__ __launch_bounds__(256) void maskprop_table_kernel(const unsigned* __restrict__ hist, float* __restrict__ app, float eps)
{
    __shared__ unsigned long long red[2][256];
    unsigned long long sb = 0, sf = 0;
    for (int i = threadIdx.x; i < MP_BINS; i += 256) {
        sb += hist[i];
        sf += hist[MP_BINS + i];
    }
    red[0][threadIdx.x] = sb;
    red[1][threadIdx.x] = sf;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    const float Nb = (float)(red[0][0] ? red[0][0] : 1ull), Nf = (float)(red[1][0] ? red[1][0] : 1ull);
    for (int i = threadIdx.x; i < MP_BINS; i += 256)
        app[i] = logf(((float)hist[MP_BINS + i] / Nf + eps) / ((float)hist[i] / Nb + eps));
}

__device__ __forceinline__ float mp_bilinear(const float* __restrict__ f, int stride, int W, int xa, int xb, int ya, int yb, float tx,
                                             float ty)
{
    const float v00 = f[((size_t)ya * W + xa) * stride], v01 = f[((size_t)ya * W + xb) * stride];
    const float v10 = f[((size_t)yb * W + xa) * stride], v11 = f[((size_t)yb * W + xb) * stride];
    return (v00 * (1.f - tx) + v01 * tx) * (1.f - ty) + (v10 * (1.f - tx) + v11 * tx) * ty;
}

// One thread per pixel of frame t.
__global__ __launch_bounds__(256) void maskprop_unary_kernel(const unsigned char* __restrict__ img_t, const float* __restrict__ P_s,
                                                             const float* __restrict__ flow_ts, const float* __restrict__ flow_st,
                                                             const float* __restrict__ app, float* __restrict__ u_out,
                                                             float* __restrict__ q_out, int H, int W, float inv2tau2, float w_p,
                                                             float w_a, float U)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const float fx = flow_ts[i * 2], fy = flow_ts[i * 2 + 1];
    const float qx = (float)x + fx, qy = (float)y + fy;
    float prior = 0.f, conf = 0.f;
    if (qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1)) {       // false for a NaN flow too
        const float flx = floorf(qx), fly = floorf(qy);
        const int xa = (int)flx, ya = (int)fly;
        const int xb = min(xa + 1, W - 1), yb = min(ya + 1, H - 1);
        const float tx = qx - flx, ty = qy - fly;
        prior = mp_bilinear(P_s, 1, W, xa, xb, ya, yb, tx, ty);
        const float ex = fx + mp_bilinear(flow_st, 2, W, xa, xb, ya, yb, tx, ty);
        const float ey = fy + mp_bilinear(flow_st + 1, 2, W, xa, xb, ya, yb, tx, ty);
        conf = expf(-(ex * ex + ey * ey) * inv2tau2);
    }
    const float pc = fminf(fmaxf(prior, 1e-3f), 1.f - 1e-3f);
    const float lg = logf(pc / (1.f - pc));
    float u = w_p * conf * lg + w_a * app[mp_bin(img_t + i * 3)];
    u = fminf(fmaxf(u, -U), U);
    u_out[i] = u;
    q_out[i] = mp_sigmoid(u);
}

// One mean-field iteration on a 32 x 8 tile.  The tile and its halo of R pixels are staged once: q and the packed colour, two
// LDS planes of (32 + 2R) x (8 + 2R) words.  A pixel outside the image is staged as q = 0.5, whose 2q - 1 is exactly 0, so the
// tap loop needs no bounds test.  The bilateral weights are recomputed from the staged colours in every launch.
// Row stride 32 + 2R words: the 32 lanes of a wave's half read consecutive words, free of bank conflicts for every R.
__global__ __launch_bounds__(256) void maskprop_meanfield_kernel(const unsigned char* __restrict__ img, const float* __restrict__ u,
                                                                 const float* __restrict__ q_in, float* __restrict__ q_out, int H,
                                                                 int W, int R, float inv2sI2, float inv2sS2, float w_s)
{
    extern __shared__ unsigned mp_lds[];
    const int SW = MP_TX + 2 * R, SH = MP_TY + 2 * R, n = SW * SH;
    float* sq = (float*)mp_lds;
    unsigned* sc = mp_lds + n;
    const int bx = (int)blockIdx.x * MP_TX, by = (int)blockIdx.y * MP_TY;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int ly = i / SW, lx = i - ly * SW;
        const int gx = bx + lx - R, gy = by + ly - R;
        float q = 0.5f;
        unsigned c = 0u;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            q = q_in[g];
            c = (unsigned)img[g * 3] | ((unsigned)img[g * 3 + 1] << 8) | ((unsigned)img[g * 3 + 2] << 16);
        }
        sq[i] = q;
        sc[i] = c;
    }
    __syncthreads();
    const int tx = threadIdx.x & (MP_TX - 1), ty = threadIdx.x / MP_TX;
    const int x = bx + tx, y = by + ty;
    if (x >= W || y >= H) return;
    const int ctr = (ty + R) * SW + tx + R;
    const unsigned c0 = sc[ctr];
    const int r0 = (int)(c0 & 255u), g0 = (int)((c0 >> 8) & 255u), b0 = (int)(c0 >> 16);
    float acc = 0.f;
    for (int dy = -R; dy <= R; dy++) {
        const int base = ctr + dy * SW;
        for (int dx = -R; dx <= R; dx++) {
            if ((dx | dy) == 0) continue;
            const unsigned c = sc[base + dx];
            const int dr = (int)(c & 255u) - r0, dg = (int)((c >> 8) & 255u) - g0, db = (int)(c >> 16) - b0;
            const float k = expf(-((float)(dr * dr + dg * dg + db * db) * inv2sI2) - (float)(dx * dx + dy * dy) * inv2sS2);
            acc += k * (2.f * sq[base + dx] - 1.f);
        }
    }
    const size_t g = (size_t)y * W + x;
    q_out[g] = mp_sigmoid(u[g] + w_s * acc);
}

static bool mp_image_ok(int H, int W)
{
    return H >= 0 && W >= 0 && H <= LASR_MASKPROP_MAX_SIZE && W <= LASR_MASKPROP_MAX_SIZE && (long long)H * W <= 0x7fffffffLL / 3;
}

static bool mp_pos(float v) { return v > 0.f && v <= 3.0e38f; }       // finite and positive (false for NaN)

}  // namespace lasr

extern "C" int lasr_maskprop_hist(const unsigned char* img, const float* P, unsigned* hist, int H, int W, int x0, int y0, int x1, int y1,
                                  float hi, float lo, void* hip_stream)
{
    if (!lasr::mp_image_ok(H, W)) return LASR_E_BADARG;
    if (x0 < 0 || y0 < 0 || x1 > W || y1 > H) return LASR_E_BADARG;
    if (!(lo < hi)) return LASR_E_BADARG;                             // also refuses NaN
    if (x1 <= x0 || y1 <= y0) return LASR_OK;                         // empty window (an empty image has no other)
    if (!img || !P || !hist) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const int rows = y1 - y0;
    hipLaunchKernelGGL(lasr::maskprop_hist_kernel, dim3((unsigned)(rows < 256 ? rows : 256)), dim3(256), 0, st, img, P, hist, W, x0, y0,
                       x1, y1, hi, lo);
    return launch_ok();
}

extern "C" int lasr_maskprop_unary(const unsigned char* img_t, const float* P_s, const float* flow_ts, const float* flow_st,
                                   const unsigned* hist, float* app_table, float* u, float* q0, int H, int W, float tau, float w_p,
                                   float w_a, float eps, float U, void* hip_stream)
{
    if (!lasr::mp_image_ok(H, W)) return LASR_E_BADARG;
    if (!lasr::mp_pos(tau) || !lasr::mp_pos(eps) || !lasr::mp_pos(U)) return LASR_E_BADARG;
    if (!(w_p >= 0.f && w_p <= 3.0e38f && w_a >= 0.f && w_a <= 3.0e38f)) return LASR_E_BADARG;
    if (H == 0 || W == 0) return LASR_OK;
    if (!img_t || !P_s || !flow_ts || !flow_st || !hist || !app_table || !u || !q0) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(lasr::maskprop_table_kernel, dim3(1), dim3(256), 0, st, hist, app_table, eps);
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(lasr::maskprop_unary_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, img_t, P_s, flow_ts, flow_st,
                       (const float*)app_table, u, q0, H, W, 1.f / (2.f * tau * tau), w_p, w_a, U);
    return launch_ok();
}

extern "C" int lasr_maskprop_meanfield(const unsigned char* img, const float* u, const float* q_in, float* q_out, int H, int W, int R,
                                       float sigma_i, float sigma_s, float w_s, void* hip_stream)
{
    if (!lasr::mp_image_ok(H, W)) return LASR_E_BADARG;
    if (R < 0 || R > LASR_MASKPROP_MAX_RADIUS) return LASR_E_BADARG;
    if (!lasr::mp_pos(sigma_i) || !lasr::mp_pos(sigma_s) || !(w_s >= 0.f && w_s <= 3.0e38f)) return LASR_E_BADARG;
    if (H == 0 || W == 0) return LASR_OK;
    if (!img || !u || !q_in || !q_out || q_in == q_out) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t lds = (size_t)(lasr::MP_TX + 2 * R) * (lasr::MP_TY + 2 * R) * 8;
    hipLaunchKernelGGL(lasr::maskprop_meanfield_kernel, dim3((unsigned)((W + lasr::MP_TX - 1) / lasr::MP_TX),
                                                              (unsigned)((H + lasr::MP_TY - 1) / lasr::MP_TY)),
                       dim3(256), lds, st, img, u, q_in, q_out, H, W, R, 1.f / (2.f * sigma_i * sigma_i),
                       1.f / (2.f * sigma_s * sigma_s), w_s);
    return launch_ok();
}
