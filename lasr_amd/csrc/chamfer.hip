// chamfer.hip -- nearest neighbours between point sets of evaluation size (10 000 x 10 000), the two-directional Chamfer
// distance with its backward (third_party/chamfer3D/chamfer3D.cu of the reference) and the rigid ICP of scripts/eval_mesh.py:156
// (pytorch3d.ops.iterative_closest_point, restated) with its whole state on the device.
//
// nn_tiled_kernel: one query per thread, 256 queries per block; the target set passes through LDS in tiles of LASR_NN_TILE points
// stored as float4, and every lane reads the same LDS address (a broadcast, no bank conflict).  blockIdx.y owns a run of whole
// tiles of the target set ("split"), so that 10 000 queries fill the chip with 40 x splits blocks instead of 40.  With one split
// the block writes d2 / idx itself; with several, each block folds its minimum into a 64-bit key per query by a vector atomicMin:
// distance bits in the high word (non-negative floats order like their bit patterns), index in the low word, so the smallest key is
// the smallest distance and, among equal distances, the lowest index, in whatever order the blocks arrive.  The distance is the
// expression of nearest_point_kernel (fused.hip) under the same -ffp-contract=off: without a transform the results are its bits.
//
// ICP, three launches per iteration, none of which waits for the host: nn_tiled_kernel (queries X R + T formed as they are
// loaded), icp_moments_kernel (keys -> correspondences, keys re-armed, per-block double sums of x, y and x y^T),
// icp_solve_kernel (one block: partials summed in block order, Kabsch by a one-sided Jacobi SVD in double, the RMSE of the new
// transform over the old correspondences, the stop test).  Every kernel reads the stop flag first and leaves once it is set.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"

namespace lasr {

constexpr int NN_TILE = LASR_NN_TILE;
constexpr int NN_NO_ARG = 0x7fffffff;                          // "nothing found": unpacks to index 0, as nearest_point_kernel's does
constexpr unsigned long long NN_KEY_EMPTY = ~0ull;
constexpr int ICP_MOMENTS = 15;                                // sum x (3), sum y (3), sum x_i y_j (9)
constexpr int ICP_SOLVE_THREADS = 512;

__device__ __forceinline__ unsigned long long nn_key(float d, int arg)
{
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)arg;
}

template <bool TRANSFORM, bool KEYS>
__global__ __launch_bounds__(256) void nn_tiled_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ R, const float* __restrict__ T,
                                                       float* __restrict__ d2, int* __restrict__ idx,
                                                       unsigned long long* __restrict__ keys, const int* __restrict__ stop, int P, int Q,
                                                       int tiles_per_split)
{
    if (stop && *stop) return;
    __shared__ float4 tile[NN_TILE];
    const int n = blockIdx.z, p = blockIdx.x * 256 + threadIdx.x;
    const int q_begin = blockIdx.y * tiles_per_split * NN_TILE;
    const int q_end = min(Q, q_begin + tiles_per_split * NN_TILE);
    if (q_begin >= q_end) return;                              // a split past the end of the set (forced `splits` > tiles)
    const bool live = p < P;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { const float* s = a + ((size_t)n * P + p) * 3; x = s[0]; y = s[1]; z = s[2]; }
    if (TRANSFORM) {                                           // row vector: a R + T
        const float* r = R + (size_t)n * 9;
        const float* t = T + (size_t)n * 3;
        const float tx = x * r[0] + y * r[3] + z * r[6] + t[0];
        const float ty = x * r[1] + y * r[4] + z * r[7] + t[1];
        const float tz = x * r[2] + y * r[5] + z * r[8] + t[2];
        x = tx; y = ty; z = tz;
    }
    const float* __restrict__ bn = b + (size_t)n * Q * 3;
    float best = INFINITY; int arg = NN_NO_ARG;
    for (int q0 = q_begin; q0 < q_end; q0 += NN_TILE) {
        const int cnt = min(NN_TILE, q_end - q0);
        __syncthreads();                                       // the previous tile has been read by every wave
        for (int j = threadIdx.x; j < cnt; j += 256) {
            const float* s = bn + (size_t)(q0 + j) * 3;
            tile[j] = make_float4(s[0], s[1], s[2], 0.f);
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < cnt; j++) {                        // ascending index and a strict `<`: the first minimum stays
            const float4 c = tile[j];
            const float dx = x - c.x, dy = y - c.y, dz = z - c.z;
            const float d = dx * dx + dy * dy + dz * dz;
            if (d < best) { best = d; arg = q0 + j; }
        }
    }
    if (!live) return;
    const size_t o = (size_t)n * P + p;
    if (KEYS) {
        atomicMin(keys + o, nn_key(best, arg));
    } else {
        d2[o] = best;
        idx[o] = arg == NN_NO_ARG ? 0 : arg;
    }
}

__global__ __launch_bounds__(256) void nn_fill_keys_kernel(unsigned long long* __restrict__ keys, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) keys[i] = NN_KEY_EMPTY;
}

__global__ __launch_bounds__(256) void nn_unpack_kernel(const unsigned long long* __restrict__ keys, float* __restrict__ d2,
                                                        int* __restrict__ idx, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const unsigned long long k = keys[i];
    const int arg = (int)(unsigned)(k & 0xffffffffull);
    d2[i] = k == NN_KEY_EMPTY ? INFINITY : __uint_as_float((unsigned)(k >> 32));
    idx[i] = (k == NN_KEY_EMPTY || arg == NN_NO_ARG) ? 0 : arg;
}

// Chamfer backward with the indices fixed (chamfer3D.cu:136-180 scatters with float atomics; here every point gathers its own
// terms in a fixed order).  One thread per point of `x`: the term of its own nearest neighbour in `y`, then the terms of the y
// points that chose it, listed by (row_ptr, col) in ascending order of their index.
__global__ __launch_bounds__(256) void chamfer_backward_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const int* __restrict__ idx_x, const float* __restrict__ g_x,
                                                               const float* __restrict__ g_y, const int* __restrict__ row_ptr,
                                                               const int* __restrict__ col, float* __restrict__ grad_x, int P, int Q)
{
    const int n = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t o = (size_t)n * P + i;
    const float* __restrict__ yn = y + (size_t)n * Q * 3;
    const float px = x[3 * o], py = x[3 * o + 1], pz = x[3 * o + 2];
    double ax = 0., ay = 0., az = 0.;
    const int j0 = idx_x[o];
    if ((unsigned)j0 < (unsigned)Q) {
        const float g = 2.f * g_x[o];
        ax = (double)(g * (px - yn[3 * j0])); ay = (double)(g * (py - yn[3 * j0 + 1])); az = (double)(g * (pz - yn[3 * j0 + 2]));
    }
    const int* __restrict__ rp = row_ptr + (size_t)n * (P + 1);
    const int k0 = max(rp[i], 0), k1 = min(rp[i + 1], Q);
    for (int k = k0; k < k1; k++) {
        const int j = col[(size_t)n * Q + k];
        if ((unsigned)j >= (unsigned)Q) continue;
        const float g = 2.f * g_y[(size_t)n * Q + j];
        ax += (double)(g * (px - yn[3 * j])); ay += (double)(g * (py - yn[3 * j + 1])); az += (double)(g * (pz - yn[3 * j + 2]));
    }
    grad_x[3 * o] = (float)ax; grad_x[3 * o + 1] = (float)ay; grad_x[3 * o + 2] = (float)az;
}

// ---- ICP ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void icp_init_kernel(float* __restrict__ R, float* __restrict__ T, double* __restrict__ rmse,
                                                       int* __restrict__ status, unsigned long long* __restrict__ keys, int N,
                                                       long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) keys[i] = NN_KEY_EMPTY;
    if (i < N) {
        for (int k = 0; k < 9; k++) R[i * 9 + k] = (k % 4 == 0) ? 1.f : 0.f;
        for (int k = 0; k < 3; k++) T[i * 3 + k] = 0.f;
        rmse[i * 2] = 0.; rmse[i * 2 + 1] = 0.;
    }
    if (i == 0) { status[0] = 0; status[1] = 0; }
}

__device__ __forceinline__ double wave_sum_double(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void icp_moments_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                          unsigned long long* __restrict__ keys, int* __restrict__ idx,
                                                          double* __restrict__ partial, const int* __restrict__ status, int P, int Q)
{
    if (status[0]) return;
    __shared__ double red[4][ICP_MOMENTS];
    const int n = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    double m[ICP_MOMENTS];
#pragma unroll
    for (int k = 0; k < ICP_MOMENTS; k++) m[k] = 0.;
    if (p < P) {
        const size_t o = (size_t)n * P + p;
        const unsigned long long key = keys[o];
        keys[o] = NN_KEY_EMPTY;                                // armed for the next iteration's atomicMin
        int j = (int)(unsigned)(key & 0xffffffffull);
        if ((unsigned)j >= (unsigned)Q) j = 0;                 // nothing found (NaN row): index 0, as the search reports it
        idx[o] = j;
        const float* xs = X + o * 3;
        const float* ys = Y + ((size_t)n * Q + j) * 3;
        const double x[3] = {(double)xs[0], (double)xs[1], (double)xs[2]}, y[3] = {(double)ys[0], (double)ys[1], (double)ys[2]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            m[k] = x[k]; m[3 + k] = y[k];
#pragma unroll
            for (int l = 0; l < 3; l++) m[6 + 3 * k + l] = x[k] * y[l];
        }
    }
#pragma unroll
    for (int k = 0; k < ICP_MOMENTS; k++) {
        const double s = wave_sum_double(m[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < ICP_MOMENTS) {
        const int k = threadIdx.x;
        partial[((size_t)n * gridDim.x + blockIdx.x) * ICP_MOMENTS + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

struct SvdCol { double b[3], v[3], s; };                       // a column of A V, the matching column of V, its squared length

__host__ __device__ inline bool svd_rotate(SvdCol& p, SvdCol& q)
{
    const double alpha = p.b[0] * p.b[0] + p.b[1] * p.b[1] + p.b[2] * p.b[2];
    const double beta = q.b[0] * q.b[0] + q.b[1] * q.b[1] + q.b[2] * q.b[2];
    const double gamma = p.b[0] * q.b[0] + p.b[1] * q.b[1] + p.b[2] * q.b[2];
    if (!(gamma * gamma > 1e-30 * alpha * beta)) return false;  // orthogonal to 1e-15 already (or a zero / NaN column)
    const double zeta = (beta - alpha) / (2. * gamma);
    const double t = copysign(1., zeta) / (fabs(zeta) + sqrt(1. + zeta * zeta));
    const double c = 1. / sqrt(1. + t * t), s = c * t;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double bp = p.b[k], vp = p.v[k];
        p.b[k] = c * bp - s * q.b[k]; q.b[k] = s * bp + c * q.b[k];
        p.v[k] = c * vp - s * q.v[k]; q.v[k] = s * vp + c * q.v[k];
    }
    return true;
}

__host__ __device__ inline void svd_order(SvdCol& p, SvdCol& q)     // the longer column first
{
    if (q.s > p.s) { const SvdCol t = p; p = q; q = t; }
}

// Kabsch from the fifteen sums over P pairs (x, y): R = U diag(1, 1, det(U V^T)) V^T of the SVD of the centred covariance
// x^T y / P with descending singular values, T = mean(y) - mean(x) R.  A V = U S by one-sided Jacobi rotations of the columns of A
// (Hestenes); with the smallest singular value last, U diag(1, 1, det(U V^T)) V^T = u1 v1^T + u2 v2^T + det(V) (u1 x u2) v3^T
// whichever sign u3 carries, so the third column of U, ill-defined for a flat cloud, is never formed.  Rounded to fp32 on return.
__host__ __device__ inline void icp_kabsch(const double* m, double count, float* R, float* T)
{
    const double inv = 1. / count;
    double mx[3], my[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { mx[k] = m[k] * inv; my[k] = m[3 + k] * inv; }
    SvdCol c0, c1, c2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c0.b[k] = m[6 + 3 * k] * inv - mx[k] * my[0]; c1.b[k] = m[6 + 3 * k + 1] * inv - mx[k] * my[1];
        c2.b[k] = m[6 + 3 * k + 2] * inv - mx[k] * my[2];
        c0.v[k] = k == 0 ? 1. : 0.; c1.v[k] = k == 1 ? 1. : 0.; c2.v[k] = k == 2 ? 1. : 0.;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        const bool r01 = svd_rotate(c0, c1), r02 = svd_rotate(c0, c2), r12 = svd_rotate(c1, c2);
        if (!(r01 || r02 || r12)) break;
    }
    c0.s = c0.b[0] * c0.b[0] + c0.b[1] * c0.b[1] + c0.b[2] * c0.b[2];
    c1.s = c1.b[0] * c1.b[0] + c1.b[1] * c1.b[1] + c1.b[2] * c1.b[2];
    c2.s = c2.b[0] * c2.b[0] + c2.b[1] * c2.b[1] + c2.b[2] * c2.b[2];
    svd_order(c0, c1); svd_order(c1, c2); svd_order(c0, c1);
    const double n0 = sqrt(c0.s), n1 = sqrt(c1.s);
    double u0[3], u1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { u0[k] = c0.b[k] / n0; u1[k] = c1.b[k] / n1; }
    const double w[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
    const double det_v = c0.v[0] * (c1.v[1] * c2.v[2] - c1.v[2] * c2.v[1]) - c1.v[0] * (c0.v[1] * c2.v[2] - c0.v[2] * c2.v[1]) +
                         c2.v[0] * (c0.v[1] * c1.v[2] - c0.v[2] * c1.v[1]);
    const double sgn = det_v < 0. ? -1. : 1.;
    double Rd[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rd[3 * i + j] = u0[i] * c0.v[j] + u1[i] * c1.v[j] + sgn * w[i] * c2.v[j];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = (float)Rd[k];
#pragma unroll
    for (int j = 0; j < 3; j++) T[j] = (float)(my[j] - (mx[0] * Rd[j] + mx[1] * Rd[3 + j] + mx[2] * Rd[6 + j]));
}

// One block for the whole batch: per element the partial sums in block order, the alignment (thread 0), then the RMSE of the new
// transform over the correspondences the search found with the old one; the batch stops when every element's relative decrease
// is at most thr.  status = {stop flag, iterations done}; rmse [N,2] = {this iteration's, the previous one's}.
__global__ __launch_bounds__(ICP_SOLVE_THREADS) void icp_solve_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                      const int* __restrict__ idx, const double* __restrict__ partial,
                                                                      float* __restrict__ R, float* __restrict__ T,
                                                                      double* __restrict__ rmse, int* __restrict__ status, int N, int P,
                                                                      int Q, int NB, double thr)
{
    if (status[0]) return;
    __shared__ double mom[ICP_MOMENTS];
    __shared__ float rt[12];
    __shared__ double red[ICP_SOLVE_THREADS / 64];
    __shared__ int all_converged;
    const int tid = threadIdx.x;
    if (tid == 0) all_converged = 1;
    for (int n = 0; n < N; n++) {
        __syncthreads();
        if (tid < ICP_MOMENTS) {
            double s = 0.;
            for (int k = 0; k < NB; k++) s += partial[((size_t)n * NB + k) * ICP_MOMENTS + tid];
            mom[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            float r[9], t[3];
            icp_kabsch(mom, (double)P, r, t);
#pragma unroll
            for (int k = 0; k < 9; k++) { rt[k] = r[k]; R[(size_t)n * 9 + k] = r[k]; }
#pragma unroll
            for (int k = 0; k < 3; k++) { rt[9 + k] = t[k]; T[(size_t)n * 3 + k] = t[k]; }
        }
        __syncthreads();
        double r[12];
#pragma unroll
        for (int k = 0; k < 12; k++) r[k] = (double)rt[k];
        double acc = 0.;
        for (int p = tid; p < P; p += ICP_SOLVE_THREADS) {
            const size_t o = (size_t)n * P + p;
            const int j = idx[o];                              // written by icp_moments_kernel: always inside [0, Q)
            const float* xs = X + o * 3;
            const float* ys = Y + ((size_t)n * Q + j) * 3;
            const double x = xs[0], y = xs[1], z = xs[2];
            const double ex = x * r[0] + y * r[3] + z * r[6] + r[9] - (double)ys[0];
            const double ey = x * r[1] + y * r[4] + z * r[7] + r[10] - (double)ys[1];
            const double ez = x * r[2] + y * r[5] + z * r[8] + r[11] - (double)ys[2];
            acc += ex * ex + ey * ey + ez * ez;
        }
        acc = wave_sum_double(acc);
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            double s = 0.;
#pragma unroll
            for (int k = 0; k < ICP_SOLVE_THREADS / 64; k++) s += red[k];
            const double now = sqrt(s / (double)P), prev = rmse[(size_t)n * 2];
            const double relative = status[1] == 0 ? 1. : (prev - now) / prev;
            rmse[(size_t)n * 2] = now; rmse[(size_t)n * 2 + 1] = prev;
            if (!(relative <= thr)) all_converged = 0;
        }
    }
    __syncthreads();
    if (tid == 0) {
        status[1] += 1;
        if (all_converged) status[0] = 1;
    }
}

}  // namespace lasr

// ---- host side ------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int NN_MAX_POINTS = 1 << 27;                         // 3 * points and points + a split's tiles stay inside int
constexpr int NN_MAX_BATCH = 65535, NN_MAX_SPLITS = 65535;
constexpr int NN_TARGET_BLOCKS = 1024;                         // four blocks of 256 threads per compute unit

size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

bool nn_sizes_ok(int N, int P, int Q) { return N >= 0 && N <= NN_MAX_BATCH && P >= 0 && P <= NN_MAX_POINTS && Q >= 1 && Q <= NN_MAX_POINTS; }

int nn_choose_splits(int N, int P, int Q, int splits)
{
    const int tiles = (Q + LASR_NN_TILE - 1) / LASR_NN_TILE;
    if (splits > 0) return splits;
    const long long blocks = (long long)((P + 255) / 256) * N;
    const long long want = (NN_TARGET_BLOCKS + blocks - 1) / blocks;
    return (int)(want < 1 ? 1 : want > tiles ? tiles : want);
}

// a [N,P,3] against b [N,Q,3]; keys_only: leave the result in `keys` (armed by the caller) for icp_moments_kernel
int nn_launch(const float* a, const float* b, const float* R, const float* T, float* d2, int* idx, unsigned long long* keys,
              const int* stop, bool keys_only, int N, int P, int Q, int splits, hipStream_t st)
{
    const int tiles = (Q + LASR_NN_TILE - 1) / LASR_NN_TILE;
    const int tiles_per_split = (tiles + splits - 1) / splits;
    const dim3 grid((unsigned)((P + 255) / 256), (unsigned)splits, (unsigned)N);
    const long long total = (long long)N * P;
    const unsigned fill_blocks = (unsigned)((total + 255) / 256);
    const bool use_keys = keys_only || splits > 1;
    if (use_keys && !keys_only) LASR_LAUNCH(K_NN_FILL_KEYS, lasr::nn_fill_keys_kernel, dim3(fill_blocks), dim3(256), 0, keys, total);
    if (use_keys) {
        if (R)
            LASR_LAUNCH(K_NN_TILED, (lasr::nn_tiled_kernel<true, true>), grid, dim3(256), 0, a, b, R, T, d2, idx, keys, stop, P, Q,
                        tiles_per_split);
        else
            LASR_LAUNCH(K_NN_TILED, (lasr::nn_tiled_kernel<false, true>), grid, dim3(256), 0, a, b, R, T, d2, idx, keys, stop, P, Q,
                        tiles_per_split);
    } else {
        if (R)
            LASR_LAUNCH(K_NN_TILED, (lasr::nn_tiled_kernel<true, false>), grid, dim3(256), 0, a, b, R, T, d2, idx, keys, stop, P, Q,
                        tiles_per_split);
        else
            LASR_LAUNCH(K_NN_TILED, (lasr::nn_tiled_kernel<false, false>), grid, dim3(256), 0, a, b, R, T, d2, idx, keys, stop, P, Q,
                        tiles_per_split);
    }
    if (use_keys && !keys_only) LASR_LAUNCH(K_NN_UNPACK, lasr::nn_unpack_kernel, dim3(fill_blocks), dim3(256), 0, keys, d2, idx, total);
    return launch_ok();
}

struct IcpLayout { size_t keys, idx, partial, total; int NB; };

IcpLayout icp_layout(int N, int P)
{
    IcpLayout l;
    l.NB = (P + 255) / 256;
    l.keys = 0;
    l.idx = l.keys + round256((size_t)N * P * 8);
    l.partial = l.idx + round256((size_t)N * P * 4);
    l.total = l.partial + round256((size_t)N * l.NB * lasr::ICP_MOMENTS * 8);
    return l;
}

}  // namespace

extern "C" size_t lasr_chamfer3d_workspace_bytes(int N, int P, int Q)
{
    if (N < 0 || P < 0 || Q < 0 || N > NN_MAX_BATCH || P > NN_MAX_POINTS || Q > NN_MAX_POINTS) return 0;
    return round256((size_t)N * P * 8) + round256((size_t)N * Q * 8);
}

extern "C" int lasr_nn_tiled(const float* a, const float* b, const float* R, const float* T, float* d2, int* idx, void* workspace,
                             size_t workspace_bytes, int N, int P, int Q, int splits, void* hip_stream)
{
    if (!nn_sizes_ok(N, P, Q) || splits < 0 || splits > NN_MAX_SPLITS || (R == nullptr) != (T == nullptr)) return LASR_E_BADARG;
    if (N == 0 || P == 0) return LASR_OK;
    if (!a || !b || !d2 || !idx) return LASR_E_BADARG;
    splits = nn_choose_splits(N, P, Q, splits);
    if (splits > 1) {
        if (!workspace) return LASR_E_BADARG;
        if (workspace_bytes < lasr_chamfer3d_workspace_bytes(N, P, 0)) return LASR_E_WORKSPACE;
    }
    return nn_launch(a, b, R, T, d2, idx, (unsigned long long*)workspace, nullptr, false, N, P, Q, splits, (hipStream_t)hip_stream);
}

extern "C" int lasr_chamfer3d_forward(const float* xyz1, const float* xyz2, float* dist1, float* dist2, int* idx1, int* idx2,
                                      void* workspace, size_t workspace_bytes, int N, int P, int Q, int splits, void* hip_stream)
{
    if (!nn_sizes_ok(N, P, Q) || P < 1 || splits < 0 || splits > NN_MAX_SPLITS) return LASR_E_BADARG;
    if (N == 0) return LASR_OK;
    if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2 || !workspace) return LASR_E_BADARG;
    if (workspace_bytes < lasr_chamfer3d_workspace_bytes(N, P, Q)) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    unsigned long long* k1 = (unsigned long long*)workspace;
    unsigned long long* k2 = (unsigned long long*)((char*)workspace + round256((size_t)N * P * 8));
    const int rc = nn_launch(xyz1, xyz2, nullptr, nullptr, dist1, idx1, k1, nullptr, false, N, P, Q, nn_choose_splits(N, P, Q, splits), st);
    if (rc != LASR_OK) return rc;
    return nn_launch(xyz2, xyz1, nullptr, nullptr, dist2, idx2, k2, nullptr, false, N, Q, P, nn_choose_splits(N, Q, P, splits), st);
}

extern "C" int lasr_chamfer3d_backward(const float* xyz1, const float* xyz2, const int* idx1, const int* idx2, const float* grad_dist1,
                                       const float* grad_dist2, const int* row_ptr1, const int* col1, const int* row_ptr2,
                                       const int* col2, float* grad_xyz1, float* grad_xyz2, int N, int P, int Q, void* hip_stream)
{
    if (!nn_sizes_ok(N, P, Q) || P < 1) return LASR_E_BADARG;
    if (N == 0) return LASR_OK;
    if (!xyz1 || !xyz2 || !idx1 || !idx2 || !grad_dist1 || !grad_dist2 || !row_ptr1 || !col1 || !row_ptr2 || !col2 || !grad_xyz1 ||
        !grad_xyz2)
        return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    LASR_LAUNCH(K_CHAMFER_BACKWARD, lasr::chamfer_backward_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)N), dim3(256), 0, xyz1, xyz2,
                idx1, grad_dist1, grad_dist2, row_ptr1, col1, grad_xyz1, P, Q);
    LASR_LAUNCH(K_CHAMFER_BACKWARD, lasr::chamfer_backward_kernel, dim3((unsigned)((Q + 255) / 256), (unsigned)N), dim3(256), 0, xyz2, xyz1,
                idx2, grad_dist2, grad_dist1, row_ptr2, col2, grad_xyz2, Q, P);
    return launch_ok();
}

extern "C" size_t lasr_icp_workspace_bytes(int N, int P, int Q)
{
    if (N < 1 || N > LASR_ICP_MAX_BATCH || P < 1 || P > NN_MAX_POINTS || Q < 1 || Q > NN_MAX_POINTS) return 0;
    return icp_layout(N, P).total;
}

extern "C" int lasr_icp_init(float* R, float* T, double* rmse, int* status, void* workspace, size_t workspace_bytes, int N, int P, int Q,
                             void* hip_stream)
{
    if (N < 1 || N > LASR_ICP_MAX_BATCH || P < 1 || P > NN_MAX_POINTS || Q < 1 || Q > NN_MAX_POINTS) return LASR_E_BADARG;
    if (!R || !T || !rmse || !status || !workspace) return LASR_E_BADARG;
    const IcpLayout l = icp_layout(N, P);
    if (workspace_bytes < l.total) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    const long long total = (long long)N * P;
    LASR_LAUNCH(K_ICP_INIT, lasr::icp_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, R, T, rmse, status,
                (unsigned long long*)((char*)workspace + l.keys), N, total);
    return launch_ok();
}

extern "C" int lasr_icp_iterate(const float* X, const float* Y, float* R, float* T, double* rmse, int* status, void* workspace,
                                size_t workspace_bytes, int N, int P, int Q, int n_iters, double relative_rmse_thr, int splits,
                                void* hip_stream)
{
    if (N < 1 || N > LASR_ICP_MAX_BATCH || P < 1 || P > NN_MAX_POINTS || Q < 1 || Q > NN_MAX_POINTS) return LASR_E_BADARG;
    if (n_iters < 0 || n_iters > LASR_ICP_MAX_CHUNK || splits < 0 || splits > NN_MAX_SPLITS) return LASR_E_BADARG;
    if (!X || !Y || !R || !T || !rmse || !status || !workspace) return LASR_E_BADARG;
    const IcpLayout l = icp_layout(N, P);
    if (workspace_bytes < l.total) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + l.keys);
    int* idx = (int*)((char*)workspace + l.idx);
    double* partial = (double*)((char*)workspace + l.partial);
    splits = nn_choose_splits(N, P, Q, splits);
    for (int it = 0; it < n_iters; it++) {
        const int rc = nn_launch(X, Y, R, T, nullptr, nullptr, keys, status, true, N, P, Q, splits, st);
        if (rc != LASR_OK) return rc;
        LASR_LAUNCH(K_ICP_MOMENTS, lasr::icp_moments_kernel, dim3((unsigned)l.NB, (unsigned)N), dim3(256), 0, X, Y, keys, idx, partial,
                    status, P, Q);
        LASR_LAUNCH(K_ICP_SOLVE, lasr::icp_solve_kernel, dim3(1), dim3(lasr::ICP_SOLVE_THREADS), 0, X, Y, idx, partial, R, T, rmse, status,
                    N, P, Q, l.NB, relative_rmse_thr);
    }
    return launch_ok();
}

extern "C" int lasr_icp_kabsch_host(const double* moments, int P, float* R, float* T)
{
    if (!moments || !R || !T || P < 1) return LASR_E_BADARG;
    lasr::icp_kabsch(moments, (double)P, R, T);
    return LASR_OK;
}
