// isectpen.hip -- the intersection penalty of the optimiser (optimize.py --isect_wt; scripts/isect_penalty.py runs it): a loss on the
// posed meshes of a step that is zero exactly where scripts/eval_shape.py reports n_pairs = 0, the third line of the shape report
// beside the two foldpen.hip acts on.  This is the project's own addition; the definition is the one of include/lasr_ops.h,
// tests/isectpen_restated.py and DESIGN.md section 4.22.  The pairs are those of meshcheck.hip (faces that share no vertex, closed
// boxes overlap, the six strict directed tests), the value of a test that holds is foldpen.hip's depth of the shallower end
// (foldpen_geom.h: fp_directed, shared unchanged).
// The pair set depends on the geometry of the step, so there is no list and no inverted index: isectpen_pairs_kernel is the walk of
// meshcheck_pairs_kernel (one block per (mesh, tile I, tile J >= I) of 256 faces, box rejection, per-wave ballot compaction into a
// ring in LDS, the exact test on 64 queued pairs at a time) with two differences.  It stages both tiles straight from x and faces
// (the optimiser keeps no face records): nine coordinates, the box and the three indices, for tile I too, because the testing lane
// needs them for the gradient; a face with an index outside [0, V) or a repeated index gets the empty box and takes part in nothing.
// And a hit lane evaluates the tests that hold and adds their contributions in FIXED POINT, llrint(double(c) 2^40), with 64-bit
// integer atomics: the project uses no floating-point atomics, and integer sums commute, so the result has the same bits on every
// run and under any order of the faces.  A lane first sums the quanta of its pair per vertex (six vertices) in registers, then
// issues at most 18 atomics; the loss quanta and the two counts are summed per wave and cost one atomic each per wave.
// isectpen_zero_kernel zeroes what is accumulated into, isectpen_final_kernel turns the accumulators into fp32.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"
#include "foldpen_geom.h"
#include "sr_device.h"

namespace lasr {

constexpr int IP_QCAP = 128;                                   // per wave: below 64 queued before a push of at most 64
constexpr int IP_REC_I = 12;                                   // tile I in LDS: slots 0-8 a b c, 9-11 the indices
constexpr double IP_Q = 1099511627776.;                        // 2^40
constexpr float IP_LIMIT = 1048576.f;                          // 2^20: a contribution at or above it drops its test

typedef unsigned long long ip_u64;

__device__ __forceinline__ bool ip_small(float c) { return fabsf(c) < IP_LIMIT; }              // false for NaN and infinities
__device__ __forceinline__ bool ip_small(const McV& g) { return ip_small(g.x) && ip_small(g.y) && ip_small(g.z); }
__device__ __forceinline__ long long ip_quantum(float c) { return llrint((double)c * IP_Q); }

struct IpQ {                                                   // the quanta of one vertex
    long long x, y, z;
};
__device__ __forceinline__ void ip_acc(IpQ& s, const McV& g)
{
    s.x += ip_quantum(g.x);
    s.y += ip_quantum(g.y);
    s.z += ip_quantum(g.z);
}
__device__ __forceinline__ void ip_flush(ip_u64* __restrict__ row, const IpQ& s)
{
    if (s.x != 0) atomicAdd(row, (ip_u64)s.x);
    if (s.y != 0) atomicAdd(row + 1, (ip_u64)s.y);
    if (s.z != 0) atomicAdd(row + 2, (ip_u64)s.z);
}

__global__ __launch_bounds__(256) void isectpen_zero_kernel(ip_u64* __restrict__ acc, long long n_acc, ip_u64* __restrict__ n_pairs,
                                                            ip_u64* __restrict__ n_dropped, int N)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id < n_acc) acc[id] = 0ull;
    if (id < N) {
        n_pairs[id] = 0ull;
        n_dropped[id] = 0ull;
    }
}

// acc_grad NULL: no gradient is wanted, only acc_loss and the counts are touched
__global__ __launch_bounds__(256) void isectpen_pairs_kernel(const float* __restrict__ x, const int* __restrict__ faces,
                                                             ip_u64* __restrict__ acc_loss, ip_u64* __restrict__ acc_grad,
                                                             ip_u64* __restrict__ n_pairs, ip_u64* __restrict__ n_dropped, int V, int F,
                                                             int NT)
{
    __shared__ float sI[IP_REC_I][MC_TILE];                    // the exact test reads face i by its position
    __shared__ float sJ[MC_REC][MC_TILE];
    __shared__ unsigned short ring[4][IP_QCAP];
    const int t = blockIdx.y, tid = threadIdx.x;
    int I, J;
    mc_tile_pair((int)blockIdx.x, NT, I, J);
    const int cntI = min(MC_TILE, F - I * MC_TILE), cntJ = min(MC_TILE, F - J * MC_TILE);
    const float* xm = x + (size_t)t * V * 3;
    const bool live = tid < cntI, diag = I == J;
    // the record of face f: coordinates of 0, the empty box and the indices as they are for a face that is not gathered
    auto gather = [&](int f, float* c, float* lo, float* hi, int* v) {
        v[0] = faces[(size_t)f * 3];
        v[1] = faces[(size_t)f * 3 + 1];
        v[2] = faces[(size_t)f * 3 + 2];
        const unsigned uV = (unsigned)V;
        const bool ok = (unsigned)v[0] < uV && (unsigned)v[1] < uV && (unsigned)v[2] < uV && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
#pragma unroll
        for (int k = 0; k < 9; k++) c[k] = 0.f;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            lo[d] = INFINITY;
            hi[d] = -INFINITY;
        }
        if (ok) {
#pragma unroll
            for (int d = 0; d < 3; d++) {
                c[d] = xm[(size_t)v[0] * 3 + d];
                c[3 + d] = xm[(size_t)v[1] * 3 + d];
                c[6 + d] = xm[(size_t)v[2] * 3 + d];
                lo[d] = fminf(fminf(c[d], c[3 + d]), c[6 + d]);
                hi[d] = fmaxf(fmaxf(c[d], c[3 + d]), c[6 + d]);
            }
        }
    };
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    int v[3] = {0, 0, 0};
    if (live) {
        float c[9];
        gather(I * MC_TILE + tid, c, lo, hi, v);
#pragma unroll
        for (int k = 0; k < 9; k++) sI[k][tid] = c[k];
#pragma unroll
        for (int d = 0; d < 3; d++) sI[9 + d][tid] = __int_as_float(v[d]);
        if (diag) {
#pragma unroll
            for (int k = 0; k < 9; k++) sJ[k][tid] = c[k];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                sJ[9 + d][tid] = lo[d];
                sJ[12 + d][tid] = hi[d];
                sJ[15 + d][tid] = __int_as_float(v[d]);
            }
        }
    }
    if (!diag && tid < cntJ) {
        float c[9], l[3], h[3];
        int w[3];
        gather(J * MC_TILE + tid, c, l, h, w);
#pragma unroll
        for (int k = 0; k < 9; k++) sJ[k][tid] = c[k];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            sJ[9 + d][tid] = l[d];
            sJ[12 + d][tid] = h[d];
            sJ[15 + d][tid] = __int_as_float(w[d]);
        }
    }
    __syncthreads();

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v0 = v[0], v1 = v[1], v2 = v[2];
    unsigned short* q = ring[wave];
    int head = 0, tail = 0, found = 0;                         // wave-uniform
    long long loss_q = 0;                                      // per lane: the quanta of the depths it charged
    int n_drop = 0;                                            // per lane: the tests it dropped
    const bool want = acc_grad != nullptr;
    ip_u64* gm = want ? acc_grad + (size_t)t * V * 3 : nullptr;
    // The exact test on up to 64 queued pairs; a hit lane charges its pair.
    auto drain = [&]() {
        __builtin_amdgcn_wave_barrier();
        const int avail = tail - head;
        const bool active = lane < avail;
        const int packed = q[(head + lane) & (IP_QCAP - 1)];
        head += min(avail, 64);
        bool hit = false;
        const int il = packed >> 8, jl = packed & 255;
        if (active) {
            McV A[3], B[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                A[k] = {sI[3 * k][il], sI[3 * k + 1][il], sI[3 * k + 2][il]};
                B[k] = {sJ[3 * k][jl], sJ[3 * k + 1][jl], sJ[3 * k + 2][jl]};
            }
            float da[3], db[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                da[k] = mc_orient(B[0], B[1], B[2], A[k]);
                db[k] = mc_orient(A[0], A[1], A[2], B[k]);
            }
            bool holds[6];
#pragma unroll
            for (int e = 0; e < 3; e++) {
                const int n = e == 2 ? 0 : e + 1;
                holds[e] = mc_pierces(A[e], A[n], da[e], da[n], B[0], B[1], B[2]);
                holds[3 + e] = mc_pierces(B[e], B[n], db[e], db[n], A[0], A[1], A[2]);
                hit = hit || holds[e] || holds[3 + e];
            }
            if (hit) {
                const IpQ none = {0, 0, 0};
                IpQ sA[3] = {none, none, none}, sB[3] = {none, none, none};
                const McV zero = {0.f, 0.f, 0.f};
                // one directed test: edge (X[e], X[n]) against triangle Y; sX, sY the quanta of the vertices of either face
                auto charge = [&](const McV* X, const McV* Y, const float* dx, int e, IpQ* sX, IpQ* sY) {
                    const int n = e == 2 ? 0 : e + 1;
                    McV gp = zero, gq = zero, ga = zero, gb = zero, gc = zero;
                    const float depth = fp_directed(X[e], X[n], dx[e], dx[n], Y[0], Y[1], Y[2], true, gp, gq, ga, gb, gc);
                    const McV nn = fp_cross(fp_sub(Y[1], Y[0]), fp_sub(Y[2], Y[0]));
                    const float n2 = fp_dot(nn, nn);
                    // dropped as a whole, before anything of it is added: |n|^2 of 0 or not finite, a contribution not finite or >= 2^20
                    if (!(n2 > 0.f && n2 < INFINITY) || !ip_small(depth) || !ip_small(gp) || !ip_small(gq) || !ip_small(ga) || !ip_small(gb)
                        || !ip_small(gc)) {
                        n_drop++;
                        return;
                    }
                    loss_q += ip_quantum(depth);
                    if (want) {
                        ip_acc(sX[e], gp);                             // one of the two ends got the gradient, the other zeros
                        ip_acc(sX[n], gq);
                        ip_acc(sY[0], ga);
                        ip_acc(sY[1], gb);
                        ip_acc(sY[2], gc);
                    }
                };
#pragma unroll
                for (int e = 0; e < 3; e++)
                    if (holds[e]) charge(A, B, da, e, sA, sB);
#pragma unroll
                for (int e = 0; e < 3; e++)
                    if (holds[3 + e]) charge(B, A, db, e, sB, sA);
                if (want) {
#pragma unroll
                    for (int k = 0; k < 3; k++) {                      // every index was checked when the face was gathered: inside [0, V)
                        ip_flush(gm + (size_t)__float_as_int(sI[9 + k][il]) * 3, sA[k]);
                        ip_flush(gm + (size_t)__float_as_int(sJ[15 + k][jl]) * 3, sB[k]);
                    }
                }
            }
        }
        found += __popcll(wave_mask(hit));
    };
    // The broad phase of meshcheck_pairs_kernel: face j against the 64 faces of this wave.
    const int j0 = wave * 64 >= cntI ? cntJ : (diag ? wave * 64 + 1 : 0);
    for (int j = j0; j < cntJ; j++) {
        bool keep = live & (!diag | (j > tid)) & (lo[0] <= sJ[12][j]) & (sJ[9][j] <= hi[0]) & (lo[1] <= sJ[13][j]) & (sJ[10][j] <= hi[1])
                    & (lo[2] <= sJ[14][j]) & (sJ[11][j] <= hi[2]);
        if (wave_mask(keep) == 0) continue;                    // the same in every lane
        if (keep) {
            const int w0 = __float_as_int(sJ[15][j]), w1 = __float_as_int(sJ[16][j]), w2 = __float_as_int(sJ[17][j]);
            keep = v0 != w0 && v0 != w1 && v0 != w2 && v1 != w0 && v1 != w1 && v1 != w2 && v2 != w0 && v2 != w1 && v2 != w2;
        }
        const unsigned long long mask = wave_mask(keep);
        if (keep) q[(tail + bits_below_lane(mask)) & (IP_QCAP - 1)] = (unsigned short)((tid << 8) | j);
        tail += __popcll(mask);
        if (tail - head >= 64) drain();
    }
    if (tail - head > 0) drain();
    if (found > 0) {                                           // wave-uniform: the lanes' sums by shuffles, one atomic each per wave
        long long drops = n_drop;
        for (int o = 32; o > 0; o >>= 1) {
            loss_q += __shfl_down(loss_q, o, 64);
            drops += __shfl_down(drops, o, 64);
        }
        if (lane == 0) {
            atomicAdd(&n_pairs[t], (ip_u64)found);
            if (loss_q != 0) atomicAdd(&acc_loss[t], (ip_u64)loss_q);
            if (drops != 0) atomicAdd(&n_dropped[t], (ip_u64)drops);
        }
    }
}

// element id < N: loss; then, when a gradient is wanted, N V 3 elements of gunit
__global__ __launch_bounds__(256) void isectpen_final_kernel(const long long* __restrict__ acc_loss, const long long* __restrict__ acc_grad,
                                                             float* __restrict__ loss, float* __restrict__ gunit, int N, long long n_grad)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id < N) loss[id] = (float)((double)acc_loss[id] * (1. / IP_Q));
    else if (id - N < n_grad) gunit[id - N] = (float)((double)acc_grad[id - N] * (1. / IP_Q));
}

static inline bool ip_sizes_ok(int N, int V)
{
    return N >= 0 && N <= LASR_MESHCHECK_MAX_FRAMES && V >= 0 && (long long)N * V * 3 <= 0x7fffffffLL && (long long)V * 3 <= 0x7fffffffLL;
}

}  // namespace lasr

extern "C" size_t lasr_isectpen_scratch_bytes(int N, int V)
{
    if (!lasr::ip_sizes_ok(N, V)) return 0;
    return ((size_t)N + (size_t)N * V * 3) * sizeof(long long);
}

extern "C" int lasr_isectpen_forward(const float* x, const int* faces, void* scratch, size_t scratch_bytes, float* loss, float* gunit,
                                     unsigned long long* n_pairs, unsigned long long* n_dropped, int N, int V, int F, void* hip_stream)
{
    if (!lasr::ip_sizes_ok(N, V) || !lasr::mc_sizes_ok(N, F)) return LASR_E_BADARG;
    if (N == 0 || F == 0) return LASR_OK;
    if (V < 1 || !x || !faces || !scratch || !loss || !n_pairs || !n_dropped) return LASR_E_BADARG;
    const void* bufs[7] = {x, faces, scratch, loss, n_pairs, n_dropped, gunit};
    for (int a = 0; a < 7; a++)
        for (int b = a + 1; b < 7; b++)
            if (bufs[a] && bufs[a] == bufs[b]) return LASR_E_BADARG;
    if (scratch_bytes < lasr_isectpen_scratch_bytes(N, V)) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    lasr::ip_u64* acc_loss = (lasr::ip_u64*)scratch;
    lasr::ip_u64* acc_grad = gunit ? acc_loss + N : nullptr;
    const long long n_grad = gunit ? (long long)N * V * 3 : 0;
    const long long n_acc = N + n_grad;                             // below 2^31 + 2^16
    const unsigned blocks = (unsigned)((n_acc + 255) / 256);
    hipLaunchKernelGGL(lasr::isectpen_zero_kernel, dim3(blocks), dim3(256), 0, st, acc_loss, n_acc, n_pairs, n_dropped, N);
    const int NT = lasr::mc_blocks(F);
    const long long NTP = (long long)NT * (NT + 1) / 2;             // at most 2^23 + 2^11
    hipLaunchKernelGGL(lasr::isectpen_pairs_kernel, dim3((unsigned)NTP, (unsigned)N), dim3(256), 0, st, x, faces, acc_loss, acc_grad,
                       n_pairs, n_dropped, V, F, NT);
    hipLaunchKernelGGL(lasr::isectpen_final_kernel, dim3(blocks), dim3(256), 0, st, (const long long*)acc_loss,
                       (const long long*)acc_grad, loss, gunit, N, n_grad);
    return launch_ok();
}
