// meshcheck.hip -- shape scores of scripts/eval_shape.py (lasr_amd/nnutils/meshcheck.py runs the passes): which pairs of faces of a
// reconstructed mesh pass through each other, its signed volume and its area, per frame.  This is the project's own addition; the
// reference has no counterpart, and the definition is the one of include/lasr_ops.h, tests/meshcheck_restated.py and DESIGN.md
// section 4.18.
// meshcheck_faces_kernel: one thread per (frame, face): the face record (nine coordinates, the box, the three indices) as a
// structure of arrays, the fp64 volume and area terms folded per block in a fixed order; meshcheck_fold_kernel adds the block
// partials in index order.  meshcheck_pairs_kernel, the hot path: one block per (frame, tile I, tile J >= I) of 256 faces, both
// tiles in LDS; a thread keeps the box and the indices of one face of tile I and walks tile J, every lane of a wave reading the
// same j (a broadcast).  The box and shared-vertex tests leave a few pairs in a thousand, so the survivors are compacted per wave
// (ballot + prefix count) into a queue in LDS and the exact test runs on 64 queued pairs at a time, as the backward rasteriser
// queues its pixels (sr_backward.h).  Integer atomics only: the same input gives the same counts on every run.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"
#include "meshcheck_geom.h"
#include "sr_device.h"

namespace lasr {

constexpr int MC_QCAP = 128;                                   // per wave: below 64 queued before a push of at most 64

__device__ __forceinline__ bool mc_intersect(const McV* A, const McV* B)
{
    float da[3], db[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        da[k] = mc_orient(B[0], B[1], B[2], A[k]);
        db[k] = mc_orient(A[0], A[1], A[2], B[k]);
    }
    bool hit = false;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const int n = e == 2 ? 0 : e + 1;
        hit = hit || mc_pierces(A[e], A[n], da[e], da[n], B[0], B[1], B[2]);
        hit = hit || mc_pierces(B[e], B[n], db[e], db[n], A[0], A[1], A[2]);
    }
    return hit;
}

__global__ __launch_bounds__(256) void meshcheck_faces_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                              float* __restrict__ rec, double* __restrict__ partials, int V, int F,
                                                              int NB)
{
    __shared__ double red[4][2];
    const int t = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    double vol = 0., area = 0.;
    if (f < F) {
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        const bool ok = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
        float c[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};      // an empty box
        if (ok) {
            const float* v = verts + (size_t)t * V * 3;
#pragma unroll
            for (int d = 0; d < 3; d++) {
                c[d] = v[(size_t)i0 * 3 + d];
                c[3 + d] = v[(size_t)i1 * 3 + d];
                c[6 + d] = v[(size_t)i2 * 3 + d];
                lo[d] = fminf(fminf(c[d], c[3 + d]), c[6 + d]);
                hi[d] = fmaxf(fmaxf(c[d], c[3 + d]), c[6 + d]);
            }
            const double ax = c[0], ay = c[1], az = c[2], bx = c[3], by = c[4], bz = c[5], cx = c[6], cy = c[7], cz = c[8];
            vol = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
            const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
        }
        float* r = rec + (size_t)t * MC_REC * F + f;
#pragma unroll
        for (int k = 0; k < 9; k++) r[(size_t)k * F] = c[k];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            r[(size_t)(9 + d) * F] = lo[d];
            r[(size_t)(12 + d) * F] = hi[d];
        }
        r[(size_t)15 * F] = __int_as_float(i0);
        r[(size_t)16 * F] = __int_as_float(i1);
        r[(size_t)17 * F] = __int_as_float(i2);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        vol += __shfl_down(vol, o, 64);
        area += __shfl_down(area, o, 64);
    }
    if (lane == 0) {
        red[wave][0] = vol;
        red[wave][1] = area;
    }
    __syncthreads();
    if (threadIdx.x < 2)
        partials[((size_t)t * NB + blockIdx.x) * 2 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x])
                                                                    + red[3][threadIdx.x];
}

// thread 2 t + which: the block partials of frame t in index order
__global__ __launch_bounds__(64) void meshcheck_fold_kernel(const double* __restrict__ partials, double* __restrict__ volume,
                                                            double* __restrict__ area, int T, int NB)
{
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id >= 2 * T) return;
    const int t = id >> 1, which = id & 1;
    double s = 0.;
    for (int b = 0; b < NB; b++) s += partials[((size_t)t * NB + b) * 2 + which];
    if (which) area[t] = s;
    else volume[t] = s / 6.;
}

__global__ __launch_bounds__(256) void meshcheck_pairs_kernel(const float* __restrict__ rec, int* __restrict__ face_count,
                                                              unsigned long long* __restrict__ n_pairs, unsigned* __restrict__ cursor,
                                                              int* __restrict__ pairs, int F, int NT, int max_pairs)
{
    __shared__ float sI[9][MC_TILE];                           // the exact test reads face i by its position
    __shared__ float sJ[MC_REC][MC_TILE];
    __shared__ unsigned short ring[4][MC_QCAP];
    const int t = blockIdx.y, tid = threadIdx.x;
    int I, J;
    mc_tile_pair((int)blockIdx.x, NT, I, J);
    const int cntI = min(MC_TILE, F - I * MC_TILE), cntJ = min(MC_TILE, F - J * MC_TILE);
    const float* base = rec + (size_t)t * MC_REC * F;
    const bool live = tid < cntI;
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    int v0 = 0, v1 = 0, v2 = 0;
    if (live) {
        const float* r = base + I * MC_TILE + tid;
#pragma unroll
        for (int k = 0; k < 9; k++) sI[k][tid] = r[(size_t)k * F];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            lo[d] = r[(size_t)(9 + d) * F];
            hi[d] = r[(size_t)(12 + d) * F];
        }
        v0 = __float_as_int(r[(size_t)15 * F]);
        v1 = __float_as_int(r[(size_t)16 * F]);
        v2 = __float_as_int(r[(size_t)17 * F]);
    }
    if (tid < cntJ) {
        const float* r = base + J * MC_TILE + tid;
#pragma unroll
        for (int k = 0; k < MC_REC; k++) sJ[k][tid] = r[(size_t)k * F];
    }
    __syncthreads();

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool diag = I == J;
    unsigned short* q = ring[wave];
    int head = 0, tail = 0, found = 0;                         // wave-uniform
    // The exact test on up to 64 queued pairs.
    auto drain = [&]() {
        __builtin_amdgcn_wave_barrier();
        const int avail = tail - head;
        const bool active = lane < avail;
        const int packed = q[(head + lane) & (MC_QCAP - 1)];
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
            hit = mc_intersect(A, B);
        }
        if (hit) {
            const int gi = I * MC_TILE + il, gj = J * MC_TILE + jl;       // gi < gj < F
            atomicAdd(&face_count[(size_t)t * F + gi], 1);
            atomicAdd(&face_count[(size_t)t * F + gj], 1);
            if (max_pairs > 0) {
                const unsigned slot = atomicAdd(&cursor[t], 1u);
                if (slot < (unsigned)max_pairs) {
                    pairs[((size_t)t * max_pairs + slot) * 2] = gi;
                    pairs[((size_t)t * max_pairs + slot) * 2 + 1] = gj;
                }
            }
        }
        found += __popcll(wave_mask(hit));
    };
    // The broad phase: face j against the 64 faces of this wave.  The box test is predicated (`&`, no branch per comparison); only
    // a wave with a surviving lane goes on to the indices and the queue.  In the diagonal tile only j > i
    // counts, and this wave's i start at 64 wave; a wave without a face of tile I walks nothing.
    const int j0 = wave * 64 >= cntI ? cntJ : (diag ? wave * 64 + 1 : 0);
#pragma unroll 4
    for (int j = j0; j < cntJ; j++) {
        bool keep = live & (!diag | (j > tid)) & (lo[0] <= sJ[12][j]) & (sJ[9][j] <= hi[0]) & (lo[1] <= sJ[13][j]) & (sJ[10][j] <= hi[1])
                    & (lo[2] <= sJ[14][j]) & (sJ[11][j] <= hi[2]);
        if (wave_mask(keep) == 0) continue;                    // the same in every lane
        if (keep) {
            const int w0 = __float_as_int(sJ[15][j]), w1 = __float_as_int(sJ[16][j]), w2 = __float_as_int(sJ[17][j]);
            keep = v0 != w0 && v0 != w1 && v0 != w2 && v1 != w0 && v1 != w1 && v1 != w2 && v2 != w0 && v2 != w1 && v2 != w2;
        }
        const unsigned long long mask = wave_mask(keep);
        if (keep) q[(tail + bits_below_lane(mask)) & (MC_QCAP - 1)] = (unsigned short)((tid << 8) | j);
        tail += __popcll(mask);
        if (tail - head >= 64) drain();
    }
    if (tail - head > 0) drain();
    if (lane == 0 && found > 0) atomicAdd(&n_pairs[t], (unsigned long long)found);
}

}  // namespace lasr

extern "C" size_t lasr_meshcheck_workspace_bytes(int T, int F)
{
    if (!lasr::mc_sizes_ok(T, F)) return 0;
    return (size_t)T * F * lasr::MC_REC * sizeof(float) + (size_t)T * lasr::mc_blocks(F) * 2 * sizeof(double);
}

extern "C" int lasr_meshcheck_faces(const float* verts, const int* faces, void* workspace, size_t workspace_bytes, double* volume,
                                    double* area, int T, int V, int F, void* hip_stream)
{
    if (!lasr::mc_sizes_ok(T, F) || V < 0 || (long long)V * 3 > 0x7fffffffLL) return LASR_E_BADARG;
    if (T == 0 || F == 0) return LASR_OK;
    if (V < 1 || !verts || !faces || !workspace || !volume || !area) return LASR_E_BADARG;
    const void* ins[2] = {verts, faces};
    const void* outs[3] = {workspace, volume, area};
    for (int a = 0; a < 3; a++) {
        for (int b = a + 1; b < 3; b++)
            if (outs[a] == outs[b]) return LASR_E_BADARG;
        for (int b = 0; b < 2; b++)
            if (outs[a] == ins[b]) return LASR_E_BADARG;
    }
    if (workspace_bytes < lasr_meshcheck_workspace_bytes(T, F)) return LASR_E_WORKSPACE;
    const int NB = lasr::mc_blocks(F);
    float* rec = (float*)workspace;
    double* partials = (double*)(rec + (size_t)T * F * lasr::MC_REC);
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(lasr::meshcheck_faces_kernel, dim3((unsigned)NB, (unsigned)T), dim3(256), 0, st, verts, faces, rec, partials, V,
                       F, NB);
    hipLaunchKernelGGL(lasr::meshcheck_fold_kernel, dim3((unsigned)((2 * T + 63) / 64)), dim3(64), 0, st, partials, volume, area, T, NB);
    return launch_ok();
}

extern "C" int lasr_meshcheck_pairs(const void* workspace, size_t workspace_bytes, int* face_count, unsigned long long* n_pairs,
                                    unsigned* cursor, int* pairs, int T, int F, int max_pairs, void* hip_stream)
{
    if (!lasr::mc_sizes_ok(T, F) || max_pairs < 0 || (long long)T * max_pairs * 2 > 0x7fffffffLL) return LASR_E_BADARG;
    if (T == 0 || F == 0) return LASR_OK;
    if (!workspace || !face_count || !n_pairs || !cursor || (max_pairs > 0 && !pairs)) return LASR_E_BADARG;
    const void* bufs[5] = {workspace, face_count, n_pairs, cursor, pairs};
    for (int a = 0; a < 5; a++)
        for (int b = a + 1; b < 5; b++)
            if (bufs[a] && bufs[a] == bufs[b]) return LASR_E_BADARG;
    if (workspace_bytes < lasr_meshcheck_workspace_bytes(T, F)) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    if (hipMemsetAsync(face_count, 0, (size_t)T * F * sizeof(int), st) != hipSuccess) return launch_ok();
    if (hipMemsetAsync(n_pairs, 0, (size_t)T * sizeof(unsigned long long), st) != hipSuccess) return launch_ok();
    if (hipMemsetAsync(cursor, 0, (size_t)T * sizeof(unsigned), st) != hipSuccess) return launch_ok();
    const int NT = lasr::mc_blocks(F);
    const long long NTP = (long long)NT * (NT + 1) / 2;             // at most 2^23 + 2^11
    hipLaunchKernelGGL(lasr::meshcheck_pairs_kernel, dim3((unsigned)NTP, (unsigned)T), dim3(256), 0, st, (const float*)workspace,
                       face_count, n_pairs, cursor, pairs, F, NT, max_pairs);
    return launch_ok();
}
