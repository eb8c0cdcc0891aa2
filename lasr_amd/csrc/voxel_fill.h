// voxel_fill.h -- the fill sweep of mesh voxelisation, shared by export.hip (lasr_voxelize) and manifold.hip (the refill after
// the well-composed repair of lasr_manifold_repair).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace lasr {

// Filling, voxelization.py:23-38 (voxelize_sub3 + voxelize_sub4 until visible.sum() stops changing): an empty voxel is visible
// when it is 6-connected through empty voxels to an empty voxel of the grid's boundary; the result is 1 - visible.  That is the
// unique fixed point of the reference's sweeps, reached here with no host synchronisation: one 1024-thread workgroup per mesh
// sweeps the bit grid in place until no word changes (neighbours along c0 / c1 are whole words, along c2 a shift with the carry
// of the next word, and a run of empty bits inside a word fills at once by the carry of an addition).  The sweeps are monotone
// and read their neighbours possibly mid-sweep: any value read lies between the sweep's start and the fixed point, so a sweep in
// which nothing changed proves the fixed point.  S <= 64: occupancy and visibility live in LDS (2 x 32 KiB at S = 64); larger S:
// the same code on the workspace in global memory (visibility after the occupancy).  The same launch writes the int32 output.
__device__ __forceinline__ unsigned long long ld_rel(const unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void st_rel(unsigned long long* p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// every bit of `e` above a bit of `s` within the same run of ones of `e` (s subset of e), plus s
__device__ __forceinline__ unsigned long long run_fill_up(unsigned long long e, unsigned long long s)
{
    return (((e + s) ^ e) & e) | s;
}

constexpr int kFillThreads = 1024;
constexpr int kLdsMaxS = 64;

template <bool kLds>
__global__ __launch_bounds__(kFillThreads) void voxel_fill_kernel(const unsigned long long* __restrict__ occ_g,
                                                                  unsigned long long* __restrict__ vis_g, int* __restrict__ voxels,
                                                                  int* __restrict__ sweeps, int S, int Wd)
{
    __shared__ int flag[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = S * S * Wd, plane = S * Wd;
    const unsigned long long* occ = occ_g + (size_t)b * n;
    unsigned long long *emp, *vis;
    if constexpr (kLds) {
        __shared__ unsigned long long grid[2 * kLdsMaxS * kLdsMaxS];
        emp = grid;
        vis = grid + n;
    } else {
        emp = vis_g + (size_t)b * 2 * n;                        // workspace after the occupancy: empty | visible
        vis = emp + n;
    }
    const unsigned long long top = (S & 63) ? (1ull << (S & 63)) - 1 : ~0ull;   // valid bits of the last word
    const unsigned long long hi = 1ull << ((S - 1) & 63);
    for (int i = tid; i < n; i += kFillThreads) {             // voxelize_sub3: empty voxels of the boundary are visible
        const int w = i % Wd, c1 = (i / Wd) % S, c0 = i / plane;
        const unsigned long long e = ~occ[i] & (w == Wd - 1 ? top : ~0ull);
        unsigned long long v = (c0 == 0 || c0 == S - 1 || c1 == 0 || c1 == S - 1) ? ~0ull : 0ull;
        if (w == 0) v |= 1ull;
        if (w == Wd - 1) v |= hi;
        emp[i] = e;
        vis[i] = v & e;
    }
    if (tid < 3) flag[tid] = 0;
    __syncthreads();
    int it = 0;
    for (;; it++) {                                            // voxelize_sub4 until nothing changes
        int changed = 0;
        for (int i = tid; i < n; i += kFillThreads) {
            const unsigned long long e = emp[i], v = ld_rel(vis + i);
            if (v == e) continue;                              // every empty voxel of the word already visible
            const int w = i % Wd, c1 = (i / Wd) % S, c0 = i / plane;
            unsigned long long nb = v | (v << 1) | (v >> 1);
            if (w > 0) nb |= ld_rel(vis + i - 1) >> 63;
            if (w < Wd - 1) nb |= ld_rel(vis + i + 1) << 63;
            if (c1 > 0) nb |= ld_rel(vis + i - Wd);
            if (c1 < S - 1) nb |= ld_rel(vis + i + Wd);
            if (c0 > 0) nb |= ld_rel(vis + i - plane);
            if (c0 < S - 1) nb |= ld_rel(vis + i + plane);
            unsigned long long s = nb & e;
            s = run_fill_up(e, s);
            s = __builtin_bitreverse64(run_fill_up(__builtin_bitreverse64(e), __builtin_bitreverse64(s)));
            if (s != v) {
                st_rel(vis + i, s);
                changed = 1;
            }
        }
        if (changed) flag[it % 3] = 1;
        if (tid == 0) flag[(it + 1) % 3] = 0;                  // the next sweep's flag: last read before the previous barrier,
        __syncthreads();                                       // next written after this one
        if (!flag[it % 3]) break;
    }
    if (sweeps && tid == 0) sweeps[b] = it + 1;
    int* out = voxels + (size_t)b * S * S * S;
    for (int o = tid; o < S * S * S; o += kFillThreads) {      // 1 - visible
        const int c2 = o % S, c01 = o / S;
        out[o] = 1 - (int)((vis[c01 * Wd + (c2 >> 6)] >> (c2 & 63)) & 1ull);
    }
}

}  // namespace lasr
