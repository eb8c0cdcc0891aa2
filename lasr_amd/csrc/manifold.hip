// manifold.hip -- watertight re-meshing on the GPU (lasr_amd/nnutils/manifold.py: watertight), in place of the external
// Manifold binary the reference runs at scripts/eval_mesh.py:100-105, render_vis.py:98 and nnutils/train_utils.py:422.
// The solid comes from lasr_voxelize (export.hip).  This file makes it well-composed, refills it, extracts its boundary as a
// closed 2-manifold of lattice quads, and moves the vertices onto the input.  include/lasr_ops.h states the contract and
// DESIGN.md section 4.6 the construction.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"
#include "point_triangle.h"
#include "voxel_fill.h"

namespace lasr {

// Bit grid of the solid as export.hip lays it out: [S (c0)][S (c1)][Wd words along c2], bit c2 & 63 of word c2 >> 6.
struct MfLayout {
    int S, Wd, R, Wv;        // R = (S + 1)^2 lattice rows (c0, c1) of S + 1 lattice points along c2, Wv = words per lattice row
    size_t n;                // words of one bit grid
    // workspace, in this order: solid A [n], solid B [n], fill scratch [2n], border flag [1], then per lattice row:
    // vertex mask [R * Wv], counts of boundary voxels / vertices / triangles [3R], exclusive offsets of vertices / triangles [2R]
    size_t a, b, fill, border, mask, cnt, off, bytes;
};

static MfLayout mf_layout(int S)
{
    MfLayout L;
    L.S = S;
    L.Wd = (S + 63) / 64;
    L.R = (S + 1) * (S + 1);
    L.Wv = (S + 1 + 63) / 64;
    L.n = (size_t)S * S * L.Wd;
    L.a = 0;
    L.b = L.a + L.n * 8;
    L.fill = L.b + L.n * 8;
    L.border = L.fill + 2 * L.n * 8;
    L.mask = L.border + 8;
    L.cnt = L.mask + (size_t)L.R * L.Wv * 8;
    L.off = L.cnt + (size_t)3 * L.R * 4;
    L.bytes = L.off + (size_t)2 * L.R * 4;
    return L;
}

// ===========================================================================
// Pack: int32 voxels (non-zero = solid) -> the bit grid A, one thread per word.  A solid voxel on the outer layer of the grid
// raises the border flag (the repair then refuses the solid).
// ===========================================================================
__global__ __launch_bounds__(256) void mf_pack_kernel(const int* __restrict__ voxels, unsigned long long* __restrict__ bits,
                                                      unsigned* __restrict__ border, int S, int Wd)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)S * S * Wd) return;
    const int w = (int)(i % Wd), c1 = (int)((i / Wd) % S), c0 = (int)(i / ((long long)S * Wd));
    const int* row = voxels + ((size_t)c0 * S + c1) * S;
    const int k1 = min(64, S - 64 * w);
    unsigned long long v = 0;
    for (int k = 0; k < k1; k++) v |= (unsigned long long)(row[64 * w + k] != 0) << k;
    bits[i] = v;
    if (!v) return;
    const bool edge = c0 == 0 || c0 == S - 1 || c1 == 0 || c1 == S - 1;
    if (edge || (w == 0 && (v & 1ull)) || (w == Wd - 1 && ((v >> ((S - 1) & 63)) & 1ull))) atomicOr(border, 1u);
}

// ===========================================================================
// Well-composed repair.  A configuration is critical when it is, in either colour,
//   (a) a 2x2 square of an axis plane whose diagonal pairs have opposite values (a checkerboard), or
//   (b) a 2x2x2 block whose only voxels of one value are an antipodal pair.
// A Jacobi sweep turns every empty voxel of a critical configuration solid, all at once; sweeps repeat until one changes nothing.
// Only voxels are added, so this ends.  Voxels outside the grid count as empty; no critical configuration contains one (each
// would hold two empty voxels on different diagonals, or four empty voxels of one face of a block).
// Bit-parallel along c2: for the 3 x 3 rows (c0 + d0, c1 + d1) around a word, X is the word, dn(X) has voxel c2 - 1 at bit c2 and
// up(X) voxel c2 + 1 (carries from the neighbouring words).  Every configuration containing a voxel lies in those 27 words.
// One 1024-thread workgroup runs every sweep (src -> dst, barrier, swap), as the fill does; the cold path needs no more.
// ===========================================================================
constexpr int kRepairThreads = 1024;

__device__ __forceinline__ unsigned long long checker(unsigned long long a, unsigned long long b, unsigned long long c,
                                                      unsigned long long d)
{
    return ~(a ^ d) & ~(b ^ c) & (a ^ b);                    // diagonals (a, d) and (b, c) equal, the two diagonals different
}

// block v[b0][b1][b2] (index b0 * 4 + b1 * 2 + b2): antipodal pair p, q of one value, the other six of the other
__device__ __forceinline__ unsigned long long antipodal(const unsigned long long* v)
{
    unsigned long long crit = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) {                            // pairs (p, 7 - p): 000-111, 001-110, 010-101, 011-100
        const int q = 7 - p;
        unsigned long long o = 0, a = ~0ull;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (k == p || k == q) continue;
            o |= v[k];
            a &= v[k];
        }
        crit |= (v[p] & v[q] & ~o) | (~v[p] & ~v[q] & a);
    }
    return crit;
}

__device__ __forceinline__ unsigned long long repair_word(const unsigned long long* g, int S, int Wd, int c0, int c1, int w)
{
    unsigned long long L[3][3][3];                           // [layer: c2 - 1, c2, c2 + 1][d0 + 1][d1 + 1]
#pragma unroll
    for (int d0 = 0; d0 < 3; d0++) {
#pragma unroll
        for (int d1 = 0; d1 < 3; d1++) {
            const int a0 = c0 + d0 - 1, a1 = c1 + d1 - 1;
            unsigned long long x = 0, p = 0, nx = 0;
            if (a0 >= 0 && a0 < S && a1 >= 0 && a1 < S) {
                const unsigned long long* r = g + ((size_t)a0 * S + a1) * Wd;
                x = r[w];
                if (w > 0) p = r[w - 1];
                if (w < Wd - 1) nx = r[w + 1];
            }
            L[0][d0][d1] = (x << 1) | (p >> 63);
            L[1][d0][d1] = x;
            L[2][d0][d1] = (x >> 1) | (nx << 63);
        }
    }
    unsigned long long crit = 0;
#pragma unroll
    for (int e0 = 0; e0 < 2; e0++) {                         // anchors: the block / square starts at offset e - 1
#pragma unroll
        for (int e1 = 0; e1 < 2; e1++)                       // (a) in the c0-c1 plane, at this voxel's c2
            crit |= checker(L[1][e0][e1], L[1][e0 + 1][e1], L[1][e0][e1 + 1], L[1][e0 + 1][e1 + 1]);
#pragma unroll
        for (int z = 0; z < 2; z++) {
            crit |= checker(L[z][e0][1], L[z][e0 + 1][1], L[z + 1][e0][1], L[z + 1][e0 + 1][1]);   // (a) c0-c2 plane
            crit |= checker(L[z][1][e0], L[z][1][e0 + 1], L[z + 1][1][e0], L[z + 1][1][e0 + 1]);   // (a) c1-c2 plane
#pragma unroll
            for (int e1 = 0; e1 < 2; e1++) {                 // (b)
                unsigned long long v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = L[z + (k & 1)][e0 + (k >> 2)][e1 + ((k >> 1) & 1)];
                crit |= antipodal(v);
            }
        }
    }
    const unsigned long long top = (w == Wd - 1 && (S & 63)) ? (1ull << (S & 63)) - 1 : ~0ull;
    return (L[1][1][1] | crit) & top;
}

// info[0] = sweeps run (the last one changed nothing), or -1 when the border flag is up (the solid is left as it was)
__global__ __launch_bounds__(kRepairThreads) void mf_repair_kernel(unsigned long long* a, unsigned long long* b,
                                                                   const unsigned* __restrict__ border, int* __restrict__ info,
                                                                   int S, int Wd)
{
    __shared__ int flag[3];
    const int tid = threadIdx.x;
    if (*border) {
        if (tid == 0) info[0] = -1;
        return;
    }
    const int n = S * S * Wd;
    if (tid < 3) flag[tid] = 0;
    __syncthreads();
    unsigned long long *src = a, *dst = b;
    int it = 0;
    for (;; it++) {
        int changed = 0;
        for (int i = tid; i < n; i += kRepairThreads) {
            const int w = i % Wd, c1 = (i / Wd) % S, c0 = i / (S * Wd);
            const unsigned long long v = repair_word(src, S, Wd, c0, c1, w);
            dst[i] = v;
            changed |= v != src[i];
        }
        if (changed) flag[it % 3] = 1;
        if (tid == 0) flag[(it + 1) % 3] = 0;
        __syncthreads();                                     // also orders this sweep's writes before the next sweep's reads
        if (!flag[it % 3]) break;
        unsigned long long* t = src;
        src = dst;
        dst = t;
    }
    if (tid == 0) info[0] = it + 1;
    // the last sweep wrote dst == src: both buffers hold the result, the fill reads a
}

// ===========================================================================
// Count, scan, extract.  Rows: lattice row r = p0 * (S + 1) + p1 holds lattice points (p0, p1, 0..S) and, for p0, p1 < S, the
// voxel row (p0, p1, 0..S-1).  A lattice point is a vertex when its eight voxels are not all equal (then two 6-adjacent ones
// differ, and their shared face has the point as a corner).
// ===========================================================================
__device__ __forceinline__ int vox_at(const int* v, int S, int c0, int c1, int c2)
{
    if (c0 < 0 || c0 >= S || c1 < 0 || c1 >= S || c2 < 0 || c2 >= S) return 0;
    return v[((size_t)c0 * S + c1) * S + c2] != 0;
}

__global__ __launch_bounds__(256) void mf_count_kernel(const int* __restrict__ voxels, unsigned long long* __restrict__ mask,
                                                       int* __restrict__ cnt, int S, int Wv)
{
    const int R = (S + 1) * (S + 1);
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int p0 = r / (S + 1), p1 = r % (S + 1);
    unsigned long long* m = mask + (size_t)r * Wv;
    for (int k = 0; k < Wv; k++) m[k] = 0;
    int nv = 0;
    int lo = 0, hi = 0;                                      // OR / AND of the four voxels (p0 - 1..p0, p1 - 1..p1) at c2 = k - 1
    for (int k = 0; k <= S; k++) {
        int o = 0, a = 1;                                    // ... and at c2 = k
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int x = vox_at(voxels, S, p0 - 1 + (q >> 1), p1 - 1 + (q & 1), k);
            o |= x;
            a &= x;
        }
        if ((lo | o) != 0 && (hi & a) == 0) {                // neither all empty nor all solid
            m[k >> 6] |= 1ull << (k & 63);
            nv++;
        }
        lo = o;
        hi = a;
    }
    int nb = 0, nt = 0;
    if (p0 < S && p1 < S) {
        for (int k = 0; k < S; k++) {
            if (!vox_at(voxels, S, p0, p1, k)) continue;
            const int e = !vox_at(voxels, S, p0 - 1, p1, k) + !vox_at(voxels, S, p0 + 1, p1, k) + !vox_at(voxels, S, p0, p1 - 1, k) +
                          !vox_at(voxels, S, p0, p1 + 1, k) + !vox_at(voxels, S, p0, p1, k - 1) + !vox_at(voxels, S, p0, p1, k + 1);
            nb += e > 0;
            nt += 2 * e;
        }
    }
    cnt[r] = nb;
    cnt[R + r] = nv;
    cnt[2 * R + r] = nt;
}

// Exclusive scans of the vertex and triangle counts over the rows, and the totals: one 1024-thread workgroup, each thread a
// contiguous run of rows; integer sums, so the result does not depend on the schedule.
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kScanThreads) void mf_scan_kernel(const int* __restrict__ cnt, int* __restrict__ off,
                                                               int* __restrict__ counts, int R)
{
    __shared__ int part[3][kScanThreads];
    const int tid = threadIdx.x;
    const int per = (R + kScanThreads - 1) / kScanThreads;
    const int r0 = min(R, tid * per), r1 = min(R, r0 + per);
    int s[3] = {0, 0, 0};
    for (int r = r0; r < r1; r++) {
#pragma unroll
        for (int j = 0; j < 3; j++) s[j] += cnt[j * R + r];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) part[j][tid] = s[j];
    __syncthreads();
    if (tid < 3) {                                           // one thread per array: 1024 serial adds
        int acc = 0;
        for (int t = 0; t < kScanThreads; t++) {
            const int x = part[tid][t];
            part[tid][t] = acc;
            acc += x;
        }
        counts[tid] = acc;
    }
    __syncthreads();
    int v = part[1][tid], t = part[2][tid];
    for (int r = r0; r < r1; r++) {
        off[r] = v;
        off[R + r] = t;
        v += cnt[R + r];
        t += cnt[2 * R + r];
    }
}

__device__ __forceinline__ long long vert_index(const unsigned long long* __restrict__ mask, const int* __restrict__ voff, int S, int Wv,
                                                int p0, int p1, int p2)
{
    const int r = p0 * (S + 1) + p1;
    const unsigned long long* m = mask + (size_t)r * Wv;
    int rank = 0;
    for (int k = 0; k < (p2 >> 6); k++) rank += __popcll(m[k]);
    rank += __popcll(m[p2 >> 6] & ((1ull << (p2 & 63)) - 1));
    return (long long)voff[r] + rank;
}

// One thread per lattice row: its vertices (lattice coordinates, in lattice order) and, for a voxel row, its triangles in voxel
// order then direction -c0, +c0, -c1, +c1, -c2, +c2.  The quad of direction +/-a lies in the plane c_a = voxel + (1 or 0); with
// (b, c) = (a + 1, a + 2) mod 3 its corners are q0 = (0, 0), q1 = (1, 0), q2 = (1, 1), q3 = (0, 1) in (b, c) for +a and
// q0, q3, q2, q1 for -a (counter-clockwise seen from the empty side), split into (q0, q1, q2), (q0, q2, q3).  Writes past V or F
// (counts that do not belong to this solid) are dropped.
__global__ __launch_bounds__(256) void mf_extract_kernel(const int* __restrict__ voxels, const unsigned long long* __restrict__ mask,
                                                         const int* __restrict__ off, float* __restrict__ verts,
                                                         long long* __restrict__ faces, int S, int Wv, int V, int F)
{
    const int R = (S + 1) * (S + 1);
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int p0 = r / (S + 1), p1 = r % (S + 1);
    const unsigned long long* m = mask + (size_t)r * Wv;
    long long v = off[r];
    for (int k = 0; k <= S; k++) {
        if (!((m[k >> 6] >> (k & 63)) & 1ull)) continue;
        if (v < V) {
            verts[3 * v] = (float)p0;
            verts[3 * v + 1] = (float)p1;
            verts[3 * v + 2] = (float)k;
        }
        v++;
    }
    if (p0 >= S || p1 >= S) return;
    const int* voff = off;
    long long t = off[R + r];
    for (int k = 0; k < S; k++) {
        if (!vox_at(voxels, S, p0, p1, k)) continue;
        const int c[3] = {p0, p1, k};
        for (int dir = 0; dir < 6; dir++) {
            const int a = dir >> 1, s = dir & 1;             // axis, sign (0: -, 1: +)
            int nb[3] = {c[0], c[1], c[2]};
            nb[a] += s ? 1 : -1;
            if (vox_at(voxels, S, nb[0], nb[1], nb[2])) continue;
            const int b = (a + 1) % 3, cc = (a + 2) % 3;
            long long q[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int jj = s ? j : (4 - j) & 3;          // -a: q0, q3, q2, q1
                int p[3] = {c[0], c[1], c[2]};
                p[a] += s;
                p[b] += (jj == 1 || jj == 2);
                p[cc] += (jj >= 2);
                q[j] = vert_index(mask, voff, S, Wv, p[0], p[1], p[2]);
            }
            if (t + 1 < F) {
                long long* f = faces + 3 * t;
                f[0] = q[0]; f[1] = q[1]; f[2] = q[2];
                f[3] = q[0]; f[4] = q[2]; f[5] = q[3];
            }
            t += 2;
        }
    }
}

// ===========================================================================
// Projection and guard, in lattice units (voxel edge h = 1).
// ===========================================================================
__global__ __launch_bounds__(256) void mf_project_kernel(const float* __restrict__ lat, const float* __restrict__ in_verts,
                                                         const long long* __restrict__ in_faces, const int* __restrict__ arg,
                                                         float* __restrict__ verts, int V, int Vin, int Fin)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float p[3] = {lat[3 * v], lat[3 * v + 1], lat[3 * v + 2]};
    const int f = arg[v];
    bool ok = f >= 0 && f < Fin;
    long long i[3] = {0, 0, 0};
    if (ok) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            i[j] = in_faces[3 * (size_t)f + j];
            ok = ok && i[j] >= 0 && i[j] < Vin;
        }
    }
    if (!ok) {                                               // no face: the vertex stays on the lattice
#pragma unroll
        for (int d = 0; d < 3; d++) verts[3 * v + d] = p[d];
        return;
    }
    float a[3], b[3], c[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        a[d] = in_verts[3 * i[0] + d];
        b[d] = in_verts[3 * i[1] + d];
        c[d] = in_verts[3 * i[2] + d];
    }
    const Closest cl = point_triangle(p, a, b, c);
#pragma unroll
    for (int d = 0; d < 3; d++) verts[3 * v + d] = cl.w[0] * a[d] + cl.w[1] * b[d] + cl.w[2] * c[d];
}

__device__ __forceinline__ void tri_normal(const float* P, const long long* f, float* n)
{
    const float* a = P + 3 * f[0];
    const float* b = P + 3 * f[1];
    const float* c = P + 3 * f[2];
    const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    n[0] = u[1] * w[2] - u[2] * w[1];
    n[1] = u[2] * w[0] - u[0] * w[2];
    n[2] = u[0] * w[1] - u[1] * w[0];
}

// Rounds of: flag every face whose normal has a non-positive dot product with its lattice normal or whose area is below
// min_area; then move every vertex of a flagged face back to the lattice.  Both phases read only what the previous one wrote,
// so the result does not depend on the schedule.  An all-lattice face passes (its normal is its lattice normal, area 1/2), so
// each round reverts at least one vertex and the loop ends.  rounds[0] = rounds that reverted something.
constexpr int kGuardThreads = 1024;

__global__ __launch_bounds__(kGuardThreads) void mf_guard_kernel(const float* __restrict__ lat, float* verts,
                                                                 const long long* __restrict__ faces, int* flags,
                                                                 int* __restrict__ rounds, int V, int F, float min_area)
{
    __shared__ int any[3];
    const int tid = threadIdx.x;
    if (tid < 3) any[tid] = 0;
    __syncthreads();
    int it = 0;
    for (; it <= V; it++) {
        int bad = 0;
        for (int f = tid; f < F; f += kGuardThreads) {
            const long long* fi = faces + 3 * (size_t)f;
            if (fi[0] < 0 || fi[0] >= V || fi[1] < 0 || fi[1] >= V || fi[2] < 0 || fi[2] >= V) continue;
            float n[3], nl[3];
            tri_normal(verts, fi, n);
            tri_normal(lat, fi, nl);
            const float dt = n[0] * nl[0] + n[1] * nl[1] + n[2] * nl[2];
            const float area = 0.5f * sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (!(dt > 0.f) || !(area >= min_area)) {
                flags[fi[0]] = 1;
                flags[fi[1]] = 1;
                flags[fi[2]] = 1;
                bad = 1;
            }
        }
        if (bad) any[it % 3] = 1;
        if (tid == 0) any[(it + 1) % 3] = 0;
        __syncthreads();
        if (!any[it % 3]) break;
        for (int v = tid; v < V; v += kGuardThreads) {
            if (!flags[v]) continue;
            flags[v] = 0;
            verts[3 * v] = lat[3 * v];
            verts[3 * v + 1] = lat[3 * v + 1];
            verts[3 * v + 2] = lat[3 * v + 2];
        }
        __syncthreads();
    }
    if (tid == 0) rounds[0] = it;
}

static bool size_ok(int S) { return S >= LASR_MANIFOLD_MIN_SIZE && S <= LASR_MANIFOLD_MAX_SIZE; }

}  // namespace lasr

extern "C" size_t lasr_manifold_workspace_bytes(int S)
{
    if (!lasr::size_ok(S)) return 0;
    return lasr::mf_layout(S).bytes;
}

extern "C" int lasr_manifold_repair(int* voxels, int* info, void* workspace, size_t workspace_bytes, int S, void* hip_stream)
{
    using namespace lasr;
    if (!size_ok(S) || !voxels || !info) return LASR_E_BADARG;
    const MfLayout L = mf_layout(S);
    if (!workspace || workspace_bytes < L.bytes) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    char* ws = (char*)workspace;
    unsigned long long* a = (unsigned long long*)(ws + L.a);
    unsigned long long* b = (unsigned long long*)(ws + L.b);
    unsigned* border = (unsigned*)(ws + L.border);
    if (hipMemsetAsync(border, 0, 8, st) != hipSuccess) return launch_ok();
    LASR_LAUNCH(K_MF_PACK, mf_pack_kernel, dim3((unsigned)((L.n + 255) / 256)), dim3(256), 0, voxels, a, border, S, L.Wd);
    LASR_LAUNCH(K_MF_REPAIR, mf_repair_kernel, dim3(1), dim3(kRepairThreads), 0, a, b, border, info, S, L.Wd);
    // the refill: export.hip's fill sweep on the repaired bit grid (global-memory variant), writing the int32 solid
    LASR_LAUNCH(K_VOXEL_FILL, voxel_fill_kernel<false>, dim3(1), dim3(kFillThreads), 0, a, (unsigned long long*)(ws + L.fill), voxels,
                info + 1, S, L.Wd);
    return launch_ok();
}

extern "C" int lasr_manifold_count(const int* voxels, int* counts, void* workspace, size_t workspace_bytes, int S, void* hip_stream)
{
    using namespace lasr;
    if (!size_ok(S) || !voxels || !counts) return LASR_E_BADARG;
    const MfLayout L = mf_layout(S);
    if (!workspace || workspace_bytes < L.bytes) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    char* ws = (char*)workspace;
    unsigned long long* mask = (unsigned long long*)(ws + L.mask);
    int* cnt = (int*)(ws + L.cnt);
    int* off = (int*)(ws + L.off);
    LASR_LAUNCH(K_MF_COUNT, mf_count_kernel, dim3((unsigned)((L.R + 255) / 256)), dim3(256), 0, voxels, mask, cnt, S, L.Wv);
    LASR_LAUNCH(K_MF_SCAN, mf_scan_kernel, dim3(1), dim3(kScanThreads), 0, cnt, off, counts, L.R);
    return launch_ok();
}

extern "C" int lasr_manifold_extract(const int* voxels, float* verts, long long* faces, int V, int F, void* workspace,
                                     size_t workspace_bytes, int S, void* hip_stream)
{
    using namespace lasr;
    if (!size_ok(S) || !voxels || V < 0 || F < 0 || F % 2) return LASR_E_BADARG;
    if ((V > 0 && !verts) || (F > 0 && !faces)) return LASR_E_BADARG;
    const MfLayout L = mf_layout(S);
    if (!workspace || workspace_bytes < L.bytes) return LASR_E_WORKSPACE;
    if (V == 0 && F == 0) return LASR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    char* ws = (char*)workspace;
    LASR_LAUNCH(K_MF_EXTRACT, mf_extract_kernel, dim3((unsigned)((L.R + 255) / 256)), dim3(256), 0, voxels,
                (const unsigned long long*)(ws + L.mask), (const int*)(ws + L.off), verts, faces, S, L.Wv, V, F);
    return launch_ok();
}

extern "C" int lasr_manifold_project(const float* lattice, const float* in_verts, const long long* in_faces, const int* arg_face,
                                     float* verts, int V, int Vin, int Fin, void* hip_stream)
{
    using namespace lasr;
    if (V < 0 || Vin < 1 || Fin < 1) return LASR_E_BADARG;
    if (V == 0) return LASR_OK;
    if (!lattice || !in_verts || !in_faces || !arg_face || !verts) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    LASR_LAUNCH(K_MF_PROJECT, mf_project_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, lattice, in_verts, in_faces, arg_face,
                verts, V, Vin, Fin);
    return launch_ok();
}

extern "C" int lasr_manifold_guard(const float* lattice, float* verts, const long long* faces, int* flags, int* rounds, int V, int F,
                                   float min_area, void* hip_stream)
{
    using namespace lasr;
    if (V < 0 || F < 0 || !(min_area >= 0.f)) return LASR_E_BADARG;
    if (!rounds || (V > 0 && (!lattice || !verts || !flags)) || (F > 0 && !faces)) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    if (V > 0 && hipMemsetAsync(flags, 0, (size_t)V * sizeof(int), st) != hipSuccess) return launch_ok();
    LASR_LAUNCH(K_MF_GUARD, mf_guard_kernel, dim3(1), dim3(kGuardThreads), 0, lattice, verts, faces, flags, rounds, V, F, min_area);
    return launch_ok();
}
