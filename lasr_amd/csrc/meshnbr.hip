// meshnbr.hip -- the neighbour pass of scripts/eval_shape.py --neighbours (scripts/shape_neighbours.py runs it): folds between
// faces that share a vertex or an edge, which the pair pass of meshcheck.hip never tests.  This is the project's own addition; the
// definition is the one of include/lasr_ops.h, tests/meshnbr_restated.py and DESIGN.md section 4.18.
// Why only the opposite edge of a vertex pair is tested: the planes of two triangles that share a vertex meet in a line through
// that vertex.  If the triangles overlap beyond it, the overlap segment ends where the nearer of the two edges opposite the shared
// corner enters the other triangle, so one of those two edges pierces.  The four edges through the shared vertex touch the other
// triangle in that vertex: their plane determinants are zero in exact arithmetic and noise in fp32, and must not be tested.
// An edge pair is judged by its dihedral angle alone: non-coplanar faces that share an edge cannot intersect outside that edge, so
// "creased" is an angle criterion (interior angle below fold_deg), not an intersection test.  Edge lengths from about 1e-4 to 1e4
// keep q, the eighth power of a length, inside fp32; a pair whose products overflow or vanish is not creased.
// meshnbr_list_kernel, the topology pass: one block per (tile I, tile J >= I) of 256 faces over the int32 index triples only.  A
// thread keeps the indices of one face of tile I and walks tile J in LDS, every lane reading the same j (a broadcast); the nine
// comparisons give the shared-corner count and the code.  Survivors are compacted per wave (ballot + prefix count) into a queue in
// LDS and leave 64 at a time through one integer atomicAdd on the list's counter per wave and batch.
// meshnbr_test_kernel, the hot path: one lane per (list entry, frame) gathers the two face records lasr_meshcheck_faces left and
// runs the definition.  Integer atomics only: the same input gives the same counts on every run, and the same hits once sorted.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"
#include "meshcheck_geom.h"
#include "sr_device.h"

namespace lasr {

constexpr int MN_QCAP = 128;                                   // per wave: below 64 queued before a push of at most 64
constexpr unsigned MN_COS_ONE = 0xBF800000u;                   // mn_encode(+1.f)

// Degenerate faces are staged as index triples no face can hold (valid indices are >= 0): they match nothing, each other included.
__device__ __forceinline__ void mn_stage(const int* __restrict__ faces, int f, int which, int& a, int& b, int& c, bool& degenerate)
{
    a = faces[(size_t)f * 3];
    b = faces[(size_t)f * 3 + 1];
    c = faces[(size_t)f * 3 + 2];
    degenerate = a == b || b == c || a == c;
    if (degenerate) {
        a = -1 - 3 * which;
        b = -2 - 3 * which;
        c = -3 - 3 * which;
    }
}

__global__ __launch_bounds__(256) void meshnbr_list_kernel(const int* __restrict__ faces, unsigned long long* __restrict__ list,
                                                           unsigned long long* __restrict__ counters, int F, int NT, int capacity)
{
    __shared__ int sJ[3][MC_TILE];
    __shared__ unsigned long long ring[4][MN_QCAP];
    const int tid = threadIdx.x;
    int I, J;
    mc_tile_pair((int)blockIdx.x, NT, I, J);
    const int cntI = min(MC_TILE, F - I * MC_TILE), cntJ = min(MC_TILE, F - J * MC_TILE);
    const bool live = tid < cntI, diag = I == J;
    int v0 = -1, v1 = -2, v2 = -3;
    bool degI = false;
    if (live) mn_stage(faces, I * MC_TILE + tid, 0, v0, v1, v2, degI);
    if (tid < cntJ) {
        int w0, w1, w2;
        bool degJ;
        mn_stage(faces, J * MC_TILE + tid, 1, w0, w1, w2, degJ);
        sJ[0][tid] = w0;
        sJ[1][tid] = w1;
        sJ[2][tid] = w2;
    }
    __syncthreads();

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned long long* q = ring[wave];
    int head = 0, tail = 0, n_dup = 0, n_same = 0;             // wave-uniform
    // Up to 64 queued keys leave through one atomicAdd of this wave; the count stays exact past the capacity.
    auto flush = [&]() {
        __builtin_amdgcn_wave_barrier();
        const int n = min(tail - head, 64);
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&counters[0], (unsigned long long)n);
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32));
        const unsigned long long slot = (((unsigned long long)hi << 32) | lo) + (unsigned)lane;
        const unsigned long long key = q[(head + lane) & (MN_QCAP - 1)];
        if (lane < n && slot < (unsigned long long)capacity) list[slot] = key;
        head += n;
        __builtin_amdgcn_wave_barrier();
    };
    const int gi = I * MC_TILE + tid;
    const int j0 = wave * 64 >= cntI ? cntJ : (diag ? wave * 64 + 1 : 0);
#pragma unroll 4
    for (int j = j0; j < cntJ; j++) {
        const int w0 = sJ[0][j], w1 = sJ[1][j], w2 = sJ[2][j];
        const bool e00 = v0 == w0, e01 = v0 == w1, e02 = v0 == w2, e10 = v1 == w0, e11 = v1 == w1, e12 = v1 == w2, e20 = v2 == w0,
                   e21 = v2 == w1, e22 = v2 == w2;
        const bool m0 = e00 | e01 | e02, m1 = e10 | e11 | e12, m2 = e20 | e21 | e22;
        const bool any = live & (!diag | (j > tid)) & (m0 | m1 | m2);
        if (wave_mask(any) == 0) continue;                     // the same in every lane
        const bool n0 = e00 | e10 | e20, n1 = e01 | e11 | e21;
        const int s = (int)m0 + (int)m1 + (int)m2;
        const bool edge = any && s == 2, keep = any && s <= 2;
        // the shared corner of a vertex pair, the apex of an edge pair
        const int ca = edge ? (!m0 ? 0 : (!m1 ? 1 : 2)) : (m0 ? 0 : (m1 ? 1 : 2));
        const int cb = edge ? (!n0 ? 0 : (!n1 ? 1 : 2)) : (n0 ? 0 : (n1 ? 1 : 2));
        // i's shared edge runs from corner ca + 1 to ca + 2, j's from cb + 1 to cb + 2: the same direction iff the first ends agree
        const int va = ca == 0 ? v1 : (ca == 1 ? v2 : v0), wb = cb == 0 ? w1 : (cb == 1 ? w2 : w0);
        const bool same = edge && va == wb;
        n_dup += __popcll(wave_mask(any && s == 3));
        n_same += __popcll(wave_mask(same));
        const unsigned long long mask = wave_mask(keep);
        if (keep) {
            const unsigned low = ((unsigned)(J * MC_TILE + j) << 8) | (unsigned)ca | ((unsigned)cb << 2) | ((unsigned)edge << 4)
                                 | ((unsigned)same << 5);
            q[(tail + bits_below_lane(mask)) & (MN_QCAP - 1)] = ((unsigned long long)(unsigned)gi << 32) | low;
        }
        tail += __popcll(mask);
        if (tail - head >= 64) flush();
    }
    if (tail - head > 0) flush();
    if (lane == 0) {
        if (n_dup > 0) atomicAdd(&counters[1], (unsigned long long)n_dup);
        if (n_same > 0) atomicAdd(&counters[3], (unsigned long long)n_same);
    }
    if (diag) {                                                // every face has one diagonal block
        const int n_deg = __popcll(wave_mask(live && degI));
        if (lane == 0 && n_deg > 0) atomicAdd(&counters[2], (unsigned long long)n_deg);
    }
}

// Order-preserving: a < b as floats iff mn_encode(a) < mn_encode(b) as unsigned (no NaN is ever encoded).
__device__ __forceinline__ unsigned mn_encode(float x)
{
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float mn_decode(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

__device__ __forceinline__ float mn_pick(float a, float b, float c, int which) { return which == 0 ? a : (which == 1 ? b : c); }

// corner `which` of a triangle, by selects: the corners stay in registers
__device__ __forceinline__ McV mn_corner(const McV& a, const McV& b, const McV& c, int which)
{
    return {mn_pick(a.x, b.x, c.x, which), mn_pick(a.y, b.y, c.y, which), mn_pick(a.z, b.z, c.z, which)};
}

__device__ __forceinline__ McV mn_load(const float* __restrict__ r, int corner, int F)
{
    return {r[(size_t)(3 * corner) * F], r[(size_t)(3 * corner + 1) * F], r[(size_t)(3 * corner + 2) * F]};
}

__global__ __launch_bounds__(256) void meshnbr_test_kernel(const float* __restrict__ rec, const unsigned long long* __restrict__ list,
                                                           int n_list, float k, int* __restrict__ nbr_count,
                                                           unsigned long long* __restrict__ totals, unsigned* __restrict__ cursor,
                                                           int* __restrict__ hits, unsigned* __restrict__ min_cos, int F, int max_pairs)
{
    const int t = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool pierced = false, creased = false;
    int i = 0, j = 0;
    unsigned cosine = MN_COS_ONE;
    if (e < n_list) {
        const unsigned long long key = list[e];
        const unsigned low = (unsigned)key;
        i = (int)(unsigned)(key >> 32);
        j = (int)(low >> 8);
        const int ca = low & 3, cb = (low >> 2) & 3;
        const bool edge = (low >> 4) & 1, same = (low >> 5) & 1;
        if ((unsigned)i < (unsigned)F && (unsigned)j < (unsigned)F && ca < 3 && cb < 3) {     // (a list that is not this pass's own)
            const float* ra = rec + (size_t)t * MC_REC * F + i;
            const float* rb = rec + (size_t)t * MC_REC * F + j;
            const McV A0 = mn_load(ra, 0, F), A1 = mn_load(ra, 1, F), A2 = mn_load(ra, 2, F);
            const McV B0 = mn_load(rb, 0, F), B1 = mn_load(rb, 1, F), B2 = mn_load(rb, 2, F);
            if (!edge) {
                const McV pa = mn_corner(A0, A1, A2, ca == 2 ? 0 : ca + 1), qa = mn_corner(A0, A1, A2, ca == 0 ? 2 : ca - 1);
                const McV pb = mn_corner(B0, B1, B2, cb == 2 ? 0 : cb + 1), qb = mn_corner(B0, B1, B2, cb == 0 ? 2 : cb - 1);
                // the four plane determinants first; the edge determinants only for an edge that crosses
                const float dpa = mc_orient(B0, B1, B2, pa), dqa = mc_orient(B0, B1, B2, qa);
                const float dpb = mc_orient(A0, A1, A2, pb), dqb = mc_orient(A0, A1, A2, qb);
                pierced = mc_pierces(pa, qa, dpa, dqa, B0, B1, B2) || mc_pierces(pb, qb, dpb, dqb, A0, A1, A2);
            } else {
                const float ux = A1.x - A0.x, uy = A1.y - A0.y, uz = A1.z - A0.z;
                const float wx = A2.x - A0.x, wy = A2.y - A0.y, wz = A2.z - A0.z;
                const float ax = uy * wz - uz * wy, ay = uz * wx - ux * wz, az = ux * wy - uy * wx;
                const float sx = B1.x - B0.x, sy = B1.y - B0.y, sz = B1.z - B0.z;
                const float tx = B2.x - B0.x, ty = B2.y - B0.y, tz = B2.z - B0.z;
                const float bx = sy * tz - sz * ty, by = sz * tx - sx * tz, bz = sx * ty - sy * tx;
                float d = (ax * bx + ay * by) + az * bz;
                if (same) d = -d;
                const float qa = (ax * ax + ay * ay) + az * az, qb = (bx * bx + by * by) + bz * bz;
                const float q = qa * qb, dd = d * d;
                const bool good = q > 0.f && q < INFINITY;
                creased = good && dd < INFINITY && d < 0.f && dd > k * q;
                if (good) {
                    const float c = d / sqrtf(q);
                    if (c == c) cosine = mn_encode(fminf(fmaxf(c, -1.f), 1.f));
                }
            }
        }
    }
    const bool hit = pierced || creased;
    if (hit) {
        int* count = nbr_count + ((size_t)t * 2 + (creased ? 1 : 0)) * F;
        atomicAdd(&count[i], 1);
        atomicAdd(&count[j], 1);
        if (max_pairs > 0) {
            const unsigned slot = atomicAdd(&cursor[t], 1u);
            if (slot < (unsigned)max_pairs) {
                int* h = hits + ((size_t)t * max_pairs + slot) * 3;
                h[0] = i;
                h[1] = j;
                h[2] = creased ? 1 : 0;
            }
        }
    }
    const int np = __popcll(wave_mask(pierced)), nc = __popcll(wave_mask(creased));
    if (lane == 0) {
        if (np > 0) atomicAdd(&totals[(size_t)t * 2], (unsigned long long)np);
        if (nc > 0) atomicAdd(&totals[(size_t)t * 2 + 1], (unsigned long long)nc);
    }
    if (cosine < MN_COS_ONE) atomicMin(&min_cos[t], cosine);
}

// the encoded minima -> fp32, in place
__global__ __launch_bounds__(64) void meshnbr_decode_kernel(unsigned* __restrict__ min_cos, int T)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < T) min_cos[t] = __float_as_uint(mn_decode(min_cos[t]));
}

}  // namespace lasr

extern "C" int lasr_meshnbr_list(const int* faces, unsigned long long* list, unsigned long long* counters, int F, int capacity,
                                 void* hip_stream)
{
    if (F < 0 || F > LASR_MESHCHECK_MAX_FACES || capacity < 0) return LASR_E_BADARG;
    if (F == 0) return LASR_OK;
    if (!faces || !counters || (capacity > 0 && !list)) return LASR_E_BADARG;
    const void* bufs[3] = {faces, counters, list};
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++)
            if (bufs[a] && bufs[a] == bufs[b]) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    if (hipMemsetAsync(counters, 0, LASR_MESHNBR_COUNTERS * sizeof(unsigned long long), st) != hipSuccess) return launch_ok();
    const int NT = lasr::mc_blocks(F);
    const long long NTP = (long long)NT * (NT + 1) / 2;             // at most 2^23 + 2^11
    hipLaunchKernelGGL(lasr::meshnbr_list_kernel, dim3((unsigned)NTP), dim3(256), 0, st, faces, list, counters, F, NT, capacity);
    return launch_ok();
}

extern "C" int lasr_meshnbr_test(const void* workspace, size_t workspace_bytes, const unsigned long long* list, int n_list, float k,
                                 int* nbr_count, unsigned long long* totals, unsigned* cursor, int* hits, float* min_cos, int T, int F,
                                 int max_pairs, void* hip_stream)
{
    if (!lasr::mc_sizes_ok(T, F) || n_list < 0 || max_pairs < 0 || (long long)T * max_pairs * 3 > 0x7fffffffLL || !(k >= 0.f && k <= 1.f))
        return LASR_E_BADARG;
    if (T == 0 || F == 0 || n_list == 0) return LASR_OK;
    if (!workspace || !list || !nbr_count || !totals || !cursor || !min_cos || (max_pairs > 0 && !hits)) return LASR_E_BADARG;
    const void* bufs[7] = {workspace, list, nbr_count, totals, cursor, min_cos, hits};
    for (int a = 0; a < 7; a++)
        for (int b = a + 1; b < 7; b++)
            if (bufs[a] && bufs[a] == bufs[b]) return LASR_E_BADARG;
    if (workspace_bytes < lasr_meshcheck_workspace_bytes(T, F)) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    if (hipMemsetAsync(nbr_count, 0, (size_t)T * 2 * F * sizeof(int), st) != hipSuccess) return launch_ok();
    if (hipMemsetAsync(totals, 0, (size_t)T * 2 * sizeof(unsigned long long), st) != hipSuccess) return launch_ok();
    if (hipMemsetAsync(cursor, 0, (size_t)T * sizeof(unsigned), st) != hipSuccess) return launch_ok();
    if (hipMemsetD32Async((hipDeviceptr_t)min_cos, (int)lasr::MN_COS_ONE, (size_t)T, st) != hipSuccess) return launch_ok();
    hipLaunchKernelGGL(lasr::meshnbr_test_kernel, dim3((unsigned)((n_list + 255) / 256), (unsigned)T), dim3(256), 0, st,
                       (const float*)workspace, list, n_list, k, nbr_count, totals, cursor, hits, (unsigned*)min_cos, F, max_pairs);
    hipLaunchKernelGGL(lasr::meshnbr_decode_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, st, (unsigned*)min_cos, T);
    return launch_ok();
}
