// foldpen.hip -- the fold penalty of the optimiser (optimize.py --fold_wt / --pierce_wt; scripts/fold_penalty.py runs it): a loss on
// the posed meshes of a step that is zero exactly where scripts/eval_shape.py --neighbours reports nothing.  This is the project's
// own addition; the definition is the one of include/lasr_ops.h, tests/foldpen_restated.py and DESIGN.md section 4.21, and the list
// it walks is the neighbour pass's (meshnbr.hip), whose determinants and strict tests it shares (meshcheck_geom.h).
// An edge pair is charged (phi - theta)^2 for its interior dihedral angle theta below phi.  The penalty is a function of the angle,
// not of its cosine: d cos / d theta vanishes at the complete fold, the hinge gradient d theta / d x of discrete shells does not.
// A vertex pair is charged the depth of the shallower end of an opposite edge that passes through the other face: linear, so that
// a descent step moves the end point by the same length however shallow it sits, and it crosses the plane.
// foldpen_forward_kernel: one lane per (list entry, mesh) gathers the six corners through `faces`, writes the entry's value and,
// when gradients are wanted, its contribution row of five 3-vectors (zeros for an entry that is not charged: nothing depends on
// what the buffer held); the values are folded per block of 256 entries in fp64 in a fixed order and foldpen_fold_kernel adds the
// block partials in index order.  foldpen_backward_kernel: one thread per (mesh, vertex) walks the vertex's incidences (a CSR the
// Python layer builds once per topology) in ascending order and overwrites its gradient: a store pass and a per-destination sum,
// no floating-point atomics, the same bits on every run.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"
#include "foldpen_geom.h"

namespace lasr {

__global__ __launch_bounds__(256) void foldpen_forward_kernel(const float* __restrict__ x, const int* __restrict__ faces,
                                                              const unsigned long long* __restrict__ list, int n_list, float phi,
                                                              float* __restrict__ values, float* __restrict__ rows,
                                                              double* __restrict__ partials, int V, int F, int NB)
{
    __shared__ double red[4][2];
    const int m = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    const bool want = rows != nullptr;
    const McV zero = {0.f, 0.f, 0.f};
    float crease = 0.f, pierce = 0.f;
    McV g0 = zero, g1 = zero, g2 = zero, g3 = zero, g4 = zero;
    if (e < n_list) {
        const unsigned long long key = list[e];
        const unsigned low = (unsigned)key;
        const int i = (int)(unsigned)(key >> 32), j = (int)(low >> 8);
        const int ca = low & 3, cb = (low >> 2) & 3;
        const bool edge = (low >> 4) & 1, same = (low >> 5) & 1;
        if ((unsigned)i < (unsigned)F && (unsigned)j < (unsigned)F && ca < 3 && cb < 3) {     // (a list that is not the neighbour pass's own)
            const int a0 = faces[(size_t)i * 3], a1 = faces[(size_t)i * 3 + 1], a2 = faces[(size_t)i * 3 + 2];
            const int b0 = faces[(size_t)j * 3], b1 = faces[(size_t)j * 3 + 1], b2 = faces[(size_t)j * 3 + 2];
            const unsigned uV = (unsigned)V;
            if ((unsigned)a0 < uV && (unsigned)a1 < uV && (unsigned)a2 < uV && (unsigned)b0 < uV && (unsigned)b1 < uV && (unsigned)b2 < uV) {
                const float* xm = x + (size_t)m * V * 3;
                const McV A0 = fp_vertex(xm, a0), A1 = fp_vertex(xm, a1), A2 = fp_vertex(xm, a2);
                const McV B0 = fp_vertex(xm, b0), B1 = fp_vertex(xm, b1), B2 = fp_vertex(xm, b2);
                const int ca1 = fp_next(ca), ca2 = fp_next(ca1), cb1 = fp_next(cb), cb2 = fp_next(cb1);
                if (!edge) {
                    const McV pa = fp_corner(A0, A1, A2, ca1), qa = fp_corner(A0, A1, A2, ca2);
                    const McV pb = fp_corner(B0, B1, B2, cb1), qb = fp_corner(B0, B1, B2, cb2);
                    const float dpa = mc_orient(B0, B1, B2, pa), dqa = mc_orient(B0, B1, B2, qa);
                    const float dpb = mc_orient(A0, A1, A2, pb), dqb = mc_orient(A0, A1, A2, qb);
                    // the gradients by stored corner of the triangle, then dealt to the slots: corner cb / ca is the shared vertex
                    McV tA = zero, tB = zero, tC = zero;
                    const float d1 = fp_directed(pa, qa, dpa, dqa, B0, B1, B2, want, g1, g2, tA, tB, tC);
                    g0 = fp_add(g0, fp_corner(tA, tB, tC, cb));
                    g3 = fp_add(g3, fp_corner(tA, tB, tC, cb1));
                    g4 = fp_add(g4, fp_corner(tA, tB, tC, cb2));
                    tA = tB = tC = zero;
                    const float d2 = fp_directed(pb, qb, dpb, dqb, A0, A1, A2, want, g3, g4, tA, tB, tC);
                    g0 = fp_add(g0, fp_corner(tA, tB, tC, ca));
                    g1 = fp_add(g1, fp_corner(tA, tB, tC, ca1));
                    g2 = fp_add(g2, fp_corner(tA, tB, tC, ca2));
                    pierce = d1 + d2;
                } else {
                    const McV nA = fp_cross(fp_sub(A1, A0), fp_sub(A2, A0)), nB = fp_cross(fp_sub(B1, B0), fp_sub(B2, B0));
                    float d = fp_dot(nA, nB);
                    if (same) d = -d;
                    const float qa = fp_dot(nA, nA), qb = fp_dot(nB, nB), q = qa * qb;
                    if (q > 0.f && q < INFINITY) {
                        const McV c = fp_cross(nA, nB);
                        const float theta = atan2f(sqrtf(fp_dot(c, c)), -d);
                        if (theta < phi) {
                            const float gap = phi - theta;
                            crease = gap * gap;
                            if (want) {
                                const McV x0 = fp_corner(A0, A1, A2, ca1), x1 = fp_corner(A0, A1, A2, ca2);
                                const McV x2 = fp_corner(A0, A1, A2, ca), x3 = fp_corner(B0, B1, B2, cb);
                                const McV ed = fp_sub(x1, x0);
                                const float le2 = fp_dot(ed, ed), le = sqrtf(le2);
                                const float sa = fp_sign(mc_orient(A0, A1, A2, x3)), sb = fp_sign(mc_orient(B0, B1, B2, x2));
                                const McV GA = fp_scale((-sa * le) / qa, nA), GB = fp_scale((-sb * le) / qb, nB);
                                const float tA = fp_dot(fp_sub(x2, x0), ed) / le2, tB = fp_dot(fp_sub(x3, x0), ed) / le2;
                                const McV h0 = fp_sub(fp_scale(-(1.f - tA), GA), fp_scale(1.f - tB, GB));
                                const McV h1 = fp_sub(fp_scale(-tA, GA), fp_scale(tB, GB));
                                const float k = -2.f * gap;
                                g0 = fp_scale(k, GA);
                                g1 = fp_scale(k, h0);
                                g2 = fp_scale(k, h1);
                                g3 = fp_scale(k, GB);
                            }
                        }
                    }
                }
            }
        }
        values[(size_t)m * n_list + e] = crease + pierce;                          // one of the two is 0
        if (want) {
            float* r = rows + ((size_t)m * n_list + e) * 15;
            r[0] = g0.x; r[1] = g0.y; r[2] = g0.z;
            r[3] = g1.x; r[4] = g1.y; r[5] = g1.z;
            r[6] = g2.x; r[7] = g2.y; r[8] = g2.z;
            r[9] = g3.x; r[10] = g3.y; r[11] = g3.z;
            r[12] = g4.x; r[13] = g4.y; r[14] = g4.z;
        }
    }
    // the two sums of the block in fp64: the lanes of a wave by shuffles, then the four waves in order (as meshcheck_faces_kernel)
    double sc = (double)crease, sp = (double)pierce;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        sc += __shfl_down(sc, o, 64);
        sp += __shfl_down(sp, o, 64);
    }
    if (lane == 0) {
        red[wave][0] = sc;
        red[wave][1] = sp;
    }
    __syncthreads();
    if (threadIdx.x < 2)
        partials[((size_t)m * NB + blockIdx.x) * 2 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x])
                                                                    + red[3][threadIdx.x];
}

// thread 2 m + which: the block partials of mesh m in index order, rounded once
__global__ __launch_bounds__(64) void foldpen_fold_kernel(const double* __restrict__ partials, float* __restrict__ loss, int N, int NB)
{
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id >= 2 * N) return;
    const int m = id >> 1, which = id & 1;
    double s = 0.;
    for (int b = 0; b < NB; b++) s += partials[((size_t)m * NB + b) * 2 + which];
    loss[id] = (float)s;
}

// inc[k] = (entry 5 + slot) 2 + (1 for an edge pair: the crease plane of grad_loss; 0: the pierce plane)
__global__ __launch_bounds__(256) void foldpen_backward_kernel(const float* __restrict__ rows, const int* __restrict__ vstart,
                                                               const int* __restrict__ inc, int n_inc, const float* __restrict__ grad_loss,
                                                               float* __restrict__ gverts, int V, int n_list)
{
    const int m = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int lo = min(max(vstart[v], 0), n_inc), hi = min(max(vstart[v + 1], lo), n_inc);
    const float gc = grad_loss[(size_t)m * 2], gp = grad_loss[(size_t)m * 2 + 1];
    const float* base = rows + (size_t)m * n_list * 15;
    const unsigned n_slots = (unsigned)n_list * 5u;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int k = lo; k < hi; k++) {
        const int code = inc[k];
        const unsigned r = (unsigned)code >> 1;
        if (code < 0 || r >= n_slots) continue;                                    // (an index that is not the Python layer's own)
        const float g = (code & 1) ? gc : gp;
        const float* p = base + (size_t)r * 3;
        ax = ax + g * p[0];
        ay = ay + g * p[1];
        az = az + g * p[2];
    }
    float* out = gverts + ((size_t)m * V + v) * 3;
    out[0] = ax;
    out[1] = ay;
    out[2] = az;
}

static inline bool fp_sizes_ok(int N, int V, int n_list)
{
    return N >= 0 && N <= LASR_MESHCHECK_MAX_FRAMES && V >= 0 && (long long)V * 3 <= 0x7fffffffLL && n_list >= 0
           && n_list <= LASR_FOLDPEN_MAX_LIST && (long long)N * n_list <= 0x7fffffffLL;
}

}  // namespace lasr

extern "C" size_t lasr_foldpen_scratch_bytes(int N, int n_list)
{
    if (!lasr::fp_sizes_ok(N, 0, n_list)) return 0;
    return (size_t)N * (size_t)((n_list + 255) / 256) * 2 * sizeof(double);
}

extern "C" int lasr_foldpen_forward(const float* x, const int* faces, const unsigned long long* list, int n_list, float phi,
                                    float* values, float* rows, void* scratch, size_t scratch_bytes, float* loss, int N, int V, int F,
                                    void* hip_stream)
{
    if (!lasr::fp_sizes_ok(N, V, n_list) || F < 0 || F > LASR_MESHCHECK_MAX_FACES || !(phi > 0.f && phi <= 1.5707964f))
        return LASR_E_BADARG;
    if (N == 0 || F == 0 || n_list == 0) return LASR_OK;
    if (V < 1 || !x || !faces || !list || !values || !scratch || !loss) return LASR_E_BADARG;
    const void* bufs[7] = {x, faces, list, values, scratch, loss, rows};
    for (int a = 0; a < 7; a++)
        for (int b = a + 1; b < 7; b++)
            if (bufs[a] && bufs[a] == bufs[b]) return LASR_E_BADARG;
    if (scratch_bytes < lasr_foldpen_scratch_bytes(N, n_list)) return LASR_E_WORKSPACE;
    hipStream_t st = (hipStream_t)hip_stream;
    const int NB = (n_list + 255) / 256;
    hipLaunchKernelGGL(lasr::foldpen_forward_kernel, dim3((unsigned)NB, (unsigned)N), dim3(256), 0, st, x, faces, list, n_list, phi,
                       values, rows, (double*)scratch, V, F, NB);
    hipLaunchKernelGGL(lasr::foldpen_fold_kernel, dim3((unsigned)((2 * N + 63) / 64)), dim3(64), 0, st, (const double*)scratch, loss, N,
                       NB);
    return launch_ok();
}

extern "C" int lasr_foldpen_backward(const float* rows, const int* vstart, const int* inc, int n_inc, const float* grad_loss,
                                     float* gverts, int N, int V, int n_list, void* hip_stream)
{
    if (!lasr::fp_sizes_ok(N, V, n_list) || n_inc < 0 || (long long)n_inc > 5LL * n_list) return LASR_E_BADARG;
    if (N == 0 || V == 0) return LASR_OK;
    if (!gverts) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_list == 0 || n_inc == 0) {                                              // no entry, or none that names a vertex: a zeroed gradient
        if (hipMemsetAsync(gverts, 0, (size_t)N * V * 3 * sizeof(float), st) != hipSuccess) return launch_ok();
        return LASR_OK;
    }
    if (!rows || !vstart || !inc || !grad_loss) return LASR_E_BADARG;
    const void* bufs[5] = {rows, vstart, inc, grad_loss, gverts};
    for (int a = 0; a < 5; a++)
        for (int b = a + 1; b < 5; b++)
            if (bufs[a] == bufs[b]) return LASR_E_BADARG;
    hipLaunchKernelGGL(lasr::foldpen_backward_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)N), dim3(256), 0, st, rows, vstart, inc,
                       n_inc, grad_loss, gverts, V, n_list);
    return launch_ok();
}
