// foldpen_geom.h -- what foldpen.hip (the fold penalty between neighbouring faces) and isectpen.hip (the penalty between faces that
// share no vertex) share: the small vector helpers and the depth of a piercing edge with its gradient, fp_directed, the one definition
// of include/lasr_ops.h and tests/foldpen_restated.py (_directed).  Both translation units are built with -ffp-contract=off.
#pragma once
#include "meshcheck_geom.h"

namespace lasr {

__device__ __forceinline__ McV fp_sub(const McV& a, const McV& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ McV fp_add(const McV& a, const McV& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ McV fp_scale(float s, const McV& a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float fp_dot(const McV& a, const McV& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// the component order of mc_orient's cross product
__device__ __forceinline__ McV fp_cross(const McV& u, const McV& w)
{
    return {u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
__device__ __forceinline__ float fp_pick(float a, float b, float c, int which) { return which == 0 ? a : (which == 1 ? b : c); }
// corner `which` of a triangle, by selects: the corners stay in registers
__device__ __forceinline__ McV fp_corner(const McV& a, const McV& b, const McV& c, int which)
{
    return {fp_pick(a.x, b.x, c.x, which), fp_pick(a.y, b.y, c.y, which), fp_pick(a.z, b.z, c.z, which)};
}
__device__ __forceinline__ int fp_next(int c) { return c == 2 ? 0 : c + 1; }
__device__ __forceinline__ float fp_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ McV fp_vertex(const float* __restrict__ x, int v)
{
    return {x[(size_t)v * 3], x[(size_t)v * 3 + 1], x[(size_t)v * 3 + 2]};
}

// Edge (p, q) against triangle (a, b, c), dp, dq its plane determinants: the depth of the shallower end when the edge pierces, else
// 0.  want: the gradient of the depth is ADDED to gp or gq (the shallower end; p on a tie) and to ga, gb, gc.
__device__ __forceinline__ float fp_directed(const McV& p, const McV& q, float dp, float dq, const McV& a, const McV& b, const McV& c,
                                             bool want, McV& gp, McV& gq, McV& ga, McV& gb, McV& gc)
{
    if (!mc_pierces(p, q, dp, dq, a, b, c)) return 0.f;
    const McV u = fp_sub(b, a), w = fp_sub(c, a), n = fp_cross(u, w);
    const float n2 = fp_dot(n, n), rt = sqrtf(n2);
    const bool at_q = fabsf(dq) < fabsf(dp);
    const float dr = at_q ? dq : dp;
    if (want) {
        const McV r = at_q ? q : p, e = fp_sub(r, a);
        const float sg = fp_sign(dr);
        const McV unit = {(sg * n.x) / rt, (sg * n.y) / rt, (sg * n.z) / rt};
        const float lb = fp_dot(fp_cross(e, w), n) / n2, lc = fp_dot(fp_cross(u, e), n) / n2, la = (1.f - lb) - lc;
        if (at_q) gq = fp_add(gq, unit);
        else gp = fp_add(gp, unit);
        ga = fp_add(ga, fp_scale(-la, unit));
        gb = fp_add(gb, fp_scale(-lb, unit));
        gc = fp_add(gc, fp_scale(-lc, unit));
    }
    return fabsf(dr) / rt;
}

}  // namespace lasr
