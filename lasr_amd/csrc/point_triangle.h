// point_triangle.h -- closest point of a triangle to a point, shared by fused.hip (point <-> mesh distance) and manifold.hip
// (projection of the re-meshed lattice vertices onto the input).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace lasr {

// The closest point on a triangle is the interior projection when it falls inside, otherwise the nearest of the
// three clamped edge projections (Ericson, Real-Time Collision Detection 5.1.5, written as a min over candidates so
// that degenerate triangles fall back to their edges).  bary = barycentric weights of the closest point.
struct Closest { float d2; float w[3]; };

__device__ __forceinline__ float dot3(const float* u, const float* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }

__device__ __forceinline__ Closest point_triangle(const float* p, const float* a, const float* b, const float* c)
{
    float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { ab[d] = b[d] - a[d]; ac[d] = c[d] - a[d]; ap[d] = p[d] - a[d]; bp[d] = p[d] - b[d]; cp[d] = p[d] - c[d]; }
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
    const float eps = 1e-12f;
    Closest best;
    best.d2 = INFINITY; best.w[0] = 1.f; best.w[1] = 0.f; best.w[2] = 0.f;
    auto consider = [&](float w0, float w1, float w2) {
        float e = 0.f;
#pragma unroll
        for (int d = 0; d < 3; d++) { const float q = w0 * a[d] + w1 * b[d] + w2 * c[d] - p[d]; e += q * q; }
        if (e < best.d2) { best.d2 = e; best.w[0] = w0; best.w[1] = w1; best.w[2] = w2; }
    };
    if (va >= 0.f && vb >= 0.f && vc >= 0.f) {
        const float den = fmaxf(va + vb + vc, eps);
        const float v = vb / den, w = vc / den;
        consider(1.f - v - w, v, w);
    }
    const float tab = fminf(fmaxf(d1 / fmaxf(d1 - d3, eps), 0.f), 1.f);
    const float tac = fminf(fmaxf(d2 / fmaxf(d2 - d6, eps), 0.f), 1.f);
    const float tbc = fminf(fmaxf((d4 - d3) / fmaxf((d4 - d3) + (d5 - d6), eps), 0.f), 1.f);
    consider(1.f - tab, tab, 0.f);
    consider(1.f - tac, 0.f, tac);
    consider(0.f, 1.f - tbc, tbc);
    return best;
}

}  // namespace lasr
