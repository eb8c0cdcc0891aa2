// meshcheck_geom.h -- what the two passes over the face records of scripts/eval_shape.py share: meshcheck.hip (faces that share no
// vertex) and meshnbr.hip (faces that do).  The record layout, the determinant and the edge-against-triangle test of
// include/lasr_ops.h, the (tile I, tile J >= I) numbering of the blocks and the size limits.  Both translation units are built with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lasr_ops.h"

namespace lasr {

constexpr int MC_TILE = LASR_MESHCHECK_TILE;
constexpr int MC_REC = 18;                                     // slots 0-8 a b c, 9-11 box min, 12-14 box max, 15-17 the indices

static_assert(MC_TILE == 256, "a tile is one block of 256 threads, and a queue entry packs two 8-bit positions");

struct McV {
    float x, y, z;
};

// ((b - a) x (c - a)) . (d - a) in the order include/lasr_ops.h states (this translation unit is built with -ffp-contract=off)
__device__ __forceinline__ float mc_orient(const McV& a, const McV& b, const McV& c, const McV& d)
{
    const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const float wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
    const float cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    const float ex = d.x - a.x, ey = d.y - a.y, ez = d.z - a.z;
    return (cx * ex + cy * ey) + cz * ez;
}

// dp, dq = orient(a, b, c, p), orient(a, b, c, q): the three edge determinants are formed only for an edge that crosses the plane
__device__ __forceinline__ bool mc_pierces(const McV& p, const McV& q, float dp, float dq, const McV& a, const McV& b, const McV& c)
{
    if (!((dp > 0.f && dq < 0.f) || (dp < 0.f && dq > 0.f))) return false;
    const float s0 = mc_orient(p, q, a, b), s1 = mc_orient(p, q, b, c), s2 = mc_orient(p, q, c, a);
    return (s0 > 0.f && s1 > 0.f && s2 > 0.f) || (s0 < 0.f && s1 < 0.f && s2 < 0.f);
}

// Block p of a frame -> (I, J), I <= J < NT: row I starts at I NT - I (I - 1) / 2.
__device__ __forceinline__ void mc_tile_pair(int p, int NT, int& I, int& J)
{
    const double b = 2. * NT + 1.;
    int i = (int)((b - sqrt(b * b - 8. * (double)p)) * 0.5);
    i = min(max(i, 0), NT - 1);
    auto start = [NT](int r) { return (long long)r * NT - (long long)r * (r - 1) / 2; };
    while (i > 0 && start(i) > p) i--;
    while (i + 1 < NT && start(i + 1) <= p) i++;
    I = i;
    J = i + (int)(p - start(i));
}

static inline bool mc_sizes_ok(int T, int F)
{
    return T >= 0 && T <= LASR_MESHCHECK_MAX_FRAMES && F >= 0 && F <= LASR_MESHCHECK_MAX_FACES && (long long)T * F <= 0x7fffffffLL;
}

static inline int mc_blocks(int F) { return (F + MC_TILE - 1) / MC_TILE; }

}  // namespace lasr
