// sr_common.h -- what the raster translation units share: the kernel argument block and the block -> work mapping.
#pragma once
#include <hip/hip_runtime.h>

#include "sr_device.h"

namespace lasr {

struct RasterArgs {
    const float* __restrict__ recs;      // [N*F, REC]
    const short4* __restrict__ rects;    // [N*F] exact pixel rectangle (x0,x1,row0,row1) of the bbox test
    const short4* __restrict__ grects;   // [N, ceil(F/64)] union of the pixel rects of 64 consecutive faces
    const float* __restrict__ textures;  // [N,F,T,3]
    int N, F, T, res, IS;
    float near, far, eps, sigma, gamma, thr;
    const float* __restrict__ near_far_dev;   // optional: {near, far} read on the device (no host sync)
    Modes m;
    int overwrite_grads;                      // backward, vertex attributes: store the face's gradients instead of adding to them
    int use_bg;                               // forward: the background colour comes from bg[] instead of the pre-filled soft_colors
    const int* __restrict__ choice;           // forward, optional: device word written by sr_choose_kernel; a forward kernel whose
                                              // id (CHOICE_*) differs returns at once (both candidates are launched)
    int choice_max;                           // < 0: *choice is the id; else *choice is the launch's number of non-empty tiles
                                              // (sr_order_kernel) and the id is CHOICE_COOP iff it is at most this
    const int* __restrict__ order;            // forward, optional: block -> (image, 8x8 tile) table written by sr_order_kernel
    float bg[9];
    // launch constants of the backward pass, computed once on the host (IEEE division / square root: the bits the device
    // expansions gave, without ~30 VALU instructions per face): 1 / IS, the pixel-centre fma coefficients 2 / IS, (1 - IS) / IS,
    // (IS - 1) / IS, and stage 1's reject distance -sqrt(1.05 thr)
    float inv_is, cx_a, cx_b, cy_b, far_t;
    // ... and of a wave's (image, face) split: gw / F as a multiplication and a shift (face_div below)
    unsigned fdiv_m;
    int fdiv_s;
    // ... and whether the backward reads its pixel planes through scalar bases and 32-bit byte offsets (plane_offsets_fit32 below)
    int plane_off32;
};

// The backward kernel (sr_backward.h) reads the pixel planes of an image through one wave-uniform base pointer per (image, tensor)
// and a 32-bit per-lane byte offset that spans the tensor's nch + 1 planes of 4 IS^2 bytes.  That holds while the span stays below
// 2^32 bytes (image sides up to 16383 / 12385 / 10362 at three / six / nine channels); beyond it the launcher takes the
// instantiation that keeps 64-bit per-lane addresses.
inline unsigned long long plane_offset_span(int nch, int IS)
{
    return (unsigned long long)(nch + 1) * (unsigned long long)IS * (unsigned long long)IS * 4ull;
}
inline int plane_offsets_fit32(int nch, int IS) { return plane_offset_span(nch, IS) < (1ull << 32); }

// n / F for 0 <= n < 2^25 -- the wave index of the backward pass; check_common admits N F <= (2^31 - 1) / 64 = 2^25 - 1 -- by an exact
// magic multiplier instead of the integer-division expansion (v_rcp_iflag and a chain of s_mul_hi / s_cselect in every wave).
// With l = ceil(log2 F), s = 25 + l and m = ceil(2^s / F) = (2^s + e) / F, 0 <= e < F:
//     n m / 2^s = n / F + n e / (F 2^s),   and   n e < 2^25 2^l = 2^s,   so the excess is below 1 / F:
// floor(n / F) leaves a fraction of at most (F - 1) / F, the sum stays below the next integer, and floor(n m / 2^s) = floor(n / F)
// for every such n (Granlund & Montgomery 1994, theorem 4.2 with N = 25).  F > 2^(l - 1) gives m < 2^26: the product is below 2^51
// and takes one 32 x 32 -> 64 bit multiplication.  (tests/test_face_constants_cases.py walks the boundaries through lasr_selftest_face_div.)
struct FaceDiv { unsigned m; int s; };
inline FaceDiv face_div_of(int F)
{
    int l = 0;
    while ((1ll << l) < (long long)F) l++;
    FaceDiv d;
    d.s = 25 + l;
    d.m = F > 0 ? (unsigned)(((1ull << d.s) + (unsigned long long)F - 1) / (unsigned long long)F) : 0u;
    return d;
}
__host__ __device__ __forceinline__ int face_div(int n, unsigned m, int s)
{
    return (int)(((unsigned long long)(unsigned)n * (unsigned long long)m) >> s);
}

constexpr int CHOICE_ONE_WAVE = 0, CHOICE_COOP = 1;
__device__ __forceinline__ int chosen_kernel(const RasterArgs& A)
{
    const int w = *A.choice;
    return A.choice_max < 0 ? w : (w <= A.choice_max ? CHOICE_COOP : CHOICE_ONE_WAVE);
}

// Block -> (image, tile) with all tiles of an image kept on one XCD (block b runs
// on XCD b % 8; an image's records are then fetched into a single L2).
__device__ __forceinline__ int xcd_remap(int b, int total)
{
    const int per = total >> 3;
    if ((total & 7) == 0) return (b & 7) * per + (b >> 3);
    return b;
}

}  // namespace lasr
