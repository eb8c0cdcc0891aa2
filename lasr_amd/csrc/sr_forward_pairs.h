// sr_forward_pairs.h -- the forward raster kernel of LASR's mode combination for launches that fill the chip: every LANE walks
// the (pixel, face) pairs of its own pixel.
//
// The one-wave-per-tile kernel (sr_raster.hip: forward_tile_body) keeps the face index wave-uniform: every one of the ~290
// instructions of a list entry is issued for the 64 pixels of the tile while ~27 of them lie within the face's reach (41.5 % live
// lanes, profiles/r05_valu.json), and the record arrives as SGPR operands, which halve the issue rate of an fp32 instruction
// (profiles/r02_valu_issue.txt).  Here the face index is PER LANE:
//
//   list     four waves share a 16x16-pixel tile and build its ordered face list as before (group rects, pixel rects, corner cull);
//   stage    64 list entries at a time: their records (+ vertex attributes) are copied into LDS in a layout made for per-lane
//            gathers -- 16-byte quads grouped by use, each edge's constants in a block of its own (so the edge an outside pixel
//            projects to is ONE run-time offset, not three exec-masked code variants), the obtuse-corner test's operands
//            precomputed -- at an odd quad stride, so that 16 lanes reading the same quad of 16 different entries hit 16
//            different bank groups;
//   spans    (lane = ENTRY) every lane turns its own staged entry into the columns of the wave's four tile rows that the entry does
//            not certainly miss: the not-far region of a well-conditioned face is the intersection of the three half-planes
//            w_k >= far[k] (the backward's conservative line-distance reject, sr_backward.h: stage 1), its cut with a pixel row is ONE
//            run of columns -- one fma per edge and row, rounded outward, cut with the entry's exact pixel rect (span_edge / span_row
//            below).  An entry the reject does not apply to keeps its whole rect.  Four 16-bit runs make the lane's 64-bit word;
//   transpose the 64 x 64 bit matrix (entry x pixel of the wave) is transposed across the wave in six block-swap stages
//            (wave_transpose64 below: v_permlane32_swap, v_permlane16_swap, DPP, ds_swizzle): pixel lane p = 16 j + c now holds
//            the mask of the entries whose span covers its pixel.  (Before: every lane popped the rect candidates of its pixel one per
//            iteration -- 49 VALU each, 835 k candidates per bench frame, a fifth of the kernel's vector instructions -- after
//            ranking, partnering and handing masks back and forth to even the loop out; profiles/r16_row_spans_ab.txt.)
//            Records that are not tame get no bit: they are SLOW entries, handled wave-uniform by the generic arithmetic at the end
//            of the chunk for the pixels of their rect;
//   balance  the lanes are ranked by their pair count (six ballots), rank r partnered with rank 63 - r: the lighter partner takes
//            the upper half of the difference from the heavier one's mask and folds it into a private partial state, at the
//            heavier lane's pixel centre;
//   walk     every lane pops its own mask, gathers the entry's record from LDS with 16-byte reads and applies the pair with the
//            arithmetic of forward_face; whether the pixel lies inside the face follows from the pair's own barycentrics.  Inside and
//            outside pixels share ONE clamped edge projection: an inside pixel's nearest edge line follows from the three products
//            w_k^2 hk2_k (sr_device.h: euclid_one_ext); only where two lines are equidistant within 1.5 % or within the face's
//            rounding scale (sr_device.h: near_tie) -- the reference's own choice is then decided by its rounding -- the
//            reference's three projections run (a region most iterations skip);
//   merge    partial states (alpha product, running maximum, rescaled sums) are folded into their pixel's state.
//
// What changes against the one-wave kernel is the ORDER in which a pixel's fragments meet its state: chunk by chunk, and a round's
// list is DEALT over its chunks (chunk c of nch holds the list positions c, c + nch, ...: see chunk_pos below), so a pixel meets
// the faces of residue 0 first, then those of residue 1, ...; within a chunk in index order (inside and outside fragments alike),
// a stolen run merged at the end of the chunk; with two teams, the odd chunks' state merged at the very end.  Alpha
// product and depth softmax are symmetric in the fragments, only the rounding sequence moves (image within ~1e-6 of the
// reference-order kernels; the running maximum is exact).  Every (pixel, face) pair itself goes through the same instruction
// sequence as in forward_face (K.cu:370-453).
#pragma once

namespace lasr {

constexpr int PW_CAP = 64;            // list entries per staged chunk = bits per lane mask
constexpr int PW_LIST = 1024;         // tile list entries per round (u16 ids relative to the round's first face)
constexpr int PW_TILE = 16;

typedef unsigned long long u64_t;

// ---- which list entries a chunk holds.  A round's `count` entries go into nch = ceil(count / 64) chunks, DEALT round-robin: chunk c
// holds the list positions c, c + nch, c + 2 nch, ... -- count / nch of them, one more in the first count % nch chunks.  The list is
// in face order and face order is spatially coherent (subdivided icospheres), so 64 CONSECUTIVE entries cover one corner of the
// tile: a few lanes hold most of the chunk's pairs and both per-lane loops run as long as their fullest lane.  Dealt, every chunk
// is a sample of the whole list and its pairs spread over the tile (tools/pair_stats.py: walk iterations -8.9 %, classification
// -5.7 % on the bench frames).  Bit e of every mask is still lane e's entry, and a chunk's entries are still in ascending face order.
// (A/B against 64 consecutive entries per chunk: profiles/r12_chunk_deal_ab.txt.)
__host__ __device__ constexpr int chunk_count(int count) { return (count + PW_CAP - 1) / PW_CAP; }
__host__ __device__ constexpr int chunk_size(int count, int nch, int c) { return c < nch ? count / nch + (c < count % nch ? 1 : 0) : 0; }
__host__ __device__ constexpr int chunk_pos(int nch, int c, int l) { return c + l * nch; }
static_assert(chunk_count(0) == 0 && chunk_count(1) == 1 && chunk_count(64) == 1 && chunk_count(65) == 2 && chunk_count(PW_LIST) == PW_LIST / PW_CAP, "chunks per round");
static_assert(chunk_size(65, 2, 0) == 33 && chunk_size(65, 2, 1) == 32 && chunk_size(65, 2, 2) == 0, "sizes differ by at most one; a trip past the last chunk is empty");
static_assert(chunk_size(128, 2, 1) == 64 && chunk_size(129, 3, 0) == 43 && chunk_size(129, 3, 2) == 43 && chunk_size(PW_LIST, 16, 15) == PW_CAP, "no chunk beyond 64 entries");
static_assert(chunk_pos(3, 2, 0) == 2 && chunk_pos(3, 2, 42) == 128 && chunk_pos(2, 0, 32) == 64, "chunk c: positions c, c + nch, ...; the last one is the list's last");

// ---- the staged record (floats; 14 quads + the attributes)
//   q0  inv0..3      q1  inv4..7      q2  inv8, flags, rect lo, edge table
//   q3  far[0..2], rect ext: far[k] = -sqrt(1.05 thr / hk2[k]), the barycentric w_k below which a pixel is certainly beyond the threshold
//       edge table: which edge an OUTSIDE pixel projects to (K.cu:113-125), two bits per case: bit pair n0 + 2 n1 + 4 n2
//       (n_k = "w_k <= 0") of the low half, or of the high half when the pixel lies beyond the face's obtuse corner (q7's test)
//   q4  x0 y0 x1 y1  q5  x2 y2 z0 z1  q6  z2, 1/z0, 1/z1, 1/z2
//   q7  obtuse corner c (flags bit0..2): x_c, y_c, x_o - x_c, y_o - y_c with o = (c + 2) % 3   (K.cu:113-125's override test)
//   q8 + 2k, q9 + 2k   edge k: e[k][0..2], e[k][(k+1)%3]  |  den[k], 1/den[k], -, -
//   q14 hq[0..2]: the squared height over edge k's line (hk2 of the vertex opposite edge k; 0 unless the face is well conditioned),
//       hq[3]: the face's absolute near-tie scale (sr_device.h: near_tie_scale)
//   60 ..  attributes [vertex][channel]
constexpr int PR_INV = 0, PR_FLAGS = 9, PR_BB = 10, PR_ETBL = 11, PR_HK2 = 12, PR_BBE = 15, PR_XY = 16, PR_Z = 22, PR_IZ = 25, PR_OBT = 28, PR_EDGE = 32, PR_HQ = 56, PR_TEX = 60;

// record field (sr_device.h index) -> staged slot; compile-time for the generic arithmetic, which indexes with constants
__host__ __device__ constexpr int pr_of(int i)
{
    return i == R_BB ? PR_BB : i == R_BB + 1 ? PR_BBE : i == R_FLAGS ? PR_FLAGS
         : (i >= R_INV && i < R_INV + 9) ? PR_INV + (i - R_INV)
         : (i >= R_HK2 && i < R_HK2 + 3) ? PR_HK2 + (i - R_HK2)
         : (i >= R_FACE && i < R_FACE + 9) ? ((i - R_FACE) % 3 == 2 ? PR_Z + (i - R_FACE) / 3 : PR_XY + 2 * ((i - R_FACE) / 3) + (i - R_FACE) % 3)
         : (i >= R_DEN && i < R_DEN + 3) ? PR_EDGE + 8 * (i - R_DEN) + 4
         : (i >= R_IDEN && i < R_IDEN + 3) ? PR_EDGE + 8 * (i - R_IDEN) + 5
         : (i >= R_E && i < R_E + 9) ? PR_EDGE + 8 * ((i - R_E) / 3) + (i - R_E) % 3
         : (i >= R_IZ && i < R_IZ + 3) ? PR_IZ + (i - R_IZ) : 15;
}
struct PairRecView {                                   // the staged record behind the record indices of sr_device.h
    const float* p;
    __device__ __forceinline__ float operator[](int i) const { return p[pr_of(i)]; }
};

// LDS: the chunk's staged records at an ODD number of quads per slot, the tile's list, the list builder's counts
// SPLIT teams of four waves share a tile (SPLIT = 2: launches whose time is the heaviest tile's chain of dependent phases, not the
// chip's throughput): they build the list together, team t walks the chunks t, t + SPLIT, ... in its own staging buffer, and the
// teams' partial states meet in `merge` at the end.
template <int NCH, int SPLIT = 1>
struct PairLds {
    static constexpr int Q0 = (PR_TEX + 3 * NCH + 3) / 4;
    static constexpr int RS = 4 * (Q0 | 1);
    float rec[SPLIT][PW_CAP * RS];
    unsigned short list[PW_LIST];
    int wcnt[2][4 * SPLIT];
    float sel[32];                    // edge k: (k == 0, k == 1, k == 2 | k + 1 == 0, k + 1 == 1, k + 1 == 2 mod 3) as 0 / 1, 8 floats apart;
                                      // [24..31]: zeros, the block a 2-bit edge index of 3 would name (see pairs_tile_body)
    float merge[SPLIT > 1 ? (SPLIT - 1) * 256 * (3 + NCH) : 1];       // partial states of the teams >= 1, [team - 1][field][pixel lane]
};

__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }

// the conservative corner cull of the tile kernels on a block of pixels [xlo, xhi] x [ylo, yhi]: false when all four corners lie
// beyond one edge's line by more than sqrt(thr_cull)
template <typename RP>
__device__ __forceinline__ bool reaches_block(RP R, float xlo, float xhi, float ylo, float yhi, float thr_cull)
{
    bool hit = true;
    if (__float_as_int(R[R_FLAGS]) & 16) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float a = R[R_INV + 3 * k], b = R[R_INV + 3 * k + 1], c = R[R_INV + 3 * k + 2];
            const float w00 = a * xlo + b * ylo + c, w01 = a * xhi + b * ylo + c;
            const float w10 = a * xlo + b * yhi + c, w11 = a * xhi + b * yhi + c;
            const float wmax = fmaxf(fmaxf(w00, w01), fmaxf(w10, w11));
            if (wmax < 0.f && wmax * wmax * R[R_HK2 + k] > thr_cull) hit = false;
        }
    }
    return hit;
}

// staging: source quads [Q0, Q1) of a record (global layout, sr_device.h) into their staged slots
__host__ __device__ constexpr bool rec_used(int i) { return i < 15 || (i >= 16 && i < 31) || (i >= 32 && i < 44); }
template <int Q0, int Q1>
__device__ __forceinline__ void stage_quads(const float4* __restrict__ src, float* __restrict__ dst, float thr_far, bool well)
{
    float4 v[Q1 - Q0];
#pragma unroll
    for (int q = Q0; q < Q1; q++) v[q - Q0] = src[q];
#pragma unroll
    for (int q = Q0; q < Q1; q++) {
        const float w[4] = {v[q - Q0].x, v[q - Q0].y, v[q - Q0].z, v[q - Q0].w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = 4 * q + j;
            if (!rec_used(i)) continue;
            if (i >= R_HK2 && i < R_HK2 + 3) {                 // the far threshold; -inf (never far) unless the face is well conditioned
                dst[pr_of(i)] = well ? -sqrtf(thr_far / w[j]) : -__builtin_huge_valf();
                dst[PR_HQ + (i - R_HK2 + 1) % 3] = well ? w[j] : 0.f;     // vertex k lies opposite edge (k + 1) % 3
                if (i == R_HK2) dst[PR_HQ + 3] = near_tie_scale(w[0], w[1], w[2]);        // (R_HK2 .. + 2 are words 0..2 of this source quad)
                continue;
            }
            dst[pr_of(i)] = w[j];
            if (i == R_E + 1) dst[PR_EDGE + 3] = w[j];            // e[k][(k+1)%3] once more, as the fourth word of edge k's block
            if (i == R_E + 5) dst[PR_EDGE + 8 + 3] = w[j];
            if (i == R_E + 6) dst[PR_EDGE + 16 + 3] = w[j];
        }
    }
}

// (edge_table, the 2-bit table of the edge an outside pixel projects to, lives in sr_device.h: the backward raster reads it too)

// a / b from y = RN(1 / b) with ONE Newton-Markstein correction: the correctly rounded quotient unless a / b lies within 2^-48
// (relative) of a rounding boundary -- about one quotient in 2^24 then differs from div_by_recip's by an ulp.  For the
// well-conditioned quotients after the distance code (clip / normalise, depth, softmax exponents); the edge projection, whose
// result decides `dis >= threshold`, keeps the two-correction form.
__device__ __forceinline__ float div_by_recip1(float a, float b, float y)
{
    const float q = a * y;
    return __builtin_fmaf(__builtin_fmaf(-b, q, a), y, q);
}

// (float)(1. / (1. + (double)e)) for 0 < e < 2^116 (K.cu:397,403 promote the sigmoid to double) as v_rcp_f64 and ONE Newton step:
// v_rcp_f64 is good to 4.6e-8, the step squares that -- far below what narrowing to float can see (tools/ubench/acc.hip: no
// mismatch against recip64_noscale's full expansion in 2^24 arguments)
__device__ __forceinline__ float sigmoid_from_exp(float e)
{
    const double x = 1. + (double)e;
    const double y = __builtin_amdgcn_rcp(x);
    return (float)__builtin_fma(__builtin_fma(-x, y, 1.), y, y);
}

// clamp to [0, 1] of a finite value as the output modifier of a multiplication by one (v_mul_f32 issues at the fma rate, v_med3 /
// v_max at 0.6 of it, profiles/r04_ubench_mix.txt); same value as v_med3(x, 0, 1) up to the sign of a zero
__device__ __forceinline__ float clamp01(float x)
{
    float r;
    asm("v_mul_f32_e64 %0, 1.0, %1 clamp" : "=v"(r) : "v"(x));
    return r;
}

// merge of a partial state P (fragments folded on their own, starting from "no fragment": a = 1, sum 0, reference level
// smax = eps) into S:  a = a_S a_P;  m = max(m_S, m_P);  sum = sum_S e^((m_S - m) / gamma) + sum_P e^((m_P - m) / gamma)
template <int NCH>
__device__ __forceinline__ void merge_partial(PixState<NCH>& S, float pa, float pm, float ps, const float (&pc)[NCH],
                                              float gamma, float inv_gamma)
{
    S.a = (float)((double)S.a * (double)pa);
    const float mx = fmaxf(S.smax, pm);
    const float ds = S.smax - mx, dp = pm - mx;            // one of them is exactly 0
    const float es = exp_1ulp(div_by_recip(ds, gamma, inv_gamma));
    const float ep = exp_1ulp(div_by_recip(dp, gamma, inv_gamma));
    S.ssum = S.ssum * es + ps * ep;
#pragma unroll
    for (int k = 0; k < NCH; k++) S.c[k] = S.c[k] * es + pc[k] * ep;
    S.smax = mx;
}

// One (pixel, face) pair of a TAME record against the pixel state: forward_face<LASR, MK = true> (sr_raster.hip) with the record
// gathered per lane from its staged slot R.  Whether the pixel lies inside the face follows from the pair's own barycentrics (the
// same predicate on the same operands as euclid<.., TAME>).  Same operations in the same order per pair: the fragment's D, depth
// and weights are the bits the one-wave kernel computes.
template <int NCH>
__device__ __forceinline__ void pair_apply(const RasterArgs& A, const UniRecip& U, const float* __restrict__ R, const float* __restrict__ SEL,
                                           bool has, float xp, float yp, PixState<NCH>& s)
{
#pragma clang fp contract(off)
    float4 q0 = ld4(R), q1 = ld4(R + 4), q2 = ld4(R + 8);
    float4 q4 = ld4(R + PR_XY), q5 = ld4(R + PR_XY + 4), ob = ld4(R + PR_OBT);      // one LDS round trip for the six quads
    const float w0 = q0.x * xp + q0.y * yp + q0.z;                    // K.cu:24-29 (barycentric())
    const float w1 = q0.w * xp + q1.x * yp + q1.y;
    const float w2 = q1.z * xp + q1.w * yp + q2.x;
    const bool is_in = (bool)((int)has & (int)(fminf(fminf(w0, w1), w2) > 0) & (int)(fmaxf(fmaxf(w0, w1), w2) < 1));
    const float x0 = q4.x, y0 = q4.y, x1 = q4.z, y1 = q4.w, x2 = q5.x, y2 = q5.y, z0 = q5.z, z1 = q5.w;
    float narg;
    // which edge: an inside pixel's nearest edge LINE from the three products w^2 hk2 (sr_device.h: euclid_one_ext), an outside pixel's
    // from the sign pattern of its barycentrics (K.cu:113-125); inside pixels near an angle bisector -- or of a face that is not
    // well conditioned (hq = 0) -- take the reference's three projections.  (Not behind a "some lane is inside" branch: inside pairs
    // are no longer walked first, some lane holds one in nearly every iteration.)
    bool tie = false;
    int k_in = 0;
    {
        const float4 hq = ld4(R + PR_HQ);
        const float g0 = w2 * w2 * hq.x, g1 = w0 * w0 * hq.y, g2 = w1 * w1 * hq.z;
        const float glo = fminf(fminf(g0, g1), g2), gmid = __builtin_amdgcn_fmed3f(g0, g1, g2);
        tie = (bool)((int)is_in & (int)near_tie(glo, gmid, hq.w));
        k_in = g1 == glo ? 1 : g2 == glo ? 2 : 0;
    }
    if (tie) {
        // K.cu:61-110: project on all three edges, keep the nearest (euclid<.., FWD>'s inside branch)
        float best = 100000000.f, bx = 0, by = 0;
#pragma unroll
        for (int K = 0; K < 3; K++) {
            const float4 ea = ld4(R + PR_EDGE + 8 * K);
            const float2 eb = *(const float2*)(R + PR_EDGE + 8 * K + 4);
            const float num = w0 * ea.x + w1 * ea.y + w2 * ea.z - ea.w;
            const float ta = div_by_recip(num, eb.x, eb.y);
            const float tb = 1 - ta;
            float t[3];
            t[K] = ta; t[(K + 1) % 3] = tb; t[(K + 2) % 3] = 0;
            const float u0 = t[0] - w0, u1 = t[1] - w1, u2 = t[2] - w2;
            const float px = u0 * x0 + u1 * x1 + u2 * x2;
            const float py = u0 * y0 + u1 * y1 + u2 * y2;
            const float d2 = px * px + py * py;
            if (d2 < best) { best = d2; bx = px; by = py; }
        }
        narg = (-bx) * bx - by * by;
    } else {
        // K.cu:113-150: which edge (sign pattern of the barycentrics, obtuse-corner override), ONE clamped projection (the clamp
        // leaves an inside pixel's projection on its nearest line as it is: the foot lies on the triangle's boundary)
        const bool over = (xp - ob.x) * ob.z + (yp - ob.y) * ob.w > 0;
        const int sh = (w0 <= 0 ? 2 : 0) | (w1 <= 0 ? 4 : 0) | (w2 <= 0 ? 8 : 0) | (over ? 16 : 0);
        int k = (int)__builtin_amdgcn_ubfe(__float_as_uint(q2.w), (unsigned)sh, 2u);
        k = is_in ? k_in : k;
        const float* E = R + PR_EDGE + 8 * k;
        const float4 ea = ld4(E);
        const float2 eb = *(const float2*)(E + 4);
        const float num = w0 * ea.x + w1 * ea.y + w2 * ea.z - ea.w;
        float ta = div_by_recip(num, eb.x, eb.y);
        float tb = 1 - ta;
        ta = clamp01(ta);
        tb = clamp01(tb);
        // t[k] = ta, t[(k + 1) % 3] = tb, the third 0, by exact 0 / 1 factors (ta, tb lie in [0, 1]: every product and sum is exact)
        const float4 fa = ld4(SEL + 8 * k);
        const float2 fb = *(const float2*)(SEL + 8 * k + 4);
        const float t0 = __builtin_fmaf(tb, fa.w, ta * fa.x), t1 = __builtin_fmaf(tb, fb.x, ta * fa.y), t2 = __builtin_fmaf(tb, fb.y, ta * fa.z);
        const float u0 = t0 - w0, u1 = t1 - w1, u2 = t2 - w2;
        const float dx = u0 * x0 + u1 * x1 + u2 * x2;
        const float dy = u0 * y0 + u1 * y1 + u2 * y2;
        const float d2 = dx * dx + dy * dy;
        narg = is_in ? -d2 : d2;                        // inside: (-dx) dx - dy dy, the same bits
        if ((bool)((int)!is_in & ((int)(d2 >= A.thr) | (int)!has))) return;          // K.cu:402 (has: false for a lane that rides along)
    }
    float4 q6 = ld4(R + PR_XY + 8);                                                  // z2, 1/z0, 1/z1, 1/z2
    float4 tq[(3 * NCH + 3) / 4];
#pragma unroll
    for (int q = 0; q < (3 * NCH + 3) / 4; q++) tq[q] = ld4(R + PR_TEX + 4 * q);
    const float D = sigmoid_from_exp(exp_1ulp(div_by_recip1(narg, A.sigma, U.inv_sigma)));
    // K.cu:409-417, (float)((double)a * (1. - (double)D)): a - a D in ONE rounding is that product rounded once -- the same float
    // except where the double rounding of the reference's form shows (about one product in 2^29)
    s.a = __builtin_fmaf(-s.a, D, s.a);
    // clip / normalise (K.cu:53-58) and depth (K.cu:423) with single-correction quotients (div_by_recip1)
    float c0 = clamp01(w0), c1 = clamp01(w1), c2 = clamp01(w2);
    {
        const float sm = fmaxf(c0 + c1 + c2, 1e-5f);
        float y = __builtin_amdgcn_rcpf(sm);
        y = __builtin_fmaf(__builtin_fmaf(-sm, y, 1.f), y, y);
        c0 = div_by_recip1(c0, sm, y); c1 = div_by_recip1(c1, sm, y); c2 = div_by_recip1(c2, sm, y);
    }
    const float zs = div_by_recip1(c0, z0, q6.y) + div_by_recip1(c1, z1, q6.z) + div_by_recip1(c2, q6.x, q6.w);
    float zp;
    {
        float y = __builtin_amdgcn_rcpf(zs);
        y = __builtin_fmaf(__builtin_fmaf(-zs, y, 1.f), y, y);
        zp = __builtin_fmaf(__builtin_fmaf(-zs, y, 1.f), y, y);
    }
    if (!(zp >= A.near && zp <= A.far)) return;
    const float zn = div_by_recip1(A.far - zp, A.far - A.near, U.inv_fmn);
    const bool up = zn > s.smax;
    const float d = -fabsf(zn - s.smax);
    const float Ex = exp_1ulp(div_by_recip1(d, A.gamma, U.inv_gamma));
    const float hist = up ? Ex : 1.f, wgt = up ? D : Ex * D;
    s.smax = max_finite(zn, s.smax);
    // (the sums as fused multiply-adds: the pair walk folds a pixel's fragments in its own order anyway, see the header)
    s.ssum = __builtin_fmaf(hist, s.ssum, wgt);
    float tex[3 * NCH];
#pragma unroll
    for (int q = 0; q < (3 * NCH + 3) / 4; q++) {
        const float4 t = tq[q];
        tex[4 * q] = t.x;
        if (4 * q + 1 < 3 * NCH) tex[4 * q + 1] = t.y;
        if (4 * q + 2 < 3 * NCH) tex[4 * q + 2] = t.z;
        if (4 * q + 3 < 3 * NCH) tex[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int k = 0; k < NCH; k++) {
        const float col = __builtin_fmaf(c2, tex[2 * NCH + k], __builtin_fmaf(c1, tex[NCH + k], c0 * tex[k]));
        s.c[k] = __builtin_fmaf(wgt, col, hist * s.c[k]);
    }
}

// The rank of this lane when the wave's lanes are sorted by k (0..63), heaviest first, ties by lane: six ballots.  A function of the
// 64 counts alone.
__device__ __forceinline__ int rank_of(int k)
{
    u64_t Gm = ~0ull;
    int greater = 0;
#pragma unroll
    for (int b = 5; b >= 0; b--) {
        const bool mine = (k >> b) & 1;
        const u64_t B = wave_mask(mine);
        const u64_t GB = Gm & B;
        if (!mine) { greater += __popcll(GB); Gm ^= GB; }
        else Gm = GB;
    }
    return greater + bits_below_lane(Gm);
}

// the bits of hm above the smallest position whose upper part holds at most `moved` bits (all of hm when it has no more than that)
__device__ __forceinline__ u64_t upper_bits(u64_t hm, int moved)
{
    if (moved <= 0) return 0ull;
    if (__popcll(hm) <= moved) return hm;
    int p = 0;
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1)
        if (p + sft <= 63 && __popcll(hm >> (p + sft)) > moved) p += sft;
    return p >= 63 ? 0ull : (hm >> (p + 1)) << (p + 1);
}

// ---- spans: which pixels of a tile row entry e does not certainly miss, as ONE run of columns (lane = entry).
// The not-far region of a well-conditioned face is the intersection of the three half-planes w_k >= far[k]; with w_k = A x + B y + C
// its cut with the pixel row y is the x interval  A x >= far[k] - (B y + C)  over the three edges: a lower bound where A > 0, an upper
// bound where A < 0.  In tile columns (pixel centre x_c = (2 c + 1 - IS) / IS, so c = (x IS + IS - 1) / 2) the bound of edge k is
//     c_k(y) = g (far[k] - C - B y) + off = y p + q,    g = (IS / 2) / A,  off = (IS - 1) / 2 - tile's first column,
// one fma per edge and row with p = -B g and q = (far[k] - C) g + off prepared once per edge and entry (one v_rcp_f32 per edge).
// A == 0 needs no case of its own: g is clamped to +-2^40, the bound becomes +-2^40 t and the whole row passes or fails by the sign
// of t = far[k] - (B y + C).  The bounds are rounded OUTWARD, ceil(lo - slack) .. floor(hi + slack), and cut with the entry's pixel
// rect and the tile.
// The slack.  A pixel that matters (d^2 < thr, or inside the face) has w_k - far[k] >= 0.024 |far[k]| on every edge: far[k] carries
// the 1.05 pad on thr, sqrt(1.05) = 1.0247.  The rounding of y p + q is that of t scaled by g -- a few ulp of |B y| + |C| + |far[k]|,
// below 1e-6 / h for a face inside a few image widths (|grad w_k| = 1 / h, h the height over edge k), against the pad's
// 0.024 sqrt(thr) / h: the pad absorbs it whatever g is, for every reach above 1e-4 of the image.  What the pad does not see is the
// rounding in COLUMN units that does not scale with t: v_rcp_f32 (1 ulp), the products forming p and q and the final fma, relative
// to the column coordinate itself, (3 + 1) ulp of at most IS columns = IS 2.4e-7 columns.  PW_SPAN_SLACK = 1/128 of a pixel covers
// that for every image side up to 32768 and costs one extra pixel at an interval end in 1/128 of the cases (tools/pair_stats.py
// counts them).  A pair the spans keep beyond the per-pixel test w_k < far[k] lies beyond the threshold and leaves at the walk's
// exact cut d^2 >= thr.
// Entries the conservative reject does not apply to (not well conditioned: far[k] = -inf) or that are not tame keep their whole pixel
// rect: span = false.
constexpr float PW_SPAN_SLACK = 1.f / 128.f;
struct SpanEdge { float pl, ql, pu, qu; };            // the edge as a lower bound y pl + ql and as an upper bound y pu + qu of the column
__device__ __forceinline__ SpanEdge span_edge(float a, float b, float c, float far, float half_is, float off, bool span)
{
    const float big = 1e9f, gmax = 1099511627776.f;           // 2^40
    const float g = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(a) * half_is, -gmax, gmax);
    const float p = -b * g, q = __builtin_fmaf(far - c, g, off);
    const bool lower = (bool)((int)span & (int)(g > 0)), upper = (bool)((int)span & (int)(g < 0));
    SpanEdge e;
    e.pl = lower ? p : 0.f; e.ql = lower ? q - PW_SPAN_SLACK : -big;
    e.pu = upper ? p : 0.f; e.qu = upper ? q + PW_SPAN_SLACK : big;
    return e;
}
// the 16-bit column mask of one row: [a0, a1] the entry's rect columns within the tile (as floats), y the row's pixel centre
__device__ __forceinline__ unsigned span_row(const SpanEdge (&E)[3], float y, float a0, float a1, bool row_in)
{
    const float lo = fmaxf(fmaxf(__builtin_fmaf(y, E[0].pl, E[0].ql), __builtin_fmaf(y, E[1].pl, E[1].ql)), __builtin_fmaf(y, E[2].pl, E[2].ql));
    const float hi = fminf(fminf(__builtin_fmaf(y, E[0].pu, E[0].qu), __builtin_fmaf(y, E[1].pu, E[1].qu)), __builtin_fmaf(y, E[2].pu, E[2].qu));
    // 0 <= a0 <= 16 and -1 <= a1 <= 15: l in [a0, 16], h in [-1, a1], both within [0, 15] when l <= h
    const int l = (int)__builtin_amdgcn_fmed3f(__builtin_ceilf(lo), a0, 16.f), h = (int)__builtin_amdgcn_fmed3f(__builtin_floorf(hi), -1.f, a1);
    return (bool)((int)row_in & (int)(l <= h)) ? (2u << (h & 15)) - (1u << (l & 15)) : 0u;
}

// ---- the 64 x 64 bit transpose across the wave: lane e comes in with the word S_e, lane p leaves with the word whose bit e is
// bit p of S_e.  Six block-swap stages: at stage s lane L and lane L ^ 2^s trade the off-diagonal blocks of their 2 x 2 block
// matrix -- the lane with bit s clear gives its bits at positions with bit s set and takes the partner's bits at positions with bit
// s clear, moved up by 2^s.  Stage 5 is one v_permlane32_swap of the two halves; stage 4 one v_permlane16_swap per half of the
// word and its rotation by 16 (after it BOTH rows of a pair hold "mine" in the low and "the partner's" in the high 16 bits of the
// wanted result, so one merge serves them); stages 3, 1, 0 fetch the partner's word by DPP (row_ror:8, quad_perm), stage 2 by
// ds_swizzle.  No ballot, no v_writelane.
template <int J>
__device__ __forceinline__ unsigned lane_xor_get(unsigned v)
{
    static_assert(J == 1 || J == 2 || J == 4 || J == 8, "");
    if (J == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);       // quad_perm:[1,0,3,2]
    if (J == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);       // quad_perm:[2,3,0,1]
    if (J == 8) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);      // row_ror:8
    return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);                                        // swizzle: and 0x1f, or 0, xor 4
}
template <int J>
__device__ __forceinline__ unsigned transpose_stage(unsigned own, bool up)
{
    constexpr unsigned M = J == 1 ? 0x55555555u : J == 2 ? 0x33333333u : J == 4 ? 0x0F0F0F0Fu : 0x00FF00FFu;    // positions with bit s clear
    const unsigned t = lane_xor_get<J>(own);
    const unsigned keep = up ? ~M : M;                  // up: this lane's index has bit s set
    return (own & keep) | ((up ? t >> J : t << J) & ~keep);
}
__device__ __forceinline__ u64_t wave_transpose64(u64_t S, int lane)
{
    unsigned lo = (unsigned)S, hi = (unsigned)(S >> 32);
    {
        const auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);     // lo of the lanes 32.. <-> hi of the lanes ..31
        lo = r[0]; hi = r[1];
    }
    {
        const auto a = __builtin_amdgcn_permlane16_swap(lo, __builtin_amdgcn_alignbit(lo, lo, 16), false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(hi, __builtin_amdgcn_alignbit(hi, hi, 16), false, false);
        lo = (a[0] & 0xFFFFu) | (a[1] << 16);
        hi = (b[0] & 0xFFFFu) | (b[1] << 16);
    }
    lo = transpose_stage<8>(lo, (lane & 8) != 0); hi = transpose_stage<8>(hi, (lane & 8) != 0);
    lo = transpose_stage<4>(lo, (lane & 4) != 0); hi = transpose_stage<4>(hi, (lane & 4) != 0);
    lo = transpose_stage<2>(lo, (lane & 2) != 0); hi = transpose_stage<2>(hi, (lane & 2) != 0);
    lo = transpose_stage<1>(lo, (lane & 1) != 0); hi = transpose_stage<1>(hi, (lane & 1) != 0);
    return (u64_t)hi << 32 | lo;
}

// A tile that no face's pixel rect overlaps (ORDER_EMPTY in the launch's order table, sr_raster.hip: sr_order_kernel): its list
// would be empty, so every pixel ends as it starts and every output bit is a function of the launch's scalars.  ONE wave writes the
// whole 16x16 tile; the values are formed with the expressions of pairs_tile_body's set-up and finalise (same operations on the
// same operands: the parent's bits).  With a background argument, a tile wholly inside an image whose side is a multiple of 4
// and 16-byte aligned tensors, lane l stores the pixel quad l & 3 of row l >> 2: one 16-byte store instruction per plane, NCH + 3
// per tile.  Everything else -- ragged edge tiles, other sides, tensors aligned to 4 bytes only, no background argument (the
// background is then what the caller left in soft_colors) -- goes pixel by pixel, four rows per trip as a wave of the tile path.
template <int NCH>
__device__ __forceinline__ void store_empty_tile(const RasterArgs& A, float* __restrict__ aggrs, float* __restrict__ colors, int bn, int tx, int ty, int lane)
{
    const int IS = A.IS, P = IS * IS;
    const int x0 = tx * PW_TILE, y0 = ty * PW_TILE;
    const float ssum = expf(A.eps / A.gamma), smax = A.eps;
    const float one = 1.f;
    const float alpha = (float)(1. - (double)one);
    float* __restrict__ cimg = colors + (size_t)bn * (NCH + 1) * P;
    float* __restrict__ aimg = aggrs + (size_t)bn * 2 * P;
    const bool quads = A.use_bg && x0 + PW_TILE <= IS && y0 + PW_TILE <= IS && (IS & 3) == 0 &&
                       ((((size_t)colors | (size_t)aggrs) & 15) == 0);           // (P is then a multiple of 16: every plane starts aligned)
    if (quads) {
        const int pn = (y0 + (lane >> 2)) * IS + x0 + 4 * (lane & 3);
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const float c = (A.bg[k] * ssum) / ssum;
            *(float4*)(cimg + (size_t)k * P + pn) = make_float4(c, c, c, c);
        }
        *(float4*)(cimg + (size_t)NCH * P + pn) = make_float4(alpha, alpha, alpha, alpha);
        *(float4*)(aimg + pn) = make_float4(ssum, ssum, ssum, ssum);
        *(float4*)(aimg + (size_t)P + pn) = make_float4(smax, smax, smax, smax);
        return;
    }
    for (int r = 0; r < 4; r++) {
        const int px = x0 + (lane & 15), py = y0 + r + 4 * (lane >> 4);
        if (px >= IS || py >= IS) continue;
        const int pn = py * IS + px;
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const float bg = A.use_bg ? A.bg[k] : cimg[(size_t)k * P + pn];
            cimg[(size_t)k * P + pn] = (bg * ssum) / ssum;
        }
        cimg[(size_t)NCH * P + pn] = alpha;
        aimg[pn] = ssum;
        aimg[(size_t)P + pn] = smax;
    }
}

template <int NCH, int SPLIT>
__device__ __forceinline__ void pairs_tile_body(RasterArgs A, float* __restrict__ aggrs, float* __restrict__ colors, PairLds<NCH, SPLIT>& L)
{
    constexpr int RS = PairLds<NCH, SPLIT>::RS;
    constexpr int NW = 4 * SPLIT;                       // waves per tile

    const int IS = A.IS, P = IS * IS;
    const int tiles_x = (IS + PW_TILE - 1) / PW_TILE;
    int bn, tx, ty;
    bool empty;
    tile_of_block(blockIdx.x, gridDim.x, tiles_x, bn, tx, ty, A.order, &empty);      // this launch's own order when the host built one (16x16 tiles)
    // (not the one-team kernel of six channels: with any code behind this branch -- inlined or called, 16-byte stores or not -- the
    // compiler's register budget for it goes from 95 to 97 VGPRs, five resident waves per SIMD to four, and a forced budget spills;
    // its empty tiles keep the tile path, which gives the same bits)
    constexpr bool STORE_ONLY = !(NCH == 6 && SPLIT == 1);
    if (STORE_ONLY && empty) {                          // wave-uniform over the workgroup: nobody is left waiting at a barrier
#if defined(LASR_PW_ABL) && LASR_PW_ABL == 5        // measurement build (wrong output): what the empty tiles cost at all
        return;
#endif
        if (threadIdx.x < 64) store_empty_tile<NCH>(A, aggrs, colors, bn, tx, ty, (int)threadIdx.x);
        return;
    }
    const Modes m = Modes{2, 1, 2, 1, 1};               // LASR's configuration: euclidean, softmax, prod, vertex, double-sided
    if (A.near_far_dev) { A.near = A.near_far_dev[0]; A.far = A.near_far_dev[1]; }
    const int tid = threadIdx.x, wave_all = tid >> 6, lane = tid & 63;
    const int team = SPLIT > 1 ? wave_all >> 2 : 0, wave = wave_all & 3;        // wave: within its team (the pixel rows it owns)
    // wave w takes the rows w, w + 4, w + 8, w + 12 of the tile (16 pixels = 64 bytes each): the four waves of a tile see the same
    // load (they meet at two barriers per chunk), and a store instruction covers whole 64-byte segments
    const int px = tx * PW_TILE + (lane & 15), py = ty * PW_TILE + wave + 4 * (lane >> 4);
    const bool valid = px < IS && py < IS;
    const int pn = py * IS + px;
    const int pxy = valid ? (px | (py << 16)) : (int)0xfffefffe;                // for rect_has (sr_device.h): no rect holds a lane outside the image

    PixState<NCH> s;
    s.a = 1.f;
    s.fbest = -1;
    s.ssum = expf(A.eps / A.gamma); s.smax = A.eps;
#pragma unroll
    for (int k = 0; k < NCH; k++) {
        const float bg = A.use_bg ? A.bg[k] : (valid ? colors[((size_t)bn * (NCH + 1) + k) * P + pn] : 1.f);
        s.c[k] = bg * s.ssum;
    }
    if (SPLIT > 1 && team > 0) {                        // "no fragment yet": merged into team 0's state at the end (merge_partial)
        s.ssum = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; k++) s.c[k] = 0.f;
    }

    if (tid < 32) {
        const int k = tid >> 3, j = tid & 7;          // edge k, slot j: [0..2] = (vertex == k), [3] = (k + 1) % 3 == 0, [4..5] = ... == 1, == 2
        L.sel[tid] = tid >= 24 ? 0.f : j < 3 ? (j == k ? 1.f : 0.f) : (j >= 3 && j < 6 && (j - 3) == (k + 1) % 3) ? 1.f : 0.f;
    }
    // A lane without work rides along the walk on slot 63 (pair_apply: !has) and reads its edge index from that slot's table word.
    // A chunk of fewer than 64 entries leaves the slot as it was: a valid table from an earlier chunk (indices 0..2), or, before the
    // first full chunk, whatever the LDS held -- then the index could be 3 and the 0 / 1 factors were read past sel[23].  The word
    // starts as an empty table (every index 0), and sel is padded, so the rider's reads stay in its own blocks.  Its result is discarded.
    // (Dealt chunks are partial whenever the round's count is no multiple of 64 -- 100 entries are 50 + 50 -- so most tiles never
    // stage the slot at all: the rider then reads this word and whatever else the slot held, all of it inside rec[team].)
    if (tid < SPLIT) L.rec[tid][63 * RS + PR_ETBL] = 0.f;
    // level 0: the groups of 64 consecutive faces whose union rect meets the 16x16 tile (every wave evaluates the same test)
    const int G = groups_of(A.F);
    const short4* __restrict__ grects = A.grects + (size_t)bn * G;
    const int tX0 = tx * PW_TILE, tX1 = tX0 + PW_TILE - 1, tY0 = ty * PW_TILE, tY1 = tY0 + PW_TILE - 1;
    u64_t gmask;
    {
        bool t = false;
        if (lane < G) {
            const short4 q = grects[lane];
            t = !(q.x > tX1 || q.y < tX0 || q.z > tY1 || q.w < tY0);
        }
        gmask = wave_mask(t);
    }
    if (gmask != 0 || G > 64) {
    float xp = pix_center(px, IS);                      // (not const: a lane that walks its partner's share holds the partner's centre here meanwhile)
    float yp = pix_center(IS - 1 - py, IS);
    float yrow[4];                                      // the centres of this wave's four rows (lane 16 j owns row j): wave-uniform
#pragma unroll
    for (int j = 0; j < 4; j++) yrow[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yp), 16 * j));
    const short4* __restrict__ rects = A.rects + (size_t)bn * A.F;
    const float* __restrict__ recs = A.recs + (size_t)bn * A.F * REC;
    const int texstride = A.T * NCH;
    const float* __restrict__ texs = A.textures + (size_t)bn * A.F * texstride;
    const UniRecip U = uni_recip(A);
    const int ok_bit = U.ok ? 32 : 0;
    const float thr_cull = A.thr * 1.10f, thr_far = A.thr * 1.05f;
    // corners of the tile (list building); wave-uniform values the VALU computed (divisions) go back to scalar registers
    auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    const float t_xlo = uni(pix_center(tX0, IS)), t_xhi = uni(pix_center(min(tX1, IS - 1), IS));
    const float t_yhi = uni(pix_center(IS - 1 - tY0, IS)), t_ylo = uni(pix_center(IS - 1 - min(tY1, IS - 1), IS));
    int g_next = 64, g_mask0 = 0;
    bool more = true;
    while (more) {                                    // one round unless the tile meets more than PW_LIST - 256 faces
        // ---- ordered list of the faces that reach the tile: four touched groups per step, one per wave
        int count = 0, flip = 0, base = -1;
        for (;;) {
            if (gmask == 0) {
                if (g_next >= G) { more = false; break; }
                g_mask0 = g_next;
                bool t = false;
                if (g_next + lane < G) {
                    const short4 q = grects[g_next + lane];
                    t = !(q.x > tX1 || q.y < tX0 || q.z > tY1 || q.w < tY0);
                }
                gmask = wave_mask(t);
                g_next += 64;
                continue;
            }
            u64_t mm = gmask;
            int mine_g = -1, last_g = 0;
#pragma unroll
            for (int k = 0; k < NW; k++) {
                if (mm) {
                    const int bit = __builtin_ctzll(mm);
                    mm &= mm - 1;
                    if (k == wave_all) mine_g = g_mask0 + bit;
                    last_g = g_mask0 + bit;
                }
            }
            const int first_g = g_mask0 + __builtin_ctzll(gmask);
            if (base < 0) base = first_g * GROUP;
            if (count + 64 * NW > PW_LIST || (last_g + 1) * GROUP - base > 65536) break;  // walk what we have, then continue
            gmask = mm;
            const int f = mine_g * GROUP + lane;
            bool hit = false;
            if (mine_g >= 0 && f < A.F) {
                const short4 q = rects[f];
                hit = !(q.x > tX1 || q.y < tX0 || q.z > tY1 || q.w < tY0);
                if (hit) hit = reaches_block(recs + (size_t)f * REC, t_xlo, t_xhi, t_ylo, t_yhi, thr_cull);
            }
            const u64_t mask = wave_mask(hit);
            if (lane == 0) L.wcnt[flip][wave_all] = __popcll(mask);
            __syncthreads();
            int before = 0, step_total = 0;
#pragma unroll
            for (int k = 0; k < NW; k++) {
                const int ck = L.wcnt[flip][k];
                before += k < wave_all ? ck : 0;
                step_total += ck;
            }
            if (hit) L.list[count + before + bits_below_lane(mask)] = (unsigned short)(f - base);
            count += step_total;
            flip ^= 1;
        }
        if (base < 0) base = 0;
        __syncthreads();

        float* const Lrec = L.rec[team];
        // the round's chunks (chunk_count / chunk_size / chunk_pos above); quotient and remainder once per round, in scalar registers
        const int cnt = __builtin_amdgcn_readfirstlane(count);
        const int nch = chunk_count(cnt);
        const int n_lo = nch ? cnt / nch : 0, n_rem = nch ? cnt % nch : 0;
        for (int cb = 0; cb < nch; cb += SPLIT) {       // team t takes the chunks t, t + SPLIT, ...: same trip count, same barriers
            const int c = cb + team;                    // (a trip past the last chunk runs with n = 0)
            const int n = c < nch ? n_lo + (c < n_rem ? 1 : 0) : 0;            // chunk_size(cnt, nch, c)
            const int lpos = c + lane * nch;                                   // chunk_pos(nch, c, lane)
            // ---- stage: lane = entry, every wave a quarter of the record's source quads (all loads of a chunk in flight at once)
            int ca0 = PW_TILE, ca1 = -1, rm = 0;      // the entry's rect: its columns [ca0, ca1] within the tile, its rows as a 16-bit mask
            if (lane < n) {
                const int fn = base + (int)L.list[lpos];
                {
                    const short4 q = rects[fn];       // x0, x1, row0, row1 (empty: 32767, -1, 32767, -1)
                    ca0 = min(max((int)q.x - tX0, 0), PW_TILE); ca1 = max(min((int)q.y - tX0, PW_TILE - 1), -1);
                    const int b0 = max((int)q.z - tY0, 0), b1 = min((int)q.w - tY0, PW_TILE - 1);
                    if (b0 <= b1) rm = (2 << b1) - (1 << b0);
                }
                const float4* __restrict__ src = (const float4*)(recs + (size_t)fn * REC);
                const float* __restrict__ ta = texs + (size_t)fn * texstride;
                float* dst = Lrec + lane * RS;
                float tv[(3 * NCH + 3) / 4];
#pragma unroll
                for (int i = 0; i < (3 * NCH + 3) / 4; i++) tv[i] = wave + 4 * i < 3 * NCH ? ta[wave + 4 * i] : 0.f;
                const bool well = (__float_as_int(((const float*)src)[R_FLAGS]) & 16) != 0;
                if (wave == 0) stage_quads<0, 3>(src, dst, thr_far, well);
                else if (wave == 1) stage_quads<3, 6>(src, dst, thr_far, well);
                else if (wave == 2) stage_quads<6, 9>(src, dst, thr_far, well);
                else {
                    stage_quads<9, 11>(src, dst, thr_far, well);
                    // the obtuse corner's operands (see the layout above)
                    const float* f = (const float*)src;
                    const int fl = __float_as_int(f[R_FLAGS]);
                    const int c = (fl & 1) ? 0 : (fl & 2) ? 1 : 2, o = c == 0 ? 2 : c - 1;
                    const float xc = f[R_FACE + 3 * c], yc = f[R_FACE + 3 * c + 1], xo = f[R_FACE + 3 * o], yo = f[R_FACE + 3 * o + 1];
                    *(float4*)(dst + PR_OBT) = make_float4(xc, yc, xo - xc, yo - yc);
                    const unsigned tb = (fl & 1) ? edge_table(1) : (fl & 2) ? edge_table(2) : (fl & 4) ? edge_table(4) : edge_table(0);
                    dst[PR_ETBL] = __uint_as_float(tb);
                }
#pragma unroll
                for (int i = 0; i < (3 * NCH + 3) / 4; i++)
                    if (wave + 4 * i < 3 * NCH) dst[PR_TEX + wave + 4 * i] = tv[i];
            }
            __syncthreads();                            // the staged records, before anybody reads a slot another wave wrote

            // ---- spans: lane = entry.  The columns of this wave's four rows that the entry does not certainly miss (span_edge /
            // span_row above) as the word S: bit 16 j + c = row wave + 4 j, column c of the tile.  Entries that are not tame (or every
            // entry of a launch whose uniforms are not safe for the reciprocal arithmetic) get no bit: they are the slow entries below.
            u64_t mn = 0;                               // per pixel lane: the near pairs of the chunk's tame entries
            u64_t slow_mask = 0;                        // wave-uniform: the chunk's entries that are not tame
#if !(defined(LASR_PW_ABL) && LASR_PW_ABL == 2)     // (2: measurement build, list + stage only)
            {
                u64_t S = 0;
                bool tame_e = false;
                if (lane < n) tame_e = (__float_as_int(Lrec[lane * RS + PR_FLAGS]) & ok_bit) != 0;
                if (tame_e) {
                    const float* R = Lrec + lane * RS;
                    const float4 q0 = ld4(R), q1 = ld4(R + 4), q2 = ld4(R + 8), q3 = ld4(R + PR_HK2);
                    const int fl = __float_as_int(q2.y);
                    const bool span = (fl & 16) != 0;                         // else: the conservative reject does not apply, the rect as it is
                    const float half_is = 0.5f * (float)IS, off = 0.5f * (float)(IS - 1) - (float)tX0;
                    const SpanEdge E[3] = {span_edge(q0.x, q0.y, q0.z, q3.x, half_is, off, span),
                                           span_edge(q0.w, q1.x, q1.y, q3.y, half_is, off, span),
                                           span_edge(q1.z, q1.w, q2.x, q3.z, half_is, off, span)};
                    const float a0 = (float)ca0, a1 = (float)ca1;
                    unsigned m[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) m[j] = span_row(E, yrow[j], a0, a1, ((rm >> (wave + 4 * j)) & 1) != 0);
                    S = (u64_t)(m[2] | m[3] << 16) << 32 | (m[0] | m[1] << 16);
                }
                // ---- transpose: pixel lane p = 16 j + c gets the word whose bit e is entry e's bit for that pixel
                slow_mask = wave_mask((bool)((int)(lane < n) & (int)!tame_e));
                const u64_t T = wave_transpose64(S, lane);
                mn = valid ? T : 0ull;
            }
#endif

#if defined(LASR_PW_ABL) && LASR_PW_ABL == 1        // measurement build: no walk
            s.a += (float)__popcll(mn); mn = 0;
#endif
#if defined(LASR_PW_ABL) && LASR_PW_ABL == 3        // measurement build: no balance (every lane its own pairs)
            const bool no_steal = true;
#else
            const bool no_steal = false;
#endif
            // ---- balance: rank the lanes by their pair count (heaviest first), partner rank r with rank 63 - r
            const int kmine = min((int)__popcll(mn), 63);
            const int rank = rank_of(kmine);
            const int id_at_rank = __builtin_amdgcn_ds_permute(rank << 2, lane);                 // lane r: the lane of rank r
            const int partner = __builtin_amdgcn_ds_bpermute((63 - rank) << 2, id_at_rank);
            const int kpart = __builtin_amdgcn_ds_bpermute(partner << 2, kmine);
            const unsigned pmn_lo = (unsigned)__builtin_amdgcn_ds_bpermute(partner << 2, (int)(unsigned)mn);
            const unsigned pmn_hi = (unsigned)__builtin_amdgcn_ds_bpermute(partner << 2, (int)(unsigned)(mn >> 32));
            float xq = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(xp)));
            float yq = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(yp)));
            const bool heavy = rank < 32;
            // the heavier partner's mask and the number of its pairs that change hands (both partners compute the same); any pair may
            // move: whether it is an inside pair shows in its own barycentrics, at the heavier lane's pixel centre
            const u64_t hm = heavy ? mn : ((u64_t)pmn_hi << 32 | pmn_lo);
            const int moved = (heavy ? kmine - kpart : kpart - kmine) >> 1;
            u64_t st = 0;                                                       // light lane: the pairs it takes over
            bool gave = false;
            if (moved > 0 && !no_steal) {
                const u64_t top = upper_bits(hm, moved);
                if (heavy) { mn ^= top; gave = top != 0; }
                else st = top;
            }

            // ---- walk: every lane pops its run of pairs, then the partner's share, one pair per iteration; a lane moves on to the
            // stolen run inside the (rarely entered) region below
            bool in_stolen = false;
            PixState<NCH> saved = s;
            u64_t cur = mn;
            u64_t more_m = ~0ull;
            auto advance = [&]() {
                if ((wave_mask(cur == 0) & more_m) != 0) {
                    if ((bool)((int)(cur == 0) & (int)(st != 0))) {                 // the partner's share, into a fresh partial state
                        saved = s;
                        s.a = 1.f; s.ssum = 0.f; s.smax = A.eps;
#pragma unroll
                        for (int k = 0; k < NCH; k++) s.c[k] = 0.f;
                        { const float ox = xp, oy = yp; xp = xq; yp = yq; xq = ox; yq = oy; }     // the two centres trade places (and back after the walk)
                        cur = st; st = 0; in_stolen = true;
                    }
                    more_m = wave_mask(st != 0);
                }
            };
            advance();
            if (wave_mask(cur != 0) != 0) do {
                // (no divergent region around the pair: a lane without work rides along the outside branch on entry 63's slot and
                // leaves at the threshold cut -- the instructions are issued for the wave either way)
                const bool has = cur != 0;
                const int e = __builtin_ctzll(cur | (1ull << 63));
                cur &= cur - 1;
                pair_apply<NCH>(A, U, Lrec + e * RS, L.sel, has, xp, yp, s);
                advance();
            } while (wave_mask(cur != 0) != 0);
            // ---- merge the partial states into their pixels
            float pa = s.a, pm = s.smax, ps = s.ssum, pc[NCH];
#pragma unroll
            for (int k = 0; k < NCH; k++) pc[k] = s.c[k];
            if (in_stolen) { s = saved; xp = xq; yp = yq; }
            if (wave_mask(gave) != 0) {
                pa = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(pa)));
                pm = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(pm)));
                ps = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(ps)));
#pragma unroll
                for (int k = 0; k < NCH; k++) pc[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(pc[k])));
                if (gave) merge_partial<NCH>(s, pa, pm, ps, pc, A.gamma, U.inv_gamma);
            }
            // ---- the chunk's slow pairs (records that are not tame): wave-uniform entry, generic arithmetic, for the pixels of the entry's
            // exact rect (the staged rect words: no mask is carried across the walk for them)
            for (u64_t sm = slow_mask; sm != 0; sm &= sm - 1) {
                const int e = __builtin_ctzll(sm);
                const PairRecView R{Lrec + e * RS};
                if (rect_has(__float_as_int(Lrec[e * RS + PR_BB]), __float_as_int(Lrec[e * RS + PR_BBE]), pxy)) {
                    float w0, w1, w2;
                    barycentric(R, xp, yp, w0, w1, w2);
                    forward_face<true, false, NCH>(A, m, R, Lrec + e * RS + PR_TEX, 0, 0, xp, yp, w0, w1, w2, s, U);
                }
            }
            __syncthreads();                            // the slots are rewritten by the next chunk
        }
    }
    }   // tile meets at least one group

    if (SPLIT > 1) {
        // ---- the teams' partial states meet: team t >= 1 leaves its state in LDS, team 0 folds them in (team order) and finalises
        const int pl = wave * 64 + lane;                    // the pixel's slot: same (wave, lane) -> pixel mapping in every team
        if (team > 0) {
            float* o = L.merge + (size_t)(team - 1) * (3 + NCH) * 256 + pl;
            o[0] = s.a; o[256] = s.smax; o[512] = s.ssum;
#pragma unroll
            for (int k = 0; k < NCH; k++) o[(3 + k) * 256] = s.c[k];
        }
        __syncthreads();
        if (team > 0) return;
        const float inv_gamma = 1.f / A.gamma;
#pragma unroll
        for (int t = 1; t < SPLIT; t++) {
            const float* o = L.merge + (size_t)(t - 1) * (3 + NCH) * 256 + pl;
            float pc[NCH];
#pragma unroll
            for (int k = 0; k < NCH; k++) pc[k] = o[(3 + k) * 256];
            merge_partial<NCH>(s, o[0], o[256], o[512], pc, A.gamma, inv_gamma);
        }
    }
    if (!valid) return;
    // ---- finalise (K.cu:458-482); the pixel's index once more from the packed coordinates (one register across the walk, not two)
    const int pe = (int)((unsigned)pxy >> 16) * IS + (pxy & 0xffff);
    colors[((size_t)bn * (NCH + 1) + NCH) * P + pe] = (float)(1. - (double)s.a);
#pragma unroll
    for (int k = 0; k < NCH; k++) colors[((size_t)bn * (NCH + 1) + k) * P + pe] = s.c[k] / s.ssum;
    aggrs[((size_t)bn * 2 + 0) * P + pe] = s.ssum;
    aggrs[((size_t)bn * 2 + 1) * P + pe] = s.smax;
}

// six / nine channels: the compiler's own register budget (95 / 112 VGPRs)
template <int NCH>
__global__ __launch_bounds__(256) void sr_forward_pairs_kernel(RasterArgs A, float* __restrict__ aggrs, float* __restrict__ colors)
{
    __shared__ __attribute__((aligned(16))) PairLds<NCH, 1> L;
    pairs_tile_body<NCH, 1>(A, aggrs, colors, L);
}
// three channels: no occupancy request (87 VGPRs = 5 waves per SIMD; six / seven forced were slower, profiles/experiments/README.md)
__global__ __launch_bounds__(256)
void sr_forward_pairs3_kernel(RasterArgs A, float* __restrict__ aggrs, float* __restrict__ colors)
{
    __shared__ __attribute__((aligned(16))) PairLds<3, 1> L;
    pairs_tile_body<3, 1>(A, aggrs, colors, L);
}
// two / four teams of four waves per tile (512 / 1024 threads): launches bound by the heaviest tile's chain of phases, not by throughput
template <int NCH, int SPLIT>
__global__ __launch_bounds__(256 * SPLIT) void sr_forward_pairs_teams_kernel(RasterArgs A, float* __restrict__ aggrs, float* __restrict__ colors)
{
    __shared__ __attribute__((aligned(16))) PairLds<NCH, SPLIT> L;
    pairs_tile_body<NCH, SPLIT>(A, aggrs, colors, L);
}

}  // namespace lasr
