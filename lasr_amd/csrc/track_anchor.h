// track_anchor.h -- the surface anchoring shared by tracks.hip (lasr_track_anchor / lasr_track_project) and reproj.hip
// (lasr_reproj_pixels): face frame, the point of a face, the raster's named face and step 3 of lasr_track_anchor's contract in
// include/lasr_ops.h.  Both translation units are built with the pattern rule's flags (-ffp-contract=off), so a pixel centre
// anchored by either kernel gets the same bits.
#pragma once

namespace lasr {

struct TrackFace { float ax, ay, az, e1x, e1y, e1z, e2x, e2y, e2z, nx, ny, nz; };

// Corner 0, the two EDGE vectors and their cross product of face (i0, i1, i2) in the vertex array v of one frame.
__device__ __forceinline__ TrackFace track_face(const float* __restrict__ v, int i0, int i1, int i2)
{
    TrackFace t;
    t.ax = v[i0 * 3]; t.ay = v[i0 * 3 + 1]; t.az = v[i0 * 3 + 2];
    t.e1x = v[i1 * 3] - t.ax; t.e1y = v[i1 * 3 + 1] - t.ay; t.e1z = v[i1 * 3 + 2] - t.az;
    t.e2x = v[i2 * 3] - t.ax; t.e2y = v[i2 * 3 + 1] - t.ay; t.e2z = v[i2 * 3 + 2] - t.az;
    t.nx = t.e1y * t.e2z - t.e1z * t.e2y;
    t.ny = t.e1z * t.e2x - t.e1x * t.e2z;
    t.nz = t.e1x * t.e2y - t.e1y * t.e2x;
    return t;
}

// P = c0 V0 + c1 V1 + c2 V2 written on the edges: V0 + c1 e1 + c2 e2 (c0 = 1 - c1 - c2).
__device__ __forceinline__ void track_point(const TrackFace& t, float c1, float c2, float& px, float& py, float& pz)
{
    px = t.ax + (c1 * t.e1x + c2 * t.e2x);
    py = t.ay + (c1 * t.e1y + c2 * t.e2y);
    pz = t.az + (c1 * t.e1z + c2 * t.e2z);
}

// The pixel coordinates of the camera-space point P (P.z > 0) under k = fx fy px py: what lasr_track_project writes.
__device__ __forceinline__ void track_pinhole(const float4 k, float px, float py, float pz, float& u, float& v)
{
    u = k.x * px / pz + k.z;
    v = k.y * py / pz + k.w;
}

__device__ __forceinline__ float track_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// The face plane 1 of the raster names at (row, col), or -1 (also for a value outside [0, F)).
__device__ __forceinline__ int track_named(const float* __restrict__ plane, int IS, int row, int col, int F)
{
    const float fo = plane[(size_t)row * IS + col];
    return (fo >= 0.f && fo < (float)F) ? (int)fo : -1;
}

// Step 3 of lasr_track_anchor: the barycentrics c1, c2 (c0 = 1 - c1 - c2) of the point of face tf that the camera ray through
// (u, v) meets, k = fx fy px py.  false: a zero-area face, det = 0 or a barycentric that is not finite (c1, c2 untouched).
__device__ __forceinline__ bool track_barycentrics(const TrackFace& tf, const float4 k, float u, float v, float& c1, float& c2)
{
    // Moeller-Trumbore along d = ((u - px)/fx, (v - py)/fy, 1) from the ray's point at V0's depth, O = V0.z d, so that
    // tvec = O - V0 is of the size of the face and not of its distance (the barycentrics do not depend on the origin)
    const float dx = (u - k.z) / k.x, dy = (v - k.w) / k.y, dz = 1.f;
    const float pvx = dy * tf.e2z - dz * tf.e2y, pvy = dz * tf.e2x - dx * tf.e2z, pvz = dx * tf.e2y - dy * tf.e2x;
    const float det = tf.e1x * pvx + tf.e1y * pvy + tf.e1z * pvz;
    const float tx = dx * tf.az - tf.ax, ty = dy * tf.az - tf.ay, tz = 0.f;
    const float qx = ty * tf.e1z - tz * tf.e1y, qy = tz * tf.e1x - tx * tf.e1z, qz = tx * tf.e1y - ty * tf.e1x;
    const float b1 = (tx * pvx + ty * pvy + tz * pvz) / det;
    const float b2 = (dx * qx + dy * qy + dz * qz) / det;
    const float nn = tf.nx * tf.nx + tf.ny * tf.ny + tf.nz * tf.nz;
    if (!(nn > 0.f && det != 0.f && fabsf(b1) < 3.4e38f && fabsf(b2) < 3.4e38f)) return false;
    const float a0 = track_clamp01(1.f - b1 - b2), a1 = track_clamp01(b1), a2 = track_clamp01(b2);
    const float s = a0 + a1 + a2;                                    // >= 1/3: the largest of three numbers that sum to 1
    c1 = a1 / s;
    c2 = a2 / s;
    return true;
}

}  // namespace lasr
