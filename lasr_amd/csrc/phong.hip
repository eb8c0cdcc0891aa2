// phong.hip -- the shading and blend pass of extract.py --render and scripts/eval_mesh.py --render (lasr_amd/phong.py assembles
// the scene).  It restates pytorch3d 0.4.0's SoftPhongShader (phong_shading + softmax_rgb_blend) under the reference's one
// configuration: OrthographicCameras(), PointLights() at (0, 1, 0) with white ambient / diffuse / specular, default materials
// (shininess 64) and BlendParams (sigma = gamma = 1e-4), K = 1 face per pixel, blur radius 0.  Visibility comes from the hard-mode
// rasteriser (lasr_sr_forward_bg, func_id_rgb = func_id_alpha = 0): plane 1 of its aggrs_info names the nearest face of every
// pixel.  One thread per output pixel; the RGBA result is one float4 store.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "ops_common.h"

namespace lasr {

constexpr float PHONG_EPS_AREA = 1e-8f;       // pytorch3d's kEpsilon (barycentric denominator, degenerate edges)
constexpr float PHONG_SIGMA = 1e-4f, PHONG_GAMMA = 1e-4f, PHONG_ZNEAR = 1.f, PHONG_ZFAR = 100.f, PHONG_BLEND_EPS = 1e-10f;

// (p - a) x (b - a) in 2-D: pytorch3d's EdgeFunctionForward(p, a, b)
__device__ __forceinline__ float phong_edge(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// squared distance from p to segment a-b (PointLineDistanceForward)
__device__ __forceinline__ float phong_seg_d2(float px, float py, float ax, float ay, float bx, float by)
{
    const float ex = bx - ax, ey = by - ay;
    const float l2 = ex * ex + ey * ey;
    if (l2 <= PHONG_EPS_AREA) return (px - bx) * (px - bx) + (py - by) * (py - by);
    float t = (ex * (px - ax) + ey * (py - ay)) / l2;
    t = fminf(fmaxf(t, 0.f), 1.f);
    const float dx = ax + t * ex - px, dy = ay + t * ey - py;
    return dx * dx + dy * dy;
}

// x / max(|x|, 1e-6): torch.nn.functional.normalize
__device__ __forceinline__ void phong_normalize(float& x, float& y, float& z)
{
    const float n = fmaxf(sqrtf(x * x + y * y + z * z), 1e-6f);
    x /= n;
    y /= n;
    z /= n;
}

// Vertex record [12 floats]: position x y z, 0 | unit normal x y z, 0 | colour r g b, 0.
__global__ __launch_bounds__(256) void phong_shade_kernel(const float4* __restrict__ vert_rec, const int4* __restrict__ faces,
                                                          const float* __restrict__ raster, float4* __restrict__ out, int V, int F,
                                                          int S, float bg_r, float bg_g, float bg_b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int P = S * S;
    if (i >= P) return;
    const int n = blockIdx.y;
    const int r = i / S, c = i - r * S;
    float4 o = make_float4(bg_r, bg_g, bg_b, 0.f);
    const float fo = raster[((size_t)n * 2 + 1) * P + i];
    if (fo >= 0.f && fo < (float)F) {
        const int4 fi = faces[(int)fo];
        if ((unsigned)fi.x < (unsigned)V && (unsigned)fi.y < (unsigned)V && (unsigned)fi.z < (unsigned)V) {
            const float xp = 1.f - (float)(2 * c + 1) / (float)S;       // pytorch3d NDC of the pixel centre: +X left, +Y up
            const float yp = 1.f - (float)(2 * r + 1) / (float)S;
            const float4* vr = vert_rec + (size_t)n * V * 3;
            const float4 p0 = vr[(size_t)fi.x * 3], n0 = vr[(size_t)fi.x * 3 + 1], t0 = vr[(size_t)fi.x * 3 + 2];
            const float4 p1 = vr[(size_t)fi.y * 3], n1 = vr[(size_t)fi.y * 3 + 1], t1 = vr[(size_t)fi.y * 3 + 2];
            const float4 p2 = vr[(size_t)fi.z * 3], n2 = vr[(size_t)fi.z * 3 + 1], t2 = vr[(size_t)fi.z * 3 + 2];
            // BarycentricCoordsForward: no perspective correction under an orthographic camera
            const float area = phong_edge(p2.x, p2.y, p0.x, p0.y, p1.x, p1.y) + PHONG_EPS_AREA;
            const float w0 = phong_edge(xp, yp, p1.x, p1.y, p2.x, p2.y) / area;
            const float w1 = phong_edge(xp, yp, p2.x, p2.y, p0.x, p0.y) / area;
            const float w2 = phong_edge(xp, yp, p0.x, p0.y, p1.x, p1.y) / area;
            const float px = w0 * p0.x + w1 * p1.x + w2 * p2.x;
            const float py = w0 * p0.y + w1 * p1.y + w2 * p2.y;
            const float pz = w0 * p0.z + w1 * p1.z + w2 * p2.z;
            float nx = w0 * n0.x + w1 * n1.x + w2 * n2.x;
            float ny = w0 * n0.y + w1 * n1.y + w2 * n2.y;
            float nz = w0 * n0.z + w1 * n1.z + w2 * n2.z;
            phong_normalize(nx, ny, nz);
            float lx = -px, ly = 1.f - py, lz = -pz;                     // PointLights location (0, 1, 0)
            phong_normalize(lx, ly, lz);
            float vx = -px, vy = -py, vz = -pz;                          // camera centre at the origin
            phong_normalize(vx, vy, vz);
            const float ndl = nx * lx + ny * ly + nz * lz;
            const float diffuse = fmaxf(ndl, 0.f);
            float spec = 0.f;
            if (ndl > 0.f) {
                const float rx = 2.f * ndl * nx - lx, ry = 2.f * ndl * ny - ly, rz = 2.f * ndl * nz - lz;
                float a = fmaxf(vx * rx + vy * ry + vz * rz, 0.f);
                a *= a;                                                  // a^64 by six squarings
                a *= a;
                a *= a;
                a *= a;
                a *= a;
                a *= a;
                spec = a;
            }
            const float k = 1.f + diffuse;                               // ambient 1 + diffuse
            const float cr = k * (w0 * t0.x + w1 * t1.x + w2 * t2.x) + spec;
            const float cg = k * (w0 * t0.y + w1 * t1.y + w2 * t2.y) + spec;
            const float cb = k * (w0 * t0.z + w1 * t1.z + w2 * t2.z) + spec;
            // softmax_rgb_blend for one face: prob from the squared distance to the nearest edge (the pixel is inside)
            const float d2 = fminf(fminf(phong_seg_d2(xp, yp, p0.x, p0.y, p1.x, p1.y), phong_seg_d2(xp, yp, p1.x, p1.y, p2.x, p2.y)),
                                   phong_seg_d2(xp, yp, p2.x, p2.y, p0.x, p0.y));
            const float prob = 1.f / (1.f + expf(-d2 / PHONG_SIGMA));
            const float z_inv = (PHONG_ZFAR - pz) / (PHONG_ZFAR - PHONG_ZNEAR);
            const float m = fmaxf(z_inv, PHONG_BLEND_EPS);
            const float w = prob * expf((z_inv - m) / PHONG_GAMMA);
            const float delta = fmaxf(expf((PHONG_BLEND_EPS - m) / PHONG_GAMMA), PHONG_BLEND_EPS);
            const float den = w + delta;
            o.x = (w * cr + delta * bg_r) / den;
            o.y = (w * cg + delta * bg_g) / den;
            o.z = (w * cb + delta * bg_b) / den;
            o.w = prob;
        }
    }
    out[(size_t)n * P + i] = o;
}

}  // namespace lasr

extern "C" int lasr_phong_shade(const float* vert_rec, const int* faces, const float* raster, const float* background, float* out,
                                int N, int V, int F, int S, void* hip_stream)
{
    if (N < 0 || N > 65535 || V < 1 || F < 1 || S < 1 || S > LASR_PHONG_MAX_SIZE) return LASR_E_BADARG;
    if ((long long)V * 12 > 0x7fffffffLL || (long long)F * 4 > 0x7fffffffLL) return LASR_E_BADARG;
    if (N == 0) return LASR_OK;
    if (!vert_rec || !faces || !raster || !background || !out) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const long long P = (long long)S * S;
    LASR_LAUNCH(K_PHONG_SHADE, lasr::phong_shade_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)N), dim3(256), 0,
                (const float4*)vert_rec, (const int4*)faces, raster, (float4*)out, V, F, S, background[0], background[1], background[2]);
    return launch_ok();
}
