// rig.hip -- the per-vertex and per-frame work of scripts/export_gltf.py (lasr_amd/nnutils/rig.py assembles the file's arrays,
// lasr_amd/ext_utils/gltf.py writes them): a reconstruction as a skinned, animated glTF asset.  This is the project's own
// addition; the reference has no exporter, and the definition is the one of include/lasr_ops.h and DESIGN.md section 4.12.
// Four kernels: the k largest skinning weights of every vertex (glTF stores 4-wide influence sets, LASR's are dense), the
// rotation keys as sign-continuous unit quaternions, glTF's own skinning of the packed arrays (what a viewer will show), and
// the per-frame deviation of that from the full-weight blend.  No atomics anywhere: two runs give the same bits.
// Compiled with -ffp-contract=off (FLAGS of the pattern rule): every product and sum below rounds once, in the order written,
// which is the order tests/rig_restated.py restates.
#include <stdint.h>

#include "../../include/lasr_ops.h"
#include "host_common.h"

namespace lasr {

// One thread per vertex.  The k best (weight, bone) pairs are kept sorted in registers; bone j enters below every pair that is
// at least as heavy, so a larger weight comes first and, among equal weights, the lower bone index.
template <int KI>
__global__ __launch_bounds__(256) void rig_pack_kernel(const float* __restrict__ skin, int J, int V, unsigned char* __restrict__ joints,
                                                       float* __restrict__ weights, float* __restrict__ dropped)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float sw[KI];
    int sj[KI];
#pragma unroll
    for (int p = 0; p < KI; p++) { sw[p] = -1.f; sj[p] = -1; }             // below every weight a skin holds (they are >= 0)
    for (int j = 0; j < J; j++) {
        float cw = skin[(size_t)j * V + v];                                 // column read: consecutive threads, consecutive floats
        int cj = j;
        bool in = false;                                                    // once placed, the pairs behind shift down by one
#pragma unroll
        for (int p = 0; p < KI; p++) {
            if (in || cw > sw[p]) {                                         // strict: an equal, earlier bone stays in front
                in = true;
                const float tw = sw[p]; const int tj = sj[p];
                sw[p] = cw; sj[p] = cj;
                cw = tw; cj = tj;
            }
        }
    }
    unsigned long long chosen = 0ull;
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < KI; p++) {
        if (sj[p] >= 0) { chosen |= 1ull << sj[p]; s += sw[p]; }            // selection order
    }
    float d = 0.f;
    for (int j = 0; j < J; j++) {
        if (!((chosen >> j) & 1ull)) d += skin[(size_t)j * V + v];          // ascending bone order
    }
    dropped[v] = d;
#pragma unroll
    for (int p = 0; p < KI; p++) {
        float w = (sj[p] >= 0 && s > 0.f) ? sw[p] / s : 0.f;
        int j = w > 0.f ? sj[p] : 0;                                        // a zero weight carries joint 0
        if (p == 0 && !(s > 0.f)) w = 1.f;                                  // nothing to blend: bound to joint 0 alone
        joints[(size_t)v * KI + p] = (unsigned char)j;
        weights[(size_t)v * KI + p] = w;
    }
}

// One thread per bone walks the frames in order.  q = unit quaternion (x, y, z, w) of M = R^T (R holds row-vector matrices:
// p' = p R), by Shepperd's method: the largest of the trace and the three diagonal entries picks the component that is
// computed from a square root, so the divisor is at least 1/2 for a rotation.  Sign: q_0.w >= 0, q_t . q_{t-1} >= 0.
__global__ __launch_bounds__(64) void rig_quats_kernel(const float* __restrict__ R, int T, int K, float* __restrict__ quat)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= K) return;
    float px = 0.f, py = 0.f, pz = 0.f, pw = 0.f;
    for (int t = 0; t < T; t++) {
        const float* r = R + ((size_t)t * K + b) * 9;
        // m[i][j] = r[j][i]
        const float m00 = r[0], m01 = r[3], m02 = r[6];
        const float m10 = r[1], m11 = r[4], m12 = r[7];
        const float m20 = r[2], m21 = r[5], m22 = r[8];
        const float tr = (m00 + m11) + m22;
        float x, y, z, w;
        if (tr >= m00 && tr >= m11 && tr >= m22) {
            w = 0.5f * sqrtf(1.f + tr);
            const float f = 0.25f / w;
            x = (m21 - m12) * f; y = (m02 - m20) * f; z = (m10 - m01) * f;
        } else if (m00 >= m11 && m00 >= m22) {
            x = 0.5f * sqrtf(((1.f + m00) - m11) - m22);
            const float f = 0.25f / x;
            w = (m21 - m12) * f; y = (m01 + m10) * f; z = (m02 + m20) * f;
        } else if (m11 >= m22) {
            y = 0.5f * sqrtf(((1.f + m11) - m00) - m22);
            const float f = 0.25f / y;
            w = (m02 - m20) * f; x = (m01 + m10) * f; z = (m12 + m21) * f;
        } else {
            z = 0.5f * sqrtf(((1.f + m22) - m00) - m11);
            const float f = 0.25f / z;
            w = (m10 - m01) * f; x = (m02 + m20) * f; y = (m12 + m21) * f;
        }
        const float n = sqrtf(((x * x + y * y) + z * z) + w * w);
        x = x / n; y = y / n; z = z / n; w = w / n;
        const bool flip = t == 0 ? (w < 0.f) : ((((x * px + y * py) + z * pz) + w * pw) < 0.f);
        if (flip) { x = -x; y = -y; z = -z; w = -w; }
        float* q = quat + ((size_t)t * K + b) * 4;
        q[0] = x; q[1] = y; q[2] = z; q[3] = w;
        px = x; py = y; pz = z; pw = w;
    }
}

#define RIG_LDS_BONES (LASR_RIG_MAX_BONES + 1)

// glTF's skinning of the arrays that go into the file: one block serves 256 vertices of one frame; the frame's K matrices are
// rebuilt from its quaternions (column convention, the standard formula, no renormalisation: a viewer does none) into LDS.
// out = M_0 (sum_i weights_i M_{joints_i + 1} [p; 1]), summed in the order the influences are stored.
__global__ __launch_bounds__(256) void rig_skin_kernel(const float* __restrict__ rest, const unsigned char* __restrict__ joints,
                                                       const float* __restrict__ weights, const float* __restrict__ quat,
                                                       const float* __restrict__ trans, int K, int V, int k, int blocks_per_frame,
                                                       float* __restrict__ out)
{
    __shared__ float M[RIG_LDS_BONES][12];
    const int t = blockIdx.x / blocks_per_frame;
    const int v = (blockIdx.x - t * blocks_per_frame) * 256 + threadIdx.x;
    for (int b = threadIdx.x; b < K; b += 256) {
        const float* q = quat + ((size_t)t * K + b) * 4;
        const float* tr = trans + ((size_t)t * K + b) * 3;
        const float x = q[0], y = q[1], z = q[2], w = q[3];
        M[b][0] = 1.f - 2.f * (y * y + z * z); M[b][1] = 2.f * (x * y - z * w);       M[b][2] = 2.f * (x * z + y * w);
        M[b][3] = 2.f * (x * y + z * w);       M[b][4] = 1.f - 2.f * (x * x + z * z); M[b][5] = 2.f * (y * z - x * w);
        M[b][6] = 2.f * (x * z - y * w);       M[b][7] = 2.f * (y * z + x * w);       M[b][8] = 1.f - 2.f * (x * x + y * y);
        M[b][9] = tr[0]; M[b][10] = tr[1]; M[b][11] = tr[2];
    }
    __syncthreads();
    if (v >= V) return;
    const float p0 = rest[(size_t)v * 3], p1 = rest[(size_t)v * 3 + 1], p2 = rest[(size_t)v * 3 + 2];
    float a0 = p0, a1 = p1, a2 = p2;
    if (k > 0) {
        a0 = a1 = a2 = 0.f;
        for (int i = 0; i < k; i++) {
            const int b = (int)joints[(size_t)v * k + i] + 1;
            if (b >= K) continue;                                           // not a joint of this skin: no influence
            const float wi = weights[(size_t)v * k + i];
            const float* m = M[b];
            a0 += wi * (((m[0] * p0 + m[1] * p1) + m[2] * p2) + m[9]);
            a1 += wi * (((m[3] * p0 + m[4] * p1) + m[5] * p2) + m[10]);
            a2 += wi * (((m[6] * p0 + m[7] * p1) + m[8] * p2) + m[11]);
        }
    }
    const float* m = M[0];
    float* o = out + ((size_t)t * V + v) * 3;
    o[0] = ((m[0] * a0 + m[1] * a1) + m[2] * a2) + m[9];
    o[1] = ((m[3] * a0 + m[4] * a1) + m[5] * a2) + m[10];
    o[2] = ((m[6] * a0 + m[7] * a1) + m[8] * a2) + m[11];
}

// One block per frame, two levels in a fixed order: thread i folds vertices i, i + 256, ... in increasing order, then the 256
// partial results fold pairwise across halves (128, 64, ... 1) in LDS.  stats[t] = (max |posed - ref|, sum |posed - ref|^2,
// min x, min y, min z, max x, max y, max z of posed).
__global__ __launch_bounds__(256) void rig_stats_kernel(const float* __restrict__ posed, const float* __restrict__ ref, int V,
                                                        float* __restrict__ stats)
{
    __shared__ float red[8][256];
    const int t = blockIdx.x, i = threadIdx.x;
    const float inf = __builtin_huge_valf();
    float mx = 0.f, ss = 0.f, lo0 = inf, lo1 = inf, lo2 = inf, hi0 = -inf, hi1 = -inf, hi2 = -inf;
    for (int v = i; v < V; v += 256) {
        const float* a = posed + ((size_t)t * V + v) * 3;
        const float* b = ref + ((size_t)t * V + v) * 3;
        const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
        const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
        mx = fmaxf(mx, dd);
        ss += dd;
        lo0 = fminf(lo0, a[0]); lo1 = fminf(lo1, a[1]); lo2 = fminf(lo2, a[2]);
        hi0 = fmaxf(hi0, a[0]); hi1 = fmaxf(hi1, a[1]); hi2 = fmaxf(hi2, a[2]);
    }
    red[0][i] = mx; red[1][i] = ss; red[2][i] = lo0; red[3][i] = lo1; red[4][i] = lo2; red[5][i] = hi0; red[6][i] = hi1; red[7][i] = hi2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (i < o) {
            red[0][i] = fmaxf(red[0][i], red[0][i + o]);
            red[1][i] = red[1][i] + red[1][i + o];
#pragma unroll
            for (int c = 2; c < 5; c++) red[c][i] = fminf(red[c][i], red[c][i + o]);
#pragma unroll
            for (int c = 5; c < 8; c++) red[c][i] = fmaxf(red[c][i], red[c][i + o]);
        }
        __syncthreads();
    }
    if (i == 0) {
        float* s = stats + (size_t)t * 8;
        s[0] = sqrtf(red[0][0]);
        for (int c = 1; c < 8; c++) s[c] = red[c][0];
    }
}

static bool rig_frames_ok(int T, int V) { return T >= 0 && V >= 0 && (long long)T * V * 3 <= 0x7fffffffLL; }

}  // namespace lasr

extern "C" int lasr_rig_pack(const float* skin, int J, int V, int k, unsigned char* joints, float* weights, float* dropped,
                             void* hip_stream)
{
    if (J < 0 || J > LASR_RIG_MAX_BONES || V < 0 || (k != 4 && k != LASR_RIG_MAX_INFLUENCES)) return LASR_E_BADARG;
    if ((long long)V * LASR_RIG_MAX_BONES > 0x7fffffffLL) return LASR_E_BADARG;
    if (V == 0) return LASR_OK;
    if ((J > 0 && !skin) || !joints || !weights || !dropped) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)((V + 255) / 256)), block(256);
    if (k == 4)
        hipLaunchKernelGGL(lasr::rig_pack_kernel<4>, grid, block, 0, st, skin, J, V, joints, weights, dropped);
    else
        hipLaunchKernelGGL(lasr::rig_pack_kernel<8>, grid, block, 0, st, skin, J, V, joints, weights, dropped);
    return launch_ok();
}

extern "C" int lasr_rig_quats(const float* R, int T, int K, float* quat, void* hip_stream)
{
    if (T < 0 || K < 0 || K > LASR_RIG_MAX_BONES + 1 || (long long)T * K * 9 > 0x7fffffffLL) return LASR_E_BADARG;
    if (T == 0 || K == 0) return LASR_OK;
    if (!R || !quat) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(lasr::rig_quats_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, R, T, K, quat);
    return launch_ok();
}

extern "C" int lasr_rig_skin(const float* rest, const unsigned char* joints, const float* weights, const float* quat,
                             const float* trans, int T, int K, int V, int k, float* out, void* hip_stream)
{
    if (!lasr::rig_frames_ok(T, V) || K < 1 || K > LASR_RIG_MAX_BONES + 1) return LASR_E_BADARG;
    if (K == 1 ? k != 0 : (k != 4 && k != LASR_RIG_MAX_INFLUENCES)) return LASR_E_BADARG;
    if (T == 0 || V == 0) return LASR_OK;
    if (!rest || !quat || !trans || !out || (k > 0 && (!joints || !weights))) return LASR_E_BADARG;
    const long long bpf = (V + 255) / 256;
    if (bpf * T > 0x7fffffffLL) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(lasr::rig_skin_kernel, dim3((unsigned)(bpf * T)), dim3(256), 0, st, rest, joints, weights, quat, trans, K, V, k,
                       (int)bpf, out);
    return launch_ok();
}

extern "C" int lasr_rig_stats(const float* posed, const float* ref, int T, int V, float* stats, void* hip_stream)
{
    if (!lasr::rig_frames_ok(T, V)) return LASR_E_BADARG;
    if (T == 0 || V == 0) return LASR_OK;
    if (!posed || !ref || !stats) return LASR_E_BADARG;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(lasr::rig_stats_kernel, dim3((unsigned)T), dim3(256), 0, st, posed, ref, V, stats);
    return launch_ok();
}
