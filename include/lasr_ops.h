/*
 * lasr_ops.h -- C ABI of the geometry / loss kernels that sit around the rasteriser on the LASR hot
 * path (same library, liblasr_hip.so; same conventions as lasr_sr.h: device pointers, fp32, sizes,
 * hipStream_t as void*, 0 / negative LASR_E_* return codes, nothing printed, nothing synchronised).
 *
 * The reference implements all of these as chains of eager PyTorch ops (no native interface to bind
 * to); each entry point names the Python function it replaces.  Paths are relative to /root/reference/.
 */
#ifndef LASR_OPS_H_
#define LASR_OPS_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Linear-blend skinning, nnutils/geom_utils.py:45-71 (obj_to_cam):
 *   vs[n,v]  = sum_{k=1..K-1} skin[n,k-1,v] * (verts[n,v] @ R[n*K+k] + T[n*K+k])      (K > 1; else vs = verts)
 *   out[n,v] = tocam ? vs[n,v] @ R[n*K] + T[n*K] : vs[n,v]
 * verts [N,V,3], Rmat [N*K,3,3] (row-vector convention, bone-major inside a mesh), Tmat [N*K,3],
 * skin [N,K-1,V] (may be NULL when K == 1), out [N,V,3].
 * Forward: the blend contraction skin^T[V,K-1] x RT[K-1,12] runs on the matrix cores
 * (v_mfma_f32_16x16x4_f32, exact fp32).  Backward overwrites (does not accumulate) all four gradients;
 * it is deterministic (no atomics).  Any gradient pointer may be NULL to skip it.
 */
int lasr_lbs_forward(const float* verts, const float* Rmat, const float* Tmat, const float* skin, float* out,
                     int N, int V, int K, int tocam, void* hip_stream);
/* Both results of one blend: out_cam (tocam = 1) and out_blend (the vertices before the body transform, tocam = 0) -- what
 * LASR.forward needs as verts_cam and deform_v (nnutils/mesh_net.py:291,298; two obj_to_cam calls in the reference). */
int lasr_lbs_forward_both(const float* verts, const float* Rmat, const float* Tmat, const float* skin, float* out_cam,
                          float* out_blend, int N, int V, int K, void* hip_stream);
size_t lasr_lbs_backward_scratch_floats(int N, int V, int K);     /* chunk partials of the transform gradients */
/* Backward.  The three contractions (blended transform, g_skin, the transposed g_RT) run on v_mfma_f32_16x16x4_f32 (K <= 65;
 * more bones: the VALU kernel of ABI version 1); a second small launch folds the chunk partials of grad_Rmat / grad_Tmat.  With
 * grad_Rmat == grad_Tmat == NULL that contraction and the fold are skipped (scratch may then be NULL). */
int lasr_lbs_backward(const float* verts, const float* Rmat, const float* Tmat, const float* skin,
                      const float* grad_out, float* grad_verts, float* grad_Rmat, float* grad_Tmat,
                      float* grad_skin, float* scratch, int N, int V, int K, int tocam, void* hip_stream);
int lasr_lbs_backward_both(const float* verts, const float* Rmat, const float* Tmat, const float* skin,
                           const float* grad_out_cam, const float* grad_out_blend, float* grad_verts, float* grad_Rmat,
                           float* grad_Tmat, float* grad_skin, float* scratch, int N, int V, int K, void* hip_stream);

/*
 * Joint centres and control points into the image: the two obj_to_cam calls with an identity skin and the pinhole_cam of
 * nnutils/mesh_net.py:285-288, :302 in one launch each way.  rest_ts / ctl_ts [H, K-1, 3]; Rmat [M*K,3,3], Tmat [M*K,3] with
 * M = images x H (hypothesis fastest); pp [M/H, 2] per image, fl [M].  Point j of hypothesis h rides on part bone (j mod (K-1)) + 1
 * and then the body transform (bone 0) of every m = img * H + h:  proj [M, 2(K-1), 4] = (pp + xy * fl / z, z, 1), joints first.
 * The transforms and intrinsics are constants (the reference detaches them); backward: grad_rest / grad_ctl [H, K-1, 3], summed
 * over the images in image order (overwritten).  Same association of the sums as lasr_lbs_forward + lasr_pinhole_forward.
 */
int lasr_project_points_forward(const float* rest_ts, const float* ctl_ts, const float* Rmat, const float* Tmat, const float* pp,
                                const float* fl, float* proj, int M, int H, int K, void* hip_stream);
int lasr_project_points_backward(const float* rest_ts, const float* ctl_ts, const float* Rmat, const float* Tmat, const float* fl,
                                 const float* grad_proj, float* grad_rest, float* grad_ctl, int M, int H, int K, void* hip_stream);

/*
 * The pose chain of LASR.forward in ONE launch each way (round 6; nnutils/mesh_net.py:204-217 intrinsics bookkeeping, :232 quaternion ->
 * matrix, :259-283 bone fix-up with the rotation distance of :514-516, :285-288 + :302 joint / control-point projection): the
 * phases of lasr_intrinsics_*, lasr_quat_to_rotmat_*, lasr_bone_fixup_pair_* and lasr_project_points_* run by one workgroup, with
 * the `.repeat(1, H, 1, 1)` of trans / depth (:237-238) inside.  B image pairs, H hypotheses, K bones, M = 2B*H:
 *   in   cams [2B, cam_stride] (column 0 = crop scale), pp [2B,2], scale [2B,H], depth [2B,K], ppoint [2B,2], quat4 [M*K,4] (x,y,z,w),
 *        trans [2B*K,2], rest_ts / ctl_ts [H,K-1,3] (NULL when K == 1)
 *   out  scale_out [2B,H], depth_out [2B,K], ppoint_out [2B,2], trans_rep [M*K,2], depth_rep [M*K], rmat [M*K,3,3], tmat [M*K,3],
 *        pair_angle [M*K/2] (NULL: not wanted), proj [M, 2(K-1), 4] (K > 1)
 * Backward: gradients of the outputs (any of grad_scale_out / grad_ppoint_out / grad_trans_rep / grad_depth_rep / grad_pair_angle /
 * grad_proj may be NULL = zero) -> gradients of scale, depth, ppoint, quat4, trans, rest_ts, ctl_ts (overwritten); the
 * projection treats transforms and intrinsics as constants like lasr_project_points_backward; scratch = M*K*3 floats.
 */
int lasr_pose_chain_forward(const float* cams, int cam_stride, const float* pp, const float* scale, const float* depth,
                            const float* ppoint, const float* quat4, const float* trans, const float* rest_ts, const float* ctl_ts,
                            float* scale_out, float* depth_out, float* ppoint_out, float* trans_rep, float* depth_rep, float* rmat,
                            float* tmat, float* pair_angle, float* proj, int B, int H, int K, float half_size, void* hip_stream);
int lasr_pose_chain_backward(const float* cams, int cam_stride, const float* quat4, const float* rest_ts, const float* ctl_ts,
                             const float* rmat, const float* tmat, const float* scale_out, const float* grad_scale_out,
                             const float* grad_ppoint_out, const float* grad_trans_rep, const float* grad_depth_rep,
                             const float* grad_rmat, const float* grad_tmat, const float* grad_pair_angle, const float* grad_proj,
                             float* grad_scale, float* grad_depth, float* grad_ppoint, float* grad_quat4, float* grad_trans,
                             float* grad_rest, float* grad_ctl, float* scratch, int B, int H, int K, void* hip_stream);

/*
 * Pinhole projection, nnutils/geom_utils.py:27-34 (pinhole_cam), with pp / fl already expanded per mesh:
 *   out.x = pp[n,0] + x * fl[n] / z ;  out.y = pp[n,1] + y * fl[n] / z ;  out.z = z ; out.w = w
 * verts/out [N,V,4], pp [N,2], fl [N].  Backward overwrites grad_verts [N,V,4], grad_pp [N,2], grad_fl [N].
 */
int lasr_pinhole_forward(const float* verts, const float* pp, const float* fl, float* out, int N, int V,
                         void* hip_stream);
int lasr_pinhole_backward(const float* verts, const float* pp, const float* fl, const float* grad_out,
                          float* grad_verts, float* grad_pp, float* grad_fl, int N, int V, void* hip_stream);

/*
 * The three loss tables below split every (image, hypothesis) row into chunks so that small tables still fill
 * the chip, and fold the chunk partials in a fixed order.  `scratch` (lasr_loss_scratch_floats(I,H,P) floats,
 * caller-allocated) carries the partials and the per-row counts from a forward call to the matching backward call.
 */
size_t lasr_loss_scratch_floats(int I, int H, int P);

/*
 * Silhouette loss table, nnutils/mesh_net.py:374-388:
 *   loss[i,j] = 0.5 * mean_{p : occ[i,p] != 0} (mask_pred[i,j,p] - masks[i,p])^2
 * mask_pred [I,H,P], masks [I,P], occ [I,P] -> loss [I,H].  (Empty selection -> NaN like torch's mean of
 * an empty tensor.)  Backward: grad_pred [I,H,P] = grad_loss[i,j] * (pred - mask) / count on selected pixels.
 */
int lasr_mask_loss_forward(const float* mask_pred, const float* masks, const float* occ, float* loss,
                           float* scratch, int I, int H, int P, void* hip_stream);
int lasr_mask_loss_backward(const float* mask_pred, const float* masks, const float* occ, const float* grad_loss,
                            const float* scratch, float* grad_pred, int I, int H, int P, void* hip_stream);

/*
 * Optical-flow loss table, nnutils/mesh_net.py:393-413:
 *   sel[i,j,p] = !bg[i,j,p] && occ[i,p] != 0 && masks[i,p] > 0
 *   w[i,p]     = sigmoid(-occ[i,p]) / mean_{(j,p) in sel[i]} sigmoid(-occ[i,p])
 *   loss[i,j]  = 0.5 * mean_{p in sel[i,j]} ||flow_rd[i,j,p,:] - flow_obs[i,:,p]||_2 * w[i,p]     (0 if sel[i,j] empty)
 * flow_rd [I,H,P,2], flow_obs: channel planes of P floats, images obs_image_stride floats apart (the first two
 * channels of the [I,3,P] observation), bg [I,H,P] uint8,
 * occ/masks [I,P] -> loss [I,H], and the weighted error map flow_rd_map [I,H,P] the trainer logs.
 * Backward: gradient w.r.t. flow_rd only (the weights are data).
 */
int lasr_flow_loss_forward(const float* flow_rd, const float* flow_obs, const unsigned char* bg, const float* occ,
                           const float* masks, float* loss, float* flow_rd_map, float* scratch,
                           int I, int H, int P, int obs_image_stride, void* hip_stream);
int lasr_flow_loss_backward(const float* flow_rd, const float* flow_obs, const unsigned char* bg, const float* occ,
                            const float* masks, const float* scratch, const float* grad_loss, float* grad_flow_rd,
                            int I, int H, int P, int obs_image_stride, void* hip_stream);
/* The same, also writing sel as vis_mask [I,H,P] uint8 (the `vis_mask` LASR.forward returns, nnutils/mesh_net.py:405). */
int lasr_flow_loss_forward_vis(const float* flow_rd, const float* flow_obs, const unsigned char* bg, const float* occ,
                               const float* masks, float* loss, float* flow_rd_map, unsigned char* vis_mask, float* scratch,
                               int I, int H, int P, int obs_image_stride, void* hip_stream);

/*
 * L1 texture loss table, nnutils/mesh_net.py:425-441 (without the perceptual term):
 *   loss[i,j] = 2*wt * ( mean_{occ[i]!=0} mean_c |img_obs[i,c,p] - rnd[i,j,c,p]*fg[i,j,p]|
 *                      + mean_{occ[i]!=0} mean_c |img_white[i,c,p] - rnd[i,j,c,p]| )
 * img_obs/img_white [I,3,P], rnd [I,H,3,P], fg [I,H,P], occ [I,P] -> loss [I,H].
 * Backward: grad_rnd [I,H,3,P] and grad_fg [I,H,P] (overwritten).
 */
int lasr_tex_loss_forward(const float* img_obs, const float* img_white, const float* rnd, const float* fg,
                          const float* occ, float* loss, float* scratch, float wt, int I, int H, int P,
                          void* hip_stream);
int lasr_tex_loss_backward(const float* img_obs, const float* img_white, const float* rnd, const float* fg,
                           const float* occ, const float* grad_loss, const float* scratch, float* grad_rnd,
                           float* grad_fg, float wt, int I, int H, int P, void* hip_stream);

/*
 * Mesh regularisers on sparse adjacency instead of dense [V,V] operators.
 *
 * ARAP, nnutils/loss_utils.py:46-64:  loss[n] = mean over directed edges (v,u), u in nbr(v), of
 *   | ||x[n,u]-x[n,v]||^2 - ||dx[n,u]-dx[n,v]||^2 |     (the reference builds six dense [N,V,V] tensors for this).
 * Laplacian, third_party/ext_nnutils/loss_utils.py:34-65:  loss[n] = sum_v || x_v - mean_{u in nbr(v)} x_u ||^2 ;
 *   vertices without neighbours contribute 0 (the reference leaves their row at zero, :50-51).
 * Both take the mesh adjacency as CSR (row_ptr [V+1], col [nnz], unique neighbours, symmetric), x/dx [N,V,3]
 * -> loss [N].  Backward entry points overwrite the gradients and are deterministic (vertex-centric gathers).
 */
int lasr_arap_forward(const float* dx, const float* x, const int* row_ptr, const int* col, float* loss,
                      int N, int V, void* hip_stream);
int lasr_arap_backward(const float* dx, const float* x, const int* row_ptr, const int* col, const float* grad_loss,
                       float* grad_dx, float* grad_x, int N, int V, void* hip_stream);
int lasr_laplacian_forward(const float* x, const int* row_ptr, const int* col, float* loss, int N, int V,
                           void* hip_stream);
int lasr_laplacian_backward(const float* x, const int* row_ptr, const int* col, const float* grad_loss,
                            float* grad_x, float* scratch_lx /*[N,V,3]*/, int N, int V, void* hip_stream);

/*
 * The three shape regularisers of a step in ONE launch each way (nnutils/mesh_net.py:449-459 Laplacian + flatten on the mean shape
 * x [N,V,3]; :494-497 ARAP between the two frames' deformed shapes arap_dx / arap_x [NA,V,3]); the same arithmetic and summation
 * orders as lasr_laplacian_* / lasr_flatten_* / lasr_arap_*, results bit-identical to calling those one by one:
 *   lap_loss [N], flat_loss [N], arap_loss [NA];  lap_coords [N,V,3] = the Laplacian coordinates, kept by the caller for the backward.
 * Index buffers as for the separate entry points (CSR adjacency of the Laplacian and of ARAP, quads [E,4], incidence CSR of the
 * flatten backward).  Backward: grad_x [N,V,3] = Laplacian part + flatten part (overwritten), grad_arap_dx / grad_arap_x [NA,V,3]
 * (either may be NULL).  N or NA may be 0.
 */
int lasr_mesh_regularisers_forward(const float* x, const float* arap_dx, const float* arap_x, const int* lap_row_ptr,
                                   const int* lap_col, const int* arap_row_ptr, const int* arap_col, const int* quads,
                                   float* lap_loss, float* lap_coords, float* flat_loss, float* arap_loss, int N, int NA, int V,
                                   int E, void* hip_stream);
int lasr_mesh_regularisers_backward(const float* x, const float* arap_dx, const float* arap_x, const int* lap_row_ptr,
                                    const int* lap_col, const int* arap_row_ptr, const int* arap_col, const int* quads,
                                    const int* inc_ptr, const int* inc, const float* lap_coords, const float* grad_lap,
                                    const float* grad_flat, const float* grad_arap, float* grad_x, float* grad_arap_dx,
                                    float* grad_arap_x, int N, int NA, int V, int E, void* hip_stream);
/* The same two launches with a fourth criterion riding along: the symmetric squared Chamfer distance of NC pairs of small point sets
 * (the bones' control points against their mirror images, nnutils/mesh_net.py:500-503) -- cham_a [NC,P,3], cham_b [NC,Q,3] ->
 * cham_loss [NC], nn_ab [NC,P] / nn_ba [NC,Q] (int32, kept by the caller for the backward); the values and gradients of
 * lasr_chamfer_forward / _backward, bit for bit, without their two launches.  NC = 0: exactly lasr_mesh_regularisers_*. */
int lasr_step_regularisers_forward(const float* x, const float* arap_dx, const float* arap_x, const int* lap_row_ptr,
                                   const int* lap_col, const int* arap_row_ptr, const int* arap_col, const int* quads,
                                   float* lap_loss, float* lap_coords, float* flat_loss, float* arap_loss, int N, int NA, int V,
                                   int E, const float* cham_a, const float* cham_b, float* cham_loss, int* nn_ab, int* nn_ba, int NC,
                                   int P, int Q, void* hip_stream);
int lasr_step_regularisers_backward(const float* x, const float* arap_dx, const float* arap_x, const int* lap_row_ptr,
                                    const int* lap_col, const int* arap_row_ptr, const int* arap_col, const int* quads,
                                    const int* inc_ptr, const int* inc, const float* lap_coords, const float* grad_lap,
                                    const float* grad_flat, const float* grad_arap, float* grad_x, float* grad_arap_dx,
                                    float* grad_arap_x, int N, int NA, int V, int E, const float* cham_a, const float* cham_b,
                                    const int* nn_ab, const int* nn_ba, const float* grad_cham, float* grad_cham_a,
                                    float* grad_cham_b, int NC, int P, int Q, void* hip_stream);

/*
 * Flow reprojection, nnutils/mesh_net.py:93-104 (the tail of render_flow_soft_2 after the render).
 * px [N,7,P] = the 6-attribute render (lasr_sr_forward_attr): planes 0-2 camera-space position of frame t seen at each
 * pixel, planes 3-5 of frame t', plane 6 alpha.  bgmask = (px[2] < 1e-9) | (px[5] < 1e-9); background pixels take the
 * point (10,10,10) (:93-95); flow[n,p] = proj(p1; pp1[n], fl1[n]) - proj(p0; pp0[n], fl0[n]) with
 * proj(q; pp, fl) = pp + (q.xy * fl) / q.z (:98-101).  pp0/pp1 [N,2], fl0/fl1 [N] -> flow [N,P,2], bgmask [N,P] (0/1 bytes).
 * Backward: the frame-t projection and all background pixels are detached (:102-103), so the gradient reaches
 * px planes 3-5 (grad_px [N,7,P] is overwritten whole, zeros elsewhere), pp1 [N,2] and fl1 [N].
 * scratch: lasr_flow_reproject_scratch_floats(N, P) floats.
 */
size_t lasr_flow_reproject_scratch_floats(int N, int P);
int lasr_flow_reproject_forward(const float* px, const float* pp0, const float* pp1, const float* fl0, const float* fl1,
                                float* flow, unsigned char* bgmask, int N, int P, void* hip_stream);
int lasr_flow_reproject_backward(const float* px, const float* fl1, const float* grad_flow, float* grad_px,
                                 float* grad_pp1, float* grad_fl1, float* scratch, int N, int P, void* hip_stream);

/*
 * The same on six position planes that sit inside a wider render (LASR.forward renders texture + both position triples in
 * one 9-attribute pass, [N,10,P]): pos6 points at the first position plane of image 0, consecutive images are batch_stride
 * floats apart (>= 6 P), the six planes of an image are contiguous.  grad_pos6 is a dense [N,6,P] tensor.
 */
int lasr_flow_reproject_planes_forward(const float* pos6, long long batch_stride, const float* pp0, const float* pp1,
                                       const float* fl0, const float* fl1, float* flow, unsigned char* bgmask, int N, int P,
                                       void* hip_stream);
int lasr_flow_reproject_planes_backward(const float* pos6, long long batch_stride, const float* fl1, const float* grad_flow,
                                        float* grad_pos6, float* grad_pp1, float* grad_fl1, float* scratch, int N, int P,
                                        void* hip_stream);

/*
 * Unit quaternion -> rotation matrix, kornia 0.5.3 `quaternion_to_rotation_matrix` semantics (not vendored in the
 * reference; call sites nnutils/mesh_net.py:232,250,265 and third_party/ext_nnutils/net_blocks.py:359): coefficient
 * order (x,y,z,w); the quaternion is normalised first (q / max(|q|, 1e-12));
 *   R = [[1-2(yy+zz), 2(xy-zw), 2(xz+yw)], [2(xy+zw), 1-2(xx+zz), 2(yz-xw)], [2(xz-yw), 2(yz+xw), 1-2(xx+yy)]].
 * quat [M,4] -> rotmat [M,9] row-major.  Backward: grad_rotmat [M,9] -> grad_quat [M,4] (overwritten).
 */
int lasr_quat_to_rotmat_forward(const float* quat, float* rotmat, int M, void* hip_stream);
int lasr_quat_to_rotmat_backward(const float* quat, const float* grad_rotmat, float* grad_quat, int M, void* hip_stream);

/*
 * GMM skinning weights, nnutils/mesh_net.py:264-271:
 *   skin[h,k,v] = softmax over k of  -10 * sum_d exp(log_ctl[h,k,d]) * ((ctl_ts[h,k] - verts[h,v]) * R(ctl_rs[h,k]))_d^2
 * ctl_ts, log_ctl [H*J,3], ctl_rs [H*J,4] (x,y,z,w, normalised inside), verts [H,V,3] (frame-0 mean shape, a constant:
 * :266 detaches it) -> skin [H,J,V].  J <= 64.
 * Backward: grad_skin [H,J,V] -> grad_ts [H*J,3], grad_rs [H*J,4], grad_log_ctl [H*J,3] (overwritten);
 * scratch: H*V floats.
 */
int lasr_skin_weights_forward(const float* ctl_ts, const float* ctl_rs, const float* log_ctl, const float* verts,
                              float* skin, int H, int J, int V, void* hip_stream);
int lasr_skin_weights_backward(const float* ctl_ts, const float* ctl_rs, const float* log_ctl, const float* verts,
                               const float* skin, const float* grad_skin, float* grad_ts, float* grad_rs,
                               float* grad_log_ctl, float* scratch, int H, int J, int V, void* hip_stream);

/*
 * Flatten loss, third_party/ext_nnutils/loss_utils.py:110-152: loss[n] = sum over the listed interior edges of
 * (cos + 1)^2 where cos is the cosine between the parts of (v2 - v0) and (v3 - v0) orthogonal to the edge (v1 - v0),
 * every eps = 1e-6 as in the reference (:120-147).  quads [E,4] int32 = (v0,v1,v2,v3) per edge (built on the host from
 * the faces, :73-108), x [N,V,3] -> loss [N].
 * Backward: per-edge gradients into scratch (N*E*12 floats), then a vertex-centric gather through the incidence lists
 * inc_ptr [V+1], inc [4E] (entry = edge*4 + slot, ascending) -> grad_x [N,V,3] (overwritten, deterministic).
 */
int lasr_flatten_forward(const float* x, const int* quads, float* loss, int N, int V, int E, void* hip_stream);
int lasr_flatten_backward(const float* x, const int* quads, const int* inc_ptr, const int* inc, const float* grad_loss,
                          float* grad_x, float* scratch, int N, int V, int E, void* hip_stream);

/*
 * Per-face gather of per-vertex attributes, third_party/softras/soft_renderer/functional/face_vertices.py:4-22:
 *   out[n,f,c,:] = attr[n, faces[n,f,c], :]      attr [N,V,C], faces [N,F,3] int64 (torch's index type) -> out [N,F,3,C].
 * Indices must lie in [0,V) (the reference asserts nothing either; out-of-range is undefined behaviour).
 * Backward: grad_out [N,F,3,C] -> grad_attr [N,V,C], overwritten; the sum over a vertex's corners runs in ascending
 * corner order (deterministic; the reference's autograd uses atomic index_add_).
 */
int lasr_face_gather_forward(const float* attr, const long long* faces, float* out, int N, int V, int F, int C,
                             void* hip_stream);
int lasr_face_gather_backward(const float* grad_out, const long long* faces, float* grad_attr, int N, int V, int F, int C,
                              void* hip_stream);
/* The same backward over a CSR incidence structure the caller built once for the connectivity (the layout of
 * lasr_raster_faces_backward: inc_ptr int32 [N or 1, V+1], inc int32 [N or 1, 3F] = corner ids 3 f + c grouped by vertex, ascending
 * inside a vertex; inc_shared = 1 when all meshes share one).  Same summation order, hence the same bits, without the scan of the
 * face tensor: for callers whose connectivity outlives a call (LASR's does; the Python operator caches the structure per face
 * tensor). */
int lasr_face_gather_backward_csr(const float* grad_out, const int* inc_ptr, const int* inc, int inc_shared, float* grad_attr,
                                  int N, int V, int F, int C, void* hip_stream);

/*
 * Brute-force nearest neighbour between two small point sets (the idx1/dist1 outputs of third_party/chamfer3D/chamfer3D.cu
 * as used at nnutils/mesh_net.py:477, and the inner minimum of pytorch3d's chamfer_distance, :503):
 * a [N,P,3], b [N,Q,3] -> d2 [N,P] squared distance to, and idx [N,P] (int32) index of, the nearest b point
 * (lowest index on ties).  No backward entry point: the caller differentiates |a - b[idx]|^2 with the indices fixed.
 */
int lasr_nearest_point(const float* a, const float* b, float* d2, int* idx, int N, int P, int Q, void* hip_stream);

/*
 * Point <-> triangle-mesh distance, pytorch3d.loss.point_mesh_face_distance as used at nnutils/mesh_net.py:470-471
 * (pytorch3d 0.4.0 is not vendored: semantics restated, parity unpinned):
 *   dmin_point[n,p] = min_f d2(points[n,p], tri[n,f]),  dmin_face[n,f] = min_p d2(points[n,p], tri[n,f])
 * with the arg-min indices (int32, lowest index on ties); the caller forms mean_n(mean_p dmin_point + mean_f dmin_face).
 * verts [N,V,3], faces [F,3] int64 shared by the batch, points [N,P,3].
 * Backward: given d loss / d dmin_point = grad_point_term and d loss / d dmin_face = grad_face_term (uniform weights,
 * as the means produce), writes grad_tri [N,F,3,3] (per face corner; reduce to vertices with lasr_face_gather_backward)
 * and grad_points [N,P,3].  d d2/d p = 2 (p - q), d d2/d corner_i = -2 w_i (p - q) for the closest point q = sum w_i corner_i.
 */
size_t lasr_point_mesh_scratch_floats(int N, int F, int P);            /* per-chunk minima of the two-launch forward */
int lasr_point_mesh_forward(const float* verts, const long long* faces, const float* points, float* dmin_point,
                            int* arg_point, float* dmin_face, int* arg_face, float* scratch, int N, int V, int F, int P,
                            void* hip_stream);
int lasr_point_mesh_backward(const float* verts, const long long* faces, const float* points, const int* arg_point,
                             const int* arg_face, float grad_point_term, float grad_face_term, float* grad_tri,
                             float* grad_points, int N, int V, int F, int P, void* hip_stream);

/*
 * Perceptual-distance reduction, third_party/PerceptualSimilarity/util/util.py:71-83 (normalize_tensor, cos_sim) and
 * models/networks_basic.py:51-57 (1 - cos_sim per feature layer), the reduction behind `ptex_loss.forward_pair` at
 * nnutils/mesh_net.py:442:   dist[n] = 1 - mean_p sum_c a_hat[c,p] * b_hat[c,p],   x_hat = x / (sqrt(sum_c x_c^2) + 1e-10).
 * feat_obs [N/rep, C, P] (features of the observed images, each shared by `rep` consecutive rendered images -- the
 * reference feeds rep identical copies through the network), feat_rnd [N, C, P] -> dist [N].  scratch:
 * lasr_cosdist_scratch_floats(N, P).  Backward: gradient w.r.t. feat_rnd only (grad_rnd [N,C,P], overwritten); the
 * observed side is data.  Where a rendered feature vector is exactly zero the reference's autograd yields NaN
 * (sqrt'(0)); here the ill-defined term is dropped (finite gradient).
 */
size_t lasr_cosdist_scratch_floats(int N, int P);
int lasr_cosdist_forward(const float* feat_obs, const float* feat_rnd, float* dist, float* scratch, int N, int C, int P,
                         int rep, void* hip_stream);
int lasr_cosdist_backward(const float* feat_obs, const float* feat_rnd, const float* grad_dist, float* grad_rnd, int N,
                          int C, int P, int rep, void* hip_stream);

/*
 * The same reduction over ALL feature layers of the perceptual network in one launch each way (the sum over layers of
 * models/networks_basic.py:51-64): dist[n] = sum_l (1 - mean_p cos_l[n,p]), layers added in list order, each layer's value
 * bit-identical to lasr_cosdist_forward's.  feat_obs / feat_rnd / grad_rnd: HOST arrays of n_layers device pointers
 * ([N/rep, C_l, P_l] / [N, C_l, P_l]); C, P: host arrays; n_layers <= LASR_COSDIST_MAX_LAYERS.
 * scratch: lasr_cosdist_multi_scratch_floats floats (tile partials; a second one-wave-per-image launch folds them).
 * Backward: every grad_rnd[l] overwritten.
 */
#define LASR_COSDIST_MAX_LAYERS 8
size_t lasr_cosdist_multi_scratch_floats(const int* P, int n_layers, int N);
int lasr_cosdist_multi_forward(const float* const* feat_obs, const float* const* feat_rnd, const int* C, const int* P,
                               int n_layers, float* dist, float* scratch, int N, int rep, void* hip_stream);
int lasr_cosdist_multi_backward(const float* const* feat_obs, const float* const* feat_rnd, const int* C, const int* P,
                                int n_layers, const float* grad_dist, float* const* grad_rnd, int N, int rep, void* hip_stream);

/*
 * Texture atlas -> per-face surface textures, replaces `soft_renderer.cuda.load_textures`
 * (third_party/softras/soft_renderer/cuda/load_textures_cuda.cpp:10-28, kernel load_textures_cuda_kernel.cu:8-66; called
 * from functional/load_obj.py when scripts/render_syn.py:71 loads its textured mesh).  image [H,W,3] (row 0 first, the caller
 * flips as load_obj.py does), faces_uv [F,3,2] in [0,1], is_update [F] or NULL (NULL = all), textures [F,R*R,3] (only the
 * faces with is_update != 0 are written).  Texel (w_x, w_y): barycentric ((w_x + 1/3)/R, (w_y + 1/3)/R, rest) for
 * w_x + w_y < R, else the mirrored upper-triangle position; bilinear sample at uv * (size - 1).
 */
int lasr_load_textures(const float* image, const float* faces_uv, const int* is_update, float* textures, int F, int R, int H,
                       int W, void* hip_stream);

/*
 * Per-face surface textures -> texture atlas, replaces `soft_renderer.cuda.create_texture_image`
 * (third_party/softras/soft_renderer/cuda/create_texture_image_cuda.cpp, kernel create_texture_image_cuda_kernel.cu:10-70; called
 * from functional/save_obj.py:9-37).  textures [F,R_in*R_in,3]; faces_uv [F,3,2] each face's triangle in pixel units of the atlas;
 * image [tile_height*R_out, tile_width*R_out, 3] with tile_width = floor(sqrt(F-1)) + 1, tile_height = (F-1) / tile_width + 1.
 * Pixel (x, y) belongs to face x / R_out + (y / R_out) * tile_width and copies the texel its barycentric coordinates pick (the
 * reference's arithmetic in its order, eps as the reference's float argument); every pixel is written, 1 past the last face.
 */
int lasr_create_texture_image(const float* faces_uv, const float* textures, float* image, int F, int R_in, int R_out, float eps,
                              void* hip_stream);
int lasr_create_texture_image_f64(const double* faces_uv, const double* textures, double* image, int F, int R_in, int R_out,
                                  float eps, void* hip_stream);

/*
 * Mesh voxelisation, replaces functional/voxelization.py:41-57 (`srf.voxelization(faces, size, normalize)` over the
 * `soft_renderer.cuda.voxelization` kernels, cuda/voxelization_cuda_kernel.cu:30-190).  faces [B,F,3,3] already scaled to voxel
 * units; voxels [B,S,S,S] int32 (overwritten), indexed by the face-vertex coordinates 0, 1, 2: 1 = surface or enclosed.  The
 * surface is the reference's column scans along the three axes and the vertex voxels (one launch, bit-packed); the fill marks
 * every empty voxel not 6-connected through empty voxels to the grid's boundary (one launch, one workgroup per mesh, no host
 * synchronisation).  sweeps [B] (may be NULL) receives the number of fill sweeps of each mesh.
 * S is limited to LASR_VOXEL_MAX_SIZE (64 MB of output per mesh; the reference has no limit).
 */
#define LASR_VOXEL_MAX_SIZE 256
size_t lasr_voxelize_workspace_bytes(int B, int S);     /* 0 for invalid sizes */
int lasr_voxelize(const float* faces, int* voxels, int* sweeps, void* workspace, size_t workspace_bytes, int B, int F, int S,
                  void* hip_stream);
int lasr_voxelize_f64(const double* faces, int* voxels, int* sweeps, void* workspace, size_t workspace_bytes, int B, int F, int S,
                      void* hip_stream);

/*
 * Shading and compositing pass of render_vis.py (lasr_amd/csrc/vis.hip; the reference renders with pyrender / OpenGL,
 * render_vis.py:226-289).  N frames share one face list of F faces over V vertices per frame, all in camera space (OpenCV axes:
 * x right, y down, z forward).  Faces [0, F0) form the opaque layer, faces [F0, F) the translucent surface layer.
 *   vert_rec  [N,V,12]  position x y z, NDC x | normal x y z, NDC y | colour r g b (0-1), 0  (the NDC of the camera raster)
 *   faces     [F,4]     vertex indices, 4th unused; an index outside [0, V) leaves its pixels uncovered
 *   face_rec  [N,F,8]   unit face normal, 0 | light-space plane a b c, 0: depth w = a u + b v + c along light_d at (u, v)
 *   raster0   [N,2,IS,IS]  hard-mode aggrs_info of the opaque layer (lasr_sr_forward_bg, func_id_rgb = func_id_alpha = 0):
 *                          plane 1 holds a face index in [0, F0) or -1
 *   raster1   [N,2,IS,IS]  the same for the surface layer (index + F0 is the face), or NULL for one layer (then F0 == F)
 *   shadow    [N,2,S,S]    hard-mode raster of all F faces from the light, orthographic: NDC = ((u, v) - (cu, cv)) / half
 *   shadow_xf [N,4]        cu, cv, 1 / half, 0 per frame
 *   frames    [N,H,W]      packed RGBA8 input frames (r in the low byte), read when params->overlay, else may be NULL
 *   out       [N,H,W]      packed RGBA8 (alpha 255): the top-left H x W of the square IS x IS render
 * Per pixel: barycentrics of the pixel centre against the face's NDC vertices (the rasteriser's convention), perspective-correct
 * position / normal / colour, two-sided normal (flipped toward the camera), c = clamp(0.6 colour (k_ambient + k_diffuse
 * max(0, n.L) s), 0, 1) with L = -light_d and s the 3x3-PCF shadow fraction (per tap, at the centre of its texel: the stored
 * face's plane depth against the receiver's face plane extended there); the surface layer, where it is nearer than the
 * opaque one, is blended over it with surface_alpha; background where no face; overlay: round(0.5 render + 0.5 frame).
 * Checked on the host before any launch: sizes, layer split and pointers (LASR_E_BADARG).  The contents of device buffers are
 * not read on the host: the kernel treats a map entry outside the layer's [0, F) (-1, too large, NaN) and a face with a vertex
 * index outside [0, V) as no face, so no gather leaves its buffer (lasr_amd/vis.py also validates `faces` before the call).
 */
typedef struct lasr_vis_params {
    float light_u[3], light_v[3], light_d[3];   /* orthonormal light frame, light_d = direction the light travels */
    float k_ambient, k_diffuse, surface_alpha;
    float shadow_bias;                          /* light-space depth margin of the shadow test */
    float background[3];                        /* 0-1 */
    int smooth;                                 /* 1: interpolated vertex normals, 0: face normals */
    int overlay;                                /* 1: blend with `frames` */
} lasr_vis_params;
#define LASR_VIS_MAX_SIZE 16384
int lasr_vis_shade(const float* vert_rec, const int* faces, const float* face_rec, const float* raster0, const float* raster1,
                   const float* shadow, const float* shadow_xf, const unsigned* frames, unsigned* out, int N, int V, int F, int F0,
                   int IS, int S, int H, int W, const lasr_vis_params* params, void* hip_stream);

/*
 * Keypoint transfer of scripts/eval_badja.py (lasr_amd/csrc/keypoints.hip; reference: scripts/eval_badja.py:225-242), for B
 * pairs (reference frame, target frame):
 *   colors [B,4,S,S]  the hard-mode raster of the reference frame's geometry with the target's projected vertices as vertex
 *                     colours (render_flow_soft_3), read in place; NULL: the zero flow (every pixel invalid, pred = kp)
 *   kp     [B,J,2]    keypoints (row, col) in pixels of the H x W crop (the top-left H x W of the S x S raster)
 *   idx    [B,J]      int64 out: flat index r * W + c of the chosen pixel (also the call's scratch: packed search keys)
 *   pred   [B,J,2]    fp32 out: (row + flow_y * H / 2, col + flow_x * W / 2), the reference's scaling
 * Per pixel, in fp32 and the reference's operation order: flow = 0 where colour channel 2 < 1e-9, else colour.xy - grid with
 * grid = (p * 2) * (1 / (S - 1)) - 1 (p = column for x, row for y); invalid where sqrt(fx * fx + fy * fy) < 1e-6; per keypoint
 * idx = argmin over the crop of (invalid * 1e6 + (row - r)^2) + (col - c)^2, the first index on ties (torch's argmin).  Exact
 * for integer keypoints in crops up to 1920 x 1080 (every key below 2^24).  A NaN keypoint gets idx = -1 and a NaN prediction.
 * Checked on the host before any launch: sizes (2 <= S <= LASR_KP_MAX_SIZE, H, W <= S, 1 <= J <= LASR_KP_MAX_JOINTS) and
 * pointers (LASR_E_BADARG).  One memset and two launches on hip_stream; no host synchronisation.
 */
#define LASR_KP_MAX_JOINTS 64
#define LASR_KP_MAX_SIZE 16384
int lasr_kp_transfer(const float* colors, const float* kp, long long* idx, float* pred, int B, int J, int S, int H, int W,
                     void* hip_stream);

/*
 * Watertight re-meshing (lasr_amd/csrc/manifold.hip), in place of the external Manifold binary the reference runs as
 * `manifold in.obj out.obj 10000` (scripts/eval_mesh.py:100-105, render_vis.py:98, nnutils/train_utils.py:422).  The caller
 * voxelises the input with lasr_voxelize into voxels [S,S,S] int32 (index c0, c1, c2; voxel i covers [i, i+1)), then:
 *   repair   makes the solid well-composed: a Jacobi sweep turns every empty voxel of a critical configuration solid -- a 2x2
 *            square of an axis plane whose diagonals hold opposite values, or a 2x2x2 block whose only voxels of one value are an
 *            antipodal pair, in either colour -- until a sweep changes nothing; then export.hip's fill sweep fills the pockets the
 *            repair closed.  voxels is rewritten in place (1 = solid).  info[0] = sweeps of the repair (the last one changes
 *            nothing); info[1] = sweeps of the fill.  A solid voxel on the grid's outer layer is refused without a host
 *            synchronisation: info[0] = -1 (LASR_E_BADARG of the caller, which reads info with the counts) and the solid is only
 *            refilled.
 *   count    counts[0] = solid voxels with an empty 6-neighbour, counts[1] = V vertices, counts[2] = F triangles of the boundary.
 *            The per-row vertex masks and offsets stay in the workspace for extract (same voxels, same workspace, no call between).
 *   extract  verts [V,3] fp32 lattice coordinates, faces [F,3] int64.  One quad per solid voxel face whose 6-neighbour is empty,
 *            counter-clockwise seen from the empty side, split along its (0,0)-(1,1) diagonal of the in-plane axes
 *            (a+1, a+2) mod 3; one vertex per lattice point whose eight voxels are not all equal.  Orders (deterministic, no
 *            atomics): vertices by lattice linear index (p0 * (S+1) + p1) * (S+1) + p2; triangles by voxel linear index
 *            (c0 * S + c1) * S + c2, then direction -c0, +c0, -c1, +c1, -c2, +c2, then the two triangles of the quad.
 *            V and F are the counts read back from count: writes past them are dropped.
 *   project  verts[v] = the closest point to lattice[v] on input face arg_face[v] (lasr_point_mesh_forward's arg_point; the
 *            closest point as point_mesh's point_triangle computes it).  An out-of-range face leaves the lattice point.
 *   guard    rounds of: flag every face whose normal has a non-positive dot product with its lattice normal, or whose area is
 *            below min_area; move every vertex of a flagged face back to lattice[]; until no face is flagged.  rounds[0] = the
 *            rounds that moved vertices back.  flags [V] int32 scratch.  One workgroup; no host synchronisation.
 * Sizes and pointers are checked on the host before any launch: LASR_MANIFOLD_MIN_SIZE <= S <= LASR_MANIFOLD_MAX_SIZE
 * (LASR_E_BADARG), workspace >= lasr_manifold_workspace_bytes(S) (LASR_E_WORKSPACE).  No call synchronises the host.
 */
#define LASR_MANIFOLD_MIN_SIZE 4
#define LASR_MANIFOLD_MAX_SIZE 256
size_t lasr_manifold_workspace_bytes(int S);      /* 0 for invalid sizes */
int lasr_manifold_repair(int* voxels, int* info, void* workspace, size_t workspace_bytes, int S, void* hip_stream);
int lasr_manifold_count(const int* voxels, int* counts, void* workspace, size_t workspace_bytes, int S, void* hip_stream);
int lasr_manifold_extract(const int* voxels, float* verts, long long* faces, int V, int F, void* workspace, size_t workspace_bytes,
                          int S, void* hip_stream);
int lasr_manifold_project(const float* lattice, const float* in_verts, const long long* in_faces, const int* arg_face, float* verts,
                          int V, int Vin, int Fin, void* hip_stream);
int lasr_manifold_guard(const float* lattice, float* verts, const long long* faces, int* flags, int* rounds, int V, int F,
                        float min_area, void* hip_stream);

/*
 * ---- Phong pass of extract.py --render and scripts/eval_mesh.py --render (lasr_amd/csrc/phong.hip, lasr_amd/phong.py) ------------
 * Replaces pytorch3d 0.4.0's MeshRenderer(MeshRasterizer(OrthographicCameras(), RasterizationSettings(cull_backfaces=True)),
 * SoftPhongShader(PointLights(ambient = diffuse = specular = white)), BlendParams()) of the reference (nnutils/predictor.py:296-335,
 * scripts/eval_mesh.py:170-192) for K = 1 face per pixel and blur radius 0.  Visibility is NOT computed here: `raster` is the
 * hard-mode aggrs_info of lasr_sr_forward_bg (func_id_rgb = func_id_alpha = 0) whose plane 1 names the nearest face per pixel.
 * N frames share one face list of F faces over V vertices per frame, in pytorch3d world (= view) coordinates.
 *   vert_rec [N,V,12]   position x y z, 0 | unit vertex normal x y z, 0 | colour (texel) r g b, 0
 *   faces    [F,4]      vertex indices, 4th unused; an index outside [0, V) leaves its pixels uncovered
 *   raster   [N,2,S,S]  plane 1: face index in [0, F) or -1 (row 0 is the top row, NDC y = +1)
 *   background          3 host floats (0-1)
 *   out      [N,S,S,4]  fp32 RGBA, unclamped
 * Pixel (row r, column c) of frame n sits at pytorch3d NDC x = 1 - (2c + 1)/S, y = 1 - (2r + 1)/S (+X left, +Y up); with the
 * default orthographic camera world x, y are NDC.  Covered by face f: 2-D barycentrics at the pixel centre (no perspective
 * correction), linear position p, normal, texel and z; n = normalize(normal, 1e-6), l = normalize((0, 1, 0) - p),
 * v = normalize(-p), colour = (1 + relu(n.l)) texel + [n.l > 0] relu(v.(2 (n.l) n - l))^64; softmax_rgb_blend with
 * sigma = gamma = 1e-4, znear = 1, zfar = 100: prob = sigmoid(d2 / sigma) with d2 the squared distance to the face's nearest
 * edge, z_inv = (zfar - z) / (zfar - znear), m = max(z_inv, 1e-10), w = prob exp((z_inv - m) / gamma),
 * delta = max(exp((1e-10 - m) / gamma), 1e-10), rgb = (w colour + delta bg) / (w + delta), alpha = prob.  Uncovered: bg, 0.
 * Checked on the host before any launch (LASR_E_BADARG): N >= 0, V, F >= 1, 1 <= S <= LASR_PHONG_MAX_SIZE, N <= 65535,
 *   every pointer non-NULL when N > 0.  Device contents are not read on the host: a map entry outside [0, F) (-1, NaN) or a face
 *   with a vertex index outside [0, V) shades as background, so no gather leaves its buffer.
 */
#define LASR_PHONG_MAX_SIZE 8192
int lasr_phong_shade(const float* vert_rec, const int* faces, const float* raster, const float* background, float* out, int N, int V,
                     int F, int S, void* hip_stream);

/*
 * ---- Nearest neighbours at evaluation size, chamfer3D and ICP (lasr_amd/csrc/chamfer.hip, lasr_amd/chamfer3D, lasr_amd/nnutils/icp.py)
 * All point sets are contiguous fp32 device arrays [N,points,3]; indices are int32.  lasr_nearest_point above is shaped for
 * LASR's <= 1.3 k-point sets; these are shaped for the 10 000 x 10 000 of scripts/eval_mesh.py:116-168.
 *
 * lasr_nn_tiled: a [N,P,3], b [N,Q,3] -> d2 [N,P], idx [N,P]: squared distance to and index of the nearest b point, lowest index
 *   on ties; a row with no finite distance (NaN) reports d2 = inf, idx = 0 (the idx1 / dist1 of NmDistanceKernel,
 *   third_party/chamfer3D/chamfer3D.cu:12-134).  R [N,3,3], T [N,3]: both NULL, or a rigid transform per batch element read from
 *   device memory and applied to every query as it is loaded, row-vector convention a R + T.  Without a transform d2 and idx
 *   equal lasr_nearest_point's bit for bit.  The target set passes through LDS in tiles of LASR_NN_TILE points; `splits` runs of
 *   whole tiles are searched by separate blocks and merged through 64-bit keys (distance bits high, index low) by atomicMin, which
 *   keeps "lowest index wins" in any arrival order.  splits = 0: chosen from the sizes; splits > 0: that many (at most 65535).
 *   workspace: lasr_chamfer3d_workspace_bytes(N, P, 0) bytes, needed when more than one split runs (may be NULL for splits = 1).
 * lasr_chamfer3d_forward: both directions of chamfer_3DFunction.forward (third_party/chamfer3D/dist_chamfer_3D.py:28-47) in one
 *   call: dist1, idx1 [N,P] of xyz1 against xyz2, dist2, idx2 [N,Q] of xyz2 against xyz1.
 *   workspace: lasr_chamfer3d_workspace_bytes(N, P, Q).
 * lasr_chamfer3d_backward: the gradient of sum grad_dist1 dist1 + sum grad_dist2 dist2 with the indices fixed
 *   (NmDistanceGradKernel, chamfer3D.cu:155-180, dist_chamfer_3D.py:50-64):
 *     grad_xyz1[i] = 2 g1[i] (x1_i - x2[idx1[i]]) + sum_{j: idx2[j] = i} 2 g2[j] (x1_i - x2_j), and symmetrically grad_xyz2.
 *   The reference scatters with float atomics; here every point gathers its terms in a fixed order, so two calls give the same
 *   bits.  The caller supplies the inverse of the index maps as CSR: row_ptr1 [N,P+1], col1 [N,Q] list, for every xyz1 point, the
 *   xyz2 points j with idx2[j] = it, ascending in j; row_ptr2 [N,Q+1], col2 [N,P] the same from idx1 (a stable sort of the
 *   indices: lasr_amd/chamfer3D/dist_chamfer_3D.py).  An index or column outside its set contributes nothing.
 * ICP: pytorch3d.ops.iterative_closest_point(X, Y, estimate_scale=False) as called at scripts/eval_mesh.py:156 (pytorch3d is not
 *   vendored: its published loop restated, parity unpinned).  Per iteration: nearest Y point of every X R + T; Kabsch alignment of
 *   the original X onto those points (centred covariance X^T Y / P, SVD with descending singular values,
 *   R = U diag(1, 1, det(U V^T)) V^T, T = mean(Y_nn) - mean(X) R); rmse = sqrt(mean |X R + T - Y_nn|^2) of the new transform over
 *   the old correspondences; relative = (previous rmse - rmse) / previous rmse, 1 on the first iteration; the batch has converged
 *   when relative <= relative_rmse_thr for every element.  The sums are taken in double over per-block partials in a fixed order
 *   and the 3x3 is solved in double on the device; three launches per iteration, no host value inside one.
 *   State, caller-owned device memory: R [N,3,3] and T [N,3] fp32, rmse [N,2] fp64 {this iteration's, the previous one's},
 *   status int32 [2] {stop flag, iterations done}.  lasr_icp_init sets R = I, T = 0, status = {0, 0} and arms the workspace.
 *   lasr_icp_iterate enqueues n_iters iterations without synchronising; every kernel reads the stop flag first and returns without
 *   writing once it is set, so the state stays that of the converging iteration.  The caller reads status[0] between calls.
 *   workspace: lasr_icp_workspace_bytes(N, P, Q), the same buffer for init and every iterate of a run.
 * lasr_icp_kabsch_host: TEST / DIAGNOSTIC entry, not part of the evaluation path and launching nothing: the alignment step alone, on the host, from the fifteen sums over P pairs {sum x (3), sum y (3),
 *   sum x_i y_j (9, row-major)}; the same code the device runs (tests compare it with a LAPACK SVD without a GPU).
 * Checked on the host before any launch (LASR_E_BADARG): N >= 0 (ICP: 1 <= N <= LASR_ICP_MAX_BATCH), N <= 65535,
 *   P >= 0 (chamfer3d, ICP: >= 1), Q >= 1, P, Q <= 2^27, 0 <= splits <= 65535, 0 <= n_iters <= LASR_ICP_MAX_CHUNK, R and T both
 *   NULL or neither, every other pointer non-NULL when there is work; LASR_E_WORKSPACE for a workspace that is too small.
 *   The *_workspace_bytes functions return 0 for sizes the calls refuse.
 */
#define LASR_NN_TILE 512
#define LASR_ICP_MAX_BATCH 64
#define LASR_ICP_MAX_CHUNK 4096
size_t lasr_chamfer3d_workspace_bytes(int N, int P, int Q);
int lasr_nn_tiled(const float* a, const float* b, const float* R, const float* T, float* d2, int* idx, void* workspace,
                  size_t workspace_bytes, int N, int P, int Q, int splits, void* hip_stream);
int lasr_chamfer3d_forward(const float* xyz1, const float* xyz2, float* dist1, float* dist2, int* idx1, int* idx2, void* workspace,
                           size_t workspace_bytes, int N, int P, int Q, int splits, void* hip_stream);
int lasr_chamfer3d_backward(const float* xyz1, const float* xyz2, const int* idx1, const int* idx2, const float* grad_dist1,
                            const float* grad_dist2, const int* row_ptr1, const int* col1, const int* row_ptr2, const int* col2,
                            float* grad_xyz1, float* grad_xyz2, int N, int P, int Q, void* hip_stream);
size_t lasr_icp_workspace_bytes(int N, int P, int Q);
int lasr_icp_init(float* R, float* T, double* rmse, int* status, void* workspace, size_t workspace_bytes, int N, int P, int Q,
                  void* hip_stream);
int lasr_icp_iterate(const float* X, const float* Y, float* R, float* T, double* rmse, int* status, void* workspace,
                     size_t workspace_bytes, int N, int P, int Q, int n_iters, double relative_rmse_thr, int splits, void* hip_stream);
int lasr_icp_kabsch_host(const double* moments, int P, float* R, float* T);   /* test / diagnostic hook, see above */

/*
 * ---- VCN optical flow, matching stage of preprocess/auto_gen.py (lasr_amd/csrc/vcn.hip, lasr_amd/ext_nnutils/vcn.py) -------
 * All tensors are contiguous fp32 device arrays; U = 2 md + 1 displacements along x, V = 2 mdv + 1 along y (mdv = md // fac).
 *
 * lasr_vcn_corr_proj replaces VCN.cost_matching's normalisation, warp and corrf (third_party/ext_nnutils/VCNplus.py:384-394,
 *   129-148, 350-373) and butterfly4D.proj's projfeat4d 1x1 projection with its BatchNorm (conv4d.py:181, 226-235), eval mode:
 *   c1n = c1 / (||c1|| + 1e-9), c2n likewise over the C channels of each pixel; t = c2n when flow is NULL (level 0), else
 *   grid_sample(c2n, q + flow(q), align_corners=True) zeroed unless |vgrid| < 1 in both axes; then
 *   out[b, f, u, v, y, x] = scale[f] * sum_c proj_w[f, c] * lrelu_0.1(c1n[b, c, y, x] * t[b, c, y + v - mdv, x + u - md]) + shift[f]
 *   with t = 0 outside the image (those entries are exactly shift[f]).  scale = gamma / sqrt(running_var + eps) and
 *   shift = beta - running_mean * scale are folded on the host.  The [b, C, U, V, h, w] cost volume is never formed.
 *   c1, c2 [B, C, H, W]; flow [B, 2, H, W] (x, y) or NULL; proj_w [F, C]; scale, shift [F]; out [B, F, U, V, H, W];
 *   workspace >= lasr_vcn_corr_proj_workspace_bytes(B, H, W) (per-pixel inverse norms).
 * lasr_vcn_flow_reg replaces flow_reg.forward (VCNplus.py:68-112) and the up-flow addition of cost_matching (:401-406):
 *   per hypothesis n = b * F + f and pixel, over cost[n, :, :, pixel] of [B, F, U, V, H, W]: first-index argmax, softmax over the
 *   7 x 7 (u, v) window around it clipped to the grid, flow = expected (u - md, v - mdv) (+ up_flow[b] when not NULL), local
 *   entropy / log 49 and global entropy (softmax over all U V) / log(U V), p clamped to [1e-9, 1 - 1e-9].
 *   flow, ent [B, 2F, H, W]: channel 2f = x-flow / local entropy, 2f + 1 = y-flow / global entropy of hypothesis f.
 * Checked on the host before any launch (LASR_E_BADARG): B >= 1, 1 <= md <= LASR_VCN_MAX_DISP, 0 <= mdv <= md, H, W >= 1,
 *   corr_proj: 1 <= C <= LASR_VCN_MAX_CHANNELS, F in {12, 16}, B (2 mdv + 1) <= 65535; flow_reg: 1 <= F <= LASR_VCN_MAX_HYPOTHESES,
 *   B F <= 65535; every pointer except flow / up_flow non-NULL; a short workspace is LASR_E_WORKSPACE.
 */
#define LASR_VCN_MAX_DISP 7
#define LASR_VCN_MAX_CHANNELS 1024
#define LASR_VCN_MAX_HYPOTHESES 1024
size_t lasr_vcn_corr_proj_workspace_bytes(int B, int H, int W);     /* 0 for invalid sizes */
int lasr_vcn_corr_proj(const float* c1, const float* c2, const float* flow, const float* proj_w, const float* scale,
                       const float* shift, float* out, void* workspace, size_t workspace_bytes, int B, int C, int F, int H, int W,
                       int md, int mdv, void* hip_stream);
int lasr_vcn_flow_reg(const float* cost, const float* up_flow, float* flow, float* ent, int B, int F, int H, int W, int md, int mdv,
                      void* hip_stream);

/*
 * ---- small-tensor glue of LASR.forward as single kernels (lasr_amd/csrc/glue.hip) -----------------------------------
 *
 * Rotation distance, third_party/ext_utils/util_rot.py:27-37 (called at nnutils/mesh_net.py:508 / :516): m1, m2 [n,3,3]
 * row-major -> angle [n] = acos((trace(m1 m2^T) - 1) / 2); where |cos| >= 1 the angle is 0 / pi with zero gradient (the
 * reference's acos(min(cos, 1)) back-propagates NaN there and its trainer skips the step).
 */
int lasr_geodesic_forward(const float* m1, const float* m2, float* angle, int n, void* hip_stream);
int lasr_geodesic_backward(const float* m1, const float* m2, const float* grad_angle, float* grad_m1, float* grad_m2, int n,
                           void* hip_stream);

/*
 * total = sum_t weights[t] * mean(terms[t]) -- the reference's chain `total_loss += w * x.mean()` at
 * nnutils/mesh_net.py:374-530.  terms: HOST array of n_terms device pointers (each a contiguous fp32 tensor of numels[t]
 * elements), weights / groups: host arrays; out [n_groups + 1] (device): out[g] = sum of the weighted means of group g (the
 * per-loss scalars LASR logs: mask_loss, flow_rd_loss, ...), out[n_groups] = total, both accumulated in term order.
 * Backward: coef[t] = grad_total * weights[t] / numels[t] (the gradient of every element of term t).
 */
#define LASR_MEANS_MAX_TERMS 24
int lasr_weighted_means_forward(const float* const* terms, const int* numels, const float* weights, const int* groups,
                                int n_terms, int n_groups, float* out, void* hip_stream);
int lasr_weighted_means_backward(const int* numels, const float* weights, int n_terms, const float* grad_total, float* coef,
                                 void* hip_stream);

/*
 * Intrinsics bookkeeping of the image pair, nnutils/mesh_net.py:204-217.  cams [2B, cam_stride] (column 0 = crop scale; rows
 * 0..B-1 frames t, B..2B-1 frames t'), pp [2B,2], predicted scale [2B,H], depth [2B,K], ppoint [2B,2], half_size = img_size/2:
 *   scale_out = cams0 * scale;  depth_out = depth with column 0 multiplied by cams0;
 *   ppoint_out[:B] = ppoint[:B];  ppoint_out[B+i] = (ppoint[i] + cams0_i pp_i / half + 1) * (cams0_{B+i} / cams0_i)
 *                                                   - cams0_{B+i} pp_{B+i} / half - 1
 * Backward: gradients w.r.t. scale, depth, ppoint (rows B.. of ppoint receive 0: the reference discards that prediction).
 */
int lasr_intrinsics_forward(const float* cams, int cam_stride, const float* pp, const float* scale, const float* depth,
                            const float* ppoint, float* scale_out, float* depth_out, float* ppoint_out, int B, int H, int K,
                            float half_size, void* hip_stream);
int lasr_intrinsics_backward(const float* cams, int cam_stride, const float* grad_scale_out, const float* grad_depth_out,
                             const float* grad_ppoint_out, float* grad_scale, float* grad_depth, float* grad_ppoint, int B, int H,
                             int K, void* hip_stream);

/*
 * Bone-transform fix-up, nnutils/mesh_net.py:259-283.  quat [M,K,9]: the 3x3 Q the pose head
 * predicts per (image-hypothesis m = image * H + h, bone k); trans [M*K,2], depth [M*K]; rest_ts [H,K-1,3] joint centres.
 *   root k = 0:  rmat = Q^T, tmat = (trans, depth)
 *   bone k >= 1: rmat = Q,   tmat = -Q^T c + (trans, depth) + c,  c = rest_ts[h, k-1]      (rotation about the joint)
 * rmat [M*K,3,3], tmat [M*K,3].  Backward: gradients of quat, trans, depth and rest_ts (summed over the images, in image
 * order: deterministic).  rest_ts / grad_rest may be NULL when K == 1.
 */
int lasr_bone_fixup_forward(const float* quat, const float* trans, const float* depth, const float* rest_ts, float* rmat,
                            float* tmat, int M, int H, int K, void* hip_stream);
int lasr_bone_fixup_backward(const float* quat, const float* rest_ts, const float* grad_rmat, const float* grad_tmat,
                             float* grad_quat, float* grad_trans, float* grad_depth, float* grad_rest, int M, int H, int K,
                             void* hip_stream);
/* The same with the rotation distance between the two frames of every pair riding along (nnutils/mesh_net.py:514-516,
 * third_party/ext_utils/util_rot.py:27-37): pair_angle[i] = angle(Q[i], Q[i + M*K/2]) for i < M*K/2 (M even: first half of the batch =
 * frame t, second half = frame t') -- the values and gradients of lasr_geodesic_forward / _backward on (Q[:half], Q[half:]),
 * bit for bit, without their two launches; grad_quat = the fix-up's part + the distance's part. */
int lasr_bone_fixup_pair_forward(const float* quat, const float* trans, const float* depth, const float* rest_ts, float* rmat,
                                 float* tmat, float* pair_angle, int M, int H, int K, void* hip_stream);
int lasr_bone_fixup_pair_backward(const float* quat, const float* rest_ts, const float* grad_rmat, const float* grad_tmat,
                                  const float* grad_pair_angle, float* grad_quat, float* grad_trans, float* grad_depth,
                                  float* grad_rest, int M, int H, int K, void* hip_stream);

/*
 * Symmetric squared Chamfer distance of small point sets -- pytorch3d.loss.chamfer_distance()[0] as used on the bones' control
 * points at nnutils/mesh_net.py:500-503: a [N,P,3], b [N,Q,3] -> out[n] = mean_i min_j |a_i - b_j|^2 + mean_j min_i |b_j - a_i|^2
 * (the caller averages over n); nn_ab [N,P] / nn_ba [N,Q] int32 receive the nearest indices (first minimum) for the backward,
 * which writes grad_a [N,P,3] and grad_b [N,Q,3] for an upstream grad_out [N] by gathers (no atomics).
 */
int lasr_chamfer_forward(const float* a, const float* b, float* out, int* nn_ab, int* nn_ba, int N, int P, int Q,
                         void* hip_stream);
int lasr_chamfer_backward(const float* a, const float* b, const int* nn_ab, const int* nn_ba, const float* grad_out, float* grad_a,
                          float* grad_b, int N, int P, int Q, void* hip_stream);

/*
 * Mean shape of the batch, third_party/ext_nnutils/mesh_net.py:128-149 (symmetrize) + :171-185 (get_mean_shape): mean_v / tex
 * [H,Vp,3] (independent + right-half vertices per hypothesis) -> out_v / out_tex [R*H, Vp+S, 3]: the last S vertices are appended
 * once more mirrored (flip [3], e.g. (-1,1,1)), positions are multiplied by mask [Vp+S,3] (NULL = none; zeros pin the plane
 * vertices), colours go through a sigmoid, and the H meshes are tiled R times (one per image).  S = 0: no symmetry.
 * Backward: grad_mean_v / grad_tex_param [H,Vp,3] (either may be NULL), summed over the R copies in order.
 */
int lasr_mean_shape_forward(const float* mean_v, const float* tex, const float* flip, const float* mask, float* out_v,
                            float* out_tex, int R, int H, int Vp, int S, void* hip_stream);
int lasr_mean_shape_backward(const float* tex, const float* flip, const float* mask, const float* grad_v, const float* grad_tex,
                             float* grad_mean_v, float* grad_tex_param, int R, int H, int Vp, int S, void* hip_stream);

/*
 * Observed images of the texture losses, nnutils/mesh_net.py:364-366: fg = masks > 0; out[:n] = imgs * fg (object on black),
 * out[n:] = 1 - fg + imgs * fg (object on white).  imgs [n,3,P], masks [n,P] -> out [2n,3,P]; data only, no gradient.
 */
int lasr_obs_pair(const float* imgs, const float* masks, float* out, int n, int P, void* hip_stream);

/*
 * A training batch as one row gather: the input side of LASRTrainer.set_input, nnutils/train_utils.py:125-181, for a sequence
 * that is resident in HBM.  table [pairs, W] holds, per distinct frame pair, the model's batch
 * dictionary of that pair key after key (key k at columns [seg_off[k], seg_off[k] + seg_len[k]), frame t then frame t');
 * ids [B] (int64, device) selects the pairs; out receives key k's [B, seg_len[k]] block at out_off[k] -- pair-major, the
 * interleaved layout of train_utils.py:179-180.  One launch; n_keys <= LASR_GATHER_MAX_KEYS.  The offset arrays are HOST memory.
 */
/*
 * Everything LASR.forward does with the render between the rasteriser and the loss sum, in one pass over the [N,10,P] output of
 * the nine-attribute render (planes 0-2 texture colours, 3-5 own camera-space position, 6-8 the other frame's position, 9 alpha;
 * N = I*H images, image ij = i*H + j, first half of the batch = frame t, second half = frame t') and one pass back:
 *   flow reprojection + background mask (nnutils/mesh_net.py:87-104), silhouette table (:374-390), flow table + weighted error
 *   map + selection mask (:393-416), texture L1 table (:419-441), and the perceptual network's input pair
 *   rndpair [2N,3,P] = (render * alpha | render) (:436-441; pass NULL to skip it).
 * masks / occ [I,P]; flow_obs [I,C>=2,P] with image stride flow_obs_image_stride; img_obs / img_white [I,3,P]; pp [N,2], fl [N]:
 * image n projects its own position with (pp[n], fl[n]) (no gradient) and the other frame's with (pp[o], fl[o]), o = (n + N/2) % N.
 * Tables [I,H] are bit-identical to lasr_mask_loss_* / lasr_flow_loss_* / lasr_tex_loss_* on contiguous copies of the planes.
 * Backward: grad_px [N,10,P] is written whole (zeros on planes 3-5), grad_pp [N,2], grad_fl [N]; grad_rndpair may be NULL.
 * scratch: lasr_render_tables_scratch_floats(I,H,P) floats, carried from forward to backward.
 */
size_t lasr_render_tables_scratch_floats(int I, int H, int P);
int lasr_render_tables_forward(const float* px, const float* masks, const float* occ, const float* flow_obs,
                               long long flow_obs_image_stride, const float* img_obs, const float* img_white, const float* pp,
                               const float* fl, float l1tex_wt, float* mask_tab, float* flow_tab, float* tex_tab, float* flow_rd,
                               unsigned char* bgmask, float* flow_map, unsigned char* vis_mask, float* rndpair, float* scratch,
                               int I, int H, int P, void* hip_stream);
/* The same pass from the observed images themselves (round 6): imgs [I,3,P]; the object on black and on white (nnutils/mesh_net.py:364-366,
 * lasr_obs_pair's values) is formed inside and written to obs_pair_out [2I,3,P] (black first) -- what the backward and the perceptual
 * term take as img_obs / img_white.  One launch (lasr_obs_pair) and three input planes less than the call above; same tables. */
int lasr_render_tables_forward_imgs(const float* px, const float* masks, const float* occ, const float* flow_obs,
                                    long long flow_obs_image_stride, const float* imgs, float* obs_pair_out, const float* pp,
                                    const float* fl, float l1tex_wt, float* mask_tab, float* flow_tab, float* tex_tab, float* flow_rd,
                                    unsigned char* bgmask, float* flow_map, unsigned char* vis_mask, float* rndpair, float* scratch,
                                    int I, int H, int P, void* hip_stream);
int lasr_render_tables_backward(const float* px, const float* masks, const float* occ, const float* flow_obs,
                                long long flow_obs_image_stride, const float* img_obs, const float* img_white, const float* pp,
                                const float* fl, float l1tex_wt, const float* grad_mask_tab, const float* grad_flow_tab,
                                const float* grad_tex_tab, const float* grad_rndpair, const float* scratch, float* grad_px,
                                float* grad_pp, float* grad_fl, int I, int H, int P, void* hip_stream);

/*
 * What LASR.forward builds from the camera-space vertices before it calls the rasteriser (nnutils/mesh_net.py:298-311, :350-356;
 * geom_utils.py:27-34), in one launch + a one-block finish: verts_pre [N,V,3] = (pinhole(verts_cam; pp, fl) + eye) * (1,-1,1),
 * attrs [N,V,9] = (tex | verts_cam | verts_cam of image (n + N/2) % N), near_far [2] = (zmin - r/2, zmax + r/2), r = zmax - zmin
 * over all N meshes.  verts_cam / tex [N,V,3], pp [N,2], fl [N], eye: 3 HOST floats; scratch: 2 N floats.  N even.
 * Backward: grad_verts_cam (projection + both attribute uses), grad_tex, grad_pp [N,2], grad_fl [N], all overwritten.
 */
int lasr_raster_inputs_forward(const float* verts_cam, const float* tex, const float* pp, const float* fl, const float* eye,
                               float* verts_pre, float* attrs, float* near_far, float* scratch, int N, int V, void* hip_stream);
int lasr_raster_inputs_backward(const float* verts_cam, const float* fl, const float* grad_verts_pre, const float* grad_attrs,
                                float* grad_verts_cam, float* grad_tex, float* grad_pp, float* grad_fl, int N, int V,
                                void* hip_stream);

/*
 * The same stage per FACE CORNER, one launch each way (what the rasteriser consumes; replaces, for LASR.forward's own render,
 * lasr_raster_inputs_forward + the camera stage's `vertices - eye` (third_party/softras/soft_renderer/functional/look_at.py:6-62
 * with a constant eye on the -z axis, rotation = identity) + two lasr_face_gather_forward calls, and their three backward
 * launches):
 *   face_vertices[n,f,c,:] = ((pinhole(verts_cam[n, faces[f,c]]) + eye) * (1,-1,1)) - eye          [N,F,3,3]
 *   face_attrs[n,f,c,:]    = (tex | verts_cam | verts_cam of mesh (n + N/2) % N) at that vertex      [N,F,3,9]
 *   near_far               = as lasr_raster_inputs_forward
 * faces: int64 [N,F,3], or [1,F,3] with faces_shared = 1 (all meshes share the connectivity).  Backward: the vertex-centric sums
 * run over a CSR incidence structure the caller builds once per connectivity: inc_ptr int32 [N or 1, V+1], inc int32 [N or 1, 3F] =
 * corner ids (3 f + c) grouped by vertex, ASCENDING inside a vertex (the summation order of lasr_face_gather_backward).
 * scratch: lasr_raster_faces_scratch_floats(N, V, F) floats (either direction; block partials of the depth range / of the
 * intrinsics' gradients, folded by a second small launch).
 */
size_t lasr_raster_faces_scratch_floats(int N, int V, int F);
int lasr_raster_faces_forward(const float* verts_cam, const float* tex, const float* pp, const float* fl, const float* eye,
                              const long long* faces, int faces_shared, float* face_vertices, float* face_attrs, float* near_far,
                              float* scratch, int N, int V, int F, void* hip_stream);
int lasr_raster_faces_backward(const float* verts_cam, const float* fl, const int* inc_ptr, const int* inc, int faces_shared,
                               const float* grad_face_vertices, const float* grad_face_attrs, float* grad_verts_cam,
                               float* grad_tex, float* grad_pp, float* grad_fl, float* scratch, int N, int V, int F,
                               void* hip_stream);

#define LASR_GATHER_MAX_KEYS 24
int lasr_gather_rows(const float* table, long long W, int pairs, const long long* ids, int B, int n_keys,
                     const long long* seg_off, const long long* seg_len, const long long* out_off, float* out,
                     void* hip_stream);

/*
 * The optimisation-step tail, nnutils/train_utils.py:282-296: clip the mean-shape gradient to
 * norm max_norm_shape (1) and the encoder + code-predictor gradients jointly to max_norm_cam (10) with
 * torch.nn.utils.clip_grad_norm_'s coefficient min(1, max / (norm + 1e-6)); if ANY gradient element is NaN / Inf every gradient
 * becomes zero (the reference's zero_grad()) and the update still runs; then AdamW (decoupled weight decay, torch.optim.AdamW
 * arithmetic: p -= lr wd p; m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)) on
 * every tensor, and each tensor's step counter += 1.  Three launches over all tensors, no host synchronisation.
 *   table   device array, one row of 8 x 64 bit per tensor: {param, grad, exp_avg, exp_avg_sq, step (float*, may be 0), numel,
 *           group index, clip class (0 none, 1 mean shape, 2 camera networks)}
 *   chunks  device int32 [n_chunks, 2] = (table row, element offset), one per lasr_tail_chunk_elems() elements of a tensor
 *   partials device DOUBLE [n_chunks] scratch (sums of squares cannot overflow into a false NaN verdict); ctl device float [8]:
 *   ctl[6] counts the steps whose gradients were zeroed (the caller zeroes it once); out {clip coefficient shape, cam, all-finite flag,
 *           shape gradient norm after clipping, camera-network gradient norm before clipping, norm of all gradients}
 *   lr .. weight_decay: HOST arrays per parameter group (n_groups <= LASR_TAIL_MAX_GROUPS); bias_correction1/2 = 1 - beta^t of
 *           the step being taken, evaluated by the caller in double.
 */
#define LASR_TAIL_MAX_GROUPS 16
int lasr_tail_chunk_elems(void);
int lasr_tail_step(const void* table, const int* chunks, int n_chunks, double* partials, float* ctl, float max_norm_shape,
                   float max_norm_cam, const float* lr, const float* beta1, const float* beta2, const float* eps,
                   const float* weight_decay, const double* bias_correction1, const double* bias_correction2, int n_groups,
                   void* hip_stream);

/*
 * Plumbing around the raster calls.
 * lasr_fill_planes: dst [N, n_values, plane_elems], plane c of every image := values[c] (host array) -- the background fill the
 *   reference does before its forward kernel (third_party/softras/soft_renderer/functional/soft_rasterize.py:50-53: colour planes =
 *   background, alpha plane = 1).
 */
#define LASR_FILL_MAX_PLANES 16
int lasr_fill_planes(float* dst, const float* values, int n_values, int N, long long plane_elems, void* hip_stream);

/*
 * ---- Training monitor: flow colour coding, epoch contact sheet, scalar ring (lasr_amd/csrc/flowvis.hip) --
 * Statistics scratch: caller-owned device words that are ZERO before the first call; every call leaves them zero again (the last
 * block of its second launch clears them), so one buffer serves any number of calls on one stream and no memset precedes a call.
 *
 * lasr_flow_to_image replaces flow_to_image / compute_color / make_color_wheel (third_party/ext_utils/flowlib.py:45-173), batched.
 *   flow [B,H,W,C] fp32, C in {2, 3}, channels 0 and 1 read; mask NULL or [B,H,W] fp32: u = v = 0 where the mask is 0, before
 *   anything else (gu[~mask] = 0 of nnutils/train_utils.py:307,311); out [B,H,W,3] uint8 RGB, 4-byte aligned;
 *   stats_scratch: lasr_flow_to_image_scratch_bytes(B) bytes.
 *   A sample with |u| or |v| > 1e7 counts as (0, 0) for the maximum and comes out black (flowlib.py:59-61, 77-78); so does a NaN
 *   sample (the reference's maximum with a NaN is an accident of Python's max()).  Per image: maxrad = max sqrt(u^2+v^2);
 *   (u, v) /= maxrad + 2.22e-16; rad = |(u, v)|; fk = (atan2(-v, -u)/pi + 1)/2 * 54 + 1; k0 = floor(fk), k1 = k0 + 1 (56 -> 1),
 *   f = fk - k0; per channel col = (1 - f) wheel[k0-1]/255 + f wheel[k1-1]/255; rad <= 1: col = 1 - rad (1 - col), else
 *   col *= 0.75; out = floor(255 col).  Two launches: per-image maximum (wave, LDS, one integer atomicMax per block on the
 *   radius' bit pattern: order-independent), then the colours, four consecutive pixels per lane.
 *   B == 0 or H * W == 0: LASR_OK, nothing launched.  LASR_E_BADARG: C not in {2, 3}, a negative size, B > 65535,
 *   B H W > 2^29, flow / out / stats_scratch NULL, out not 4-byte aligned.
 *
 * lasr_monitor_sheet composes the images the reference logs once per epoch (nnutils/train_utils.py:303-329) as one
 *   [3 IS, 3 IS, 3] uint8 sheet, tiles in row-major order: flowobs, flowrd (colour coded as above, masked by vis_mask),
 *   flow_error (flow_err * vis_mask, min-max scaled to grey), mask (mask_pred, min-max), maskgt (mask_gt, min-max), part,
 *   img1, img2, texture (floor(255 x) clipped to 0..255; part.ptr == NULL: a black tile).  Min-max scaling is
 *   floor(255 (x - min) / (max - min)) clipped; a constant panel comes out 0, NaN samples take no part and come out 0.
 *   Over the texture tile, for k < n_ctl in order: the pixels (row r, column c) with 1.5^2 <= (c - cx)^2 + (r - cy)^2 <= 4.5^2,
 *   (cx, cy) = IS/2 + IS/2 * ctl[k * ctl_stride + {0, 1}], take floor(palette[3k + {0,1,2}]) (palette in 0..255); this stands in
 *   for cv2.circle(centre, 3, colour, 3) of :328.  Every plane is described by (ptr, chan_stride, pix_stride) in floats: channel c
 *   of pixel i = r * IS + c is ptr[c * chan_stride + i * pix_stride], so planar and interleaved tensors and views need no copy.
 *   One statistics launch (two maximum radii, three min / max pairs) and one compose launch.
 *   stats_scratch: lasr_monitor_sheet_scratch_bytes() bytes.  IS == 0: LASR_OK.  LASR_E_BADARG: IS < 0 or > LASR_SHEET_MAX_SIZE,
 *   a NULL plane other than part, out not 4-byte aligned, n_ctl < 0, n_ctl > 0 with ctl or palette NULL or ctl_stride < 2.
 *
 * lasr_scalar_ring_push replaces the per-step log.add_scalar(x.mean()) calls of nnutils/train_utils.py:330-344 (each a host
 *   synchronisation there).  table: K rows of two int64 on the device {address of fp32 values, count}; writes
 *   ring[(*head % capacity) * K + k] = mean of row k's values (NaN for a NULL address or count <= 0), then *head += 1.
 *   One launch of one block; lane l of a wave adds elements l, l + 64, ... in order and the 64 partial sums fold through a fixed
 *   butterfly: no float atomics, the same bits every time.  The host reads nothing: it drains the ring with a plain device-to-host
 *   copy of lasr_scalar_ring_bytes(capacity, K) bytes.  K == 0: LASR_OK.  LASR_E_BADARG: K < 0 or > LASR_RING_MAX_SCALARS,
 *   capacity < 1, a NULL pointer.  lasr_scalar_ring_bytes returns 0 for sizes the push refuses.
 */
#define LASR_SHEET_MAX_SIZE 4096
#define LASR_RING_MAX_SCALARS 256
typedef struct lasr_sheet_plane {
    const float* ptr;
    long long chan_stride;
    long long pix_stride;
} lasr_sheet_plane;
typedef struct lasr_sheet_inputs {
    lasr_sheet_plane flow_obs, flow_rd, vis_mask, flow_err, mask_pred, mask_gt, part, img1, img2, texture;
    const float* ctl;        /* [n_ctl, ctl_stride]: projected bone centres, x and y in NDC (-1 .. 1) */
    const float* palette;    /* [n_ctl, 3] ring colours, 0..255 */
    int n_ctl;
    int ctl_stride;
} lasr_sheet_inputs;
size_t lasr_flow_to_image_scratch_bytes(int B);      /* 0 for B < 0 */
int lasr_flow_to_image(const float* flow, const float* mask, unsigned char* out, void* stats_scratch, int B, int H, int W, int C,
                       void* hip_stream);
size_t lasr_monitor_sheet_scratch_bytes(void);
int lasr_monitor_sheet(const lasr_sheet_inputs* in, unsigned char* out, void* stats_scratch, int IS, void* hip_stream);
size_t lasr_scalar_ring_bytes(int capacity, int K);
int lasr_scalar_ring_push(const void* table, int K, float* ring, unsigned* head, int capacity, void* hip_stream);

/*
 * ---- Texture baking of scripts/bake_texture.py (lasr_amd/csrc/bake.hip, lasr_amd/nnutils/bake.py) --------
 * This project's own addition: the reference has no counterpart, nothing of it is restated here, and parity is to the float64
 * restatement in tests/bake_restated.py only.  The pair fills the per-face surface textures [F, R*R, 3] the rasteriser samples
 * (texture_type 'surface') from T video frames with one camera-space mesh each (shared faces); it stands in for the per-vertex
 * colours that are otherwise the only appearance of a reconstruction.
 *
 * lasr_bake_accumulate stands in for a per-texel loop "project into every frame, test visibility, add the weighted colour":
 *   verts  [T,V,3]      camera space, OpenCV axes (x right, y down, z forward)
 *   faces  [F,3]        int32, shared by the frames; a face with an index outside [0, V) is left untouched
 *   K      [T,4]        fx fy px py in pixels of the H x W frame (16-byte aligned)
 *   raster [T,2,IS,IS]  hard-mode aggrs_info of lasr_sr_forward_bg (func_id_rgb = func_id_alpha = 0) under the NDC mapping
 *                       sx = 2u/IS - 1, sy = 1 - 2v/IS: plane 1 names the nearest face of pixel (row floor(v), column floor(u)), or -1
 *   frames [T,H,W,3]    uint8;  masks [T,H,W] uint8 or NULL
 *   accum  [F,R*R,4]    fp32 (sum w r, sum w g, sum w b, sum w), 16-byte aligned; read, added to and written back, so the caller
 *                       zeroes it once and may pass the frames of a sequence in any number of consecutive calls
 *   Texel j = iy R + ix samples the centroid of the barycentric region surface_texel(c0, c1, R) maps to j:
 *   ix + iy <= R-1: (c0, c1) = ((ix + 1/3)/R, (iy + 1/3)/R), else ((R-1-ix + 2/3)/R, (R-1-iy + 2/3)/R); c2 = 1 - c0 - c1, c_k weighs
 *   corner k.  Per frame, in increasing order: P = c0 V0 + c1 V1 + c2 V2, skipped unless P.z > 0; u = fx P.x/P.z + px,
 *   v = fy P.y/P.z + py (pixel (r, c) covers u in [c, c+1), v in [r, r+1)), skipped unless 0 <= u < W and 0 <= v < H; visible when
 *   the raster names this face at (floor(v), floor(u)) and, with masks, the mask is > 0 at all four bilinear taps; colour = bilinear
 *   sample of the frame at (u - 0.5, v - 0.5), taps clamped to the frame, / 255; w = |n . P/|P||^power with n the unit face normal
 *   (power = 0: w = 1; a zero-area face: 0).  One thread per texel, no atomics: the same bits for any split of the frames.
 * lasr_bake_resolve: textures [F,R*R,3] = accum.rgb / accum.w where accum.w > 0, else the fallback vertex colour [V,3] interpolated
 *   at the texel's centroid (fallback NULL: 0.5 grey); weight [F,R*R] = accum.w.
 * Checked on the host before any launch (LASR_E_BADARG): T >= 0, V >= 1, F >= 0, 1 <= R <= LASR_BAKE_MAX_RES,
 *   1 <= H, W <= IS <= LASR_BAKE_MAX_SIZE, 0 <= power <= LASR_BAKE_MAX_POWER, 4 F R R <= INT_MAX; then T == 0 or F == 0 is LASR_OK
 *   with nothing launched; then every pointer but masks / fallback non-NULL.  Device contents are not read on the host.
 */
#define LASR_BAKE_MAX_RES 32
#define LASR_BAKE_MAX_SIZE 8192
#define LASR_BAKE_MAX_POWER 16
int lasr_bake_accumulate(const float* verts, const int* faces, const float* K, const float* raster, const unsigned char* frames,
                         const unsigned char* masks, float* accum, int T, int V, int F, int R, int IS, int H, int W, int power,
                         void* hip_stream);
int lasr_bake_resolve(const float* accum, const int* faces, const float* fallback, float* textures, float* weight, int V, int F,
                      int R, void* hip_stream);

/*
 * ---- Completing a baked atlas where no frame looked (lasr_amd/csrc/bake_fill.hip, nnutils/bake.py) --------
 * This project's own addition, like the bake: the reference has no counterpart, nothing of it is restated here, and parity is to
 * the float64 / float32 restatement in tests/bake_fill_restated.py and to closed forms only.  A texel with weight == 0 first takes
 * the colour of its mirror image on the bilaterally symmetric rest shape (lasr_bake_mirror), then what is still unfilled is
 * smoothed from its neighbours (lasr_bake_blend, one Jacobi iteration per call).  Neither kernel is in the lasr_prof_* table.
 *
 * lasr_bake_mirror:
 *   rest_verts [V,3]     the rest mesh (rig.npz of extract.py --rig), symmetric about the plane x[axis] = 0
 *   faces      [F,3]     int32; a face with an index outside [0, V) is no source, and its own texels are not filled
 *   texels     [M]       int32, the texels to fill as i = f R R + j (the caller lists those with weight == 0); an entry outside
 *                        [0, F R R) is skipped
 *   textures   [F,R*R,3], weight [F,R*R]   what lasr_bake_resolve wrote; read only
 *   out_textures [F,R*R,3]   only the three floats of every filled texel are written (the caller passes a copy of textures);
 *                        must not overlap textures
 *   src [M] int32, d2 [M] fp32   always written, see below
 *   Per entry m with texel (f, j): p = c0 V0 + c1 V1 + c2 V2 at the centroid (c0, c1, c2) of texel j (as lasr_bake_accumulate), p'
 *   = p with coordinate `axis` negated.  g = the face of smallest squared distance to p' among the faces with indices in [0, V)
 *   (point_triangle.h: interior projection or the nearest clamped edge projection), the lowest face index among equal distances;
 *   d2[m] = that distance (+inf when there is none), (b0, b1, b2) = the barycentrics of the closest point.  Refused, src[m] = -1 - reason:
 *     reason 3 (LASR_BAKE_MIRROR_NO_FACE)   the entry is out of range, face f has an index outside [0, V), or no face is valid;
 *     reason 0 (LASR_BAKE_MIRROR_FAR)       not d2 <= max_d2;
 *     reason 1 (LASR_BAKE_MIRROR_NORMAL)    not n(f)' . n(g) > 0, with n = (V1 - V0) x (V2 - V0) unnormalised and n(f)' = n(f) with
 *                                           coordinate `axis` negated (a zero-area f or g gives 0: refused);
 *     reason 2 (LASR_BAKE_MIRROR_UNSEEN)    not weight[g, j'] > 0, with j' = surface_texel(b0', b1', R) (sr_device.h) of
 *                                           b_k' = b_k (1 - 2^-20) + 2^-20 / 3: the closest point pulled a millionth of the face
 *                                           towards its centroid, so that a point on an edge or a corner of g (b0 = 1, or b0 + b1
 *                                           rounded above 1) names a texel that touches it.
 *   Otherwise out_textures[f, j] = textures[g, j'] (the same bits) and src[m] = g R R + j'.  Only texels a frame saw are sources:
 *   fills do not chain, and the result does not depend on any order.  One entry per lane, 256 per block; the faces pass through
 *   LDS in tiles of LASR_BAKE_FILL_TILE; no atomics.
 * lasr_bake_blend: one Jacobi iteration over the texel adjacency; in, out [F,R*R,3], fixed [F,R*R] uint8, nbr [F,3] int32.
 *   Corner k of a face is weighed by c_k; face edge k is c_k = 0, from end p to end q = corners (1,2), (2,0), (0,1) for k = 0, 1, 2.
 *   Texel j = iy R + ix is the lower triangle L(ix, iy) when ix + iy <= R-1, else the upper triangle U(cx, cy), cx = R-1-ix,
 *   cy = R-1-iy.  L(ix, iy) has the neighbours n0 = U(ix-1, iy) if ix >= 1 else across face edge 0, n1 = U(ix, iy-1) if iy >= 1
 *   else across face edge 1, n2 = U(ix, iy) if ix + iy <= R-2 else across face edge 2; U(cx, cy) has n0 = L(cx+1, cy),
 *   n1 = L(cx, cy+1), n2 = L(cx, cy).  Along face edge k a border texel has the slot s counted from end p: R-1-iy (k = 0), ix
 *   (k = 1), iy (k = 2); the texel of slot s is (ix, iy) = (0, R-1-s), (s, 0), (R-1-s, s).  nbr[f, k] = ((g 3 + k') 2 + same)
 *   names the face g and its edge k' on the other side (slot s' = s when same = 1: end p of both edges is the same vertex; else
 *   s' = R-1-s), or is negative: no neighbour.  A code that names a face outside [0, F) counts as negative.
 *   fixed != 0: out = in.  Else out = (((0 + n0) + n1) + n2) / count per channel over the neighbours that exist, in that order,
 *   fp32 without contraction; count == 0: out = in.
 * Checked on the host before any launch (LASR_E_BADARG): V >= 1, F >= 0, 1 <= R <= LASR_BAKE_MAX_RES, 4 F R R <= INT_MAX (blend
 *   also: 6 F + 5 <= INT_MAX, the range of an nbr code); M >= 0; axis in 0..2; max_d2 >= 0 and finite; then M == 0 or F == 0
 *   (blend: F == 0) is LASR_OK with nothing launched; then every pointer non-NULL, out_textures != textures, in != out.  Device
 *   contents are not read on the host.
 */
#define LASR_BAKE_FILL_TILE 256
#define LASR_BAKE_MIRROR_FAR 0
#define LASR_BAKE_MIRROR_NORMAL 1
#define LASR_BAKE_MIRROR_UNSEEN 2
#define LASR_BAKE_MIRROR_NO_FACE 3
int lasr_bake_mirror(const float* rest_verts, const int* faces, const int* texels, const float* textures, const float* weight,
                     float* out_textures, int* src, float* d2, int V, int F, int R, int M, int axis, float max_d2, void* hip_stream);
int lasr_bake_blend(const float* in, float* out, const unsigned char* fixed, const int* nbr, int F, int R, void* hip_stream);

/*
 * ---- Rigged glTF export of scripts/export_gltf.py (lasr_amd/csrc/rig.hip, lasr_amd/nnutils/rig.py) --------
 * This project's own addition: the reference has no exporter, nothing of it is restated here, and parity is to the float64
 * restatement in tests/rig_restated.py and to the project's own linear-blend skinning (lasr_lbs_forward) only.  The four entry
 * points turn what extract.py --rig writes (rest mesh, dense skin, one row-vector transform per frame and bone:
 * p_cam = (sum_k w_k (p R_k + T_k)) R_0 + T_0) into the arrays of a glTF 2.0 skin and animation, and measure what the
 * truncation to k influences costs.  All arrays are dense, row major, fp32 unless noted.
 *
 * lasr_rig_pack: skin [J,V] -> joints u8 [V,k], weights [V,k], dropped [V]; k is 4 or LASR_RIG_MAX_INFLUENCES.  Per vertex the k
 *   largest weights, a larger weight first and the lower bone index first among equal ones; s = their sum in that order,
 *   weights_i = w_i / s; a slot beyond J, or one whose weight is 0, holds joint 0 with weight 0; s == 0: joint 0 with weight 1.
 *   dropped = the sum of the weights left out, in ascending bone order.  Weights are taken to be >= 0 and finite.
 * lasr_rig_quats: R [T,K,3,3] -> quat [T,K,4]: the unit quaternion (x, y, z, w) of the column-convention rotation R^T, by
 *   Shepperd's method (the largest of the trace and the three diagonal entries picks the branch), normalised, with
 *   quat[0].w >= 0 and quat[t] . quat[t-1] >= 0 for every bone.
 * lasr_rig_skin: glTF's skinning of exactly those arrays: M_b = the matrix of quat[t,b] (standard formula, as stored) with
 *   translation trans[t,b]; out[t,v] = M_0 (sum_i weights[v,i] M_{joints[v,i] + 1} [rest[v]; 1]), i in stored order; a joint
 *   index >= K - 1 contributes nothing.  K == 1: joints and weights NULL, k == 0, out = M_0 [rest; 1].  Otherwise k is 4 or 8.
 * lasr_rig_stats: posed, ref [T,V,3] -> stats [T,8] = (max_v |posed - ref|, sum_v |posed - ref|^2, min x y z, max x y z of
 *   posed).  One block per frame: thread i folds vertices i, i + 256, ... in order, then the 256 partial results fold across
 *   halves; no atomics, two runs give the same bits.
 * Checked on the host before any launch (LASR_E_BADARG): 0 <= J <= LASR_RIG_MAX_BONES, 1 <= K <= LASR_RIG_MAX_BONES + 1 (quats:
 *   0 <= K), k as above, T, V >= 0, 3 T V <= INT_MAX; then zero work (V == 0; T == 0; quats: K == 0) is LASR_OK with nothing
 *   launched; then every pointer non-NULL (skin may be NULL for J == 0).  Device contents are not read on the host.
 */
#define LASR_RIG_MAX_BONES 64
#define LASR_RIG_MAX_INFLUENCES 8
int lasr_rig_pack(const float* skin, int J, int V, int k, unsigned char* joints, float* weights, float* dropped, void* hip_stream);
int lasr_rig_quats(const float* R, int T, int K, float* quat, void* hip_stream);
int lasr_rig_skin(const float* rest, const unsigned char* joints, const float* weights, const float* quat, const float* trans, int T,
                  int K, int V, int k, float* out, void* hip_stream);
int lasr_rig_stats(const float* posed, const float* ref, int T, int V, float* stats, void* hip_stream);

/*
 * ---- Silhouette propagation of preprocess/propagate_mask.py (lasr_amd/csrc/maskprop.hip, lasr_amd/nnutils/maskprop.py, DESIGN.md
 * section 4.13) -------------------------------------------------------------------------------------------------------------------
 * This project's own addition: the reference fills Annotations/ with a detector (preprocess/mask.py), which stays out of scope;
 * nothing of it is restated here, and parity is to the float64 restatement in tests/maskprop_restated.py and to closed forms only.
 * The three entry points carry a soft mask P_s [H,W] of a source frame s to a target frame t = s +- 1 along the optical flow (the
 * DAVIS semi-supervised protocol: the user paints one frame).  Images are uint8 [H,W,3], soft masks and fields fp32 [H,W], flows
 * fp32 [H,W,2] = (x, y) in pixels; all arrays are dense and on the device.  A colour's bin is (r>>4)<<8 | (g>>4)<<4 | (b>>4).
 *
 * lasr_maskprop_hist: hist uint32 [2, LASR_MASKPROP_BINS] += the colour counts of the pixels of the window [x0,x1) x [y0,y1) of img:
 *   row 1 (foreground) counts those with P >= hi, row 0 (background) those with P <= lo (compared in fp32; defaults 0.9 / 0.1).
 *   The counts are ADDED to what hist holds (the caller zeroes it, and sums the key frames' histogram with the running one).
 *   An LDS-private histogram per workgroup, merged with integer atomics: exact, and the same whatever the order.
 * lasr_maskprop_unary: for the pixel p of t, f = flow_ts(p), q = p + f.  q outside [0,W-1] x [0,H-1] (or not a number):
 *   prior = conf = 0; else prior = the bilinear sample of P_s at q (the upper taps clamped to the image), back = the bilinear sample of
 *   flow_st at q, conf = exp(-|f + back|^2 / (2 tau^2)).  app = log((hf[b]/Nf + eps) / (hb[b]/Nb + eps)) with b the bin of img_t(p),
 *   hf / hb rows 1 / 0 of hist and Nf / Nb their totals (0 counts as 1); app_table is scratch for the 4096 values of app.
 *   u = clamp(w_p conf logit(clamp(prior, 1e-3, 1 - 1e-3)) + w_a app, -U, U), q0 = sigmoid(u).
 *   Defaults tau 1, w_p 1, w_a 0.5, eps 1e-3, U 6.  Two launches: the table (one block), then one thread per pixel.
 * lasr_maskprop_meanfield: ONE edge-aware mean-field iteration, q_out(p) = sigmoid(u(p) + w_s sum_n k(p,n) (2 q_in(n) - 1)) over the
 *   (2R+1)^2 - 1 neighbours n inside the image, k = exp(-|I(p) - I(n)|^2 / (2 sigma_i^2) - |p - n|^2 / (2 sigma_s^2)) on the uint8
 *   colours.  q_in and q_out must differ (ping-pong; the caller launches K iterations, default 5).  Defaults R 4, sigma_i 12,
 *   sigma_s 3, w_s 0.3.  Tiles of 32 x 8 pixels, one per lane, q and the packed colours of tile + halo staged in
 *   8 (32 + 2R)(8 + 2R) bytes of LDS; the weights are recomputed per launch.
 * No entry point uses floating-point atomics: the same input gives the same bits on every run.
 * Checked on the host before any launch (LASR_E_BADARG): 0 <= H, W <= LASR_MASKPROP_MAX_SIZE, 3 H W <= INT_MAX;
 *   hist: 0 <= x0, y0, x1 <= W, y1 <= H, lo < hi; unary: tau, eps, U > 0, w_p, w_a >= 0, all finite; meanfield:
 *   0 <= R <= LASR_MASKPROP_MAX_RADIUS, sigma_i, sigma_s > 0, w_s >= 0, finite; then empty work (H == 0 or W == 0; hist: an
 *   empty window, x1 <= x0 or y1 <= y0) is LASR_OK with nothing launched; then every pointer non-NULL.  Device contents are
 *   not read on the host.  These launches are not in the lasr_prof_* kernel table.
 */
#define LASR_MASKPROP_BINS 4096
#define LASR_MASKPROP_MAX_SIZE 16384
#define LASR_MASKPROP_MAX_RADIUS 8
int lasr_maskprop_hist(const unsigned char* img, const float* P, unsigned* hist, int H, int W, int x0, int y0, int x1, int y1, float hi,
                       float lo, void* hip_stream);
int lasr_maskprop_unary(const unsigned char* img_t, const float* P_s, const float* flow_ts, const float* flow_st, const unsigned* hist,
                        float* app_table, float* u, float* q0, int H, int W, float tau, float w_p, float w_a, float eps, float U,
                        void* hip_stream);
int lasr_maskprop_meanfield(const unsigned char* img, const float* u, const float* q_in, float* q_out, int H, int W, int R,
                            float sigma_i, float sigma_s, float w_s, void* hip_stream);

/*
 * ---- Dense point tracks of scripts/export_tracks.py (lasr_amd/csrc/tracks.hip, lasr_amd/nnutils/tracks.py)
 * This project's own addition: the reference only transfers annotated keypoints between frame pairs (scripts/eval_badja.py);
 * nothing of it is restated here, and parity is to the float64 restatement in tests/tracks_restated.py and to closed forms only.
 * Query pixels are anchored on the surface in the frame they name and carried through every frame with a visibility decision.
 * Conventions are those of lasr_bake_accumulate:
 *   verts  [n,V,3]      camera space, OpenCV axes (x right, y down, z forward); the n frames of the window passed
 *   faces  [F,3]        int32, shared by all frames; a face with an index outside [0, V) anchors nothing
 *   K      [n,4]        fx fy px py in pixels of the H x W frame (16-byte aligned)
 *   raster [n,2,IS,IS]  hard-mode aggrs_info of lasr_sr_forward_bg (func_id_rgb = func_id_alpha = 0) under the NDC mapping
 *                       sx = 2u/IS - 1, sy = 1 - 2v/IS: plane 1 names the nearest face of pixel (row floor(v), column floor(u)), or -1
 *   Pixel (r, c) covers u in [c, c+1), v in [r, r+1); its centre is (c + 0.5, r + 0.5).
 *
 * lasr_track_anchor: queries [Q,3] fp32 (t, v, u) = frame position, row coordinate, column coordinate (the TAP-Vid order), t a
 *   whole number.  The call holds the frames [t0, t0 + n); a query with t outside [t0, t0 + n) is left untouched (its anchor and
 *   snapped rows are neither read nor written), so the host may walk a video in windows.  Per query of the window it writes
 *   anchors [Q] = 16-byte records (int32 face, fp32 c1, fp32 c2, fp32 facing), 16-byte aligned; face -1 = no anchor (then
 *   c1 = c2 = facing = 0), and snapped [Q,2] fp32 = the (v, u) the anchor was computed at.
 *   1. (v, u) outside 0 <= u < W, 0 <= v < H (or not a number): no anchor.  Else face = the face named at (floor v, floor u).
 *   2. If that pixel is empty and snap_radius r > 0 (at most LASR_TRACK_MAX_SNAP): among the covered pixels of the (2r+1)^2 window
 *      around it, clipped to the frame, the one whose centre is nearest to (u, v) (squared distance in fp32; ties go to the lowest
 *      flat index row * IS + col) gives the face, and (u, v) moves to that pixel's centre.  None covered: no anchor, (v, u) unmoved.
 *   3. Barycentrics by Moeller-Trumbore on the EDGE vectors e1 = V1 - V0, e2 = V2 - V0 of frame t, along the camera ray
 *      d = ((u - px)/fx, (v - py)/fy, 1): p = d x e2, det = e1 . p, s = V0.z d - V0, b1 = (s . p)/det, q = s x e1,
 *      b2 = (d . q)/det, b0 = 1 - b1 - b2.  s runs from V0 to the ray's point at V0's depth, not to the camera: the barycentrics
 *      are the same for any origin on the ray, and this one keeps s as short as the face is wide.  (Origin-based products,
 *      V1 x V2 or s = -V0, are avoided: their cancellation costs a factor |V|/|edge| of precision at LASR's depths.)
 *      Each b_k is clamped to [0, 1] and the three are divided by their sum (a sub-pixel query may lie just outside the face that
 *      owns the pixel centre); c1, c2 are stored, c0 = 1 - c1 - c2.  A zero-area face (e1 x e2 = 0), det = 0 or a b that is not
 *      finite gives no anchor.
 *   4. facing = +1 if n . P >= 0 else -1, with n = e1 x e2 (not normalised) and P = V0 + c1 e1 + c2 e2 (= c0 V0 + c1 V1 + c2 V2).
 *
 * lasr_track_project: one thread per (frame, query), the query index fastest; writes tracks [n,Q,2] fp32 (u, v) and state [n,Q]
 *   uint8 for the n frames passed.  P = V0 + c1 e1 + c2 e2 of that frame; u = fx P.x/P.z + px, v = fy P.y/P.z + py.  States, tested
 *   in this order: 0 no anchor (face outside [0, F) or naming a vertex outside [0, V); track = NaN); 4 not P.z > 0 (track = NaN);
 *   3 outside 0 <= u < W, 0 <= v < H (track written); 2 hidden; 1 visible.  Visible means both
 *   (a) the sign of n . P at this frame (as in step 4) equals the anchor's facing: a back-face test that needs no winding
 *       convention, which the meshes do not guarantee; and
 *   (b) some pixel of the (2w+1)^2 window around (floor v, floor u), clipped to the frame, names the anchor's face or a face that
 *       shares at least one vertex index with it; w = window, 0 .. LASR_TRACK_MAX_WINDOW, default 1.
 *   Rule (b) is deliberate.  Identity of the named face alone flickers for points near a face edge, and a depth comparison needs
 *   a tolerance nobody can derive; the price is up to w pixels of slack at occlusion boundaries (a point up to w pixels behind an
 *   occluder's outline still counts as visible, and one whose face neighbourhood shows through within w pixels likewise).
 *   No atomics: the same bits for any split of the frames into windows.
 *
 * lasr_track_splat_keys / lasr_track_splat_resolve: the preview's two launches.  keys uint32 [n,H,W], zeroed by the caller.  Every
 *   (frame, query) with state 1 and its track inside the frame does atomicMax(keys[frame, r, c], q + 1) on the pixels
 *   (r, c) = (floor v + dy, floor u + dx) with dx^2 + dy^2 <= radius^2 in integers (radius at most LASR_TRACK_MAX_RADIUS), clipped to
 *   the frame: the highest query index wins an overlap, whatever the order.  Resolve: out uint8 [n,H,W,3] = frames where key = 0,
 *   else per channel (A colour + (255 - A) frame + 127) / 255 in unsigned integer arithmetic (the division truncates) with
 *   colour = colors[key - 1] (uint8 [Q,3]) and A = LASR_TRACK_SPLAT_ALPHA.
 *
 * Checked on the host before any launch (LASR_E_BADARG): n, Q, F >= 0, V >= 1, 1 <= H, W <= IS <= LASR_TRACK_MAX_SIZE (the splat
 *   pair: 1 <= H, W <= LASR_TRACK_MAX_SIZE), 3 V <= INT_MAX, F <= 2^24, t0 >= 0, t0 + n <= 2^24, 0 <= snap_radius <=
 *   LASR_TRACK_MAX_SNAP, 0 <= window <= LASR_TRACK_MAX_WINDOW, 0 <= radius <= LASR_TRACK_MAX_RADIUS; then an empty problem (n == 0
 *   or Q == 0; resolve: n == 0) is LASR_OK with nothing launched; then every pointer non-NULL (faces may be NULL for F == 0, colors
 *   for Q == 0).  Device contents are not read on the host.  These launches are not in the lasr_prof_* kernel table.
 */
#define LASR_TRACK_MAX_SNAP 16
#define LASR_TRACK_MAX_WINDOW 2
#define LASR_TRACK_MAX_RADIUS 8
#define LASR_TRACK_MAX_SIZE 8192
#define LASR_TRACK_SPLAT_ALPHA 192u
int lasr_track_anchor(const float* verts, const int* faces, const float* K, const float* raster, const float* queries, void* anchors,
                      float* snapped, int t0, int n, int Q, int V, int F, int IS, int H, int W, int snap_radius, void* hip_stream);
int lasr_track_project(const float* verts, const int* faces, const float* K, const float* raster, const void* anchors, float* tracks,
                       unsigned char* state, int n, int Q, int V, int F, int IS, int H, int W, int window, void* hip_stream);
int lasr_track_splat_keys(const float* tracks, const unsigned char* state, unsigned* keys, int n, int Q, int H, int W, int radius,
                          void* hip_stream);
int lasr_track_splat_resolve(const unsigned* keys, const unsigned char* colors, const unsigned char* frames, unsigned char* out, int n,
                             int Q, int H, int W, void* hip_stream);

/*
 * ---- Reprojection scores of scripts/eval_reproj.py (lasr_amd/csrc/reproj.hip, lasr_amd/nnutils/reproj.py)
 * This project's own addition: the reference has no counterpart and the DAVIS toolkit is not restated from code; the definitions
 * below are the specification, and parity is to the float64 restatement in tests/reproj_restated.py and to closed forms only.
 * Per frame the hard-mode raster of the predicted mesh is compared with what the loader was trained on: the annotation (region
 * similarity J, boundary measure F), the forward optical flow (end-point error) and the frame's colours.  Conventions are those
 * of lasr_track_anchor: verts [n,V,3] camera space, faces [F,3] int32 shared, K [n,4] = fx fy px py (16-byte aligned), raster
 * [n,2,IS,IS] whose plane 1 names the nearest face; pixel (r, c) has the centre (c + 0.5, r + 0.5).
 *   pred(r, c) = plane 1 names a face in [0, F) at (r, c), r < H, c < W;  gt(r, c) = gt[n,H,W] uint8 is non-zero.
 *
 * lasr_reproj_pixels, per frame of the n passed:
 *   bits   uint64 [n,2,H,WW], WW = ceil(W/64): map 0 = pred, map 1 = gt; column c is bit c & 63 of word c >> 6, bits at or beyond
 *          W are 0.  Written in full.
 *   counts uint64 [n,12], ADDED to (the caller zeroes them): inter = |pred & gt|, union = |pred | gt|, n_pred, n_gt, n_pb, n_gb,
 *          pm, gm (slots 4-7: lasr_reproj_boundary), n_flow, n_le1, n_le3, n_rgb.
 *   sums   double [n,2] = (sum of epe, sum of sq), written.
 *   A pixel with pred & gt whose face indexes vertices inside [0, V) is anchored at its centre by step 3 of lasr_track_anchor
 *   (the same code, no snapping): c1, c2, c0 = 1 - c1 - c2, or no anchor.
 *   Flow (verts_next [n,V,3] and K_next [n,4] = the mesh and intrinsics of each frame's successor, flow [n,H,W,3] fp32 =
 *   (u, v, valid), occ [n,H,W] fp32; the three are NULL together, occ may be NULL on its own = no occlusion test): an anchored
 *   pixel counts in n_flow when flow.valid != 0, occ < 10, flow.u and flow.v are finite, and P = V0 + c1 e1 + c2 e2 on the
 *   successor's mesh has P.z > 0.  flow_pred = (fx' P.x/P.z + px' - (c + 0.5), fy' P.y/P.z + py' - (r + 0.5)), the expression of
 *   lasr_track_project; (du, dv) = flow_pred - flow; epe = sqrt(du^2 + dv^2) in fp32 (a result that is not a number does not
 *   count); n_le1 / n_le3 count epe <= 1 / <= 3.
 *   Colour (frames uint8 [n,H,W,3], colors uint8 [n,V,3], NULL together): every anchored pixel counts in n_rgb; per channel k
 *   d_k = (c0 C0k + c1 C1k + c2 C2k) - frame_k in fp32 on the 0-255 scale, evaluated as written, sq = d_0^2 + d_1^2 + d_2^2 in
 *   fp32.  The counters of a group that is NULL stay untouched.
 *   A wave owns 64 consecutive columns of one row: a ballot is the word of the map, the counts are popcounts, added up over the
 *   sixteen waves (rows) of a workgroup and then one integer atomic per workgroup and counter.  epe and sq are summed in double: a
 *   fixed tree across the wave, the sixteen waves of a workgroup in row order,
 *   one partial per workgroup in `workspace` (lasr_reproj_workspace_bytes(n, H, W) bytes, 8-byte aligned; 0 for bad sizes), and
 *   a second launch in which thread i of one workgroup per frame folds the partials i, i + 256, ... in order and the 256 results
 *   fold across halves.  No floating-point atomics: the same bits on every run and for any split of the frames into calls.
 *
 * lasr_reproj_boundary: adds n_pb, n_gb, pm, gm to counts from bits; scratch_bits uint64 [n,2,H,WW] receives the boundary maps.
 *   b(seg) = (seg ^ e) | (seg ^ s) | (seg ^ se) with e(r,c) = seg(r,c+1), s(r,c) = seg(r+1,c), se(r,c) = seg(r+1,c+1), 0 beyond
 *   the image; then the last row is seg ^ e, the last column seg ^ s, the last pixel 0.  dil(m)(p) = some q with m(q) and
 *   |p - q|^2 <= radius^2 in integers, clipped to the image: for the row offset dy every bit within |dx| <= floor(sqrt(radius^2 -
 *   dy^2)).  n_pb = |b(pred)|, n_gb = |b(gt)|, pm = |b(pred) & dil(b(gt))|, gm = |b(gt) & dil(b(pred))|.  Two launches: the
 *   boundary words (shifts and XORs with a carry bit from the next word and the next row); then one thread per (frame, row, word)
 *   ORs the dilated words of the rows y + dy (own word: shift-OR by doubling; a neighbouring word reaches in from its extreme bit)
 *   and adds the popcounts, one integer atomic per wave and counter.  A word whose own boundary bits are 0 is skipped.
 *   Precision, recall and F are the host's (lasr_amd/nnutils/reproj.py).
 *
 * Checked on the host before any launch (LASR_E_BADARG): n >= 0, 1 <= H, W <= LASR_TRACK_MAX_SIZE; pixels: V >= 1, F >= 0,
 *   H, W <= IS <= LASR_TRACK_MAX_SIZE, 3 V <= INT_MAX, F <= 2^24, an optional group given in part; boundary: 0 <= radius <=
 *   LASR_REPROJ_MAX_RADIUS; then an empty problem (n == 0) is LASR_OK with nothing launched; then every pointer non-NULL (faces may
 *   be NULL for F == 0; the optional groups as above).  Device contents are not read on the host.  These launches are not in the
 *   lasr_prof_* kernel table.
 */
#define LASR_REPROJ_MAX_RADIUS 96
size_t lasr_reproj_workspace_bytes(int n, int H, int W);
int lasr_reproj_pixels(const float* verts, const float* verts_next, const int* faces, const float* K, const float* K_next,
                       const float* raster, const unsigned char* gt, const float* flow, const float* occ, const unsigned char* frames,
                       const unsigned char* colors, unsigned long long* bits, unsigned long long* counts, double* sums, void* workspace,
                       int n, int V, int F, int IS, int H, int W, void* hip_stream);
int lasr_reproj_boundary(const unsigned long long* bits, unsigned long long* scratch_bits, unsigned long long* counts, int n, int H,
                         int W, int radius, void* hip_stream);

/*
 * ---- Variational optical flow of preprocess/auto_gen.py --flow_method variational (lasr_amd/csrc/varflow.hip,
 * lasr_amd/nnutils/varflow.py) ------------------------------------------------------------------------------
 * This project's own addition: the reference estimates flow with a network (VCN) whose checkpoint is a download; this is the
 * classical alternative without learned weights, a coarse-to-fine, warping, robust variational flow (Brox et al. 2004,
 * simplified: brightness constancy only) solved by red-black SOR.  Nothing of the reference is restated here; the definition is
 * tests/varflow_restated.py, whose operation order the kernels follow (-ffp-contract=off), and parity is to that file in float64
 * and to closed forms only.  Images are fp32 [H,W,3] in 0..1 (uint8 / 255); inside the solver a flow field is PLANAR fp32 [2,H,W]
 * = (u, v) in pixels with I1(p) ~ I2(p + (u, v)(p)); lasr_varflow_occ takes the public layout [H,W,2].  All arrays are dense and
 * on the device.  "Clamped" = the tap index clamped to the image; the gradient of a field is 0.5 (a[x+1] - a[x-1]) and
 * 0.5 (a[y+1] - a[y-1]) on clamped taps; bilinear(f, Y, X) = (f00 (1-tx) + f01 tx)(1-ty) + (f10 (1-tx) + f11 tx) ty on the taps
 * floor and min(floor + 1, size - 1).
 *
 * lasr_varflow_reduce: one Burt-Adelson REDUCE of an image [H,W,3] to out [ceil(H/2), ceil(W/2), 3]:
 *   out(y,x) = sum_i k_i (sum_j k_j in(clamp(2y+i), clamp(2x+j))), i, j = -2..2 in that order, k = (1, 4, 6, 4, 1) / 16.
 *   Exactly one of img_u8 / in is given.  The uint8 form first writes level0 [H,W,3] = img_u8 / 255 (one more launch) and reduces
 *   that; its out may be NULL (an image with a single level).  The fp32 form takes level0 = NULL.
 * lasr_varflow_expand: uv_fine [2,h,w] = 2 bilinear(uv_coarse [2,hc,wc], y/2, x/2); hc = ceil(h/2), wc = ceil(w/2).
 * lasr_varflow_tensor: X = x + u, Y = y + v, valid = 0 <= X <= W-1 and 0 <= Y <= H-1 (false for NaN).  At (Y, X) clamped to the
 *   frame, per channel: I2w and the gradient of I2 sampled bilinearly; Ix, Iy = the mean of that and the gradient of I1 at p;
 *   It = I2w - I1.  J [6,H,W] = (sum Ix^2, sum Ix Iy, sum Iy^2, sum Ix It, sum Iy It, sum It^2) over the channels in order, 0
 *   where not valid.
 * lasr_varflow_weights: psi [2,H,W]: psi_d = 0.5 / sqrt(max(r2, 0) + eps^2) with r2 = du^2 J11 + 2 du dv J12 + dv^2 J22 + 2 du J13
 *   + 2 dv J23 + J33, and psi_s = 0.5 / sqrt(|grad(u+du)|^2 + |grad(v+dv)|^2 + eps^2); d [2,H,W] = (du, dv).
 * lasr_varflow_sor: `iters` red-black iterations on d, in place; pixels with (x + y) even first, then odd:
 *   du <- (1-w) du + w (sum_n w_n (u_n + du_n) - ws u - psi_d (J13 + J12 dv)) / (psi_d J11 + ws)
 *   dv <- (1-w) dv + w (sum_n w_n (v_n + dv_n) - ws v - psi_d (J23 + J12 du)) / (psi_d J22 + ws)      with the new du,
 *   over the 4-neighbours n = left, right, up, down in that order, w_n = alpha 0.5 (psi_s(p) + psi_s(n)) inside the image and 0
 *   outside, ws = sum_n w_n.  One launch per iteration, d -> scratch -> d ... (scratch [2,H,W]; after an odd count one device copy
 *   brings the result back to d): a workgroup owns 64 x 8 pixels, stages du, dv, u, v, psi_s of the tile and a halo of 2 in
 *   16320 bytes of LDS, runs the red half-sweep on the tile and the ring at distance 1 and the black one on the tile; a thread
 *   keeps the J planes and psi_d of its red and its black pixel in registers.  iters = n gives the bits of n calls with iters = 1.
 * lasr_varflow_occ: f_ab, f_ba fp32 [H,W,2].  q = p + f_ab(p); outside the frame (or NaN): occ = 6.  Else
 *   e = |f_ab(p) + bilinear(f_ba, q)|, occ = clamp((e - tau) / s, -6, 6), and an exact 0 is written as FLT_MIN (the loader reads 0
 *   as padding).  Defaults tau 1, s 0.5.
 * No entry point uses floating-point atomics: the same input gives the same bits on every run.
 * Checked on the host before any launch (LASR_E_BADARG): LASR_VARFLOW_MIN_SIZE <= H, W <= LASR_VARFLOW_MAX_SIZE (so one plane has
 *   fewer than 2^31 elements; expand: the fine size, and the coarse one equal to its half rounded up); reduce: exactly one
 *   input form; eps, alpha, s > 0, 0 < omega < 2, tau >= 0, all finite; iters >= 0; every pointer non-NULL (reduce as above), an
 *   output distinct from its input, d distinct from scratch.  Device contents are not read on the host.  These launches are not in
 *   the lasr_prof_* kernel table.
 */
#define LASR_VARFLOW_MIN_SIZE 2
#define LASR_VARFLOW_MAX_SIZE 16384
int lasr_varflow_reduce(const unsigned char* img_u8, const float* in, float* level0, float* out, int H, int W, void* hip_stream);
int lasr_varflow_expand(const float* uv_coarse, float* uv_fine, int hc, int wc, int h, int w, void* hip_stream);
int lasr_varflow_tensor(const float* I1, const float* I2, const float* uv, float* J, int H, int W, void* hip_stream);
int lasr_varflow_weights(const float* J, const float* uv, const float* d, float* psi, int H, int W, float eps, void* hip_stream);
int lasr_varflow_sor(const float* J, const float* psi, const float* uv, float* d, float* scratch, int H, int W, float alpha, float omega,
                     int iters, void* hip_stream);
int lasr_varflow_occ(const float* f_ab, const float* f_ba, float* occ, int H, int W, float tau, float s, void* hip_stream);

/*
 * ---- Gradient constancy for the variational optical flow (--vf_gamma; lasr_amd/csrc/robustflow.hip, preprocess/robust_flow.py,
 * DESIGN.md section 4.16) ---------------------------------------------------------------------------------------------------------
 * This project's own addition, as the flow above: Brox et al. 2004 keep the image gradient as well as the brightness along the flow,
 * grad I2(p + w) = grad I1(p), which an additive change of the lighting leaves untouched; Bruhn & Weickert 2005 give the two data
 * terms their own robust penalties.  The definition is tests/robustflow_restated.py, whose operation order the kernels follow
 * (-ffp-contract=off); layouts, "clamped", gradient and bilinear are those of the section above, and pyramid, expansion, solver and
 * consistency map are its entry points, unchanged.
 *
 * lasr_rflow_derivs: level [H,W,3] -> record [H,W,3,6], LASR_RFLOW_RECORD = 18 floats (72 bytes) per pixel: per channel
 *   (I, Ix, Iy, Ixx, Ixy, Iyy) with Ix, Iy = gradient(I); Ixx, Ixy = gradient(Ix); Iyy = the y part of gradient(Iy): the clamped
 *   central difference applied twice, so the border clamps twice.  A workgroup owns 32 x 8 pixels and stages them and a halo of 2
 *   in LDS.  A level's record is constant over its warps: one call per level and frame.
 * lasr_rflow_tensor: R1, R2 the records of I1 and I2, uv [2,H,W] -> Jb [6,H,W], Jg [6,H,W].  valid and the bilinear taps at
 *   p + uv are those of lasr_varflow_tensor, and Jb holds its very values.  Per channel, with s(.) the bilinear sample of a plane
 *   of R2: Ixx = 0.5 (s(I2xx) + I1xx), likewise Ixy and Iyy; Ixt = s(I2x) - I1x, Iyt = s(I2y) - I1y;
 *   Jg = the sum over the channels in order of (Ixx^2 + Ixy^2, Ixx Ixy + Ixy Iyy, Ixy^2 + Iyy^2, Ixx Ixt + Ixy Iyt,
 *   Ixy Ixt + Iyy Iyt, Ixt^2 + Iyt^2): the outer products of the rows (Ixx, Ixy, Ixt) and (Ixy, Iyy, Iyt).  Both are 0 where not valid.
 * lasr_rflow_weights: psi_b = 0.5 / sqrt(max(r2(Jb, d), 0) + eps^2) and psi_g likewise from Jg, r2 as in lasr_varflow_weights;
 *   J [6,H,W] = (beta psi_b) Jb + (gamma psi_g) Jg, psi [2,H,W] = (1, psi_s) with psi_s of lasr_varflow_weights: what
 *   lasr_varflow_sor takes.
 * No entry point uses floating-point atomics: the same input gives the same bits on every run.
 * Checked on the host before any launch (LASR_E_BADARG): LASR_VARFLOW_MIN_SIZE <= H, W <= LASR_VARFLOW_MAX_SIZE; eps > 0, beta >= 0,
 *   gamma >= 0, not both 0, all finite; every pointer non-NULL; record distinct from level, Jb from Jg, J from Jb, Jg and psi.
 *   Device contents are not read on the host.  These launches are not in the lasr_prof_* kernel table.
 */
#define LASR_RFLOW_RECORD 18
int lasr_rflow_derivs(const float* level, float* record, int H, int W, void* hip_stream);
int lasr_rflow_tensor(const float* R1, const float* R2, const float* uv, float* Jb, float* Jg, int H, int W, void* hip_stream);
int lasr_rflow_weights(const float* Jb, const float* Jg, const float* uv, const float* d, float* J, float* psi, int H, int W, float eps,
                       float beta, float gamma, void* hip_stream);

/*
 * ---- Large-displacement matching for the variational optical flow (--vf_match; lasr_amd/csrc/flowmatch.hip,
 * preprocess/flow_match.py) -------------------------------------------------------------------------------
 * This project's own addition, as the flow above: a factor-2 pyramid loses a structure smaller than its own motion.  At one pyramid
 * level an integer block-matching stage (SAD over 8-bit pixels) finds a displacement per pixel, and the forward-backward-consistent
 * matches that explain the images clearly better than the upsampled flow replace it there before the level's unchanged warps (the
 * "extended coarse-to-fine" idea of Xu, Jia & Matsushita 2012, reduced to a greedy per-pixel choice).  The definition is
 * tests/flowmatch_restated.py; all of it is integer arithmetic, so the kernels give its very numbers.
 *
 * A quantised frame q is [H,W] uint32, one word r | g << 8 | b << 16 per pixel.  A displacement field is [H,W,2] int32 = (dx, dy).
 *   C(p, d) = sum over q in [-r, r]^2 and the three channels of |A(clamp(p + q)) - B(clamp(p + q + d))|, both taps clamped.
 * lasr_flowmatch_quantise: exactly one of img (uint8 [H,W,3]: the bytes themselves) and level (fp32 [H,W,3]:
 *   clip(rint(255 I), 0, 255), half to even) is non-NULL -> out.
 * lasr_flowmatch_search: d(p) = the minimum of the key (C, dx^2 + dy^2, dy, dx) in lexicographic order over the d in [-R, R]^2 with
 *   p + d in the frame (d = 0 always is), c1(p) = C(p, d(p)).  A workgroup owns 32 x 8 pixels and stages A's tile with a halo of r
 *   and B's with a halo of r + R in LDS, 33952 bytes at R = 32, r = 3; one v_sad_u8 per pixel pair.
 * lasr_flowmatch_select: uv [2,H,W] fp32, the flow handed to the level.  cu = clip(rint(uv), -R, R) (half to even);
 *   ccur = C(p, cu), or (2r+1)^2 765 where p + cu leaves the frame; seeded(p) = 1 where |d_ab(p) + d_ba(p + d_ab(p))|_inf <= 1 and
 *   256 c1 < K ccur and |d_ab(p) - cu|_inf > 1, else 0; cand = d_ab where seeded, cu elsewhere.  K = rint(256 kappa).
 * lasr_flowmatch_propagate: one Jacobi iteration from (seeded_in, cand_in) to (seeded_out, cand_out).  A seeded pixel is copied.
 *   Another one looks at its left, right, upper and lower neighbour, in that order, and from one that is inside the frame and
 *   seeded in seeded_in takes d = cand_in(neighbour) where p + d is in the frame, 256 C(p, d) < K ccur and C(p, d) is strictly below
 *   the best it holds so far (ccur to begin with); it is then seeded.  Otherwise it keeps cand_in(p) and stays unseeded.
 * No entry point uses atomics: the same input gives the same bits on every run.  Every read is clamped in index space.
 * Checked on the host before any launch (LASR_E_BADARG): LASR_VARFLOW_MIN_SIZE <= H, W <= LASR_VARFLOW_MAX_SIZE;
 *   1 <= R <= LASR_FLOWMATCH_MAX_R; 1 <= r <= LASR_FLOWMATCH_MAX_PATCH; 1 <= K <= 256; every pointer non-NULL (quantise: exactly one
 *   source); no output is an input or another output.  Device contents are not read on the host: displacements within [-R, R] are a
 *   precondition of select and propagate.  These launches are not in the lasr_prof_* kernel table.
 */
#define LASR_FLOWMATCH_MAX_R 32
#define LASR_FLOWMATCH_MAX_PATCH 3
int lasr_flowmatch_quantise(const unsigned char* img, const float* level, unsigned int* out, int H, int W, void* hip_stream);
int lasr_flowmatch_search(const unsigned int* qA, const unsigned int* qB, int* d, int* c1, int H, int W, int R, int r, void* hip_stream);
int lasr_flowmatch_select(const unsigned int* qA, const unsigned int* qB, const int* d_ab, const int* c1, const int* d_ba,
                          const float* uv, unsigned char* seeded, int* cand, int* ccur, int H, int W, int R, int r, int K,
                          void* hip_stream);
int lasr_flowmatch_propagate(const unsigned int* qA, const unsigned int* qB, const unsigned char* seeded_in, const int* cand_in, const int* ccur,
                             unsigned char* seeded_out, int* cand_out, int H, int W, int r, int K, void* hip_stream);

/*
 * ---- Motion segmentation of preprocess/auto_mask.py (lasr_amd/csrc/motionseg.hip, lasr_amd/nnutils/motionseg.py, DESIGN.md
 * section 4.17) -------------------------------------------------------------------------------------------------------------------
 * This project's own addition: the reference fills Annotations/ with a detector (preprocess/mask.py), which stays out of scope;
 * nothing of it is restated here, and parity is to the float64 restatement in tests/motionseg_restated.py and to closed forms only.
 * The four entry points score every pixel of one ordered frame pair a -> b by how badly its flow follows the dominant
 * (camera-induced) motion; the key masks preprocess/propagate_mask.py starts from are made of those scores on the host.  Fields
 * are fp32 [H,W], flows fp32 [H,W,2] = (x, y) in pixels, all dense and on the device.  Per-pixel arithmetic is fp32 in the
 * restatement's operation order (-ffp-contract=off); everything summed over pixels is fp64.
 *
 * lasr_motionseg_conf: q = p + f_ab(p).  q outside [0,W-1] x [0,H-1] (or not finite): conf = 0; else
 *   conf = exp(-|f_ab(p) + bilinear(f_ba, q)|^2 / (2 tau^2)) on the taps of lasr_maskprop_unary (upper taps clamped), and a result
 *   that is not a number is 0.  Default tau 1.
 * The motion model, on normalised coordinates in fp64, s = 0.5 max(H, W), X = (x - 0.5 (W-1)) / s, Y = (y - 0.5 (H-1)) / s:
 *   u_m = t0 + t1 X + t2 Y + t6 X^2 + t7 XY,  v_m = t3 + t4 X + t5 Y + t6 XY + t7 Y^2   (the sums from left to right, X and Y
 *   rounded to fp32).  model 0 = translation (t0, t3), 1 = affine (t0..t5), 2 = quadratic (all eight: the instantaneous flow of a
 *   plane, or of a rotating camera).
 * state, double [LASR_MOTIONSEG_STATE]: theta[8], sigma, med, n (the pixels with conf >= 0.5), status (0 ok, 1 degenerate).  The
 *   caller starts from theta = 0, sigma = +inf.
 * lasr_motionseg_moments: the sums of one IRLS iteration from `state`.  A pixel with conf not > 0 or a flow that is not finite is
 *   SKIPPED (never multiplied by 0: 0 * NaN would poison every sum).  r^2 = (u - u_m)^2 + (v - v_m)^2; w = conf for sigma = inf,
 *   else conf / (1 + r^2 / sigma^2)^2 (Geman-McClure).  LASR_MOTIONSEG_MOMENTS = 28 sums: sum w X^i Y^j for i + j <= 4 (15, by
 *   degree and then by j: slot d (d + 1) / 2 + j), sum w u X^i Y^j and sum w v X^i Y^j for i + j <= 2 (6 + 6), sum w (u^2 + v^2);
 *   monomials and products in fp64.  min(LASR_MOTIONSEG_BLOCKS, ceil(HW / 256)) workgroups of 256 threads; workgroup b owns the
 *   pixels b 256 + lane, + 256 * the number of workgroups, ... (fixed by H and W); 28 fp64 accumulators per lane, folded across the
 *   wave by shuffles, across the four waves through LDS in wave order, and written as row b of partials
 *   [LASR_MOTIONSEG_BLOCKS, LASR_MOTIONSEG_MOMENTS]; workgroup 0 writes the rows of the workgroups that do not exist as zeros, so the
 *   caller need not clear partials.  hist uint32 [LASR_MOTIONSEG_BINS] += the pixels with conf >= 0.5 by
 *   min(floor(16 sqrt(r^2)), 1023): ADDED to what it holds (the caller zeroes it), LDS-private per workgroup and merged with
 *   integer atomics, as lasr_maskprop_hist.
 * lasr_motionseg_solve: one workgroup.  Folds the rows of partials in index order; assembles the 8 x 8 normal matrix
 *   sum w (B_u B_u^T + B_v B_v^T) and the right-hand side sum w (u B_u + v B_v) from the 28 sums only; a parameter that is switched
 *   off has its row and column replaced by the identity's and its right-hand side by 0; adds ridge trace(A) / 8 to the diagonal;
 *   solves the STEP A d = b - A0 theta_in (A0: the matrix before the ridge) by Cholesky in fp64 and writes theta = theta_in + d,
 *   so the fixed point is the un-ridged solution.  n = the total of hist.  A pivot not > 0, a step that is not finite or n = 0:
 *   status = 1, theta, sigma and med stay.  Else med = (the first bin at which the cumulative count reaches ceil(n / 2) + 0.5) / 16,
 *   sigma = max(k_sigma med, sigma_min), status = 0.  The scale is LAGGED: the histogram is of the residuals against theta_in.
 *   H and W are checked only.  Defaults k_sigma 3, sigma_min 0.25, ridge 1e-9, 8 iterations.
 * lasr_motionseg_evidence: e = conf clamp(r^2 / sigma^2 - kappa, -U, U) against state, 0 where the pixel is skipped; accumulate 0
 *   writes evid, 1 adds to it.  Defaults kappa 4, U 6.
 * One IRLS iteration is a memset of hist, moments and solve; theta, sigma and status never visit the host inside a pair.
 * No entry point uses floating-point atomics: the same input gives the same bits on every run.
 * Checked on the host before any launch (LASR_E_BADARG): 0 <= H, W <= LASR_MOTIONSEG_MAX_SIZE; model in {0, 1, 2}; tau, k_sigma,
 *   sigma_min, kappa, U > 0 and ridge >= 0, all finite; accumulate in {0, 1}; then empty work (H == 0 or W == 0) is LASR_OK with
 *   nothing launched; then every pointer non-NULL and every output distinct from the inputs (state is solve's input and output).
 *   Device contents are not read on the host.  These launches are not in the lasr_prof_* kernel table.
 */
#define LASR_MOTIONSEG_MAX_SIZE 16384
#define LASR_MOTIONSEG_BLOCKS 256
#define LASR_MOTIONSEG_MOMENTS 28
#define LASR_MOTIONSEG_BINS 1024
#define LASR_MOTIONSEG_STATE 12
int lasr_motionseg_conf(const float* f_ab, const float* f_ba, float* conf, int H, int W, float tau, void* hip_stream);
int lasr_motionseg_moments(const float* flow, const float* conf, const double* state, double* partials, unsigned* hist, int H, int W,
                           void* hip_stream);
int lasr_motionseg_solve(const double* partials, const unsigned* hist, double* state, int H, int W, int model, float k_sigma,
                         float sigma_min, float ridge, void* hip_stream);
int lasr_motionseg_evidence(const float* flow, const float* conf, const double* state, float* evid, int H, int W, float kappa, float U,
                            int accumulate, void* hip_stream);

/*
 * ---- Shape scores of scripts/eval_shape.py (lasr_amd/csrc/meshcheck.hip, lasr_amd/nnutils/meshcheck.py) ----
 * This project's own addition: the reference has no counterpart, nothing of it is restated here, and parity is to the restatement
 * in tests/meshcheck_restated.py and to closed forms only.  Per frame of a sequence of meshes with one topology: which pairs of
 * faces pass through each other, the signed volume and the area.  verts [T,V,3] fp32, faces [F,3] int32 shared by the frames.
 *
 * Definition.  orient(a, b, c, d) = ((b - a) x (c - a)) . (d - a) in fp32 without contraction: u = b - a, w = c - a, the cross
 *   components u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x, e = d - a, the dot (c_x e_x + c_y e_y) + c_z e_z.
 *   An edge (p, q) PIERCES the triangle (a, b, c) iff orient(a, b, c, p) and orient(a, b, c, q) have strictly opposite signs and
 *   orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a) are all > 0 or all < 0.  Faces i < j are a CANDIDATE pair iff they
 *   share no vertex index and their axis-aligned boxes overlap (closed comparisons on the fp32 inputs: no rounding).  A candidate
 *   pair INTERSECTS iff one of the edges (a, b), (b, c), (c, a) of i pierces j or one of j's pierces i.  Every sign test is strict:
 *   touching and coplanar overlap do not count.  Faces that share a vertex are never tested: a fold between neighbours goes unseen.
 *   volume[t] = (sum_f term_f) / 6 with term = (a_x (b_y c_z - b_z c_y) + a_y (b_z c_x - b_x c_z)) + a_z (b_x c_y - b_y c_x),
 *   positive for outward-facing faces; area[t] = sum_f 0.5 |(b - a) x (c - a)|; both in fp64 from the fp32 inputs.
 *
 * lasr_meshcheck_faces: one thread per (frame, face) writes the face's record into the workspace (nine coordinates, the box, the
 *   three indices; structure of arrays, slot k of face f of frame t at ((t 18 + k) F + f)) and its fp64 volume and area terms; the
 *   terms are folded per block of 256 faces (shuffles, then the four waves in order) and a second launch adds the block partials in
 *   index order: volume [T], area [T] fp64.  No floating-point atomics.
 * lasr_meshcheck_pairs: reads the records lasr_meshcheck_faces left in the same workspace.  The grid runs over (frame, tile I,
 *   tile J >= I) with tiles of LASR_MESHCHECK_TILE faces; both tiles are staged in LDS, every thread keeps the box and the indices
 *   of one face of tile I and walks tile J (the faces after its own in the diagonal tile); the candidates are compacted per wave
 *   into a queue in LDS and tested 64 at a time.  Zeroes, then fills:
 *     face_count [T,F] int32    the number of faces each face intersects
 *     n_pairs    [T]   uint64   the number of intersecting pairs
 *     cursor     [T]   uint32   scratch: counts the pairs again, modulo 2^32
 *     pairs      [T,max_pairs,2] int32   the pairs (i, j), i < j, of a frame in no defined order, filled while cursor < max_pairs:
 *                               complete iff n_pairs[t] <= max_pairs, else to be discarded (the counts stay exact); max_pairs = 0: may
 *                               be NULL
 *   Integer atomics only: the counts, and the list once sorted, are the same bits on every run.
 * Precondition: every face index lies in [0, V) (the Python layer checks it on the device before it launches).  As a defence a face
 *   that breaks it is not gathered: it gets an empty box and terms of 0, and takes part in nothing.
 * Checked on the host before any launch (LASR_E_BADARG): 0 <= T <= LASR_MESHCHECK_MAX_FRAMES, V >= 0, 3 V <= INT_MAX,
 *   0 <= F <= LASR_MESHCHECK_MAX_FACES (2^20: the tile-pair grid of a frame is then 2^23 + 2^11 blocks), T F <= INT_MAX,
 *   max_pairs >= 0, 2 T max_pairs <= INT_MAX; then T == 0 or F == 0 is LASR_OK with nothing launched; then V >= 1, every pointer
 *   non-NULL (pairs only when max_pairs > 0), no two outputs the same buffer and none of them the workspace or an input;
 *   LASR_E_WORKSPACE when workspace_bytes < lasr_meshcheck_workspace_bytes(T, F), which is 0 for sizes outside these limits.
 *   Device contents are not read on the host.  Neither kernel is in the lasr_prof_* table.
 */
#define LASR_MESHCHECK_TILE 256
#define LASR_MESHCHECK_MAX_FACES 1048576
#define LASR_MESHCHECK_MAX_FRAMES 65535
size_t lasr_meshcheck_workspace_bytes(int T, int F);
int lasr_meshcheck_faces(const float* verts, const int* faces, void* workspace, size_t workspace_bytes, double* volume, double* area,
                         int T, int V, int F, void* hip_stream);
int lasr_meshcheck_pairs(const void* workspace, size_t workspace_bytes, int* face_count, unsigned long long* n_pairs, unsigned* cursor,
                         int* pairs, int T, int F, int max_pairs, void* hip_stream);

/*
 * ---- Folds between neighbouring faces: scripts/eval_shape.py --neighbours (lasr_amd/csrc/meshnbr.hip, scripts/shape_neighbours.py,
 *      DESIGN.md section 4.18) ----
 * This project's own addition, as the block above, and its second pass: the pair pass never tests two faces that share a vertex,
 * this pass tests exactly those.  Parity is to the restatement in tests/meshnbr_restated.py and to closed forms only.  orient and
 * PIERCES are the ones above, strict and without contraction.
 *
 * Topology (faces only, once for all frames).  A face with a repeated index is DEGENERATE: counted, part of nothing.  For
 *   non-degenerate faces i < j, s = the number of corners of i whose index is a corner of j.  s = 0: no neighbour.  s = 1: a VERTEX
 *   pair, ca / cb = the position (0..2) of the shared corner in i / in j.  s = 2: an EDGE pair, ca / cb = the position of the corner
 *   that is not shared (the apex) in i / in j, and `same` is set when the shared edge runs in the same direction in both cyclic orders
 *   (an inconsistent orientation).  s = 3: a DUPLICATE, counted and never tested.  A list entry is the 64-bit key
 *   i << 32 | j << 8 | ca | cb << 2 | edge << 4 | same << 5, so sorted keys are in lexicographic (i, j) order.
 * Vertex pair, A = tri(i), B = tri(j) in stored corner order: PIERCED iff (A[(ca+1)%3], A[(ca+2)%3]) pierces B or
 *   (B[(cb+1)%3], B[(cb+2)%3]) pierces A.  Only the edge opposite the shared corner is tested: the two planes meet in a line through
 *   the shared vertex, and if the triangles overlap beyond it the overlap segment ends where the nearer opposite edge enters the other
 *   triangle.  The edges through the shared vertex touch the other triangle in that vertex; their plane determinants are zero in exact
 *   arithmetic and noise in fp32, so they are not tested.
 * Edge pair: nA = (A1 - A0) x (A2 - A0), nB likewise (the component order of orient's cross product), d = (nAx nBx + nAy nBy) +
 *   nAz nBz, negated when `same` is set, qa = (nAx^2 + nAy^2) + nAz^2, qb likewise, q = qa qb.  CREASED iff d < 0 and d d > k q,
 *   strictly, where k = cos^2(fold_deg) is computed in double by the caller and rounded once to fp32: the interior dihedral angle is
 *   then below fold_deg.  A pair with q = 0, or with q or d d not finite, is not creased.  Non-coplanar faces that share an edge cannot
 *   intersect outside that edge: this is an angle criterion, not an intersection test.  Supported edge lengths: about 1e-4 to 1e4
 *   (q is the eighth power of a length).  The callers' default fold_deg = 20 is derived from nothing measured on a real
 *   reconstruction.
 *   min_cos[t] = min(1, the minimum over the edge pairs with 0 < q < inf of d / sqrt(q), clamped to [-1, 1]); the division and the
 *   root are not part of any equality.
 *
 * lasr_meshnbr_list: faces [F,3] int32 -> list, uint64 [capacity], in no defined order (the caller sorts it), and counters, uint64
 *   [LASR_MESHNBR_COUNTERS]: n_list, n_duplicate, n_degenerate, n_same.  The grid is the pair pass's (tile I, tile J >= I) over the
 *   index triples only; a thread keeps one face of tile I, tile J's indices are staged in LDS.  Survivors are compacted per wave and
 *   written 64 at a time through one atomicAdd on n_list per wave and batch, while the slot is below capacity: the list is complete
 *   iff n_list <= capacity, and the counters are exact either way (capacity = 0: list may be NULL, a counting pass).  Zeroes the
 *   counters itself.  A closed manifold has about 6 F entries.
 * lasr_meshnbr_test: reads the records lasr_meshcheck_faces left in the workspace, n_list keys and k.  The grid is (list blocks,
 *   frames), one lane per (entry, frame).  Zeroes or initialises, then fills:
 *     nbr_count [T,2,F] int32    per face, the neighbours it is pierced by (plane 0) and creased with (plane 1)
 *     totals    [T,2]   uint64   n_pierced, n_creased
 *     cursor    [T]     uint32   scratch: counts the hits again, modulo 2^32
 *     hits      [T,max_pairs,3] int32   (i, j, kind: 0 pierced, 1 creased) in no defined order, filled while cursor < max_pairs:
 *                                complete iff n_pierced + n_creased <= max_pairs; max_pairs = 0: may be NULL
 *     min_cos   [T]     fp32     as above (an integer atomicMin on an order-preserving encoding, decoded by a second small launch)
 *   Integer atomics only: two runs give the same bits, the hits once sorted.  A key that names a face outside [0, F) is skipped.
 * Checked on the host before any launch (LASR_E_BADARG): 0 <= F <= LASR_MESHCHECK_MAX_FACES, capacity >= 0; T, F as
 *   lasr_meshcheck_pairs, n_list >= 0, max_pairs >= 0, 3 T max_pairs <= INT_MAX, 0 <= k <= 1; then F == 0 (list), or T == 0, F == 0 or
 *   n_list == 0 (test), is LASR_OK with nothing launched and nothing written; then every pointer non-NULL (list only when
 *   capacity > 0, hits only when max_pairs > 0) and no two buffers the same; LASR_E_WORKSPACE when workspace_bytes <
 *   lasr_meshcheck_workspace_bytes(T, F).  Device contents are not read on the host.  Neither kernel is in the lasr_prof_* table.
 */
#define LASR_MESHNBR_COUNTERS 4
int lasr_meshnbr_list(const int* faces, unsigned long long* list, unsigned long long* counters, int F, int capacity, void* hip_stream);
int lasr_meshnbr_test(const void* workspace, size_t workspace_bytes, const unsigned long long* list, int n_list, float k, int* nbr_count,
                      unsigned long long* totals, unsigned* cursor, int* hits, float* min_cos, int T, int F, int max_pairs,
                      void* hip_stream);

/*
 * ---- Fold penalty of the optimiser: optimize.py --fold_wt / --pierce_wt (lasr_amd/csrc/foldpen.hip, scripts/fold_penalty.py,
 *      DESIGN.md section 4.21) ----
 * This project's own addition, as the two blocks above: the reference has no counterpart, nothing of it is restated here, and parity
 * is to the restatement in tests/foldpen_restated.py and to closed forms only.  A loss on the posed meshes of a step that follows
 * the two criteria of the neighbour pass above, so that "the penalty is zero" and "eval_shape.py --neighbours reports nothing" mean
 * the same thing.  x [N,V,3] fp32, the N meshes of a step on one topology; faces [F,3] int32; list: the sorted keys of
 * lasr_meshnbr_list (layout and ca, cb, kind, same as above); phi: the penalty's angle in radians, 0 < phi <= pi / 2.  The callers'
 * defaults (weights 0: off; fold_deg 30) are derived from nothing measured on a real reconstruction.
 *
 * Crease term, per EDGE pair (i, j): nA, nB, d, qa, qb exactly as the neighbour pass defines them (d negated when `same` is set),
 *   s = |nA x nB| (the component order of orient's cross product, the dot as there, one square root), theta = atan2(s, -d) in
 *   [0, pi]: the interior dihedral angle, 0 a complete fold, pi flat.  The value is max(0, phi - theta)^2.  A pair with qa qb = 0 or
 *   not finite has value 0 and gradient 0, as the evaluation does not count it.  The penalty is a function of the angle, not of its
 *   cosine: d cos / d theta is 0 at theta = 0, so any function of the cosine alone has no gradient at the complete fold.
 *   d theta / d x is the closed-form hinge gradient of discrete shells: with x0 = A[(ca+1)%3], x1 = A[(ca+2)%3] (the shared edge),
 *   x2 = A[ca], x3 = B[cb] (the apexes), e = x1 - x0, GA = -sign(orient(A0, A1, A2, x3)) |e| nA / qa,
 *   GB = -sign(orient(B0, B1, B2, x2)) |e| nB / qb, tA = ((x2 - x0) . e) / |e|^2, tB = ((x3 - x0) . e) / |e|^2: by x2 GA, by x3 GB,
 *   by x0 -(1 - tA) GA - (1 - tB) GB, by x1 -tA GA - tB GB.  It is finite and of length 1 / height at the complete fold's
 *   neighbourhood; at exactly theta = 0 both signs are 0: the kink of the unsigned angle gets gradient 0.
 * Pierce term, per VERTEX pair: both directed tests of the neighbour pass, with orient and PIERCES as above, strict and without
 *   contraction.  For a test that holds, with edge (p, q) and triangle (a, b, c) in stored order and n = (b - a) x (c - a):
 *   delta = min(|orient(a,b,c,p)|, |orient(a,b,c,q)|) / |n|, the distance of the shallower end point from the plane.  The value is
 *   delta, the depth itself and not its square (with the square the depth decays geometrically and the end point never crosses the
 *   plane).  The gradient goes to that end point r (p on a tie), sign(orient(a,b,c,r)) n / |n|, and to a, b, c: minus that times the
 *   barycentric coordinates of r's foot in the plane, l_b = ((r - a) x (c - a)) . n / |n|^2, l_c = ((b - a) x (r - a)) . n / |n|^2,
 *   l_a = (1 - l_b) - l_c.  The value of the pair is the sum over the directed tests that hold.
 * loss [N,2] fp32: the crease sum and the pierce sum of each mesh.  Per-entry values are fp32; each sum is accumulated in fp64 over
 *   the entries in list order (blocks of 256 entries: the lanes of a wave by shuffles, the four waves in order; then the blocks in
 *   order, as lasr_meshcheck_faces folds its terms) and rounded once.
 *
 * lasr_foldpen_forward: the grid is lasr_meshnbr_test's, (list blocks, meshes), one lane per (entry, mesh), which reads the three
 *   vertices of both faces through `faces`.  Writes values [N,n_list] fp32 (0 for an entry that is not charged) and loss; scratch:
 *   lasr_foldpen_scratch_bytes(N, n_list) bytes (the block partials).  rows NULL: nothing more.  rows [N,n_list,5,3] fp32: the
 *   entry's contribution row d value / d vertex is written for lasr_foldpen_backward, zeros for an entry that is not charged (no
 *   result depends on what the buffer held).  The roles of the five slots:
 *     vertex pair: 0 the shared vertex; 1, 2 = A[(ca+1)%3], A[(ca+2)%3]; 3, 4 = B[(cb+1)%3], B[(cb+2)%3]
 *     edge pair:   0 = A[ca]; 1, 2 = A[(ca+1)%3], A[(ca+2)%3]; 3 = B[cb]; 4 unused (zeros)
 *   Two launches (entries, fold).  A key that names a face outside [0, F) is skipped (value 0, a row of zeros), and so is a pair
 *   with a face whose index is outside [0, V).
 * lasr_foldpen_backward: one thread per (mesh, vertex) gathers its rows through an inverted index, a CSR from vertex to
 *   incidences that the Python layer builds once per topology: vstart int32 [V+1] ascending, inc int32 [n_inc] with
 *   inc[k] = (entry 5 + slot) 2 + (1 for an edge pair, 0 for a vertex pair), ascending within a vertex.  gverts [N,V,3] is
 *   OVERWRITTEN with the sum over the vertex's incidences, in that order and in fp32 without contraction, of grad_loss[mesh, plane]
 *   times the row's 3-vector (plane 0 for an edge pair, 1 for a vertex pair).  An incidence outside the rows is skipped.  One launch.
 * No floating-point atomics anywhere: two runs give the same bits.  Both are launch-only with static shapes (capturable into a graph).
 * Checked on the host before any launch (LASR_E_BADARG): 0 <= N <= LASR_MESHCHECK_MAX_FRAMES, V >= 0, 3 V <= INT_MAX,
 *   0 <= n_list <= LASR_FOLDPEN_MAX_LIST (10 n_list <= INT_MAX), N n_list <= INT_MAX, 0 <= F <= LASR_MESHCHECK_MAX_FACES and
 *   0 < phi <= pi / 2 (forward), 0 <= n_inc <= 5 n_list (backward); then N == 0, F == 0 or n_list == 0 (forward) is LASR_OK with
 *   nothing launched and nothing written, and N == 0 or V == 0 (backward) likewise; n_list == 0 or n_inc == 0 (backward) zeroes
 *   gverts and launches nothing; then V >= 1, every pointer but rows (forward) non-NULL and no two buffers the same;
 *   LASR_E_WORKSPACE when scratch_bytes < lasr_foldpen_scratch_bytes(N, n_list), which is 0 for sizes outside these limits.  Device
 *   contents are not read on the host.  These launches are not in the lasr_prof_* kernel table.
 */
#define LASR_FOLDPEN_MAX_LIST 214748364
size_t lasr_foldpen_scratch_bytes(int N, int n_list);
int lasr_foldpen_forward(const float* x, const int* faces, const unsigned long long* list, int n_list, float phi, float* values,
                         float* rows, void* scratch, size_t scratch_bytes, float* loss, int N, int V, int F, void* hip_stream);
int lasr_foldpen_backward(const float* rows, const int* vstart, const int* inc, int n_inc, const float* grad_loss, float* gverts, int N,
                          int V, int n_list, void* hip_stream);

/*
 * ---- Intersection penalty of the optimiser: optimize.py --isect_wt (lasr_amd/csrc/isectpen.hip, scripts/isect_penalty.py,
 *      DESIGN.md section 4.22) ----
 * This project's own addition, as the blocks above: the reference has no counterpart, and parity is to the restatement in
 * tests/isectpen_restated.py and to closed forms only.  A loss on the posed meshes of a step that is zero exactly where
 * scripts/eval_shape.py reports n_pairs = 0: the third line of the shape report, beside the two the fold penalty above acts on.
 * x [N,V,3] fp32, the N meshes of a step on one topology; faces [F,3] int32.  Nothing is new except the set of pairs and the
 * accumulation.  The caller's weight (default 0: off) is derived from nothing measured, and the effect on real footage is unverified.
 *
 * Pairs: CANDIDATE and INTERSECTS of lasr_meshcheck_pairs above, unchanged: faces i < j that share no vertex index and whose closed
 *   fp32 boxes overlap, put to the six directed edge-against-triangle tests (the edges (0,1), (1,2), (2,0) of i against j, then those
 *   of j against i) with orient and PIERCES, strict and without contraction.  A face with an index outside [0, V) or with a repeated
 *   index is not gathered: it has the empty box and takes part in nothing.
 * Value of a pair: the sum over its directed tests that hold of the pierce depth of the fold penalty above, with edge (p, q),
 *   triangle (a, b, c) in stored order and n = (b - a) x (c - a): delta = min(|orient(a,b,c,p)|, |orient(a,b,c,q)|) / |n|; the
 *   gradient goes to the shallower end r (p on a tie), sign(orient(a,b,c,r)) n / |n|, and to a, b, c: minus that times l_a, l_b, l_c
 *   of r's foot, in that block's operation order (one device function, lasr_amd/csrc/foldpen_geom.h, serves both).  Linear in the
 *   depth, so that a descent step carries the end across the plane.
 * Accumulation: the pair set depends on the geometry, so there is no list to gather through, and the project uses no floating-point
 *   atomics: FIXED POINT with Q = 2^40.  Every fp32 contribution c of a test (its depth, or one coordinate of one of its four vertex
 *   contributions) is added as llrint((double)c Q) by a 64-bit integer atomicAdd, to acc_loss [N] and acc_grad [N,V,3], both int64
 *   in scratch.  A test whose |n|^2 is 0 or not finite, or with any contribution that is not finite or >= 2^20 in magnitude, is
 *   dropped as a whole, before its first atomic is issued, and counted in n_dropped [N].  Integer sums commute: the result has the same
 *   bits on every run and under any permutation of the rows of faces.  Each rounding is at most 2^-41; an accumulator wraps beyond a
 *   sum of 2^23, which is not checked.
 * lasr_isectpen_forward: zeroes the accumulators and the counts itself (nothing depends on what any buffer held); the grid of
 *   lasr_meshcheck_pairs, (tile pair I <= J, mesh), 256 threads, tiles of LASR_MESHCHECK_TILE faces staged in LDS straight from x
 *   and faces (nine coordinates, the box, the three indices); box rejection, per-wave compaction, the exact test 64 at a time; a hit
 *   lane evaluates its tests that hold and issues its atomics.  Then loss [N] = (float)((double)acc_loss 2^-40), gunit [N,V,3]
 *   likewise: the gradient of loss[n] by x[n]; n_pairs [N] uint64: the intersecting pairs as lasr_meshcheck_pairs counts them (one
 *   atomic per wave).  gunit NULL: no gradient is wanted, only acc_loss and the counts are touched; loss and the counts are the
 *   same.  There is no backward entry point: loss[n] is a plain sum, so the gradient by x is grad_loss[n] gunit[n].  Three launches
 *   (zero, pairs, finalise), static shapes, no host read: capturable into a graph.
 * Checked on the host before any launch (LASR_E_BADARG): 0 <= N <= LASR_MESHCHECK_MAX_FRAMES, 0 <= F <= LASR_MESHCHECK_MAX_FACES,
 *   N F <= INT_MAX, V >= 0, N V 3 <= INT_MAX; then N == 0 or F == 0 is LASR_OK with nothing launched and nothing written; then
 *   V >= 1, every pointer but gunit non-NULL and no two buffers the same; LASR_E_WORKSPACE when scratch_bytes <
 *   lasr_isectpen_scratch_bytes(N, V) = 8 (N + N V 3), which is 0 for sizes outside these limits.  Device contents are not read on
 *   the host.  These launches are not in the lasr_prof_* kernel table.
 */
size_t lasr_isectpen_scratch_bytes(int N, int V);
int lasr_isectpen_forward(const float* x, const int* faces, void* scratch, size_t scratch_bytes, float* loss, float* gunit,
                          unsigned long long* n_pairs, unsigned long long* n_dropped, int N, int V, int F, void* hip_stream);

/*
 * ---- Structural similarity as the texture term of optimize.py --ptex_method ssim (lasr_amd/csrc/ssim.hip,
 *      lasr_amd/nnutils/fused_ops.py: ssim_distance) ----
 * This project's own addition: the reference has no counterpart (its texture term is an AlexNet feature distance that needs
 * downloaded weights), nothing of it is restated here, and parity is to the restatement in tests/ssim_restated.py and to closed
 * forms only.  SSIM of Wang et al. 2004 with the 11 x 11 Gaussian window of sigma 1.5 over the valid region, as a distance per image.
 * a [M,3,H,W] fp32 (the observed images, no gradient), b [N,3,H,W] fp32 with N = M rep; image i of b is compared with image
 * i / rep of a.  L is the data range (1 for images in [0, 1], 2 for [-1, 1]).
 *
 * Definition, in fp32 without contraction and with IEEE division.  g[k] = exp(-(k - 5)^2 / (2 1.5^2)), k = 0 .. 10, normalised to
 *   sum 1 in fp64 and rounded once to fp32.  Ho = H - 10, Wo = W - 10.  The five planes a, b, a a, b b, a b (products first) are
 *   blurred horizontally, then vertically; each pass is acc = 0; for k ascending: acc = acc + g[k] p[. + k].  With the results
 *   mu_a, mu_b, E_aa, E_bb, E_ab: s_aa = E_aa - mu_a mu_a, s_bb and s_ab likewise; C1 = (0.01 L)^2, C2 = (0.03 L)^2;
 *   A1 = 2 mu_a mu_b + C1, A2 = 2 s_ab + C2, B1 = (mu_a mu_a + mu_b mu_b) + C1, B2 = (s_aa + s_bb) + C2, den = B1 B2,
 *   s = (A1 A2) / den.  d[i] = 1 - (sum of s over the 3 channels and the Ho Wo pixels) / (3 Ho Wo).
 *   The sum: a block owns a LASR_SSIM_TILE_W x LASR_SSIM_TILE_H tile of one (image, channel); thread t (of 256) adds s at row t / 32
 *   and at row t / 32 + 8 of column t % 32 (0 outside the map); the 64 lanes of a wave are folded by lane l += lane l + o for
 *   o = 32, 16, ..., 1, the four waves as ((w0 + w1) + w2) + w3, all in fp32; a second launch adds the block sums of an image in
 *   fp64 in the order channel, tile row, tile column, forms 1 - sum / (3 Ho Wo) in fp64 and rounds it to fp32.
 *   The derivatives of s, with u = (2 mu_b) s:  P1 = ((2 mu_a) (A2 - A1)) / den - (u / B1 - u / B2)  (by mu_b, the mu terms of the
 *   variances included), P2 = -(s / B2) (by E_bb), P3 = (2 A1) / den (by E_ab).  The gradient pushes them through the transposed
 *   window over the planes padded with zeros: U_j(py, qx) = acc over k ascending of g[10 - k] P_j(py, qx - 10 + k), T_j(qy, qx) =
 *   acc over k ascending of g[10 - k] U_j(qy - 10 + k, qx), v = T_1 + (2 b(q)) T_2, v = v + a(q) T_3,
 *   grad_b(q) = fp32(-fp64(grad_d[i]) / (3 Ho Wo)) v.
 *
 * lasr_ssim_forward: d [N]; scratch: lasr_ssim_scratch_floats(M, rep, H, W) floats (the block sums).  partials NULL: nothing more.
 *   partials [N,3,3,Ho,Wo] (image, channel, plane P1 P2 P3): the three derivative planes are written for lasr_ssim_backward.
 *   Two launches (tiles, fold).
 * lasr_ssim_backward: grad_b [N,3,H,W] is overwritten.  partials as the forward wrote them, or NULL: the planes are recomputed
 *   from a and b in the same order, so both forms give the same bits.  One launch.
 * No floating-point atomics: the same input gives the same bits on every run.  Both are launch-only (capturable into a graph).
 * Checked on the host before any launch (LASR_E_BADARG): M >= 1, rep >= 1, 3 M rep <= 65535 (the grid's z extent),
 *   LASR_SSIM_MIN_SIZE <= H, W <= LASR_SSIM_MAX_SIZE, L finite and > 0; then every pointer but partials non-NULL and no output the
 *   same buffer as an input or another output.  lasr_ssim_scratch_floats is 0 for sizes outside these limits.  Device contents are
 *   not read on the host.  These launches are not in the lasr_prof_* kernel table.
 */
#define LASR_SSIM_MIN_SIZE 11
#define LASR_SSIM_MAX_SIZE 4096
#define LASR_SSIM_TILE_W 32
#define LASR_SSIM_TILE_H 16
size_t lasr_ssim_scratch_floats(int M, int rep, int H, int W);
int lasr_ssim_forward(const float* a, const float* b, float* d, float* partials, float* scratch, int M, int rep, int H, int W, float L,
                      void* hip_stream);
int lasr_ssim_backward(const float* a, const float* b, const float* partials, const float* grad_d, float* grad_b, int M, int rep,
                       int H, int W, float L, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LASR_OPS_H_ */
