"""ctypes binding of liblasr_hip.so (the C ABI declared in include/lasr_sr.h).

There is deliberately NO fallback: if the library is missing or an entry point
fails, the caller gets an exception.  The CPU oracle under oracle/ is test
infrastructure and is never imported from here.
"""
import ctypes
import os

import torch                                        # (first: liblasr_hip.so must bind to the HIP runtime torch bundles, see lib())

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('LASR_HIP_LIB') or os.path.join(_HERE, 'csrc', 'liblasr_hip.so')   # env override: kernel A/B builds

# every symbol include/lasr_sr.h and include/lasr_ops.h declare (checked by tests/test_abi.py)
_f, _i, _p, _sz = ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
_RASTER_SCALARS = [_i, _i, _i, _i, _f, _f, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p]
_RASTER_SCALARS_DEV = [_i, _i, _i, _i, _p, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p]
SIGNATURES = {
    'lasr_abi_version': (_i, []),
    'lasr_strerror': (ctypes.c_char_p, [_i]),
    'lasr_last_hip_error': (_i, []),
    'lasr_sr_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'lasr_sr_forward': (_i, [_p, _p, _p, _p, _p, _p, _sz] + _RASTER_SCALARS),
    'lasr_sr_backward': (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _sz] + _RASTER_SCALARS),
    # include/lasr_ops.h
    'lasr_lbs_forward': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_lbs_forward_both': (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_lbs_backward_both': (_i, [_p] * 11 + [_i, _i, _i, _p]),
    'lasr_lbs_backward_scratch_floats': (_sz, [_i, _i, _i]),
    'lasr_lbs_backward': (_i, [_p] * 10 + [_i, _i, _i, _i, _p]),
    'lasr_project_points_forward': (_i, [_p] * 7 + [_i, _i, _i, _p]),
    'lasr_project_points_backward': (_i, [_p] * 8 + [_i, _i, _i, _p]),
    'lasr_pose_chain_forward': (_i, [_p, _i] + [_p] * 17 + [_i, _i, _i, _f, _p]),
    'lasr_pose_chain_backward': (_i, [_p, _i] + [_p] * 22 + [_i, _i, _i, _p]),
    'lasr_pinhole_forward': (_i, [_p, _p, _p, _p, _i, _i, _p]),
    'lasr_pinhole_backward': (_i, [_p] * 7 + [_i, _i, _p]),
    'lasr_loss_scratch_floats': (_sz, [_i, _i, _i]),
    'lasr_mask_loss_forward': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_mask_loss_backward': (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_flow_loss_forward': (_i, [_p] * 8 + [_i, _i, _i, _i, _p]),
    'lasr_flow_loss_backward': (_i, [_p] * 8 + [_i, _i, _i, _i, _p]),
    'lasr_flow_loss_forward_vis': (_i, [_p] * 9 + [_i, _i, _i, _i, _p]),
    'lasr_tex_loss_forward': (_i, [_p] * 7 + [_f, _i, _i, _i, _p]),
    'lasr_tex_loss_backward': (_i, [_p] * 9 + [_f, _i, _i, _i, _p]),
    'lasr_arap_forward': (_i, [_p] * 5 + [_i, _i, _p]),
    'lasr_arap_backward': (_i, [_p] * 7 + [_i, _i, _p]),
    'lasr_laplacian_forward': (_i, [_p] * 4 + [_i, _i, _p]),
    'lasr_laplacian_backward': (_i, [_p] * 6 + [_i, _i, _p]),
    'lasr_mesh_regularisers_forward': (_i, [_p] * 12 + [_i, _i, _i, _i, _p]),
    'lasr_mesh_regularisers_backward': (_i, [_p] * 17 + [_i, _i, _i, _i, _p]),
    'lasr_step_regularisers_forward': (_i, [_p] * 12 + [_i, _i, _i, _i] + [_p] * 5 + [_i, _i, _i, _p]),
    'lasr_step_regularisers_backward': (_i, [_p] * 17 + [_i, _i, _i, _i] + [_p] * 7 + [_i, _i, _i, _p]),
    'lasr_flow_reproject_scratch_floats': (_sz, [_i, _i]),
    'lasr_flow_reproject_forward': (_i, [_p] * 7 + [_i, _i, _p]),
    'lasr_flow_reproject_backward': (_i, [_p] * 7 + [_i, _i, _p]),
    'lasr_flow_reproject_planes_forward': (_i, [_p, ctypes.c_longlong] + [_p] * 6 + [_i, _i, _p]),
    'lasr_flow_reproject_planes_backward': (_i, [_p, ctypes.c_longlong] + [_p] * 6 + [_i, _i, _p]),
    'lasr_quat_to_rotmat_forward': (_i, [_p, _p, _i, _p]),
    'lasr_quat_to_rotmat_backward': (_i, [_p, _p, _p, _i, _p]),
    'lasr_skin_weights_forward': (_i, [_p] * 5 + [_i, _i, _i, _p]),
    'lasr_skin_weights_backward': (_i, [_p] * 10 + [_i, _i, _i, _p]),
    'lasr_flatten_forward': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'lasr_flatten_backward': (_i, [_p] * 7 + [_i, _i, _i, _p]),
    'lasr_face_gather_forward': (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_face_gather_backward': (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_face_gather_backward_csr': (_i, [_p, _p, _p, _i, _p, _i, _i, _i, _i, _p]),
    'lasr_nearest_point': (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_point_mesh_scratch_floats': (_sz, [_i, _i, _i]),
    'lasr_point_mesh_forward': (_i, [_p] * 8 + [_i, _i, _i, _i, _p]),
    'lasr_point_mesh_backward': (_i, [_p] * 5 + [_f, _f, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_cosdist_scratch_floats': (_sz, [_i, _i]),
    'lasr_cosdist_forward': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_cosdist_backward': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_cosdist_multi_scratch_floats': (_sz, [_p, _i, _i]),
    'lasr_cosdist_multi_forward': (_i, [_p, _p, _p, _p, _i, _p, _p, _i, _i, _p]),
    'lasr_cosdist_multi_backward': (_i, [_p, _p, _p, _p, _i, _p, _p, _i, _i, _p]),
    'lasr_load_textures': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_create_texture_image': (_i, [_p, _p, _p, _i, _i, _i, _f, _p]),
    'lasr_create_texture_image_f64': (_i, [_p, _p, _p, _i, _i, _i, _f, _p]),
    'lasr_voxelize_workspace_bytes': (_sz, [_i, _i]),
    'lasr_voxelize': (_i, [_p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    'lasr_voxelize_f64': (_i, [_p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    # lasr_amd/csrc/vis.hip
    'lasr_vis_shade': (_i, [_p] * 9 + [_i] * 8 + [_p, _p]),
    # lasr_amd/csrc/keypoints.hip
    'lasr_kp_transfer': (_i, [_p] * 4 + [_i] * 5 + [_p]),
    # lasr_amd/csrc/manifold.hip
    'lasr_manifold_workspace_bytes': (_sz, [_i]),
    'lasr_manifold_repair': (_i, [_p, _p, _p, _sz, _i, _p]),
    'lasr_manifold_count': (_i, [_p, _p, _p, _sz, _i, _p]),
    'lasr_manifold_extract': (_i, [_p, _p, _p, _i, _i, _p, _sz, _i, _p]),
    'lasr_manifold_project': (_i, [_p] * 5 + [_i, _i, _i, _p]),
    'lasr_manifold_guard': (_i, [_p] * 5 + [_i, _i, _f, _p]),
    # lasr_amd/csrc/vcn.hip
    'lasr_vcn_corr_proj_workspace_bytes': (_sz, [_i, _i, _i]),
    'lasr_vcn_corr_proj': (_i, [_p] * 8 + [_sz] + [_i] * 7 + [_p]),
    'lasr_vcn_flow_reg': (_i, [_p] * 4 + [_i] * 6 + [_p]),
    # lasr_amd/csrc/phong.hip
    'lasr_phong_shade': (_i, [_p] * 5 + [_i] * 4 + [_p]),
    # lasr_amd/csrc/chamfer.hip
    'lasr_chamfer3d_workspace_bytes': (_sz, [_i, _i, _i]),
    'lasr_nn_tiled': (_i, [_p] * 7 + [_sz] + [_i] * 4 + [_p]),
    'lasr_chamfer3d_forward': (_i, [_p] * 7 + [_sz] + [_i] * 4 + [_p]),
    'lasr_chamfer3d_backward': (_i, [_p] * 12 + [_i] * 3 + [_p]),
    'lasr_icp_workspace_bytes': (_sz, [_i, _i, _i]),
    'lasr_icp_init': (_i, [_p] * 5 + [_sz] + [_i] * 3 + [_p]),
    'lasr_icp_iterate': (_i, [_p] * 7 + [_sz] + [_i] * 4 + [ctypes.c_double, _i, _p]),
    'lasr_icp_kabsch_host': (_i, [_p, _i, _p, _p]),
    # lasr_amd/csrc/flowvis.hip
    'lasr_flow_to_image_scratch_bytes': (_sz, [_i]),
    'lasr_flow_to_image': (_i, [_p] * 4 + [_i] * 4 + [_p]),
    'lasr_monitor_sheet_scratch_bytes': (_sz, []),
    'lasr_monitor_sheet': (_i, [_p, _p, _p, _i, _p]),
    'lasr_scalar_ring_bytes': (_sz, [_i, _i]),
    'lasr_scalar_ring_push': (_i, [_p, _i, _p, _p, _i, _p]),
    # lasr_amd/csrc/bake.hip
    'lasr_bake_accumulate': (_i, [_p] * 7 + [_i] * 8 + [_p]),
    'lasr_bake_resolve': (_i, [_p] * 5 + [_i] * 3 + [_p]),
    # lasr_amd/csrc/bake_fill.hip
    'lasr_bake_mirror': (_i, [_p] * 8 + [_i] * 5 + [_f, _p]),
    'lasr_bake_blend': (_i, [_p] * 4 + [_i] * 2 + [_p]),
    # lasr_amd/csrc/rig.hip
    'lasr_rig_pack': (_i, [_p, _i, _i, _i, _p, _p, _p, _p]),
    'lasr_rig_quats': (_i, [_p, _i, _i, _p, _p]),
    'lasr_rig_skin': (_i, [_p] * 5 + [_i] * 4 + [_p, _p]),
    'lasr_rig_stats': (_i, [_p, _p, _i, _i, _p, _p]),
    # lasr_amd/csrc/maskprop.hip
    'lasr_maskprop_hist': (_i, [_p] * 3 + [_i] * 6 + [_f, _f, _p]),
    'lasr_maskprop_unary': (_i, [_p] * 8 + [_i, _i] + [_f] * 5 + [_p]),
    'lasr_maskprop_meanfield': (_i, [_p] * 4 + [_i] * 3 + [_f] * 3 + [_p]),
    # lasr_amd/csrc/tracks.hip
    'lasr_track_anchor': (_i, [_p] * 7 + [_i] * 9 + [_p]),
    'lasr_track_project': (_i, [_p] * 7 + [_i] * 8 + [_p]),
    'lasr_track_splat_keys': (_i, [_p] * 3 + [_i] * 5 + [_p]),
    'lasr_track_splat_resolve': (_i, [_p] * 4 + [_i] * 4 + [_p]),
    # lasr_amd/csrc/reproj.hip
    'lasr_reproj_workspace_bytes': (_sz, [_i, _i, _i]),
    'lasr_reproj_pixels': (_i, [_p] * 15 + [_i] * 6 + [_p]),
    'lasr_reproj_boundary': (_i, [_p] * 3 + [_i] * 4 + [_p]),
    # lasr_amd/csrc/varflow.hip
    'lasr_varflow_reduce': (_i, [_p] * 4 + [_i] * 2 + [_p]),
    'lasr_varflow_expand': (_i, [_p] * 2 + [_i] * 4 + [_p]),
    'lasr_varflow_tensor': (_i, [_p] * 4 + [_i] * 2 + [_p]),
    'lasr_varflow_weights': (_i, [_p] * 4 + [_i] * 2 + [_f, _p]),
    'lasr_varflow_sor': (_i, [_p] * 5 + [_i] * 2 + [_f, _f, _i, _p]),
    'lasr_varflow_occ': (_i, [_p] * 3 + [_i] * 2 + [_f, _f, _p]),
    # lasr_amd/csrc/robustflow.hip
    'lasr_rflow_derivs': (_i, [_p] * 2 + [_i] * 2 + [_p]),
    'lasr_rflow_tensor': (_i, [_p] * 5 + [_i] * 2 + [_p]),
    'lasr_rflow_weights': (_i, [_p] * 6 + [_i] * 2 + [_f, _f, _f, _p]),
    # lasr_amd/csrc/flowmatch.hip
    'lasr_flowmatch_quantise': (_i, [_p] * 3 + [_i] * 2 + [_p]),
    'lasr_flowmatch_search': (_i, [_p] * 4 + [_i] * 4 + [_p]),
    'lasr_flowmatch_select': (_i, [_p] * 9 + [_i] * 5 + [_p]),
    'lasr_flowmatch_propagate': (_i, [_p] * 7 + [_i] * 4 + [_p]),
    # lasr_amd/csrc/motionseg.hip
    'lasr_motionseg_conf': (_i, [_p] * 3 + [_i] * 2 + [_f, _p]),
    'lasr_motionseg_moments': (_i, [_p] * 5 + [_i] * 2 + [_p]),
    'lasr_motionseg_solve': (_i, [_p] * 3 + [_i] * 3 + [_f] * 3 + [_p]),
    'lasr_motionseg_evidence': (_i, [_p] * 4 + [_i] * 2 + [_f, _f, _i, _p]),
    # lasr_amd/csrc/meshcheck.hip
    'lasr_meshcheck_workspace_bytes': (_sz, [_i, _i]),
    'lasr_meshcheck_faces': (_i, [_p, _p, _p, _sz, _p, _p] + [_i] * 3 + [_p]),
    'lasr_meshcheck_pairs': (_i, [_p, _sz] + [_p] * 4 + [_i] * 3 + [_p]),
    # lasr_amd/csrc/meshnbr.hip
    'lasr_meshnbr_list': (_i, [_p] * 3 + [_i] * 2 + [_p]),
    'lasr_meshnbr_test': (_i, [_p, _sz, _p, _i, _f] + [_p] * 5 + [_i] * 3 + [_p]),
    # lasr_amd/csrc/foldpen.hip
    'lasr_foldpen_scratch_bytes': (_sz, [_i, _i]),
    'lasr_foldpen_forward': (_i, [_p, _p, _p, _i, _f, _p, _p, _p, _sz, _p] + [_i] * 3 + [_p]),
    'lasr_foldpen_backward': (_i, [_p, _p, _p, _i, _p, _p] + [_i] * 3 + [_p]),
    # lasr_amd/csrc/isectpen.hip
    'lasr_isectpen_scratch_bytes': (_sz, [_i, _i]),
    'lasr_isectpen_forward': (_i, [_p, _p, _p, _sz] + [_p] * 4 + [_i] * 3 + [_p]),
    # lasr_amd/csrc/ssim.hip
    'lasr_ssim_scratch_floats': (_sz, [_i] * 4),
    'lasr_ssim_forward': (_i, [_p] * 5 + [_i] * 4 + [_f, _p]),
    'lasr_ssim_backward': (_i, [_p] * 5 + [_i] * 4 + [_f, _p]),
    # lasr_amd/csrc/glue.hip
    'lasr_geodesic_forward': (_i, [_p, _p, _p, _i, _p]),
    'lasr_geodesic_backward': (_i, [_p, _p, _p, _p, _p, _i, _p]),
    'lasr_weighted_means_forward': (_i, [_p, _p, _p, _p, _i, _i, _p, _p]),
    'lasr_weighted_means_backward': (_i, [_p, _p, _i, _p, _p, _p]),
    'lasr_intrinsics_forward': (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _p]),
    'lasr_intrinsics_backward': (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_bone_fixup_forward': (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_bone_fixup_backward': (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_bone_fixup_pair_forward': (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_bone_fixup_pair_backward': (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_chamfer_forward': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_chamfer_backward': (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'lasr_fill_planes': (_i, [_p, _p, _i, _i, ctypes.c_longlong, _p]),
    'lasr_tail_chunk_elems': (_i, []),
    'lasr_tail_step': (_i, [_p, _p, _i, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
    'lasr_obs_pair': (_i, [_p, _p, _p, _i, _i, _p]),
    'lasr_render_tables_scratch_floats': (_sz, [_i, _i, _i]),
    'lasr_render_tables_forward': (_i, [_p, _p, _p, _p, ctypes.c_longlong, _p, _p, _p, _p, _f] + [_p] * 9 + [_i, _i, _i, _p]),
    'lasr_render_tables_forward_imgs': (_i, [_p, _p, _p, _p, ctypes.c_longlong, _p, _p, _p, _p, _f] + [_p] * 9 + [_i, _i, _i, _p]),
    'lasr_render_tables_backward': (_i, [_p, _p, _p, _p, ctypes.c_longlong, _p, _p, _p, _p, _f] + [_p] * 8 + [_i, _i, _i, _p]),
    'lasr_raster_inputs_forward': (_i, [_p] * 9 + [_i, _i, _p]),
    'lasr_raster_inputs_backward': (_i, [_p] * 8 + [_i, _i, _p]),
    'lasr_raster_faces_scratch_floats': (_sz, [_i, _i, _i]),
    'lasr_raster_faces_forward': (_i, [_p] * 6 + [_i] + [_p] * 4 + [_i, _i, _i, _p]),
    'lasr_raster_faces_backward': (_i, [_p] * 4 + [_i] + [_p] * 7 + [_i, _i, _i, _p]),
    'lasr_gather_rows': (_i, [_p, ctypes.c_longlong, _i, _p, _i, _i, _p, _p, _p, _p, _p]),
    'lasr_mean_shape_forward': (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_mean_shape_backward': (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'lasr_sr_forward_dev': (_i, [_p, _p, _p, _p, _p, _p, _sz] + _RASTER_SCALARS_DEV),
    'lasr_sr_backward_dev': (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _sz] + _RASTER_SCALARS_DEV),
    'lasr_sr_forward_attr': (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _i, _i, _f, _f, _p, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p]),
    'lasr_sr_backward_attr': (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _i, _f, _f, _p, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p]),
    'lasr_sr_forward_ex': (_i, [_p] * 6 + [_sz] + [_i] * 5 + [_f, _f, _p, _f, _f, _i, _f, _f, _i, _i, _i, _i, _i, _p]),
    'lasr_sr_forward_bg': (_i, [_p] * 6 + [_sz] + [_i] * 5 + [_f, _f, _p, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p, _i, _p]),
    'lasr_sr_backward_ex': (_i, [_p] * 8 + [_sz] + [_i] * 5 + [_f, _f, _p, _f, _f, _i, _f, _f, _i, _i, _i, _i, _i, _p]),
    'lasr_sr_forward_opt': (_i, [_p] * 6 + [_sz] + [_i] * 5 + [_f, _f, _p, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p, _i, _p, _p]),
    'lasr_sr_workspace_bytes_f64': (_sz, [_i, _i]),
    'lasr_sr_forward_f64': (_i, [_p] * 6 + [_sz] + [_i] * 4 + [_f, _f, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p]),
    'lasr_sr_backward_f64': (_i, [_p] * 9 + [_sz] + [_i] * 4 + [_f, _f, _f, _f, _i, _f, _f, _i, _i, _i, _i, _p]),
    'lasr_sr_peek_choice': (_i, [_p, _i, _i, ctypes.POINTER(ctypes.c_int), _p]),
    'lasr_sr_plan_forward': (_i, [_i] * 11 + [_p, _p]),
    'lasr_selftest_div': (_i, [_p, _p, _p, _i, _p]),
    'lasr_selftest_div3': (_i, [_p, _p, _p, _i, _p]),
    'lasr_selftest_face_div': (_i, [_i, _p, _i, _p]),
    'lasr_selftest_transpose64': (_i, [_p, _p, _p]),
    'lasr_prof_enable': (_i, [_p, _i]),
    'lasr_prof_kernel_count': (_i, []),
    'lasr_prof_kernel_name': (ctypes.c_char_p, [_i]),
    'lasr_prof_collect': (_i, [_p, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]),
}

ABI_VERSION = 13                                    # LASR_ABI_VERSION of include/lasr_sr.h (tests/test_abi.py compares them)
# flags of the *_ex entry points (include/lasr_sr.h)
SR_DEFAULT_FLAGS, SR_RELAXED_MATH, SR_SEGMENTED, SR_RECORDS_VALID, SR_GRADS_OVERWRITE = -1, 1, 2, 4, 8
SR_PAIR_ONE_TEAM, SR_PAIR_TWO_TEAMS = 16, 32          # forward: teams of four waves per tile of the pair-walk kernel (default: by launch size)
MEANS_MAX_TERMS, TAIL_MAX_GROUPS = 24, 16          # LASR_MEANS_MAX_TERMS / LASR_TAIL_MAX_GROUPS of include/lasr_ops.h
NN_TILE, ICP_MAX_BATCH, ICP_MAX_CHUNK = 512, 64, 4096   # LASR_NN_TILE / LASR_ICP_MAX_BATCH / LASR_ICP_MAX_CHUNK of include/lasr_ops.h
SHEET_MAX_SIZE, RING_MAX_SCALARS = 4096, 256            # LASR_SHEET_MAX_SIZE / LASR_RING_MAX_SCALARS of include/lasr_ops.h
BAKE_MAX_RES, BAKE_MAX_SIZE, BAKE_MAX_POWER = 32, 8192, 16   # LASR_BAKE_MAX_RES / LASR_BAKE_MAX_SIZE / LASR_BAKE_MAX_POWER of include/lasr_ops.h
RIG_MAX_BONES, RIG_MAX_INFLUENCES = 64, 8                    # LASR_RIG_MAX_BONES / LASR_RIG_MAX_INFLUENCES of include/lasr_ops.h
MASKPROP_BINS, MASKPROP_MAX_SIZE, MASKPROP_MAX_RADIUS = 4096, 16384, 8   # LASR_MASKPROP_* of include/lasr_ops.h
TRACK_MAX_SNAP, TRACK_MAX_WINDOW, TRACK_MAX_RADIUS, TRACK_MAX_SIZE, TRACK_SPLAT_ALPHA = 16, 2, 8, 8192, 192   # LASR_TRACK_* of include/lasr_ops.h
REPROJ_MAX_RADIUS = 96                              # LASR_REPROJ_MAX_RADIUS of include/lasr_ops.h
VARFLOW_MIN_SIZE, VARFLOW_MAX_SIZE = 2, 16384       # LASR_VARFLOW_* of include/lasr_ops.h
RFLOW_RECORD = 18                                   # LASR_RFLOW_RECORD of include/lasr_ops.h
FLOWMATCH_MAX_R, FLOWMATCH_MAX_PATCH = 32, 3        # LASR_FLOWMATCH_* of include/lasr_ops.h
MOTIONSEG_MAX_SIZE, MOTIONSEG_BLOCKS, MOTIONSEG_MOMENTS, MOTIONSEG_BINS, MOTIONSEG_STATE = 16384, 256, 28, 1024, 12   # LASR_MOTIONSEG_*
MESHCHECK_TILE, MESHCHECK_MAX_FACES, MESHCHECK_MAX_FRAMES = 256, 1 << 20, 65535   # LASR_MESHCHECK_* of include/lasr_ops.h
MESHNBR_COUNTERS = 4                                # LASR_MESHNBR_COUNTERS of include/lasr_ops.h: n_list, n_duplicate, n_degenerate, n_same
FOLDPEN_MAX_LIST = 214748364                        # LASR_FOLDPEN_MAX_LIST of include/lasr_ops.h: 10 n_list <= INT_MAX
SSIM_MIN_SIZE, SSIM_MAX_SIZE, SSIM_TILE_W, SSIM_TILE_H = 11, 4096, 32, 16         # LASR_SSIM_* of include/lasr_ops.h


class SrOptions(ctypes.Structure):
    """lasr_sr_options (include/lasr_sr.h): per-call kernel-choice thresholds of the forward pass and the size limit of the
    heaviest-first tile order; a negative field = default."""
    _fields_ = [('coop8_max_tiles', ctypes.c_longlong), ('coop_max_tiles', ctypes.c_longlong), ('choose_max_tiles', ctypes.c_longlong),
                ('order_max_tiles', ctypes.c_longlong), ('pair_min_tiles', ctypes.c_longlong)]


class SrPlan(ctypes.Structure):
    """lasr_sr_plan (include/lasr_sr.h): the forward plan lasr_sr_plan_forward reports -- kernel form, device-side choice, tile
    order and launch geometry."""
    _fields_ = [(n, _i) for n in ('form', 'both', 'choice_source', 'choice_max', 'ordered', 'order_groups', 'tile_shift', 'tso',
                                  'threads')] + [('choose_threshold', ctypes.c_longlong), ('grid', ctypes.c_longlong)]


# enum lasr_sr_form / enum lasr_sr_choice_source of include/lasr_sr.h
(SR_FORM_GENERIC, SR_FORM_ONE_WAVE, SR_FORM_ONE_WAVE_RELAXED, SR_FORM_FOUR_WAVES, SR_FORM_EIGHT_WAVES, SR_FORM_SEG_FOUR,
 SR_FORM_SEG_EIGHT, SR_FORM_PAIRS_ONE_TEAM, SR_FORM_PAIRS_TWO_TEAMS) = range(9)
SR_CHOICE_NONE, SR_CHOICE_BBOX_ESTIMATE, SR_CHOICE_NONEMPTY_TILES = range(3)


class VisParams(ctypes.Structure):
    """lasr_vis_params (include/lasr_ops.h): light frame, shading constants and output options of lasr_vis_shade."""
    _fields_ = [('light_u', _f * 3), ('light_v', _f * 3), ('light_d', _f * 3), ('k_ambient', _f), ('k_diffuse', _f),
                ('surface_alpha', _f), ('shadow_bias', _f), ('background', _f * 3), ('smooth', _i), ('overlay', _i)]


class SheetPlane(ctypes.Structure):
    """lasr_sheet_plane (include/lasr_ops.h): channel c of pixel i is ptr[c * chan_stride + i * pix_stride] (strides in floats)."""
    _fields_ = [('ptr', _p), ('chan_stride', ctypes.c_longlong), ('pix_stride', ctypes.c_longlong)]


class SheetInputs(ctypes.Structure):
    """lasr_sheet_inputs (include/lasr_ops.h): the device tensors behind the nine panels of lasr_monitor_sheet."""
    _fields_ = [(n, SheetPlane) for n in ('flow_obs', 'flow_rd', 'vis_mask', 'flow_err', 'mask_pred', 'mask_gt', 'part', 'img1',
                                          'img2', 'texture')] + [('ctl', _p), ('palette', _p), ('n_ctl', _i), ('ctl_stride', _i)]


_lib = None


class LasrNativeError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raises if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LasrNativeError(
                'liblasr_hip.so is not built (%s). Run `python -m lasr_amd.build` '
                '(hipcc --offload-arch=gfx950); there is no CPU fallback.' % LIB_PATH)
        # torch bundles its own libamdhip64.so.7; load it FIRST so that this library
        # binds to the same HIP runtime instance (stream handles are only valid
        # inside the runtime that created them): the import at the top of this module.
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)       # AttributeError here == ABI mismatch: let it propagate
            fn.restype = res
            fn.argtypes = args
        if h.lasr_abi_version() != ABI_VERSION:
            raise LasrNativeError('%s speaks ABI version %d, this package expects %d (LASR_ABI_VERSION of include/lasr_sr.h): rebuild '
                                  'with `python -m lasr_amd.build`' % (LIB_PATH, h.lasr_abi_version(), ABI_VERSION))
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        h = lib()
        msg = h.lasr_strerror(rc).decode()
        if rc == -4:
            msg += ' (hipError_t %d)' % h.lasr_last_hip_error()
        raise LasrNativeError('%s failed: %s' % (what, msg))


def stream_of(t):
    """(device-guard context, raw hipStream_t) for the device of a tensor (or for a torch.device): kernels go on torch's current
    stream."""
    dev = getattr(t, 'device', t)
    return torch.cuda.device(dev), torch.cuda.current_stream(dev).cuda_stream


_NEED_CUDA = 'lasr_amd kernels support only cuda (HIP) tensors; there is no CPU fallback'


def need_cuda(*tensors):
    for t in tensors:
        if t is not None and t.device.type != 'cuda':
            raise TypeError(_NEED_CUDA)


def call(name, *args, on=None):
    """One native launch: lib().<name>(*args, stream), checked.  Tensors go over as their data_ptr(); None, numbers, ctypes
    objects and plain integers (a pointer computed by hand, a host buffer) go over as they are.  The stream is torch's current
    one on the device of `on` (a tensor or a torch.device; default: the first tensor of args), read here and passed last, as
    every streamed entry point of include/*.h takes it.  Refused before the call: a tensor that is not on a GPU (TypeError), a
    tensor of another GPU than `on` (ValueError), a wrong number of arguments (TypeError; ctypes itself lets surplus ones pass)."""
    fn = getattr(lib(), name)
    dev = getattr(on, 'device', on)
    if dev is not None:
        if dev.type != 'cuda':
            raise TypeError(_NEED_CUDA)
        if dev.index is None:                           # 'cuda' = the current device
            dev = torch.device('cuda', torch.cuda.current_device())
    raw = []
    for a in args:
        if isinstance(a, torch.Tensor):
            d = a.device
            if d != dev:
                if d.type != 'cuda':
                    raise TypeError(_NEED_CUDA)
                if dev is not None:
                    raise ValueError('%s: a tensor of %s among arguments of %s' % (name, d, dev))
                dev = d
            a = a.data_ptr()
        raw.append(a)
    if len(raw) + 1 != len(fn.argtypes):
        raise TypeError('%s takes %d arguments and the stream, %d given' % (name, len(fn.argtypes) - 1, len(raw)))
    if dev is None:
        raise TypeError('%s: no tensor among the arguments, say on= which device' % name)
    guard, st = stream_of(dev)
    with guard:
        rc = fn(*raw, st)
    if rc != 0:
        check(rc, name)


def pointers(tensors):
    """ctypes array of the tensors' device addresses, for the entry points that take one pointer per layer or term.  The array
    keeps the tensors themselves in `.tensors`: they stay alive as long as it does, and a harness that moves a call's tensor
    arguments (tests/guarded.py) sees them where a bare array of addresses would hide them."""
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    arr.tensors = tuple(tensors)
    return arr


def f32(*tensors):
    """.contiguous().float() of each tensor (None stays None): one value for one argument, a tuple for several."""
    out = tuple(None if t is None else t.contiguous().float() for t in tensors)
    return out[0] if len(out) == 1 else out
