"""ctypes binding of libancsh_hip.so (C ABI declared in include/ancsh_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails, this module
raises.  It never imports anything from oracle/.
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ANCSH_HIP_LIB") or os.path.join(_HERE, "libancsh_hip.so")   # override: an experimental build

_c_int, _c_long, _c_float, _vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p

# name -> argtypes (every function returns int status except the two diagnostics)
SIGNATURES = {
    "ancsh_farthest_point_sample": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "ancsh_farthest_point_sample_gather": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_prob_sample": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_gather_point": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "ancsh_query_ball_point": [_c_int, _c_int, _c_int, _c_float, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_query_ball_point_multi": [_c_int] + [_vp] * 10,
    "ancsh_group_point": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "ancsh_group_point_multi": [_c_int] + [_vp] * 9,
    "ancsh_selection_sort": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "ancsh_knn_point": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_group_point_ex": [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp],
    "ancsh_three_nn": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_three_weights": [_c_int, _vp, _vp, _vp],
    "ancsh_three_nn_weights": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "ancsh_three_interpolate": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_three_interpolate_ex": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp],
    "ancsh_conv1x1": [_c_long, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _c_int, _vp],
    "ancsh_conv1x1_ex": [_c_long, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _vp],
    "ancsh_conv1x1_packed": [_c_long, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _vp],
    "ancsh_conv1x1_packed_grouped": [_c_int, _c_long, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _vp],
    "ancsh_conv1x1_grouped": [_c_int, _c_long, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _c_int, _vp],
    "ancsh_sa_module_fused_grouped": [_c_int] * 9 + [_vp] * 4 + [_vp, _vp, _vp],
    "ancsh_sa_module_fused_partial_grouped": [_c_int] * 8 + [_vp] * 7,
    "ancsh_fp_interpolate_concat_ex": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _vp],
    "ancsh_sa_pack_weights_bf16x3": [_c_int, _c_int, _vp, _vp, _vp],
    "ancsh_sa_module_fused_bf16x3": [_c_int] * 8 + [_vp] * 4 + [_vp, _vp, _vp],
    "ancsh_sa_module_fused_partial_bf16x3": [_c_int] * 7 + [_vp] * 7,
    "ancsh_sa_module_fused_bf16x3_grouped": [_c_int] * 9 + [_vp] * 4 + [_vp, _vp, _vp],
    "ancsh_sa_module_fused_partial_bf16x3_grouped": [_c_int] * 8 + [_vp] * 7,
    "ancsh_sa_pack_weights_f16x2": [_c_int, _c_int, _vp, _vp, _vp],
    "ancsh_sa_module_fused_f16x2_grouped": [_c_int] * 9 + [_vp] * 4 + [_vp, _vp, _vp],
    "ancsh_sa_module_fused_partial_f16x2_grouped": [_c_int] * 8 + [_vp] * 7,
    "ancsh_mlp_chain_grouped_fp_f16x2": [_c_int] * 5 + [_vp] * 7 + [_vp],
    "ancsh_sa3_chain_grouped_bf16x3": [_c_int] * 7 + [_vp] * 4 + [_vp],
    "ancsh_sa3_chain_grouped_f16x2": [_c_int] * 7 + [_vp] * 4 + [_vp],
    "ancsh_fp1_chain_grouped_bf16x3": [_c_int] * 6 + [_vp] * 4 + [_vp],
    "ancsh_fp1_chain_grouped_f16x2": [_c_int] * 6 + [_vp] * 4 + [_vp],
    "ancsh_fp2_chain_grouped_bf16x3": [_c_int] * 8 + [_vp] * 6 + [_vp],
    "ancsh_fp2_chain_grouped_f16x2": [_c_int] * 8 + [_vp] * 6 + [_vp],
    # the F16x2 range guard: the unguarded arguments + (unsigned *range_flags, int flag_bit0) before the stream
    "ancsh_sa_module_fused_f16x2_grouped_guarded": [_c_int] * 9 + [_vp] * 4 + [_vp, _vp, _vp, _c_int, _vp],
    "ancsh_sa_module_fused_partial_f16x2_grouped_guarded": [_c_int] * 8 + [_vp] * 6 + [_vp, _c_int, _vp],
    "ancsh_mlp_chain_grouped_fp_f16x2_guarded": [_c_int] * 5 + [_vp] * 7 + [_vp, _c_int, _vp],
    "ancsh_sa3_chain_grouped_f16x2_guarded": [_c_int] * 7 + [_vp] * 4 + [_vp, _c_int, _vp],
    "ancsh_fp1_chain_grouped_f16x2_guarded": [_c_int] * 6 + [_vp] * 4 + [_vp, _c_int, _vp],
    "ancsh_fp2_chain_grouped_f16x2_guarded": [_c_int] * 8 + [_vp] * 6 + [_vp, _c_int, _vp],
    "ancsh_iou_3d": [_c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_joint_params": [_c_int] * 5 + [_vp] * 9 + [_vp],
    "ancsh_part_extents": [_c_int] * 4 + [_vp] * 3 + [_c_int] + [_vp] * 4 + [_vp],
    "ancsh_articulation_rec": [_c_int] * 5 + [_vp] * 10 + [_vp] * 4 + [_vp],
    "ancsh_fp_interpolate_concat": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _vp],
    "ancsh_query_ball_group_xyz": [_c_int, _c_int, _c_int, _c_float, _c_int, _vp, _vp, _c_int, _vp, _vp, _vp, _c_int, _vp],
    "ancsh_query_ball_group_xyz_multi": [_c_int] + [_vp] * 13,
    "ancsh_group_max": [_c_long, _c_int, _c_int, _vp, _vp, _vp],
    "ancsh_sa_module_fused": [_c_int] * 8 + [_vp] * 4 + [_vp, _vp, _vp],
    "ancsh_sa_module_fused_partial": [_c_int] * 7 + [_vp] * 7,
    "ancsh_sa_pack_weights": [_c_int, _c_int, _vp, _vp, _vp],
    "ancsh_mlp_chain": [_c_long, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp],
    "ancsh_mlp_chain_grouped": [_c_int, _c_long, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_sa3_chain_grouped": [_c_int] * 7 + [_vp] * 4 + [_vp],
    "ancsh_fp_single_source_init": [_c_int] * 5 + [_vp] * 3 + [_vp],
    "ancsh_fp1_chain_grouped": [_c_int] * 6 + [_vp] * 4 + [_vp],
    "ancsh_fp2_chain_grouped": [_c_int] * 8 + [_vp] * 6 + [_vp],
    "ancsh_mlp_chain_grouped_fp": [_c_int] * 5 + [_vp] * 8 + [_vp],
    "ancsh_mlp_chain_grouped_fp_bf16x3": [_c_int] * 5 + [_vp] * 7 + [_vp],
    "ancsh_head_activations": [_c_long, _c_int, _c_int, _vp, _c_int] + [_vp] * 10 + [_vp],
    "ancsh_pose_partition": [_c_int, _c_int, _c_int] + [_vp] * 11 + [_vp],
    "ancsh_pose_poison_records": [_c_int, _c_int, _c_int] + [_vp] * 5 + [_vp],
    "ancsh_pose_joint_direction": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "ancsh_ransac_single": [_c_int, _vp, _vp, _vp, _c_float, _c_int, _vp, ctypes.c_ulonglong, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_ransac_single_ex": [_c_int, _vp, _vp, _vp, _c_float, _c_int, _vp, ctypes.c_ulonglong, _c_int, _vp, _vp, _vp, _vp, _vp, _c_long, _vp],
    "ancsh_ransac_single_rec": [_c_int, _vp, _vp, _vp, _c_float, _c_int, _vp, ctypes.c_ulonglong, _c_int, _vp, _vp, _vp, _vp, _vp, _c_long,
                                _vp, _c_int, _vp, _c_float, _vp],
    "ancsh_ransac_joint_rec": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, ctypes.c_ulonglong, _c_int]
                              + [_vp] * 7 + [_c_int, _vp, _c_int, _vp, ctypes.c_double, _vp],
    "ancsh_ransac_joint": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, ctypes.c_ulonglong, _c_int]
                          + [_vp] * 7 + [_vp],
    "ancsh_ransac_single_rec_dseed": [_c_int, _vp, _vp, _vp, _c_float, _c_int, _vp, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _c_long,
                                      _vp, _c_int, _vp, _c_float, _vp],
    "ancsh_ransac_joint_rec_dseed": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, _vp, _c_int]
                                    + [_vp] * 7 + [_c_int, _vp, _c_int, _vp, ctypes.c_double, _vp],
    "ancsh_input_sample_stream": [_c_int, _c_int, _c_int, _vp, _c_long, _vp, _vp, _c_int, _vp, _vp, _vp, _vp, _vp],
    # the key block (ancsh_stream_key: seed, cloud_base) in place of the bare device seed: keys that follow a cloud's global index
    "ancsh_input_sample_stream_keyed": [_c_int, _c_int, _c_int, _vp, _c_long, _vp, _vp, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_ransac_single_rec_dkey": [_c_int, _vp, _vp, _vp, _c_float, _c_int, _vp, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _c_long,
                                     _vp, _c_int, _vp, _c_float, _vp],
    "ancsh_ransac_joint_rec_dkey": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, _vp, _c_int]
                                   + [_vp] * 7 + [_c_int, _vp, _c_int, _vp, ctypes.c_double, _vp],
    "ancsh_raw_point_labels": [_c_int] * 5 + [_vp, _c_long] + [_vp] * 8 + [_vp],
    # ABI 13: the joint association from the ANCSH network's index head, and xyz-only raw rows
    "ancsh_pose_joint_direction_pred": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp],
    "ancsh_pose_poison_records_pred": [_c_int, _c_int, _c_int] + [_vp] * 4 + [_c_int, _vp, _vp, _vp],
    "ancsh_input_sample_stream_xyz": [_c_int, _c_int, _c_int, _vp, _c_long, _vp, _vp, _vp, _vp, _vp, _vp],
    "ancsh_input_sample_stream_xyz_keyed": [_c_int, _c_int, _c_int, _vp, _c_long, _vp, _vp, _vp, _vp, _vp, _vp],
    # ABI 14: a joint kind per stage-B problem (0 revolute, 1 prismatic) -- the entry's arguments, then joint_kind, then the stream
    "ancsh_ransac_joint_rec_kind": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, ctypes.c_ulonglong, _c_int]
                                   + [_vp] * 7 + [_c_int, _vp, _c_int, _vp, ctypes.c_double, _vp, _vp],
    "ancsh_ransac_joint_rec_dseed_kind": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, _vp, _c_int]
                                         + [_vp] * 7 + [_c_int, _vp, _c_int, _vp, ctypes.c_double, _vp, _vp],
    "ancsh_ransac_joint_rec_dkey_kind": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, _vp, _c_int]
                                        + [_vp] * 7 + [_c_int, _vp, _c_int, _vp, ctypes.c_double, _vp, _vp],
    # the depth front end (no ABI bump: detected by its symbol): nclouds, depth_type, depth, mask, pixel_capacity, geom, cam, rows, capacity,
    # offsets, counts, scratch, stream
    "ancsh_depth_unproject_stream": [_c_int, _c_int, _vp, _vp, _c_long, _vp, _vp, _vp, _c_long, _vp, _vp, _vp, _vp],
    # its inverse for per-row labels (no ABI bump either): nclouds, depth_type, depth, mask, pixel_capacity, geom, offsets, scratch, labels,
    # values, capacity, dest, img_labels, img_values, image_capacity, stream
    "ancsh_depth_label_images": [_c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 5 + [_c_long, _vp, _vp, _vp, _c_long, _vp],
    # the joint states behind the articulation block (no ABI bump, detected by its symbol): b, n, K, P, ldp, npcs_nocs, npcs_mask, record,
    # art, wide, stream
    "ancsh_joint_state_rec": [_c_int] * 3 + [_vp, _c_int] + [_vp] * 5 + [_vp],
    # the fit quality behind the record (no ABI bump, detected by its symbol): b, K, off, src, tgt, record, inlier_th, best_a, score_b, wide,
    # stream
    "ancsh_fit_quality_rec": [_c_int] * 2 + [_vp] * 4 + [ctypes.c_double] + [_vp] * 3 + [_vp],
    # the errors against ground truth behind the record (no ABI bump, detected by its symbol): b, n, K, nres, P, ldp, npcs_nocs, npcs_mask,
    # record, ld, gt, wide, stream
    "ancsh_gt_error_rec": [_c_int] * 4 + [_vp, _c_int] + [_vp] * 3 + [_c_int] + [_vp] * 2 + [_vp],
    # the per-point ground truth of a streamed batch behind the articulation launches (no ABI bump, detected by its symbol): b, n, K, nchan,
    # rows, capacity, offsets, perm, gocs_channels, joint_channels, the ANCSH heads W nocs gocs heatmap unitvec joint_axis joint_index, the
    # NPCS heads W nocs, art, ld_art, frame, record, ld, type_l, wide, joint_gt, stream
    "ancsh_point_gt_rec": [_c_int] * 4 + [_vp, _c_long, _vp, _vp, _c_int, _c_int] + [_vp] * 10 + [_c_int, _vp, _vp, _c_int, _c_int, _vp, _vp,
                                                                                                  _vp],
    # the per-point ground truth itself, built from annotated clouds in front of the sampler (no ABI bump, detected by its symbol): nclouds, K,
    # src, capacity, offsets, rig, rig_ld, rows, stream
    "ancsh_point_gt_build": [_c_int, _c_int, _vp, _c_long, _vp, _vp, _c_int, _vp, _vp],
    # the ground-truth poses of a streamed batch, fitted directly behind the sampler (no ABI bump, detected by its symbol): b, n, K, nchan, rows,
    # capacity, offsets, perm, P, ldp, extent, ld_extent, gt, frame, stream
    "ancsh_gt_pose_build": [_c_int] * 4 + [_vp, _c_long, _vp, _vp, _vp, _c_int, _vp, _c_int, _vp, _vp, _vp],
    # the annotated clouds themselves, made from depth and link-label crops (no ABI bump, detected by its symbol): nclouds, depth_type, depth,
    # labels, pixel_capacity, geom, scene, rows, capacity, offsets, counts, link_counts, scratch, stream
    "ancsh_depth_annotate_stream": [_c_int, _c_int, _vp, _vp, _c_long, _vp, _vp, _vp, _c_long, _vp, _vp, _vp, _vp, _vp],
    # the inverse of that entry's sort, predictions and ground truth per row back on the pixel grid (no ABI bump, detected by its symbol):
    # nclouds, depth_type, depth, link_labels, pixel_capacity, geom, scene, offsets, counts, scratch, labels, values, gt_rows, gt_nchan,
    # capacity, dest, img_labels, img_values, img_gt_labels, img_gt_values, image_capacity, stream
    "ancsh_depth_annotated_images": [_c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 8 + [_c_int, _c_long] + [_vp] * 5 + [_c_long, _vp],
    # those crops themselves, rendered from articulated triangle meshes (no ABI bump, detected by its symbol): nframes, depth_type, verts, tris,
    # tri_link, V, T, geom, render, depth, labels, zbuf, pixel_capacity, stream
    "ancsh_render_depth_labels": [_c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_long, _vp],
    # that entry's and the annotation's tables, built from an object's kinematic table and a pose per frame (no ABI bump, detected by its
    # symbol): nframes, kin, pose, render, scene, stream
    "ancsh_pose_scene_build": [_c_int, _vp, _vp, _vp, _vp, _vp],
    # crops centred on the projected object (no ABI bump, detected by its symbol): nframes, verts, tris, tri_link, V, T, render, geom, bounds,
    # stream
    "ancsh_render_centre_crops": [_c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp],
    # those three for a library of instances, the instance of a frame in render[9] / pose[28] (no ABI bump, detected by their symbols):
    # nframes, depth_type, verts, tris, tri_link, V, T, tri_off, ninst, Tmax, geom, render, depth, labels, zbuf, pixel_capacity, stream
    "ancsh_render_depth_labels_lib": [_c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_long, _vp],
    # nframes, verts, tris, tri_link, V, T, tri_off, ninst, render, geom, bounds, stream
    "ancsh_render_centre_crops_lib": [_c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp],
    # nframes, kin, ninst, pose, render, scene, stream
    "ancsh_pose_scene_build_lib": [_c_int, _vp, _c_int, _vp, _vp, _vp, _vp],
    # a depth sensor's defects on the crops of annotated frames (no ABI bump, detected by their symbols): nframes, depth_type, depth_in,
    # labels_in, pixel_capacity, geom, scene, sensor, seed (_keyed: the key block), depth_out, labels_out, stream
    "ancsh_depth_sensor_model": [_c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 6 + [_vp],
    "ancsh_depth_sensor_model_keyed": [_c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 6 + [_vp],
    # render-and-compare of a pose record (no ABI bump, detected by their symbols): nframes, K, render, scene, rig, rig_ld, norm_factor, record,
    # ld, geom, pixel_capacity, render_out, geom_out, stream
    "ancsh_reproject_scene_build": [_c_int, _c_int, _vp, _vp, _vp, _c_int, _vp, _vp, _c_int, _vp, _c_long, _vp, _vp, _vp],
    # nframes, K, depth_type, obs_depth, obs_labels, pixel_capacity, pred_depth, pred_labels, geom, scene, carried, ld, wide, stream
    "ancsh_reproject_compare_rec": [_c_int, _c_int, _c_int, _vp, _vp, _c_long, _vp, _vp, _vp, _vp, _vp, _c_int, _vp, _vp],
    # render-and-compare ICP of a pose record (no ABI bump, detected by their symbols): nframes, K, depth_type, verts, tris, tri_link, V, T,
    # obs_depth, obs_labels, pixel_capacity, pred_zbuf, pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, pass, is_last,
    # pose_in, ld_in, pose_out, best, sums, stream
    "ancsh_refine_pass": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 8 + [_c_int, _c_int, _vp, _c_int,
                          _vp, _vp, _vp, _vp],
    # nframes, K, best, carried, ld, wide, stream
    "ancsh_refine_rec": [_c_int, _c_int, _vp, _vp, _c_int, _vp, _vp],
    # the silhouette term (no ABI bump, detected by their symbols): nframes, K, depth_type, obs_depth, obs_labels, pixel_capacity, geom, scene,
    # field, stream;  ancsh_refine_pass's arguments with field behind params
    "ancsh_silhouette_field": [_c_int, _c_int, _c_int, _vp, _vp, _c_long, _vp, _vp, _vp, _vp],
    "ancsh_refine_pass_sil": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 9 + [_c_int, _c_int, _vp, _c_int,
                              _vp, _vp, _vp, _vp],
    # the coverage term (no ABI bump, detected by their symbols): nframes, K, depth_type, pred_depth, pred_labels, pixel_capacity, geom_out,
    # scene, cover, stream;  ancsh_refine_pass_sil's arguments with cover behind field
    "ancsh_coverage_field": [_c_int, _c_int, _c_int, _vp, _vp, _c_long, _vp, _vp, _vp, _vp],
    "ancsh_refine_pass_cov": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 10 + [_c_int, _c_int, _vp, _c_int,
                              _vp, _vp, _vp, _vp],
    # the scale unknown (no ABI bump, detected by its symbol): ancsh_refine_pass_cov's arguments with fitted, ld_fitted behind cover
    "ancsh_refine_pass_scale": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _c_long] + [_vp] * 11 + [_c_int, _c_int, _c_int, _vp,
                                _c_int, _vp, _vp, _vp, _vp],
    # the joint step (no ABI bump, detected by its symbol): nframes, K, kin, ninst, scene, pred_render, norm_factor, params, pass, is_last,
    # pose_in, ld_in, sums, sums_ld, pose_out, best, state, obj, xi, stream
    "ancsh_refine_joint_step": [_c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp, _c_int, _vp, _c_int] + [_vp] * 6,
    # the joint values behind the articulation block (no ABI bump, detected by its symbol): nframes, K, kin, ninst, pose, render, scene, rig,
    # rig_ld, norm_factor, record, ld, refined, art, art_ld, wide, stream
    "ancsh_joint_values_rec": [_c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp, _vp, _c_int, _vp, _vp, _c_int, _vp, _vp],
    # both stages of the pose fit in one call (no ABI bump, detected by their symbols): ancsh_ransac_single_rec*'s arguments without record / K
    # (nprob_a .. tie_window_a), ancsh_ransac_joint_rec*'s without src / tgt / max_n / record / K (nprob_b .. tie_window_b), record, K,
    # [joint_kind,] stream
    **{"ancsh_pose_fit_rec" + sfx: [_c_int, _vp, _vp, _vp, _c_float, _c_int, _vp, key, _c_int, _vp, _vp, _vp, _vp, _vp, _c_long, _vp, _c_float,
                                    _c_int, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, key] + [_vp] * 7 + [_c_int, _vp, ctypes.c_double,
                                    _vp, _c_int] + kind + [_vp]
       for sfx, key, kind in (("", ctypes.c_ulonglong, []), ("_dseed", _vp, []), ("_dkey", _vp, []),
                              ("_kind", ctypes.c_ulonglong, [_vp]), ("_dseed_kind", _vp, [_vp]), ("_dkey_kind", _vp, [_vp]))},
    "ancsh_input_sample": [_c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_test_losses": [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp],
    "ancsh_ransac_joint_ex": [_c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _c_int, _vp, ctypes.c_ulonglong, _c_int]
                             + [_vp] * 7 + [_c_int, _vp],
    "ancsh_umeyama": [_c_int, _vp, _vp, _vp, _vp, _vp],
    "ancsh_estimate_similarity_transform": [_c_int, _vp, _vp, _vp, _c_int, _vp, ctypes.c_ulonglong, _vp, _vp, _vp],
}

_lib = None


def build(force=False):
    """Compile every HIP source for gfx950 into the in-tree libancsh_hip.so (hipcc cross-compiles
    without a GPU)."""
    args = ["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is not built (run __graft_entry__.build()); "
                "there is no CPU fallback for the product path")
        L = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(L, name)   # AttributeError if the ABI is incomplete
            fn.argtypes = argtypes
            fn.restype = _c_int
        L.ancsh_last_error.restype = ctypes.c_char_p
        L.ancsh_abi_version.restype = _c_int
        L.ancsh_last_ball_query_schedule.restype = _c_int
        L.ancsh_sa_packed_weight_floats.argtypes = [_c_int, _c_int]
        L.ancsh_sa_packed_weight_floats.restype = _c_long
        L.ancsh_sa_packed_weight_bytes_bf16x3.argtypes = [_c_int, _c_int]
        L.ancsh_sa_packed_weight_bytes_bf16x3.restype = _c_long
        L.ancsh_sa_packed_weight_bytes_f16x2.argtypes = [_c_int, _c_int]
        L.ancsh_sa_packed_weight_bytes_f16x2.restype = _c_long
        L.ancsh_ransac_single_quads_floats.argtypes = [_c_long, _c_int]
        L.ancsh_ransac_single_quads_floats.restype = _c_long
        _lib = L
    return _lib


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


_prof = None   # when a list: every call is bracketed by HIP events on the launch stream
_prof_lead = (0, {})


def profile_start(lead=0, lead_for=None):
    """lead = n: every call is issued n times back-to-back before the timed launch (all entry points are pure functions of
    their inputs, so repeating one is harmless); lead_for = {abi name: n} overrides it per entry point.  The lead launches keep the chip under load between the timed ones: a kernel
    that starts on an idle chip runs at the clock the power management is still ramping (measured with s_memtime: the fused SA
    kernels take 238 / 284 us in a 20-launch loop from idle and 209 / 262 us once the loop has run for 50 ms), and the eager pass
    spends more time in Python between launches than on the GPU."""
    global _prof, _prof_lead
    _prof, _prof_lead = [], (int(lead), dict(lead_for or {}))


def profile_stop():
    """-> [(abi name, args, milliseconds)] for every call since profile_start(); synchronises."""
    global _prof
    rec, _prof = _prof, None
    torch.cuda.synchronize()
    return [(n, a, e0.elapsed_time(e1)) for n, a, e0, e1 in rec]


def call(name, *args):
    """Call an ABI function on torch's current HIP stream; raise ValueError on a bad argument
    (mirrors the reference's OP_REQUIRES -> InvalidArgument) and RuntimeError on a HIP failure."""
    L = lib()
    if _prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(_prof_lead[1].get(name, _prof_lead[0])):
            getattr(L, name)(*args, stream_ptr())
        e0.record()
        rc = getattr(L, name)(*args, stream_ptr())
        e1.record()
        _prof.append((name, args, e0, e1))
    else:
        rc = getattr(L, name)(*args, stream_ptr())
    if rc != 0:
        msg = L.ancsh_last_error().decode()
        if rc == -1:
            raise ValueError(msg)
        raise RuntimeError(f"{name}: {msg}")


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("articulated-pose_amd ops run on the MI355X only: got a CPU tensor "
                               "(no CPU fallback in the product path)")


def require_device(*on):
    """The guard an op puts in front of everything else: `on` = the tensor that names its device, or an eager wrapper's torch.device.  A
    RuntimeError, where every later check is a ValueError."""
    for t in on:
        if not (t.type == "cuda" if isinstance(t, torch.device) else t.is_cuda):
            raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")


def cuda_device(device):
    """An eager wrapper's device argument -> the torch.device; require_device's RuntimeError unless it is a GPU."""
    dev = torch.device(device)
    require_device(dev)
    return dev
