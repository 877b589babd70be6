"""ctypes binding of libclmgs_hip.so (C ABI declared in include/clmgs.h).

The library is the product: if it is missing, or if a tensor handed to an
operator is not a contiguous CUDA(HIP) tensor of the declared dtype, we raise --
there is deliberately no eager/PyTorch fallback path.
"""
import ctypes
import os
import time

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CLMGS_LIB_PATH") or os.path.join(_HERE, "libclmgs_hip.so")  # override: A/B builds

_vp, _i, _i64, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
_d = ctypes.c_double

# name -> (restype, argtypes); mirrors include/clmgs.h one to one
SIGNATURES = {
    "clmgs_version": (_i, []),
    "clmgs_last_error": (ctypes.c_char_p, []),
    "clmgs_projection_fwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "clmgs_visibility_select_temp_bytes": (_sz, [_i, _i]),
    "clmgs_visibility_select_count": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _sz, _vp]),
    "clmgs_visibility_select_count_blocks": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _sz, _vp, _vp]),
    "clmgs_visibility_select_count_blocks_sel": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _sz, _vp, _vp,
                                                      _vp, ctypes.c_uint64, _i, _i]),
    "clmgs_visibility_select_emit": (_i, [_vp, _i, _i, _vp, _vp]),
    "clmgs_visibility_raw": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp]),
    "clmgs_projection_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_sh_fwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "clmgs_sh_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "clmgs_isect_count_temp_bytes": (_sz, [_i]),
    "clmgs_isect_count": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz]),
    "clmgs_isect_sort_temp_bytes": (_sz, [_i64]),
    "clmgs_isect_emit_sort": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz]),
    "clmgs_isect_offsets": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp]),
    "clmgs_isect2_order_temp_bytes": (_sz, [_i]),
    "clmgs_isect2_order_count": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clmgs_isect2_sort_temp_bytes": (_sz, [_i64]),
    "clmgs_isect2_emit_sort": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clmgs_isect2_emit_sort_dev": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clmgs_isect3_front_temp_bytes": (_sz, [_i, _i]),
    "clmgs_isect3_front": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz]),
    "clmgs_isect3_bin_temp_bytes": (_sz, [_i64, _i]),
    "clmgs_isect3_bin": (_i, [_vp, _i, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "clmgs_isect3_bin_dev": (_i, [_vp, _i, _i64, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "clmgs_rasterize_fwd_dev": (_i, [_vp, _i, _i, _i64, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_rasterize_bwd_dev": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_rasterize_pack_bytes": (_sz, [_i, _i]),
    "clmgs_rasterize_fwd": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_rasterize_partials_bytes": (_sz, [_i64]),
    "clmgs_rasterize_bwd": (_i, [_vp, _i, _i, _i64, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # per-Gaussian blend weights (contribution pruning): integer atomics into three caller-owned arrays
    "clmgs_rasterize_contrib_pack_bytes": (_sz, [_i, _i]),
    "clmgs_rasterize_contrib": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    # median depth: per pixel the depth and row of the entry at which T falls through one half
    "clmgs_rasterize_median_pack_bytes": (_sz, [_i, _i]),
    "clmgs_rasterize_median": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    # ray depth: per pixel the depth at which the median Gaussian's 3-D density peaks along the pixel's ray
    "clmgs_ray_depth": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _d, _i, _vp]),
    "clmgs_rasterize4_fwd": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_rasterize4_bwd": (_i, [_vp, _i, _i, _i64, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # four channels on the slot route and in the device-count forms: the argument lists of the 3-channel entries
    "clmgs_rasterize4_slot_bwd": (_i, [_vp, _i, _i, _i64, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_rasterize4_fwd_dev": (_i, [_vp, _i, _i, _i64, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_rasterize4_bwd_dev": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_preprocess_grid_cap": (_i, []),
    "clmgs_preprocess_fwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_preprocess_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i]),
    # gsplat's absgrad: the plain entries' arguments (+ one trailing optional output where the plain entry unpacks)
    "clmgs_rasterize_abs_bwd": (_i, [_vp, _i, _i, _i64, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_rasterize_abs_bwd_dev": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_preprocess_abs_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    # gsplat's fully_fused_projection(calc_compensations=True): the plain entries + compensations / v_compensations
    "clmgs_projection_aa_fwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_projection_aa_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # gsplat's fully_fused_projection(camera_model="ortho"): the argument lists of the _aa_ pair
    "clmgs_projection_ortho_fwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_projection_ortho_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # gsplat's rasterization(rasterize_mode="antialiased"): the argument lists of the plain front-end entries
    "clmgs_preprocess_aa_fwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_preprocess_aa_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i]),
    "clmgs_preprocess_aa_abs_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "clmgs_ssim_fwd": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_ssim_bwd": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "clmgs_loss_slots": (_i, []),
    "clmgs_l1_ssim_loss_fwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_l1_ssim_loss_bwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "clmgs_l1_ssim_loss_masked_fwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_l1_ssim_loss_masked_bwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_exposure_partials_rows": (_i, [_i, _i]),
    "clmgs_exposure_fwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64]),
    "clmgs_exposure_bwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp]),
    "clmgs_exposure_grad_finish": (_i, [_vp, _i, _vp, _vp]),
    "clmgs_bilagrid_partials_rows": (_i, [_i, _i, _i, _i]),
    "clmgs_bilagrid_fwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _i, _i, _i, _vp, _i64, _i64, _i64]),
    "clmgs_bilagrid_bwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _i, _i, _i, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp]),
    "clmgs_bilagrid_grad_finish": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "clmgs_bilagrid_tv_grad": (_i, [_vp, _vp, _i64, _i, _i, _i, _f, _vp]),
    # learnable sky: image view, alphas, host viewmat[16] and K[9], the map and its shape; int64 fixed-point accumulator
    "clmgs_sky_fwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i, _i, _vp, _i64, _i64, _i64]),
    "clmgs_sky_bwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "clmgs_sky_acc_add": (_i, [_vp, _i64, _vp, _vp]),
    "clmgs_sky_grad_convert": (_i, [_vp, _i64, _vp, _vp]),
    # camera pose refinement: the inputs of clmgs_preprocess_bwd -> 16 floats per workgroup; the operator form
    "clmgs_pose_grad_partials_rows": (_i, [_i]),
    "clmgs_pose_grad": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "clmgs_pose_grad_finish": (_i, [_vp, _i, _vp, _vp]),
    "clmgs_projection_viewmat_partials_rows": (_i, [_i]),
    "clmgs_projection_viewmat_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_invdepth_partials_rows": (_i, [_i, _i]),
    "clmgs_invdepth_pack": (_i, [_vp, _i, _vp, _vp, _vp]),
    "clmgs_invdepth_l1_fwd_bwd": (_i, [_vp, _i, _i, _vp, _i64, _i64, _vp, _f, _f, _vp, _f, _vp, _i64, _i64, _vp]),
    "clmgs_invdepth_finish": (_i, [_vp, _i, _vp, _vp]),
    "clmgs_invdepth_rows_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    # resolution schedule: exact integer area resampling (u8 planes, one u16 plane, the loss mask + its count)
    "clmgs_area_resample_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "clmgs_area_resample_u16": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "clmgs_area_resample_mask": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    # lens distortion: sizes, the host lens record [10 doubles], the fisheye flag, fxo, fyo, src, (src_mask), dst, (valid, count)
    "clmgs_undistort_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_undistort_u16": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _d, _d, _vp, _vp]),
    # compressed models: n, K, rows, codebook, idx, (dist), temp | rows, idx, scale, acc, counts | acc, counts, scale, codebook
    "clmgs_vq_assign_temp_bytes": (_sz, [_i]),
    "clmgs_vq_assign": (_i, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _sz]),
    "clmgs_vq_accumulate": (_i, [_vp, _i64, _i, _vp, _vp, _d, _vp, _vp]),
    "clmgs_vq_finish": (_i, [_vp, _i, _vp, _vp, _d, _vp]),
    # mesh export: grid dims, grid, B, H, W, depth, alpha, rgb, host cams[B,16], near, depth_max, alpha_min, trunc, inv_trunc,
    # cull | grid, min_weight, cell_count | grid, cell_scan, V, host grid_to_world[12], verts, colours | ... quad_count | faces
    "clmgs_tsdf_integrate": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i]),
    "clmgs_tsdf_cells": (_i, [_vp, _i, _i, _i, _vp, _f, _vp]),
    "clmgs_tsdf_vertices": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "clmgs_tsdf_quad_count": (_i, [_vp, _i, _i, _i, _vp, _f, _vp, _vp]),
    "clmgs_tsdf_quads": (_i, [_vp, _i, _i, _i, _vp, _f, _vp, _vp, _i, _i, _vp]),
    # mesh cleanup: V, F, faces, parent, flag | V, parent, flag | V, F, faces, labels, count
    "clmgs_tsdf_mark": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _f, _f, _f, _f, _d]),
    "clmgs_tsdf_sparse_integrate": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i]),
    "clmgs_tsdf_sparse_extract": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                       _vp, _vp]),
    "clmgs_mesh_hook": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "clmgs_mesh_shortcut": (_i, [_vp, _i, _vp, _vp]),
    "clmgs_mesh_component_faces": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    # mesh decimation: V, F, faces, mark | V, verts, mark, cell, keys, flag | V, F, C, faces, cluster, out_faces, collapsed,
    # inc | V, F, C, verts, colours, faces, cluster_keys, vert_order, vert_start, n_members, inc, inc_start, n_inc, lane_order,
    # cell, out_verts, out_colours, code
    "clmgs_mesh_decimate_mark": (_i, [_vp, _i, _i, _vp, _vp]),
    "clmgs_mesh_decimate_keys": (_i, [_vp, _i, _vp, _vp, _d, _vp, _vp]),
    "clmgs_mesh_decimate_faces": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_mesh_decimate_place": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _d, _vp, _vp,
                                       _vp]),
    # mesh smoothing and normals: V, F, verts_in, faces, order, start, factor, verts_out | V, F, verts, faces, order, start,
    # normals
    "clmgs_mesh_smooth_step": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _d, _vp]),
    "clmgs_mesh_vertex_normals": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    # mesh evaluation: V, F, verts, faces, spacing, area, count | V, F, verts, faces, area, offsets, sample_face, S, points,
    # weight | V, N, verts, faces, ox, oy, oz, h, gx, gy, gz, count | ..., offsets, pairs, cell, prim | P, queries, V, N, verts,
    # faces, ox, oy, oz, h, gx, gy, gz, cell_start, pair_prim, pairs, max_distance, dist, prim, evaluated
    "clmgs_mesh_sample_count": (_i, [_vp, _i, _i, _vp, _vp, _d, _vp, _vp]),
    "clmgs_mesh_sample_emit": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "clmgs_mesh_bin_count": (_i, [_vp, _i, _i, _vp, _vp, _d, _d, _d, _d, _i, _i, _i, _vp]),
    "clmgs_mesh_bin_emit": (_i, [_vp, _i, _i, _vp, _vp, _d, _d, _d, _d, _i, _i, _i, _vp, _i64, _vp, _vp]),
    "clmgs_mesh_distance": (_i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _d, _d, _d, _d, _i, _i, _i, _vp, _vp, _i64, _d, _vp, _vp,
                                 _vp]),
    "clmgs_mcmc_relocation": (_i,[_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_mcmc_reg_grad": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _f, _f]),
    "clmgs_mcmc_noise": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _f, _vp]),
    "clmgs_rows_gather": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i]),
    "clmgs_rows_scatter_add": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i]),
    "clmgs_scatter_to_bit": (_i, [_vp, _vp, _i, _vp, _i64, _i]),
    "clmgs_extract_ffs": (_i, [_vp, _vp, _i, _i64, _vp]),
    "clmgs_pair_overlap_count": (_i, [_vp, _vp, _i, _i64, _i, _vp]),
    "clmgs_set_signal": (_i, [_vp, _vp, _i, ctypes.c_int32]),
    "clmgs_adam_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i64, _i, _vp, _d, _d, _d, _i, _i, _f, _i]),
    "clmgs_pack_small": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_adam_small_packed": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _d, _d, _d, _i, _i, _f, _vp, _i]),
    "clmgs_adam_catch_up": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _vp, _d, _d, _d, _i, _i, _i, _vp, _vp, _f, _i]),
    "clmgs_host_adam_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _vp, _d, _d, _d, _i, _i, _f, _i, _vp, _i]),
    "clmgs_host_pool_start": (_i, [_i]),
    "clmgs_host_usable_cpus": (_i, []),
    "clmgs_memcpy_async": (_i, [_vp, _vp, _vp, _sz, _i]),
    "clmgs_host_rows_prepare": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _vp, _d, _d, _d, _i, _i, _i, _f, _i, _vp, _i]),
    "clmgs_densify_stats": (_i, [_vp, _i64, _vp, _vp, _vp, _i, _f, _f, _vp, _vp, _vp]),
    "clmgs_morton_order_temp_bytes": (_sz, [_i64]),
    "clmgs_morton_order": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _sz]),
    "clmgs_tsp_tour": (_i, [_i, _vp, _vp]),
    "clmgs_knn3_mean_dist2": (_i, [_vp, _i, _vp, _vp, _f, _f, _f, _f, _i, _i, _i, _i, _vp]),
    "clmgs_host_groups_temp_bytes": (_sz, [_i64]),
    "clmgs_host_groups": (_i, [_vp, _i64, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz]),
    "clmgs_publish_pack": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i64, _i]),
    "clmgs_visibility_candidates": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _f, _vp]),
    "clmgs_small_rows_scatter": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clmgs_adam_small_packed_range": (_i, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _d, _d, _d, _i, _i, _f, _vp, _i]),
    "clmgs_small_deferred_kmax": (_i, []),
    "clmgs_adam_small_deferred": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _d, _d, _d,
                                       _f, _i, _vp, _vp, _i, _i, _f, _f, _f, _i, _vp]),
    "clmgs_adam_small_deferred_sel": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _d, _d, _d,
                                           _f, _i, _vp, _vp, _i, _i, _f, _f, _f, _i, _vp, _vp, _vp, ctypes.c_uint64, _i]),
    "clmgs_device_errors": (_i, [_vp, _i]),
    "clmgs_pinned_alloc": (_vp, [_sz]),
    "clmgs_pinned_free": (_i, [_vp]),
}

_lib = None

# Optional per-entry-point device timing (bench.py's roofline leg): when TIMING is a dict every
# stream-taking call is bracketed by two events recorded on the stream it is launched on.
TIMING = None
# Data-dependent sizes seen by the front end (intersections per image), for the same purpose.
STATS = {"n_isects": [], "n_emitted": [], "host_wait_s": 0.0}  # host_wait_s: time blocked in size readbacks


class ClmgsError(RuntimeError):
    pass


class _Entry:
    """One C entry point; times itself on the launch stream when TIMING is enabled."""

    def __init__(self, name, fn, takes_stream):
        self.name, self.fn, self.takes_stream = name, fn, takes_stream

    def __call__(self, *args):
        if TIMING is None or not self.takes_stream:
            return self.fn(*args)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h = getattr(args[0], "value", args[0])  # events go on the stream the kernel is launched on
        st = torch.cuda.ExternalStream(h) if h else torch.cuda.current_stream()
        s.record(st)
        rc = self.fn(*args)
        e.record(st)
        TIMING.setdefault(self.name, []).append((s, e))
        return rc


class _Namespace:
    pass


_NO_STREAM = {"clmgs_version", "clmgs_loss_slots", "clmgs_preprocess_grid_cap","clmgs_exposure_partials_rows", "clmgs_bilagrid_partials_rows", "clmgs_invdepth_partials_rows", "clmgs_pose_grad_partials_rows", "clmgs_projection_viewmat_partials_rows", "clmgs_small_deferred_kmax", "clmgs_isect3_front_temp_bytes",
              "clmgs_isect3_bin_temp_bytes", "clmgs_last_error", "clmgs_isect_count_temp_bytes",
              "clmgs_isect_sort_temp_bytes", "clmgs_host_groups_temp_bytes", "clmgs_isect2_order_temp_bytes", "clmgs_isect2_sort_temp_bytes", "clmgs_visibility_select_temp_bytes", "clmgs_rasterize_pack_bytes", "clmgs_rasterize_contrib_pack_bytes", "clmgs_rasterize_median_pack_bytes", "clmgs_rasterize_partials_bytes", "clmgs_host_adam_rows", "clmgs_host_pool_start", "clmgs_host_usable_cpus", "clmgs_host_rows_prepare", "clmgs_tsp_tour",
              "clmgs_pinned_alloc", "clmgs_pinned_free", "clmgs_device_errors", "clmgs_vq_assign_temp_bytes"}


def timing_summary():
    """name -> (n_calls, total_ms); call after torch.cuda.synchronize()."""
    out = {}
    for name, evs in (TIMING or {}).items():
        out[name] = (len(evs), sum(s.elapsed_time(e) for s, e in evs))
    return out


def lib():
    """Load (once) and return the shared library; raise loudly if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ClmgsError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C clm_gs_amd/csrc).  clm_gs_amd has no CPU/eager fallback."
            )
        l = ctypes.CDLL(LIB_PATH)
        ns = _Namespace()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError = ABI drift, also loud
            fn.restype = res
            fn.argtypes = args
            setattr(ns, name, _Entry(name, fn, name not in _NO_STREAM))
        _lib = ns
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().clmgs_last_error()
        raise ClmgsError(f"libclmgs_hip error {rc}: {msg.decode() if msg else ''}")


def check_device_errors():
    """Raises if a kernel has raised the library's device error word since the last check (clmgs_device_errors;
    synchronises the device).  Called where the host synchronises anyway.  The one value in use is 4 (the deferred
    small-attribute Adam); 1 and 2 are retired."""
    bits = ctypes.c_uint32(0)
    check(lib().clmgs_device_errors(ctypes.byref(bits), 1))
    if bits.value & 4:
        raise ClmgsError("deferred small-attribute Adam: a block of rows was further behind than the recorded step history "
                         "(clmgs_adam_small_deferred, device error bit 4): its parameters are wrong")
    if bits.value:
        raise ClmgsError(f"device error word {bits.value}: no kernel of this library raises that value (4 is the only one "
                         "in use); the results since the last check cannot be trusted")


HOST_REGIONS = None  # set to {} to accumulate host wall time per engine region (diagnostics)
REGION_TRACE = None  # set to {} (with HOST_REGIONS) to keep every occurrence's time as well
_ROCTX = None        # libroctx64 handle when CLMGS_ROCTX=1 (ranges show up in `rocprofv3 --marker-trace`)


def roctx():
    """roctx range markers around the engine's regions (the reference's torch.cuda.nvtx.range_push / pop,
    train.py:238-250): off unless CLMGS_ROCTX=1, so the product path makes no extra calls."""
    global _ROCTX
    if _ROCTX is None:
        _ROCTX = False
        if os.environ.get("CLMGS_ROCTX") == "1":
            for name in ("librocprofiler-sdk-roctx.so", "libroctx64.so"):
                try:
                    l = ctypes.CDLL(name)
                    l.roctxRangePushA.argtypes = [ctypes.c_char_p]
                    l.roctxRangePushA.restype = ctypes.c_int
                    l.roctxRangePop.restype = ctypes.c_int
                    _ROCTX = l
                    break
                except (OSError, AttributeError):
                    continue
    return _ROCTX


class host_region:
    """with host_region("name"): ...   -- adds the block's host wall time to HOST_REGIONS[name]; with
    CLMGS_ROCTX=1 the block is also a roctx range."""
    __slots__ = ("name", "t0", "rx")

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.rx = roctx()
        if self.rx:
            self.rx.roctxRangePushA(self.name.encode())
        if HOST_REGIONS is not None:
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if HOST_REGIONS is not None:
            dt = time.perf_counter() - self.t0
            HOST_REGIONS[self.name] = HOST_REGIONS.get(self.name, 0.0) + dt
            if REGION_TRACE is not None:  # per-occurrence times (diagnostics: which batch paid)
                REGION_TRACE.setdefault(self.name, []).append(round(dt * 1e3, 2))
        if self.rx:
            self.rx.roctxRangePop()
        return False


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t, dtype=None, allow_none=False, allow_host=False):
    """Raw pointer of a contiguous device tensor (or pinned host tensor if allowed)."""
    if t is None:
        if allow_none:
            return None
        raise ClmgsError("required tensor is None")
    if dtype is not None and t.dtype != dtype:
        raise ClmgsError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ClmgsError("tensor must be contiguous")
    if not t.is_cuda:
        if not (allow_host and (t.is_pinned() or getattr(t, "_clmgs_pinned", False))):
            raise ClmgsError("tensor must live on the GPU (no CPU fallback in clm_gs_amd)")
    return ctypes.c_void_p(t.data_ptr())
