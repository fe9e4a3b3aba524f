"""Loader and builder of ``libmmmot_hip.so`` (the C-ABI of include/mmmot_hip.h).

The library is built in-tree with ``hipcc --offload-arch=gfx950`` (no torch
headers, no CMake) and loaded with ctypes.  There is NO fallback: if the shared
object is missing or fails to load, every op raises - the product path never
computes on the CPU.
"""
import ctypes
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_PATH = os.environ.get('MMMOT_LIB_PATH', os.path.join(_HERE, 'libmmmot_hip.so'))  # override: tools' timing-experiment builds
SOURCES = ['conv3x3.hip', 'hl16_format.hip', 'conv3x3_hl16_patch.hip', 'gemm_rows.hip', 'gemm_wide.hip',
           'gemm_ares.hip', 'gemm_wres.hip', 'gemm_wreg.hip', 'pn_mlp64.hip', 'gram.hip', 'points_gather.hip', 'crop_resize.hip', 'crop_augment.hip','small_kernels.hip', 'backward.hip', 'train.hip', 'train_vgg.hip', 'gemm_tn_f16.hip',
           'assign.hip', 'assign_chain.hip', 'assign_sequence.hip','track_ids.hip', 'clear_mot.hip', 'hota.hip', 'mot3d.hip','align_points.hip', 'fill_tracks.hip', 'labels.hip', 'adam_step.hip', 'dropout.hip']
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
HIPFLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC']

_lock = threading.Lock()
_lib = None

c_f = ctypes.c_void_p  # device pointers travel as integers
c_i = ctypes.c_int


class GemmArgs(ctypes.Structure):
    """Mirror of ``mmmot_gemm_args`` (include/mmmot_hip.h)."""
    _fields_ = [
        ('X', c_f), ('ldx', c_i),
        ('W', c_f),
        ('bias', c_f),
        ('dbias', c_f), ('rowidx', c_f), ('lddb', c_i),
        ('Y', c_f), ('ldy', c_i),
        ('part', c_f),
        ('sc', c_f), ('sh', c_f), ('ldsc', c_i),
        ('FA', c_f), ('FB', c_f), ('ldf', c_i),
        ('tile_row0', c_f), ('tile_nrows', c_f), ('tile_group', c_f),
        ('grp_row0', c_f), ('grp_M', c_f), ('grp_aoff', c_f), ('grp_boff', c_f),
        ('T', c_i), ('N', c_i), ('K', c_i),
        ('amode', c_i), ('pairop', c_i), ('act', c_i),
        ('w_hl16', c_i), ('oscale', ctypes.c_float),
        ('osc', c_f), ('osh', c_f), ('ldosc', c_i),
        ('colsum', c_f),
        ('pair_uniform32', c_i),
    ]


class GemmAresArgs(ctypes.Structure):
    """Mirror of ``mmmot_gemm_ares_args`` (include/mmmot_hip.h)."""
    _fields_ = [
        ('X', c_f), ('ldx', c_i),
        ('sc', c_f), ('sh', c_f), ('ldsc', c_i),
        ('W', c_f),
        ('bias', c_f),
        ('dbias', c_f), ('tile_dbrow', c_f), ('lddb', c_i),
        ('tile_row0', c_f), ('tile_nrows', c_f), ('tile_group', c_f),
        ('part', c_f),
        ('osc', c_f), ('osh', c_f), ('ldosc', c_i),
        ('colsum', c_f),
        ('T', c_i), ('N', c_i), ('K', c_i),
        ('oscale', ctypes.c_float),
    ]


class GemmTnArgs(ctypes.Structure):
    """Mirror of ``mmmot_gemm_tn_args`` (include/mmmot_hip.h)."""
    _fields_ = [
        ('dY', c_f), ('lddy', c_i),
        ('X', c_f), ('ldx', c_i),
        ('sc', c_f), ('sh', c_f), ('ldsc', c_i),
        ('FA', c_f), ('FB', c_f), ('ldf', c_i),
        ('tile_row0', c_f), ('tile_nrows', c_f), ('tile_group', c_f),
        ('grp_row0', c_f), ('grp_M', c_f), ('grp_aoff', c_f), ('grp_boff', c_f),
        ('T', c_i), ('N', c_i), ('K', c_i), ('amode', c_i), ('pairop', c_i), ('nsplit', c_i),
        ('dW', c_f), ('db', c_f),
    ]


# name -> argtypes; every entry point declared in include/mmmot_hip.h
SIGNATURES = {
    'mmmot_abi_version': [],
    'mmmot_device_info': [c_i, ctypes.POINTER(c_i), ctypes.c_char_p, c_i],
    'mmmot_conv3x3_bn_relu': [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
    'mmmot_gemm_rows': [ctypes.POINTER(GemmArgs), c_f],
    'mmmot_set_gemm_rows_variant': [c_i],
    'mmmot_set_gemm_wide_grid_limit': [c_i],
    'mmmot_gemm_rows_choice': [ctypes.POINTER(GemmArgs), ctypes.POINTER(c_i), ctypes.POINTER(c_i), ctypes.POINTER(c_i),
                               ctypes.POINTER(c_i)],
    'mmmot_gemm_ares': [ctypes.POINTER(GemmAresArgs), c_f],
    'mmmot_set_gemm_ares_variant': [c_i],
    'mmmot_gram_rows': [c_f, c_i, c_i, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_f],
    'mmmot_set_gram128_variant': [c_i],
    'mmmot_gn_finalize_gram': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_i, c_f, c_f, ctypes.c_float, c_f, c_f, c_f, c_f],
    # Gp, Sp, grp_tile0, grp_ntiles, grp_count, G, tile_nrows, tile_det, K, W, dbias, lddb, N, gamma, beta, eps, work, sc, sh, stream
    'mmmot_gn_finalize_gram_dbias': [c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_f, c_f, ctypes.c_float,
                                     c_f, c_f, c_f, c_f],
    'mmmot_gn_finalize': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_f, ctypes.c_float, c_f, c_f, c_f],
    'mmmot_segment_mean': [c_f, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_f, c_i, c_i, c_f],
    'mmmot_conv3x3_bn_relu_hl16_patch': [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f],
    'mmmot_conv1_fused_hl16': [c_f, c_f, c_f, ctypes.c_float, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f],
    'mmmot_conv3x3_bn_relu_hq8': [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f],
    'mmmot_conv1_fused_u8': [c_f, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                             ctypes.c_float, c_f, c_f, ctypes.c_float, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
    'mmmot_u8_normalize': [c_f, c_i, c_i, c_f, c_f, c_f],
    'mmmot_conv1_fused_hq8': [c_f, c_f, c_f, ctypes.c_float, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f],
    'mmmot_conv3x3_first_hl16': [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
    'mmmot_set_patch_grid_limit': [c_i],
    'mmmot_set_patch_min_block': [c_i],
    'mmmot_set_patch_tile_width': [c_i],
    'mmmot_patch_choice': [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i), ctypes.POINTER(c_i), ctypes.POINTER(c_i), ctypes.POINTER(c_i)],
    'mmmot_trunk_range_read': [ctypes.POINTER(ctypes.c_uint), c_i],
    'mmmot_trunk_range_bind': [c_f],
    'mmmot_hl16_pack': [c_f, c_f, ctypes.c_long, c_f],
    'mmmot_hl16_unpack': [c_f, c_f, ctypes.c_long, c_f],
    'mmmot_hl16_pack_pow2': [c_f, c_f, ctypes.c_long, c_f, c_i, c_f],
    'mmmot_pow2_oscale': [c_f, c_i, c_f, c_i, c_f, c_i, c_f],
    'mmmot_conv3x3_raw_hl16': [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f],
    'mmmot_hq8_pack': [c_f, c_f, ctypes.c_long, c_f],
    'mmmot_hq8_unpack': [c_f, c_f, ctypes.c_long, c_f],
    'mmmot_rowdot': [c_f, c_i, c_i, c_f, ctypes.c_float, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i,
                     ctypes.c_float, c_f, c_f, c_f],
    'mmmot_row_layernorm': [c_f, c_i, c_i, c_f, c_f, ctypes.c_float, c_i, c_f, c_i, c_i, c_f],
    'mmmot_skippool_head': [c_f, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, ctypes.c_float, c_f, c_i, c_i,
                            c_f],
    'mmmot_pointnet_layer1': [c_f, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_f],
    'mmmot_pn_mlp64': [c_f, c_i, c_f, c_f, c_i, c_f, ctypes.c_float, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_i, c_f],
    'mmmot_affine_act': [c_f, c_i, c_i, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_f, c_i, c_f],
    'mmmot_fusion_combine': [c_i, c_f, c_f, c_i, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f,
                             c_i, c_i, c_f],
    'mmmot_softmax_pairs': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f],
    'mmmot_points_count': [c_f, c_i, c_i, c_f, c_i, c_i, c_f, c_f, c_f],
    'mmmot_points_scatter': [c_f, c_i, c_i, c_f, c_i, c_f, c_f, c_f, c_i, c_f],
    'mmmot_crop_resize_norm': [c_f, c_i, c_i, c_f, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f],
    # images, NI, img_of, boxes, N, S, kmax, mean_std, work, out, out_u8, stream
    'mmmot_crop_resize_norm_multi': [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f],
    # crops_u8, params, L, S, mean_std, out, out_u8, stream
    'mmmot_crop_augment': [c_f, c_f, c_i, c_i, c_f, c_f, c_f, c_f],
    'mmmot_points_count_batched': [c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_f],
    'mmmot_points_scatter_batched': [c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_f],
    # pts, F, Q, NS, seg_row0, xf, chain, out, out_row0, ldo, stream
    'mmmot_align_points': [c_f, c_i, c_i, c_i, c_f, c_f, c_i, c_f, ctypes.c_long, c_i, c_f],
    # det, ids, frame_start, frame_no, seq_start, xf, wtab, L, F, S, max_fill, capacity, work, fill_start, out, out_id,
    # out_src, info, stream
    'mmmot_fill_tracks': [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f],
    'mmmot_selftest_mfma': [c_f, c_f, c_f, c_i, c_f],
    'mmmot_gn_bwd_partial': [c_f, c_i, c_f, c_i, c_i, c_f, c_f, c_i, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_f],
    'mmmot_gn_bwd_finalize': [c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f],
    'mmmot_gn_bwd_apply': [c_f, c_i, c_f, c_i, c_i, c_f, c_f, c_i, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_f, c_i, c_f],
    'mmmot_gemm_tn': [ctypes.POINTER(GemmTnArgs), c_f],
    'mmmot_gemm_tn_f16': [ctypes.POINTER(GemmTnArgs), c_f, c_f],
    'mmmot_absmax': [c_f, c_i, ctypes.c_long, c_i, c_f, c_f],
    'mmmot_pair_bwd': [c_f, c_i, c_f, c_i, c_f, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f],
    'mmmot_pair_expand_bwd': [c_f, c_i, c_f, c_i, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_f],
    # X, ldx, C, seg_start, seg_count, seg_stride, seg_group, nseg, sc, sh, ldsc, relu, idx_out, ldo, stream
    'mmmot_segment_argmax': [c_f, c_i, c_i, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_f, c_i, c_f],
    # dV, lddv, idx, ldi, dA, ldda, C, tile_row0, tile_nrows, tile_group, T, grp_row0, grp_N, grp_M, grp_vrow0, stream
    'mmmot_pair_expand_max_bwd': [c_f, c_i, c_f, c_i, c_f, c_i, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_f],
    'mmmot_rowdot_bwd': [c_f, c_i, c_i, c_f, ctypes.c_float, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_f, c_i,
                         c_f, c_i, c_f],
    'mmmot_softmax_pairs_bwd': [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f],
    'mmmot_fusion_c_bwd': [c_f, c_f, c_i, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_i, c_f, c_f, c_i, c_f],
    'mmmot_add_rows': [c_f, c_i, c_f, c_i, c_f, c_i, ctypes.c_long, c_i, c_f],
    'mmmot_conv3x3_raw': [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
    'mmmot_rows_stats': [c_f, c_i, c_i, c_f, c_f, c_i, c_f, c_f],
    'mmmot_bn_relu_pool': [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_f],
    'mmmot_maxpool_bwd': [c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f],
    'mmmot_conv3x3_wgrad': [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f],
    'mmmot_conv3x3_wgrad_f16': [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f],
    'mmmot_conv3x3_first_wgrad': [c_f, c_f, c_i, c_i, c_i, c_f, c_i, c_f],
    'mmmot_rows_gather_scale': [c_f, c_i, c_f, c_f, c_f, c_i, ctypes.c_long, c_i, c_f],
    'mmmot_pointnet_layer1_bwd': [c_f, c_f, c_i, c_f, c_f, c_i, c_f, c_f],
    'mmmot_score_loss': [c_f, c_i, c_f, c_f, c_f, c_i, c_i, ctypes.c_float, c_i, ctypes.c_float, c_i, c_i, c_f, c_i, c_f,
                         c_i, c_i, c_f],
    'mmmot_ghm_loss': [c_f, c_i, c_f, ctypes.c_float, ctypes.c_float, c_i, c_i, c_i, ctypes.c_float, c_f, c_f, c_i, c_f, c_i,
                       c_f],
    'mmmot_associate_pairs': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_f, c_f],
    'mmmot_set_assign_variant': [c_i],
    'mmmot_associate_chains': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f, c_f],
    'mmmot_set_chain_variant': [c_i],
    # det, new, end, link, seqs, nts, B, n_nts, max_T, max_n, max_L, n_scores, n_link, out, n_out, ids, objective, info, ws,
    # ws_units, stream
    'mmmot_associate_sequences': [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_longlong, c_f,
                                  ctypes.c_longlong, c_f, c_f, c_f, c_f, ctypes.c_longlong, c_f],
    'mmmot_set_sequence_variant': [c_i],
    # det, new, end, link, seqs, nts, B, n_nts, max_T, max_n, max_L, max_gap, n_scores, n_link, out, n_out, ids, objective,
    # info, ws, ws_units, stream
    'mmmot_associate_sequences_gap': [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_longlong,
                                      c_f, ctypes.c_longlong, c_f, c_f, c_f, c_f, ctypes.c_longlong, c_f],
    'mmmot_set_sequence_gap_variant': [c_i],
    'mmmot_track_ids': [c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_f],
    # blocks, chains, out_off, frame_idx, B, max_n, state, ids_out, stream
    'mmmot_track_chain_ids': [c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_f],
    # blocks, pairs | chains, out_off, frame_idx, seq_start, S, B, max_n, states, ids_out, stream
    'mmmot_track_ids_multi': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f],
    'mmmot_track_chain_ids_multi': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f],
    'mmmot_clear_mot': [c_f, c_i, c_i, c_i, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_f, c_i, ctypes.c_double, ctypes.c_double,
                        ctypes.c_double, ctypes.c_double, c_f, c_f, c_f, c_f, c_f, c_f, c_f],
    # boxes, nG, nT, nD, frames, NF, frame_seq, g_attr, t_id, seq_tab, S, cells, sumG, sumT, max_boxes, max_dontcare,
    # min_height, max_truncation, max_occlusion, prepare, work, work_bytes, frame_d, frame_i, seq_d, seq_i, stream
    'mmmot_hota': [c_f, c_i, c_i, c_i, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_double,
                   ctypes.c_double, ctypes.c_double, c_i, c_f, ctypes.c_longlong, c_f, c_f, c_f, c_f, c_f],
    # boxes, box3d, sigma, nG, nT, nD, frames, cell_off, NF, g_attr, t_attr, traj_off, traj_obj, NTr, seq_off, S, mode,
    # levels, phase, gate, min_height, max_truncation, max_occlusion, table, cells, msig, frame_d, frame_i, gt_out,
    # traj_i, seq_d, seq_i, thr, reach, stream
    'mmmot_mot3d': [c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i,
                    ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_f, ctypes.c_longlong, c_f, c_f,
                    c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f],
    # ids, cls, chains, B, max_n, max_L, out, out_off, stream
    'mmmot_generate_gt': [c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f],
    # det_xywh, gt_xywh, gt_id, gt_name, frames, NF, car_code, dontcare_code, max_iou, max_n, det_id, det_cls, stream
    'mmmot_match_dets': [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, ctypes.c_double, c_i, c_f, c_f, c_f],
    # table, n_tensors, chunks, n_chunks, beta1, beta2, eps, stream
    'mmmot_adam_step': [c_f, c_i, c_f, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_f],
    'mmmot_adam_chunk_elems': [],
    # h_numel, n_tensors, h_chunks, cap, h_count  (host pointers)
    'mmmot_adam_chunks': [c_f, c_i, c_f, ctypes.c_longlong, c_f],
    # X, ldx, C, seg_start, seg_count, seg_group, nseg, sc, sh, ldsc, seed, threshold, scale, out, ldo, stream
    'mmmot_segment_mean_dropout': [c_f, c_i, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_i, ctypes.c_ulonglong, ctypes.c_uint,
                                   ctypes.c_float, c_f, c_i, c_f],
    # S, lds, rowidx, scale, X, ldx, R, C, seed, threshold, dscale, stream
    'mmmot_rows_gather_scale_dropout': [c_f, c_i, c_f, c_f, c_f, c_i, ctypes.c_long, c_i, ctypes.c_ulonglong, ctypes.c_uint,
                                        ctypes.c_float, c_f],
    # seed, threshold, R, C, out, stream
    'mmmot_dropout_mask': [ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_long, c_i, c_f, c_f],
}


# entry points that exist only in -DMMMOT_DEBUG builds (timing experiments of tools/; never the product library)
DEBUG_SIGNATURES = {
    'mmmot_set_patch_variant': [c_i],
    'mmmot_debug_read_patch_timers': [ctypes.POINTER(ctypes.c_ulonglong), c_i],
}
DEBUG_LIB_PATH = os.path.join(_HERE, 'libmmmot_hip_debug.so')


def build(force=False, verbose=False, debug=False):
    """Compile every HIP source for gfx950 and link libmmmot_hip.so in-tree.  ``debug=True`` builds the
    -DMMMOT_DEBUG variant (timing experiments of the patch kernel) as libmmmot_hip_debug.so; load it by setting
    MMMOT_LIB_PATH before importing mmmot_amd (tools/ do)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    # headers and the textual parts of the trunk kernel (csrc/patch_*.inc): any of them newer than the library rebuilds it
    deps = srcs + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(('.h', '.inc'))] + \
        [os.path.join(_HERE, '..', 'include', 'mmmot_hip.h')]
    lib_path = DEBUG_LIB_PATH if debug else LIB_PATH
    if not force and os.path.exists(lib_path):
        if all(os.path.getmtime(lib_path) >= os.path.getmtime(d) for d in deps):
            return lib_path
    objs = []
    procs = []
    for s in srcs:
        o = s[:-4] + ('.dbg.o' if debug else '.o')
        objs.append(o)
        cmd = [HIPCC] + HIPFLAGS + (['-DMMMOT_DEBUG'] if debug else []) + ['-c', s, '-o', o]
        if verbose:
            print(' '.join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError('hipcc failed: %s\n%s' % (' '.join(cmd), out.decode()))
    cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib_path] + objs
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    return lib_path


def load():
    """Return the ctypes handle; raises (never falls back) when unavailable."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    'libmmmot_hip.so is not built (%s). Run `python -c "import __graft_entry__ as g; '
                    'g.build()"`. There is no CPU fallback for the HIP path.' % LIB_PATH)
            lib = ctypes.CDLL(LIB_PATH)
            # MMMOT_LIB_ALLOW_MISSING=1 (tools/ab_forward.py only: an OLDER build of the library beside the current one)
            # tolerates entry points the other build does not have yet; the product never sets it
            lenient = os.environ.get('MMMOT_LIB_ALLOW_MISSING', '0') == '1'
            for name, argtypes in SIGNATURES.items():
                fn = getattr(lib, name, None) if lenient else getattr(lib, name)  # AttributeError if the symbol is missing
                if fn is None:
                    continue
                fn.argtypes = argtypes
                fn.restype = c_i
            for name, argtypes in DEBUG_SIGNATURES.items():  # present in -DMMMOT_DEBUG builds only
                fn = getattr(lib, name, None)
                if fn is not None:
                    fn.argtypes = argtypes
                    fn.restype = c_i
            _lib = lib
    return _lib


def check(status, what):
    if status != 0:
        raise RuntimeError('%s failed with status %d%s' % (
            what, status, ' (MMMOT_EINVAL: contract violation)' if status == -1 else ' (hipError_t)'))
