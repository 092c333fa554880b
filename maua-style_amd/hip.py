"""ctypes binding of libmaua_hip.so (declared in include/maua_hip.h).

There is NO fallback: if the library cannot be loaded, or a kernel reports an error, a
`HipError` is raised.  Tensors handed to the wrappers must be contiguous float32 ROCm
tensors; every call is enqueued on torch's current stream.
"""
import ctypes
import threading
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmaua_hip.so")

c_f = ctypes.c_float
c_i = ctypes.c_int
c_i64 = ctypes.c_int64
c_p = ctypes.c_void_p
c_sz = ctypes.c_size_t
c_u64 = ctypes.c_uint64

# name -> (restype, argtypes); mirrors include/maua_hip.h one to one
SIGNATURES = {
    "maua_abi_version": (c_i, []),
    "maua_last_error": (ctypes.c_char_p, []),
    "maua_conv_pack_filters": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "maua_conv_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv2d_fwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv2d_bwd_data": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz,
                                   c_p]),
    "maua_conv_x6_bank_bytes": (c_sz, [c_i, c_i]),
    "maua_conv_pack_filters_x6": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p]),
    "maua_conv_x6_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3_bank_bytes": (c_sz, [c_i, c_i]),
    "maua_conv_pack_filters_x3": (c_i, [c_p, c_p, c_p, c_i, c_i, c_f, c_p]),
    "maua_conv_x3w_bank_bytes": (c_sz, [c_i, c_i]),
    "maua_conv_pack_filters_x3w": (c_i, [c_p, c_p, c_p, c_i, c_i, c_f, c_p]),
    "maua_conv_x3w_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "maua_conv_x3w_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv3x3_x3w": (c_i, [c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv_kxk_x3_bank_bytes": (c_sz, [c_i, c_i, c_i]),
    "maua_conv_pack_filters_kxk_x3": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p]),
    "maua_conv_kxk_x3_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_kxk_x3": (c_i, [c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv1x1_x3_workspace_bytes": (c_sz, [c_i, c_i, c_i64, c_i]),
    "maua_conv1x1_x3": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv_x3_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv3x3_x3": (c_i, [c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv3x3_x6": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv_image_bank_bytes": (c_sz, [c_i, c_i]),
    "maua_conv_pack_filters_image": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p]),
    "maua_conv3x3_image": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_conv_image_gram_slabs": (c_i, [c_i, c_i, c_i]),
    "maua_conv_image_supported": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv3x3_image_gram": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "maua_relu_fwd": (c_i, [c_p, c_i64, c_p]),
    "maua_relu_bwd": (c_i, [c_p, c_p, c_p, c_i64, c_p]),
    "maua_pool_out_size": (c_i, [c_i, c_i, c_i, c_i]),
    "maua_pool2d_fwd": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_pool2d_bwd": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_pool2x2_codes_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "maua_pool2x2_fwd_codes": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "maua_pool2x2_bwd_codes": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_gram_workspace_bytes": (c_sz, [c_i, c_i64]),
    "maua_gram_block": (c_i, [c_i, c_i64]),
    "maua_gram_fwd": (c_i, [c_p, c_p, c_p, c_i, c_i64, c_f, c_i, c_p, c_sz, c_p]),
    "maua_reduce_workspace_bytes": (c_sz, [c_i64]),
    "maua_mse_fwd_bwd": (c_i, [c_p, c_p, c_p, c_i64, c_f, c_f, c_i, c_i, c_p, c_p, c_sz, c_p]),
    "maua_mse_weighted_fwd_bwd": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i64, c_i, c_f, c_f, c_i, c_p, c_p, c_sz, c_p]),
    "maua_gram_bwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_p, c_sz, c_p]),
    "maua_gram_guided_supported": (c_i, [c_i, c_i, c_i64]),
    "maua_gram_guided_workspace_bytes": (c_sz, [c_i, c_i, c_i64]),
    "maua_gram_guided_mass": (c_i, [c_p, c_p, c_i, c_i64, c_p]),
    "maua_gram_guided_fwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_p, c_sz, c_p]),
    "maua_gram_guided_bwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_p]),
    "maua_gram_shift_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "maua_gram_shift_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "maua_gram_shift_fwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_gram_shift_bwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_gram_flip_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "maua_gram_flip_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "maua_gram_flip_fwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_gram_flip_bwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_feat_hist_supported": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "maua_feat_hist_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "maua_feat_hist_state_bytes": (c_sz, [c_i, c_i]),
    "maua_feat_hist_fwd": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_feat_hist_bwd": (c_i, [c_p, c_p, c_p, c_p, ctypes.c_double, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_mrf_supported": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_mrf_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_mrf_state_bytes": (c_sz, [c_i, c_i]),
    "maua_mrf_bank": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "maua_mrf_fwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_mrf_bwd": (c_i, [c_p, c_p, c_p, c_p, c_p, ctypes.c_double, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_swd_supported": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_swd_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_swd_state_bytes": (c_sz, [c_i, c_i]),
    "maua_swd_project": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_swd_match": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_swd_bwd": (c_i, [c_p, c_p, c_p, ctypes.c_double, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_guided_gram_mse_ledger_supported": (c_i, [c_i, c_i]),
    "maua_guided_gram_fwd_mse_ledger": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_sz, c_p]),
    "maua_guided_gram_bwd_masked": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_p]),
    "maua_shift_gram_mse_ledger_supported": (c_i, [c_i, c_i]),
    "maua_shift_gram_fwd_mse_ledger": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_sz, c_p]),
    "maua_shift_gram_bwd_masked": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_flip_gram_mse_ledger_supported": (c_i, [c_i, c_i]),
    "maua_flip_gram_fwd_mse_ledger": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_sz, c_p]),
    "maua_flip_gram_bwd_masked": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_tv_fwd_bwd": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_p, c_p, c_sz, c_p]),
    "maua_fill": (c_i, [c_p, c_i64, c_f, c_p]),
    "maua_depth_to_space": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_conv_few_mfma_bank_bytes": (c_sz, []),
    "maua_conv_pack_filters_few_mfma": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "maua_conv_few_mfma_supported": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv3x3_few_mfma": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_space_to_depth": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_axpy": (c_i, [c_p, c_p, c_f, c_i64, c_p]),
    "maua_sum_small": (c_i, [c_p, c_i, c_p, c_p]),
    "maua_adam_step": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i, c_f, c_f, c_f, c_f, c_p]),
    "maua_channel_stats_workspace_bytes": (c_sz, [c_i, c_i]),
    "maua_channel_stats": (c_i, [c_p, c_p, c_f, c_i, c_i, c_i, c_i, c_p, c_p, c_sz, c_p]),
    "maua_color_match_solve": (c_i, [c_p, c_i, c_i64, c_p, c_i64, c_f, c_p, c_p]),
    "maua_color_match_apply": (c_i, [c_p, c_p, c_f, c_p, c_p, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "maua_resize_bilinear": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "maua_deprocess_u8": (c_i, [c_p, c_p, c_i, c_i, c_f, c_f, c_f, c_p]),
    "maua_flow_warp_grid_workspace_bytes": (c_sz, [c_i, c_i]),
    "maua_flow_warp_grid": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_grid_sample_border": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, ctypes.c_double, c_p, c_p]),
    "maua_mask_u8_resize": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "maua_gauss_wrap_supported": (c_i, [c_i, c_i, c_i, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "maua_gauss_wrap_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "maua_gauss_wrap": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i, c_p, c_sz, c_p]),
    "maua_set_tuning": (c_i, [ctypes.c_char_p, ctypes.c_double]),
    "maua_get_tuning": (ctypes.c_double, [ctypes.c_char_p, ctypes.c_double]),
    "maua_set_split_batch_hint": (None, [c_i]),
    "maua_conv_arm_workspace": (c_i, [c_p, c_p, c_sz, c_i, c_p]),
    "maua_get_split_batch_hint": (c_i, []),
    "maua_conv_x3w_split": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3q_bank_bytes": (c_sz, [c_i, c_i]),
    "maua_conv_pack_filters_x3q": (c_i, [c_p, c_p, c_p, c_i, c_i, c_f, c_p]),
    "maua_conv_x3q_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "maua_conv_x3q_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3q_split": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3q_preferred": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv3x3_x3q": (c_i, [c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv3x3_x3q_relu_pool": (c_i, [c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv3x3_x3q_unpool": (c_i, [c_p, c_p, c_i, c_p, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv_x3p_supported": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3p_split": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3p_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3p_preferred": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "maua_conv_x3p_set_max_groups": (c_i, [c_i]),
    "maua_conv3x3_x3p": (c_i, [c_p, c_p, c_i, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv3x3_x3w_relu_pool": (c_i, [c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv_x3w_dmat_bank_bytes": (c_sz, [c_i]),
    "maua_conv_pack_dmat_x3w": (c_i, [c_p, c_i, c_p, c_p, c_p]),
    "maua_conv_pack_dmat_x3w_batch": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p]),
    "maua_conv3x3_x3w_gram": (c_i, [c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_conv3x3_x3w_unpool": (c_i, [c_p, c_p, c_i, c_p, c_f, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_loss_ledger_bytes": (c_sz, [c_i, c_i]),
    "maua_mse_fwd_bwd_ledger": (c_i, [c_p, c_p, c_p, c_i64, c_f, c_f, c_i, c_i, c_p, c_i, c_p]),
    "maua_tv_fwd_bwd_ledger": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_p, c_i, c_p]),
    "maua_gram_mse_ledger_supported": (c_i, [c_i]),
    "maua_gram_fwd_mse_ledger": (c_i, [c_p, c_p, c_p, c_i, c_i64, c_f, c_i, c_p, c_p, c_f, c_f, c_p, c_i, c_p, c_sz, c_p]),
    "maua_gram_partial": (c_i, [c_p, c_p, c_i, c_i64, c_i, c_p, c_sz, c_p]),
    "maua_gram_finish_mse_batch": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "maua_gram_partial_batch": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "maua_gram_row_means": (c_i, [c_p, c_p, c_i, c_i64, c_p, c_sz, c_p]),
    "maua_loss_ledger_sum": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p]),
    "maua_loss_ledger_sum_f64": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p]),
    "maua_lbfgs_state_bytes": (c_sz, [c_i64, c_i]),
    "maua_lbfgs_init": (c_i, [c_p, c_sz, c_i64, c_i, c_p]),
    "maua_lbfgs_iterate": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i, c_f, c_f, c_f, c_p]),
    "maua_lbfgs_status": (c_i, [c_p, c_i64, c_i, c_p, c_p]),
    "maua_flow_levels": (c_i, [c_i, c_i, c_i]),
    "maua_flow_grey_u8": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "maua_flow_pyr_down": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "maua_flow_warp_prep": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_p]),
    "maua_flow_tvl1_step": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p]),
    "maua_flow_tvl1_blocked": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "maua_flow_median5": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p]),
    "maua_flow_upsample": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_f, c_p]),
    "maua_flow_consistency_workspace_bytes": (c_sz, [c_i, c_i]),
    "maua_flow_consistency": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "maua_flow_tvl1_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "maua_flow_tvl1": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "maua_nca_supported": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "maua_nca_param_count": (c_i64, [c_i, c_i]),
    "maua_nca_step": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_u64, c_i64, c_p]),
    "maua_nca_bwd_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "maua_nca_step_bwd": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_u64, c_i64, c_i, c_p, c_sz, c_p]),
    "maua_nca_grad_finish": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_i, c_p]),
}


class HipError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libmaua_hip.so once; raise HipError when it is missing (no CPU path exists)."""
    global _lib, LIB_PATH
    if _lib is None:
        LIB_PATH = os.environ.get("MAUA_HIP_LIB", LIB_PATH)  # developer knob: A/B another build of the same library
        if not os.path.exists(LIB_PATH):
            raise HipError(
                f"{LIB_PATH} not found: build it with `python maua-style_amd/build_native.py` "
                "(this package has no CPU or PyTorch fallback)")
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise HipError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the .so is stale: also loud
            fn.restype = res
            fn.argtypes = args
        _lib = L
        here = os.path.dirname(os.path.abspath(__file__))
        if here not in sys.path:  # (tools that load this module by path: the planner configuration lives beside it)
            sys.path.insert(0, here)
        import plan
        plan.forward_to_library(L)  # the library's share of the planner configuration (it never reads the environment)
        plan.warn_ignored()         # MAUA_* variables nothing reads any more: said once, loudly
    return _lib


def apply_plan():
    """Hand the planner configuration's library fields to the library again (after a programmatic change of plan.OVERRIDES)."""
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import plan
    plan.forward_to_library(lib())


def _check(rc, what):
    if rc != 0:
        msg = lib().maua_last_error().decode(errors="replace")
        raise HipError(f"{what} failed (rc={rc}): {msg}")


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError("libmaua_hip needs ROCm device tensors (got a CPU tensor): there is no CPU path")
    if t.dtype != torch.float32 and t.dtype != torch.uint8 and t.dtype != torch.float64:
        raise HipError(f"unsupported dtype {t.dtype}")
    if not t.is_contiguous():
        raise HipError("tensor must be contiguous")
    return t.data_ptr()


def _stream():
    """hipStream_t of torch's current stream on the current device.  The raw getters are ~20x cheaper than building a
    torch.cuda.Stream object per launch (19 us, which made eager iterations at 512x512 CPU-bound)."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:  # private API moved: the public, slower spelling
        return torch.cuda.current_stream().cuda_stream


def _f32(t, name):
    if t is not None and t.dtype != torch.float32:
        raise HipError(f"{name}: expected float32, got {t.dtype}")
    return t


# ------------------------------------------------------------------------------------------
# thin, shape-aware wrappers
# ------------------------------------------------------------------------------------------
def conv_pack_filters(w):
    """OIHW weights -> (forward bank [taps][cin][cout], backward bank [taps][cout][cin])."""
    cout, cin, kh, kw = w.shape
    wf = torch.empty(kh * kw, cin, cout, device=w.device, dtype=torch.float32)
    wb = torch.empty(kh * kw, cout, cin, device=w.device, dtype=torch.float32)
    _check(lib().maua_conv_pack_filters(_ptr(_f32(w, "w")), _ptr(wf), _ptr(wb), cout, cin, kh, kw, _stream()),
           "maua_conv_pack_filters")
    return wf, wb


def conv_out_hw(h, w, k, stride, pad):
    if stride <= 0 or k <= 0 or pad < 0:
        raise HipError(f"conv geometry k={k} stride={stride} pad={pad} is invalid")
    if h + 2 * pad < k or w + 2 * pad < k:
        raise HipError(f"conv input {h}x{w} (pad {pad}) smaller than the {k}x{k} filter")
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv_workspace_bytes(n, cin, h, w, cout, k, stride, pad):
    return lib().maua_conv_workspace_bytes(n, cin, h, w, cout, k, k, stride, pad)


def _ws_args(workspace, need, device):
    """(pointer, bytes) of a split-K workspace: the caller's when given, a fresh one when the geometry wants one."""
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    if workspace is None:
        return None, 0
    return workspace.data_ptr(), workspace.numel() * workspace.element_size()


def conv2d_fwd(x, wf, bias, k, stride, pad, relu, out=None, in_mask=None, accumulate=False, workspace=None):
    n, cin, h, w = x.shape
    cout = wf.shape[2]
    oh, ow = conv_out_hw(h, w, k, stride, pad)
    if out is None:
        out = torch.empty(n, cout, oh, ow, device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_workspace_bytes(n, cin, h, w, cout, k, stride, pad) if workspace is None else 0, x.device)
    _check(lib().maua_conv2d_fwd(_ptr(_f32(x, "x")), _ptr(in_mask), _ptr(wf), _ptr(bias), _ptr(out), n, cin, h, w, cout,
                                 k, k, stride, pad, int(relu), int(accumulate), wp, wn, _stream()), "maua_conv2d_fwd")
    return out


def conv2d_bwd_data(gy, out_mask, wb, w_oihw, in_shape, k, stride, pad, out=None, accumulate=False, in_relu_mask=None,
                    workspace=None):
    n, cin, h, w = in_shape
    cout = gy.shape[1]
    if out is None:
        out = torch.empty(n, cin, h, w, device=gy.device, dtype=torch.float32)
    need = 0
    if workspace is None and stride == 1 and k - 1 - pad >= 0:
        need = conv_workspace_bytes(n, cout, gy.shape[2], gy.shape[3], cin, k, 1, k - 1 - pad)
    wp, wn = _ws_args(workspace, need, gy.device)
    _check(lib().maua_conv2d_bwd_data(_ptr(_f32(gy, "gy")), _ptr(out_mask), _ptr(wb), _ptr(w_oihw), _ptr(in_relu_mask),
                                      _ptr(out), n, cin, h, w, cout, k, k, stride, pad, int(accumulate), wp, wn, _stream()),
           "maua_conv2d_bwd_data")
    return out


def conv_pack_filters_x6(w):
    """OIHW 3x3 weights -> (forward bank, backward-data bank) of pre-split bf16 triples (uint8 tensors)."""
    cout, cin, kh, kw = w.shape
    if kh != 3 or kw != 3:
        raise HipError("the bf16x6 path covers 3x3 filters")
    bf = torch.empty(lib().maua_conv_x6_bank_bytes(cout, cin), dtype=torch.uint8, device=w.device)
    bb = torch.empty(lib().maua_conv_x6_bank_bytes(cin, cout), dtype=torch.uint8, device=w.device)
    _check(lib().maua_conv_pack_filters_x6(_ptr(_f32(w, "w")), bf.data_ptr(), bb.data_ptr(), cout, cin, _stream()),
           "maua_conv_pack_filters_x6")
    return bf, bb


def _pack_filters_fp16x3(family, w, *ks):
    """(forward bank, backward-data bank, w_scale) of an fp16x3 family: w_scale is the power of two that brings max|w| into [32, 64)
    (one host read of the maximum per weight version); `ks`: the filter size, for the family whose entry points take one."""
    import math
    cout, cin = w.shape[:2]
    m = float(w.abs().max())
    w_scale = 2.0 ** (5 - math.floor(math.log2(m))) if m > 0 and math.isfinite(m) else 1.0
    wc = _f32(w, "w").contiguous()
    bank_bytes = getattr(lib(), f"maua_conv_{family}_bank_bytes")
    bf = torch.empty(bank_bytes(cout, cin, *ks), dtype=torch.uint8, device=w.device)
    bb = torch.empty(bank_bytes(cin, cout, *ks), dtype=torch.uint8, device=w.device)
    _check(getattr(lib(), f"maua_conv_pack_filters_{family}")(_ptr(wc), bf.data_ptr(), bb.data_ptr(), cout, cin, *ks, w_scale, _stream()),
           f"maua_conv_pack_filters_{family}")
    return bf, bb, w_scale


def conv_pack_filters_x3(w):
    """OIHW 3x3 weights -> (forward bank, backward-data bank, w_scale) of pre-split, pre-scaled fp16 pairs.  w_scale is the
    power of two that brings max|w| into [32, 64) (one host read of the maximum per weight version)."""
    return _pack_filters_fp16x3("x3", w)


def conv_x3_workspace_bytes(n, cin, h, w, cout, pad):
    return lib().maua_conv_x3_workspace_bytes(n, cin, h, w, cout, pad)


def conv3x3_x3(x, bank, w_scale, bias, cout, pad, relu, out=None, out_relu_mask=None, accumulate=False, workspace=None):
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_x3_workspace_bytes(n, cin, h, w, cout, pad) if workspace is None else 0, x.device)
    _check(lib().maua_conv3x3_x3(_ptr(_f32(x, "x")), bank.data_ptr(), float(w_scale), _ptr(bias), _ptr(out_relu_mask), _ptr(out), n,
                                 cin, h, w, cout, pad, int(relu), int(accumulate), wp, wn, _stream()), "maua_conv3x3_x3")
    return out


def conv_pack_filters_x3w(w):
    """OIHW 3x3 weights -> (forward bank, backward-data bank, w_scale) for conv_x3w.hip (16-channel chunks; same split and
    the same power-of-two filter scale as conv_pack_filters_x3)."""
    return _pack_filters_fp16x3("x3w", w)


def conv_x3w_supported(cin, h, w, pad):
    return bool(lib().maua_conv_x3w_supported(int(cin), int(h), int(w), int(pad)))


def conv_x3w_workspace_bytes(n, cin, h, w, cout, pad):
    return lib().maua_conv_x3w_workspace_bytes(n, cin, h, w, cout, pad)


def conv3x3_x3w(x, bank, w_scale, bias, cout, pad, relu, out=None, out_relu_mask=None, accumulate=False, workspace=None):
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_x3w_workspace_bytes(n, cin, h, w, cout, pad) if workspace is None else 0, x.device)
    _check(lib().maua_conv3x3_x3w(_ptr(_f32(x, "x")), bank.data_ptr(), float(w_scale), _ptr(bias), _ptr(out_relu_mask), _ptr(out), n,
                                  cin, h, w, cout, pad, int(relu), int(accumulate), wp, wn, _stream()), "maua_conv3x3_x3w")
    return out


def conv_pack_filters_x3q(w):
    """OIHW 3x3 weights -> (forward bank, backward-data bank, w_scale) for conv_x3q.hip (32-channel chunks; same split and
    the same power-of-two filter scale as conv_pack_filters_x3)."""
    return _pack_filters_fp16x3("x3q", w)


def conv_x3q_supported(cin, h, w, pad):
    return bool(lib().maua_conv_x3q_supported(int(cin), int(h), int(w), int(pad)))


def conv_x3q_workspace_bytes(n, cin, h, w, cout, pad):
    return lib().maua_conv_x3q_workspace_bytes(n, cin, h, w, cout, pad)


def conv_x3q_preferred(n, cin, h, w, cout, pad):
    return bool(lib().maua_conv_x3q_preferred(int(n), int(cin), int(h), int(w), int(cout), int(pad)))


def conv_x3q_split(n, cin, h, w, cout, pad):
    return int(lib().maua_conv_x3q_split(int(n), int(cin), int(h), int(w), int(cout), int(pad)))


def conv3x3_x3q(x, bank, w_scale, bias, cout, pad, relu, out=None, out_relu_mask=None, accumulate=False, workspace=None):
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_x3q_workspace_bytes(n, cin, h, w, cout, pad) if workspace is None else 0, x.device)
    _check(lib().maua_conv3x3_x3q(_ptr(_f32(x, "x")), bank.data_ptr(), float(w_scale), _ptr(bias), _ptr(out_relu_mask), _ptr(out), n,
                                  cin, h, w, cout, pad, int(relu), int(accumulate), wp, wn, _stream()), "maua_conv3x3_x3q")
    return out


def _unpooled_hw(ph, pw, pad, out):
    """Extent of the plane a 2x2 / 2 floor-mode max pool reduced to ph x pw: taken from the output the caller provides (the plane may be
    odd: 181 -> 90), 2 ph x 2 pw without one."""
    if out is None:
        return 2 * ph, 2 * pw
    h, w = out.shape[2] - 2 * pad + 2, out.shape[3] - 2 * pad + 2
    if h // 2 != ph or w // 2 != pw:
        raise ValueError(f"unpool: a {ph}x{pw} pooled map does not come from a {h}x{w} plane")
    return h, w


def conv3x3_x3q_relu_pool(x, bank, w_scale, bias, cout, pad, pooled, codes, workspace=None):
    """conv + bias + ReLU + 2x2 / 2 max pool on conv_x3q.hip: writes `pooled` and the pool's decision bytes only (conv3x3_x3w_relu_pool's
    contract)."""
    n, cin, h, w = x.shape
    wp, wn = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if workspace is not None else (None, 0)
    _check(lib().maua_conv3x3_x3q_relu_pool(_ptr(_f32(x, "x")), bank.data_ptr(), float(w_scale), _ptr(bias), _ptr(pooled),
                                            codes.data_ptr(), n, cin, h, w, cout, pad, wp, wn, _stream()), "maua_conv3x3_x3q_relu_pool")
    return pooled


def conv3x3_x3q_unpool(pooled_x, codes, honour_relu_bit, bank, w_scale, cout, pad, out=None, out_relu_mask=None, workspace=None):
    """Backward-data pass on conv_x3q.hip staged straight from the pooled map's gradient and the pool's decision bytes
    (conv3x3_x3w_unpool's contract, without the Gram term)."""
    n, cin, hp, wp_ = pooled_x.shape
    h, w = _unpooled_hw(hp, wp_, pad, out)
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=pooled_x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_x3q_workspace_bytes(n, cin, h, w, cout, pad) if workspace is None else 0, pooled_x.device)
    _check(lib().maua_conv3x3_x3q_unpool(_ptr(_f32(pooled_x, "pooled_x")), codes.data_ptr(), int(bool(honour_relu_bit)), bank.data_ptr(),
                                         float(w_scale), _ptr(out_relu_mask) if out_relu_mask is not None else None, _ptr(out), n, cin, h, w,
                                         cout, pad, wp, wn, _stream()), "maua_conv3x3_x3q_unpool")
    return out


def conv_x3p_supported(cin, h, w, cout, pad):
    return bool(lib().maua_conv_x3p_supported(int(cin), int(h), int(w), int(cout), int(pad)))


def conv_x3p_split(n, cin, h, w, cout, pad):
    return int(lib().maua_conv_x3p_split(int(n), int(cin), int(h), int(w), int(cout), int(pad)))


def conv_x3p_preferred(n, cin, h, w, cout, pad):
    return bool(lib().maua_conv_x3p_preferred(int(n), int(cin), int(h), int(w), int(cout), int(pad)))


def conv_x3p_set_max_groups(groups):
    """Tests: workgroups a conv_x3p launch may use (multiple of 8; 0 = no override: one per CU / the planner's x3p_groups); returns the
    previous override (0 = none), so passing it back restores the state exactly."""
    return int(lib().maua_conv_x3p_set_max_groups(int(groups)))


def conv_x3p_workspace_bytes(n, cin, h, w, cout, pad):
    return lib().maua_conv_x3p_workspace_bytes(n, cin, h, w, cout, pad)


def conv3x3_x3p(x, bank, w_scale, bias, cout, pad, relu, out=None, out_relu_mask=None, workspace=None, in_codes=None, honour_relu_bit=True,
                dmat_bank=None, dmat_inv_scale=None, pool_codes=None):
    """The persistent fp16x3 3x3 kernel (conv_x3p.hip) in any of its forms: plain / masked, staged from a pooled gradient (`in_codes`: x is
    the pooled map's gradient, `out` fixes the full-size plane), with the Gram backward along (`dmat_bank`, out_relu_mask = F), or with ReLU
    + 2x2 max pool in the epilogue (`pool_codes`: out = the pooled map).  Banks: conv_pack_filters_x3q's."""
    n, cin = x.shape[0], x.shape[1]
    if in_codes is not None:
        h, w = _unpooled_hw(x.shape[2], x.shape[3], pad, out)
    else:
        h, w = x.shape[2], x.shape[3]
    oh, ow = h + 2 * pad - 2, w + 2 * pad - 2
    if out is None:
        out = torch.empty((n, cout, oh // 2, ow // 2) if pool_codes is not None else (n, cout, oh, ow), device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_x3p_workspace_bytes(n, cin, h, w, cout, pad) if workspace is None else 0, x.device)
    _check(lib().maua_conv3x3_x3p(_ptr(_f32(x, "x")), in_codes.data_ptr() if in_codes is not None else None, int(bool(honour_relu_bit)),
                                  bank.data_ptr(), float(w_scale), _ptr(bias), _ptr(out_relu_mask) if out_relu_mask is not None else None,
                                  dmat_bank.data_ptr() if dmat_bank is not None else None,
                                  _ptr(dmat_inv_scale) if dmat_inv_scale is not None else None, _ptr(out),
                                  pool_codes.data_ptr() if pool_codes is not None else None, n, cin, h, w, cout, pad, int(relu), wp, wn,
                                  _stream()), "maua_conv3x3_x3p")
    return out


def conv_x3w_split(n, cin, h, w, cout, pad):
    """Channel-loop splits conv3x3_x3w would use for this geometry under the current batch hint (1 = one pass)."""
    return int(lib().maua_conv_x3w_split(int(n), int(cin), int(h), int(w), int(cout), int(pad)))


def conv3x3_x3w_relu_pool(x, bank, w_scale, bias, cout, pad, pooled, codes, workspace=None):
    """conv + bias + ReLU + 2x2 / 2 max pool: writes `pooled` and the pool's decision bytes only.  One launch without a workspace (one
    pass over the channels); with one, small grids split the channel loop and the pass that adds the slabs applies ReLU and pool."""
    n, cin, h, w = x.shape
    wp, wn = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if workspace is not None else (None, 0)
    _check(lib().maua_conv3x3_x3w_relu_pool(_ptr(_f32(x, "x")), bank.data_ptr(), float(w_scale), _ptr(bias), _ptr(pooled),
                                            codes.data_ptr(), n, cin, h, w, cout, pad, wp, wn, _stream()), "maua_conv3x3_x3w_relu_pool")
    return pooled


def conv_x3w_dmat_bank(c, device, frames=1):
    """(banks (frames, bytes), inverse scales (frames,)) for conv_pack_dmat_x3w / conv3x3_x3w_gram; None when c is not a multiple
    of 16."""
    nbytes = lib().maua_conv_x3w_dmat_bank_bytes(int(c))
    if nbytes == 0:
        return None
    return torch.empty(frames, nbytes, dtype=torch.uint8, device=device), torch.ones(frames, dtype=torch.float32, device=device)


def conv_pack_dmat_x3w(dmat, bank, inv_scale):
    c = dmat.shape[0]
    _check(lib().maua_conv_pack_dmat_x3w(_ptr(_f32(dmat, "dmat")), c, bank.data_ptr(), _ptr(inv_scale), _stream()),
           "maua_conv_pack_dmat_x3w")


class DmatPackBatch:
    """conv_pack_dmat_x3w for up to four layers in one launch; the argument arrays are built once per engine plan."""

    def __init__(self, items):
        """items: list of (dmat (C, C), bank, inv_scale) as for conv_pack_dmat_x3w"""
        n = len(items)
        self.n, self.keep = n, items
        self.args = ((ctypes.c_void_p * n)(*[_ptr(_f32(d, "dmat")) for d, _, _ in items]), (ctypes.c_int * n)(*[int(d.shape[0]) for d, _, _ in items]),
                     (ctypes.c_void_p * n)(*[b.data_ptr() for _, b, _ in items]), (ctypes.c_void_p * n)(*[_ptr(i) for _, _, i in items]))

    def run(self):
        a = self.args
        _check(lib().maua_conv_pack_dmat_x3w_batch(self.n, a[0], a[1], a[2], a[3], _stream()), "maua_conv_pack_dmat_x3w_batch")


def conv3x3_x3w_gram(x, bank, w_scale, feature_map, dmat_bank, dmat_inv_scale, cout, pad, out=None, accumulate=False,
                     workspace=None):
    """Backward-data pass + Gram backward in one launch: out = [F > 0] * (conv(x) + D . F)."""
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_x3w_workspace_bytes(n, cin, h, w, cout, pad) if workspace is None else 0, x.device)
    _check(lib().maua_conv3x3_x3w_gram(_ptr(_f32(x, "x")), bank.data_ptr(), float(w_scale), _ptr(_f32(feature_map, "feature_map")),
                                       dmat_bank.data_ptr(), _ptr(dmat_inv_scale), _ptr(out), n, cin, h, w, cout, pad,
                                       int(accumulate), wp, wn, _stream()), "maua_conv3x3_x3w_gram")
    return out


def conv3x3_x3w_unpool(pooled_x, codes, honour_relu_bit, bank, w_scale, cout, pad, out=None, out_relu_mask=None, dmat_bank=None,
                       dmat_inv_scale=None, workspace=None):
    """Backward-data pass of a conv + ReLU + 2x2 max pool group straight from the POOLED gradient and the pool's decision bytes (the
    pool's backward pass happens while the kernel stages its input); with `dmat_bank`, the Gram backward of the style loss on the
    layer's input (out_relu_mask = F) goes along as in conv3x3_x3w_gram."""
    n, cin, ph, pw = pooled_x.shape
    h, w = _unpooled_hw(ph, pw, pad, out)
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=pooled_x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_x3w_workspace_bytes(n, cin, h, w, cout, pad) if workspace is None else 0, pooled_x.device)
    _check(lib().maua_conv3x3_x3w_unpool(_ptr(_f32(pooled_x, "pooled_x")), codes.data_ptr(), int(bool(honour_relu_bit)), bank.data_ptr(),
                                         float(w_scale), _ptr(out_relu_mask) if out_relu_mask is not None else None,
                                         dmat_bank.data_ptr() if dmat_bank is not None else None,
                                         _ptr(dmat_inv_scale) if dmat_inv_scale is not None else None, _ptr(out), n, cin, h, w, cout, pad,
                                         wp, wn, _stream()), "maua_conv3x3_x3w_unpool")
    return out


def conv_pack_filters_kxk_x3(w):
    """OIHW k x k weights -> (forward bank, backward-data bank, w_scale) of pre-split, pre-scaled fp16 pairs (as
    conv_pack_filters_x3, with k*k taps)."""
    return _pack_filters_fp16x3("kxk_x3", w, w.shape[2])


def conv_kxk_x3_workspace_bytes(n, cin, h, w, cout, ks, pad):
    return lib().maua_conv_kxk_x3_workspace_bytes(n, cin, h, w, cout, ks, pad)


def conv_kxk_x3(x, bank, w_scale, bias, cout, ks, pad, relu, out=None, out_relu_mask=None, accumulate=False, workspace=None):
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - ks + 1, w + 2 * pad - ks + 1, device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv_kxk_x3_workspace_bytes(n, cin, h, w, cout, ks, pad) if workspace is None else 0, x.device)
    _check(lib().maua_conv_kxk_x3(_ptr(_f32(x, "x")), bank.data_ptr(), float(w_scale), _ptr(bias), _ptr(out_relu_mask), _ptr(out), n,
                                  cin, h, w, cout, ks, pad, int(relu), int(accumulate), wp, wn, _stream()), "maua_conv_kxk_x3")
    return out


def conv1x1_x3_workspace_bytes(n, cin, hw, cout):
    return lib().maua_conv1x1_x3_workspace_bytes(n, cin, hw, cout)


def conv1x1_x3(x, w_rowmajor, bias=None, relu=False, out=None, out_relu_mask=None, accumulate=False, workspace=None,
               x_shift=None):
    """y[n][co][p] (+)= sum_ci w[co][ci] x[n][ci][p] in fp16x3 arithmetic; x is [n, cin, ...] (any trailing plane shape);
    x_shift ([cin], optional) is subtracted from x first."""
    n, cin = x.shape[:2]
    hw = x[0, 0].numel()
    cout = w_rowmajor.shape[0]
    assert w_rowmajor.numel() == cout * cin and w_rowmajor.is_contiguous()
    if out is None:
        out = torch.empty((n, cout) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    wp, wn = _ws_args(workspace, conv1x1_x3_workspace_bytes(n, cin, hw, cout) if workspace is None else 0, x.device)
    _check(lib().maua_conv1x1_x3(_ptr(_f32(x, "x")), _ptr(x_shift), _ptr(_f32(w_rowmajor, "w")), _ptr(bias), _ptr(out_relu_mask), _ptr(out), n, cin,
                                 hw, cout, int(relu), int(accumulate), wp, wn, _stream()), "maua_conv1x1_x3")
    return out


def conv_x6_workspace_bytes(n, cin, h, w, cout, pad):
    return lib().maua_conv_x6_workspace_bytes(n, cin, h, w, cout, pad)



def conv_pack_filters_image(w, bias=None):
    """OIHW 3x3 weights (and the bias) of a layer that consumes 1-3 channels -> the bank of conv3x3_image (bf16 triples in MFMA lane
    order; the bias as one more filter column)."""
    cout, cin = w.shape[:2]
    bank = torch.empty(lib().maua_conv_image_bank_bytes(cout, cin), dtype=torch.uint8, device=w.device)
    _check(lib().maua_conv_pack_filters_image(_ptr(_f32(w, "w").contiguous()), _ptr(bias), bank.data_ptr(), cout, cin, _stream()),
           "maua_conv_pack_filters_image")
    return bank


def conv3x3_image(x, bank, cout, pad, relu, out=None):
    """The image layer (1-3 input channels) in exact bf16x6 arithmetic, forward; the bias is part of the bank."""
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=x.device, dtype=torch.float32)
    _check(lib().maua_conv3x3_image(_ptr(_f32(x, "x")), bank.data_ptr(), _ptr(out), n, cin, h, w, cout, pad, int(relu), _stream()),
           "maua_conv3x3_image")
    return out


def conv_image_supported(n, cin, h, w, cout, pad):
    """Whether conv3x3_image takes this layer (1-3 channels, planes of fewer than 2^24 pixels: its offsets are 32-bit)."""
    return bool(lib().maua_conv_image_supported(int(n), int(cin), int(h), int(w), int(cout), int(pad)))


def conv_image_gram_slabs(h, w, pad):
    """Number of 64 x 64 slabs conv3x3_image_gram leaves for an h x w image."""
    return int(lib().maua_conv_image_gram_slabs(int(h), int(w), int(pad)))


def conv3x3_image_gram(x, bank, pad, out, gram_slabs):
    """conv3x3_image (one image, 64 channels, ReLU) that also leaves the partial Gram matrices of its output as split-K slabs in
    `gram_slabs` (a byte or float buffer of at least conv_image_gram_slabs(...) * 16 KiB)."""
    n, cin, h, w = x.shape
    assert n == 1 and gram_slabs.numel() * gram_slabs.element_size() >= conv_image_gram_slabs(h, w, pad) * 64 * 64 * 4
    _check(lib().maua_conv3x3_image_gram(_ptr(_f32(x, "x")), bank.data_ptr(), _ptr(out), gram_slabs.data_ptr(), cin, h, w, pad, _stream()),
           "maua_conv3x3_image_gram")
    return out


def conv3x3_x6(x, bank, bias, cout, pad, relu, out=None, out_relu_mask=None, accumulate=False, workspace=None):
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, device=x.device, dtype=torch.float32)
    if workspace is None:
        need = conv_x6_workspace_bytes(n, cin, h, w, cout, pad)
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    _check(lib().maua_conv3x3_x6(_ptr(_f32(x, "x")), bank.data_ptr(), _ptr(bias), _ptr(out_relu_mask), _ptr(out), n, cin, h,
                                 w, cout, pad, int(relu), int(accumulate),
                                 workspace.data_ptr() if workspace is not None else None,
                                 workspace.numel() * workspace.element_size() if workspace is not None else 0, _stream()),
           "maua_conv3x3_x6")
    return out


def relu_(x):
    _check(lib().maua_relu_fwd(_ptr(_f32(x, "x")), x.numel(), _stream()), "maua_relu_fwd")
    return x


def relu_bwd(gy, y, out=None):
    if out is None:
        out = torch.empty_like(gy)
    _check(lib().maua_relu_bwd(_ptr(gy), _ptr(y), _ptr(out), gy.numel(), _stream()), "maua_relu_bwd")
    return out


def pool_out_size(n, k, stride, ceil_mode):
    return lib().maua_pool_out_size(n, k, stride, int(ceil_mode))


def pool2d_fwd(x, k, stride, ceil_mode, mode, out=None):
    n, c, h, w = x.shape
    oh, ow = pool_out_size(h, k, stride, ceil_mode), pool_out_size(w, k, stride, ceil_mode)
    if out is None:
        out = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
    _check(lib().maua_pool2d_fwd(_ptr(_f32(x, "x")), _ptr(out), n, c, h, w, k, stride, int(ceil_mode),
                                 0 if mode == "max" else 1, _stream()), "maua_pool2d_fwd")
    return out


def pool2d_bwd(gy, x, k, stride, ceil_mode, mode, out=None, relu_mask_by_x=False):
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty_like(x)
    _check(lib().maua_pool2d_bwd(_ptr(_f32(gy, "gy")), _ptr(x), _ptr(out), n, c, h, w, k, stride, int(ceil_mode),
                                 0 if mode == "max" else 1, int(relu_mask_by_x), _stream()), "maua_pool2d_bwd")
    return out


def pool2x2_codes_supported(n, c, h, w):
    return bool(lib().maua_pool2x2_codes_supported(int(n), int(c), int(h), int(w)))


def pool2x2_fwd_codes(x, out, codes):
    """2x2/2 max pooling that also records each window's decision (one byte) for pool2x2_bwd_codes."""
    n, c, h, w = x.shape
    _check(lib().maua_pool2x2_fwd_codes(_ptr(_f32(x, "x")), _ptr(out), codes.data_ptr(), n, c, h, w, _stream()),
           "maua_pool2x2_fwd_codes")
    return out


def pool2x2_bwd_codes(gy, codes, out, relu_mask):
    n, c, h, w = out.shape
    _check(lib().maua_pool2x2_bwd_codes(_ptr(_f32(gy, "gy")), codes.data_ptr(), _ptr(out), n, c, h, w, int(relu_mask), _stream()),
           "maua_pool2x2_bwd_codes")
    return out


def gram_workspace_bytes(c, hw):
    return lib().maua_gram_workspace_bytes(c, hw)


def reduce_workspace_bytes(count):
    return lib().maua_reduce_workspace_bytes(count)


def _ws(workspace, need, device):
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
    return workspace


def gram_block(c, hw):
    """Edge of the blocks the Gram kernels multiply this shape in: 64, or 128 (MAUA_GRAM_T128=1, large layers)."""
    return int(lib().maua_gram_block(int(c), int(hw)))


def gram_fwd(f, scale, center=False, out=None, mean_out=None, workspace=None):
    """f: (1,C,H,W) or (C,HW).  Returns (gram CxC, row means or None)."""
    c = f.shape[1] if f.dim() == 4 else f.shape[0]
    hw = f.numel() // c
    if out is None:
        out = torch.empty(c, c, device=f.device, dtype=torch.float32)
    if center and mean_out is None:
        mean_out = torch.empty(c, device=f.device, dtype=torch.float32)
    need = gram_workspace_bytes(c, hw)
    workspace = _ws(workspace, need, f.device)
    _check(lib().maua_gram_fwd(_ptr(_f32(f, "f")), _ptr(out), _ptr(mean_out) if center else None, c, hw, float(scale),
                               int(center), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                               _stream()), "maua_gram_fwd")
    return out, (mean_out if center else None)


def loss_ledger(frames, slots, device):
    """Zero-filled ledger of frames x slots records for the *_ledger entry points (float64 tensor, frames x slots x stride)."""
    n = lib().maua_loss_ledger_bytes(int(frames), int(slots)) // 8
    return torch.zeros(frames, slots, n // (frames * slots), dtype=torch.float64, device=device)


def gram_mse_ledger_supported(c):
    return bool(lib().maua_gram_mse_ledger_supported(int(c)))


def gram_fwd_mse_ledger(f, scale, center, out, mean_out, target, dmat, loss_scale, grad_scale, ledger, slot, workspace=None):
    """gram_fwd + mse_fwd_bwd(gram, target -> dmat) with the loss left in record `slot` of `ledger` (one frame's records)."""
    c = f.shape[1] if f.dim() == 4 else f.shape[0]
    hw = f.numel() // c
    workspace = _ws(workspace, gram_workspace_bytes(c, hw), f.device)
    _check(lib().maua_gram_fwd_mse_ledger(_ptr(_f32(f, "f")), _ptr(out), _ptr(mean_out) if center else None, c, hw, float(scale),
                                          int(center), _ptr(_f32(target, "target")), _ptr(dmat), float(loss_scale),
                                          float(grad_scale), ledger.data_ptr(), int(slot), workspace.data_ptr(),
                                          workspace.numel() * workspace.element_size(), _stream()), "maua_gram_fwd_mse_ledger")
    return out


def gram_row_means(f, mean_out, workspace):
    """Row means of the covariance form into `mean_out` (the layer's workspace holds the fp64 partial sums meanwhile)."""
    c = f.shape[1] if f.dim() == 4 else f.shape[0]
    _check(lib().maua_gram_row_means(_ptr(_f32(f, "f")), _ptr(mean_out), c, f.numel() // c, workspace.data_ptr(),
                                     workspace.numel() * workspace.element_size(), _stream()), "maua_gram_row_means")


def gram_partial(f, center, mean_out, workspace):
    """First half of gram_fwd_mse_ledger: the split-K slabs of F F^T (and the row means) into the layer's own `workspace`."""
    c = f.shape[1] if f.dim() == 4 else f.shape[0]
    hw = f.numel() // c
    _check(lib().maua_gram_partial(_ptr(_f32(f, "f")), _ptr(mean_out) if center else None, c, hw, int(center), workspace.data_ptr(),
                                   workspace.numel() * workspace.element_size(), _stream()), "maua_gram_partial")


class GramFinishBatch:
    """Second half for up to eight layers in one launch.  The argument arrays are built once (device addresses and coefficients of a
    fixed engine plan) and reused by every evaluation."""

    def __init__(self, layers):
        """layers: list of dicts with workspace, gram, target, dmat, c, hw, scale, loss_scale, grad_scale, ledger (one frame's records), slot;
        optional: f (the feature map, for run_partial), mean (covariance form: the array run_partial leaves the row means in before it
        centres the product), slabs (> 0: that many slabs are in the workspace already, conv3x3_image_gram)."""
        n = len(layers)
        self.n = n
        self.keep = layers  # (the tensors must outlive the addresses)
        arr = lambda ct, vals: (ct * n)(*vals)
        self.args = (
            arr(ctypes.c_void_p, [l["workspace"].data_ptr() for l in layers]), arr(ctypes.c_void_p, [_ptr(l["gram"]) for l in layers]),
            arr(ctypes.c_void_p, [_ptr(_f32(l["target"], "target")) for l in layers]), arr(ctypes.c_void_p, [_ptr(l["dmat"]) for l in layers]),
            arr(ctypes.c_int, [int(l["c"]) for l in layers]), arr(ctypes.c_int64, [int(l["hw"]) for l in layers]),
            arr(ctypes.c_float, [float(l["scale"]) for l in layers]), arr(ctypes.c_float, [float(l["loss_scale"]) for l in layers]),
            arr(ctypes.c_float, [float(l["grad_scale"]) for l in layers]), arr(ctypes.c_void_p, [l["ledger"].data_ptr() for l in layers]),
            arr(ctypes.c_int, [int(l["slot"]) for l in layers]), arr(ctypes.c_int, [int(l.get("slabs") or 0) for l in layers]))

        self.partial_args = (
            arr(ctypes.c_void_p, [_ptr(_f32(l["f"], "f")) if l.get("f") is not None else None for l in layers]), self.args[4], self.args[5],
            self.args[0], arr(ctypes.c_size_t, [l["workspace"].numel() * l["workspace"].element_size() for l in layers]),
            arr(ctypes.c_void_p, [_ptr(l["mean"]) if l.get("mean") is not None else None for l in layers]))

    def run_partial(self):
        """maua_gram_partial of every layer (each dict's "f" = its feature map) in at most three launches."""
        a = self.partial_args
        _check(lib().maua_gram_partial_batch(self.n, a[0], a[5], a[1], a[2], a[3], a[4], self.args[11], _stream()), "maua_gram_partial_batch")

    def run(self):
        a = self.args
        _check(lib().maua_gram_finish_mse_batch(self.n, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], _stream()),
               "maua_gram_finish_mse_batch")


def mse_fwd_bwd_ledger(x, target, grad, loss_scale, grad_scale, accumulate, ledger, slot, mask_grad_by_x=False):
    _check(lib().maua_mse_fwd_bwd_ledger(_ptr(_f32(x, "x")), _ptr(_f32(target, "target")), _ptr(grad), x.numel(), float(loss_scale),
                                         float(grad_scale), int(accumulate), int(mask_grad_by_x), ledger.data_ptr(), int(slot),
                                         _stream()), "maua_mse_fwd_bwd_ledger")


def tv_fwd_bwd_ledger(x, grad, strength, accumulate, ledger, slot):
    n, c, h, w = x.shape
    _check(lib().maua_tv_fwd_bwd_ledger(_ptr(_f32(x, "x")), _ptr(grad), n, c, h, w, float(strength), int(accumulate),
                                        ledger.data_ptr(), int(slot), _stream()), "maua_tv_fwd_bwd_ledger")


def loss_ledger_sum(ledger, losses, totals, losses_f64=None):
    """losses: (frames, slots) or (slots,) float32; totals: (frames,) float32; losses_f64 (optional, float64, same shape as
    losses): every filled record's loss before its rounding to fp32."""
    frames, slots = ledger.shape[0], ledger.shape[1]
    if losses_f64 is not None:
        assert losses_f64.dtype == torch.float64 and losses_f64.numel() == frames * slots and losses_f64.is_contiguous()
        _check(lib().maua_loss_ledger_sum_f64(ledger.data_ptr(), frames, slots, _ptr(losses), _ptr(totals), losses_f64.data_ptr(),
                                              _stream()), "maua_loss_ledger_sum_f64")
        return
    _check(lib().maua_loss_ledger_sum(ledger.data_ptr(), frames, slots, _ptr(losses), _ptr(totals), _stream()),
           "maua_loss_ledger_sum")


def gram_bwd(d_sym, f, row_mean, gf, accumulate, workspace=None, relu_mask=None):
    c = d_sym.shape[0]
    hw = f.numel() // c
    workspace = _ws(workspace, 4 * c + 256, f.device)
    _check(lib().maua_gram_bwd(_ptr(_f32(d_sym, "d")), _ptr(f), _ptr(row_mean), _ptr(relu_mask), _ptr(gf), c, hw, int(accumulate),
                               workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
           "maua_gram_bwd")
    return gf


def gram_guided_workspace_bytes(regions, c, hw):
    return lib().maua_gram_guided_workspace_bytes(int(regions), int(c), int(hw))


def _guides_2d(guides, hw):
    if guides.dim() < 2 or guides.numel() != guides.shape[0] * hw:
        raise HipError(f"guides of shape {tuple(guides.shape)} do not cover {hw} pixels per region")
    return guides.shape[0]


def gram_guided_mass(guides, out=None):
    """guides: (R, HW) or (R, H, W) -> mass (R,) float64 device tensor, mass[r] = sum guides[r]^2 (fixed order)."""
    r = guides.shape[0]
    hw = guides.numel() // max(r, 1)
    if out is None:
        out = torch.empty(r, dtype=torch.float64, device=guides.device)
    _check(lib().maua_gram_guided_mass(_ptr(_f32(guides, "guides")), _ptr(out), r, hw, _stream()), "maua_gram_guided_mass")
    return out


def gram_guided_fwd(f, guides, scale, center=False, mass=None, out=None, mean_out=None, workspace=None):
    """f: (1,C,H,W) or (C,HW); guides: (R,HW) or (R,H,W); scale: (R,) float32 (0 = inactive region); mass: (R,) float64 (needed to
    centre).  Returns (grams (R,C,C), weighted row means (R,C) or None)."""
    c = f.shape[1] if f.dim() == 4 else f.shape[0]
    hw = f.numel() // c
    r = _guides_2d(guides, hw)
    if scale.numel() != r or (center and (mass is None or mass.numel() != r or mass.dtype != torch.float64)):
        raise HipError("gram_guided_fwd: one scale (float32) and, to centre, one mass (float64) per region")
    if out is None:
        out = torch.empty(r, c, c, device=f.device, dtype=torch.float32)
    if center and mean_out is None:
        mean_out = torch.empty(r, c, device=f.device, dtype=torch.float32)
    workspace = _ws(workspace, gram_guided_workspace_bytes(r, c, hw), f.device)
    _check(lib().maua_gram_guided_fwd(_ptr(_f32(f, "f")), _ptr(_f32(guides, "guides")), _ptr(_f32(scale, "scale")), _ptr(mass) if center else None,
                                      _ptr(out), _ptr(mean_out) if center else None, r, c, hw, int(center), workspace.data_ptr(),
                                      workspace.numel() * workspace.element_size(), _stream()), "maua_gram_guided_fwd")
    return out, (mean_out if center else None)


def gram_guided_bwd(d_sym, f, guides, coef, mean, gf, accumulate):
    """gf (+)= sum_r coef[r] guides[r]^2 d_sym[r] (f - mean[r]); d_sym: (R,C,C) symmetric, mean: (R,C) or None."""
    r, c = d_sym.shape[0], d_sym.shape[1]
    hw = f.numel() // c
    if _guides_2d(guides, hw) != r or coef.numel() != r or gf.numel() != f.numel() or (mean is not None and mean.numel() != r * c):
        raise HipError("gram_guided_bwd: shapes of d_sym, guides, coef, mean and gf do not agree")
    _check(lib().maua_gram_guided_bwd(_ptr(_f32(d_sym, "d")), _ptr(_f32(f, "f")), _ptr(_f32(guides, "guides")), _ptr(_f32(coef, "coef")),
                                      _ptr(_f32(mean, "mean")), _ptr(_f32(gf, "gf")), r, c, hw, int(accumulate), _stream()), "maua_gram_guided_bwd")
    return gf


def gram_shift_supported(shifts, c, h, w):
    return bool(lib().maua_gram_shift_supported(int(shifts), int(c), int(h), int(w)))


def gram_shift_workspace_bytes(shifts, c, h, w):
    return lib().maua_gram_shift_workspace_bytes(int(shifts), int(c), int(h), int(w))


def _shift_args(shifts, factors):
    """shifts: [(axis, delta), ...] with axis 0 = x, 1 = y -> the three host arrays of the gram_shift entry points."""
    n = len(shifts)
    if n != len(factors):
        raise HipError(f"{n} shifts and {len(factors)} factors")
    return ((ctypes.c_int * n)(*[int(a) for a, _ in shifts]), (ctypes.c_int * n)(*[int(d) for _, d in shifts]),
            (ctypes.c_double * n)(*[float(v) for v in factors]))


def gram_shift_fwd(f, shifts, scales, mean=None, out=None, workspace=None):
    """f: (1,C,H,W) or (C,H,W); shifts: [(axis, delta), ...]; scales: one float per shift; mean: (C,) row means to subtract or None.
    Returns grams (S,C,C), gram[s][c][k] = scales[s] sum_p X[c][p + off_s] X[k][p] over the pairs inside the map."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    if f.numel() != c * h * w or (mean is not None and mean.numel() != c):
        raise HipError("gram_shift_fwd: f is one (C, H, W) map and mean holds C values")
    n = len(shifts)
    axes, deltas, fac = _shift_args(shifts, scales)
    if out is None:
        out = torch.empty(n, c, c, device=f.device, dtype=torch.float32)
    elif out.numel() != n * c * c:
        raise HipError("gram_shift_fwd: out is (S, C, C)")
    workspace = _ws(workspace, gram_shift_workspace_bytes(n, c, h, w), f.device)
    _check(lib().maua_gram_shift_fwd(_ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), axes, deltas, fac, _ptr(_f32(out, "out")), n, c, h, w,
                                     workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()), "maua_gram_shift_fwd")
    return out


def gram_shift_bwd(d, f, shifts, coefs, mean, gx, accumulate):
    """gx (+)= sum_s coefs[s] (d[s] X shifted back by off_s + d[s]^T X shifted on by off_s), X = f - mean; d: (S,C,C) as given (not
    symmetrised).  The gradient with respect to X: the caller subtracts the row means of gx in the covariance form."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    n = len(shifts)
    if f.numel() != c * h * w or d.numel() != n * c * c or gx.numel() != f.numel() or (mean is not None and mean.numel() != c):
        raise HipError("gram_shift_bwd: shapes of d, f, mean and gx do not agree")
    axes, deltas, fac = _shift_args(shifts, coefs)
    _check(lib().maua_gram_shift_bwd(_ptr(_f32(d, "d")), _ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), axes, deltas, fac, _ptr(_f32(gx, "gx")),
                                     n, c, h, w, int(accumulate), _stream()), "maua_gram_shift_bwd")
    return gx


def gram_flip_supported(mirrors, c, h, w):
    return bool(lib().maua_gram_flip_supported(int(mirrors), int(c), int(h), int(w)))


def gram_flip_workspace_bytes(mirrors, c, h, w):
    return lib().maua_gram_flip_workspace_bytes(int(mirrors), int(c), int(h), int(w))


def _flip_args(kinds, factors):
    """kinds: [0 = LR | 1 = UD | 2 = point mirror, ...] -> the two host arrays of the gram_flip entry points."""
    n = len(kinds)
    if n != len(factors):
        raise HipError(f"{n} mirrors and {len(factors)} factors")
    return (ctypes.c_int * n)(*[int(k) for k in kinds]), (ctypes.c_double * n)(*[float(v) for v in factors])


def gram_flip_fwd(f, kinds, scales, mean=None, out=None, workspace=None):
    """f: (1,C,H,W) or (C,H,W); kinds: [0 = LR | 1 = UD | 2 = point mirror, ...]; scales: one float per mirror; mean: (C,) row means to
    subtract or None.  Returns grams (M,C,C), gram[m][c][k] = scales[m] sum_p X[c][sigma_m(p)] X[k][p] over all pixels (bit-symmetric)."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    if f.numel() != c * h * w or (mean is not None and mean.numel() != c):
        raise HipError("gram_flip_fwd: f is one (C, H, W) map and mean holds C values")
    n = len(kinds)
    kd, fac = _flip_args(kinds, scales)
    if out is None:
        out = torch.empty(n, c, c, device=f.device, dtype=torch.float32)
    elif out.numel() != n * c * c:
        raise HipError("gram_flip_fwd: out is (M, C, C)")
    workspace = _ws(workspace, gram_flip_workspace_bytes(n, c, h, w), f.device)
    _check(lib().maua_gram_flip_fwd(_ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), kd, fac, _ptr(_f32(out, "out")), n, c, h, w,
                                    workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()), "maua_gram_flip_fwd")
    return out


def gram_flip_bwd(d, f, kinds, coefs, mean, gx, accumulate):
    """gx (+)= sum_m coefs[m] (d[m] + d[m]^T) X mirrored by sigma_m, X = f - mean; d: (M,C,C) as given (not symmetrised).  The gradient with
    respect to f in the covariance form too: the term through the row means vanishes."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    n = len(kinds)
    if f.numel() != c * h * w or d.numel() != n * c * c or gx.numel() != f.numel() or (mean is not None and mean.numel() != c):
        raise HipError("gram_flip_bwd: shapes of d, f, mean and gx do not agree")
    kd, fac = _flip_args(kinds, coefs)
    _check(lib().maua_gram_flip_bwd(_ptr(_f32(d, "d")), _ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), kd, fac, _ptr(_f32(gx, "gx")),
                                    n, c, h, w, int(accumulate), _stream()), "maua_gram_flip_bwd")
    return gx


def feat_hist_supported(c, h, w, bins, knots):
    return bool(lib().maua_feat_hist_supported(int(c), int(h), int(w), int(bins), int(knots)))


def feat_hist_workspace_bytes(c, h, w, bins, knots):
    return lib().maua_feat_hist_workspace_bytes(int(c), int(h), int(w), int(bins), int(knots))


def feat_hist_state_bytes(c, bins):
    return lib().maua_feat_hist_state_bytes(int(c), int(bins))


def feat_hist_quantiles(f, knots):
    """The target table of one style frame f (1,C,H,W) or (C,H,W): per channel the sorted activation s[0 .. N - 1] read at
    min(N - 1, floor((k + 0.5) N / knots)), k = 0 .. knots - 1 -> (C, knots) float32, non-decreasing along a row.  Sort and gather on the
    device (torch.sort): this runs once per style image and scale, not per iteration."""
    c = f.shape[-3]
    n = f.shape[-2] * f.shape[-1]
    if f.numel() != c * n or not 2 <= int(knots) <= 4096:
        raise HipError("feat_hist_quantiles: f is one (C, H, W) map and 2 <= knots <= 4096")
    if not f.is_cuda:
        raise HipError("feat_hist_quantiles: a ROCm device tensor is needed (there is no CPU path)")
    k = int(knots)
    at = torch.tensor([min(n - 1, ((2 * i + 1) * n) // (2 * k)) for i in range(k)], dtype=torch.int64, device=f.device)
    return torch.sort(_f32(f, "f").reshape(c, n), dim=1).values.index_select(1, at).contiguous()


def feat_hist_state_parts(state, c, bins):
    """(lo (C,) float32, hi (C,) float32, cum (C, bins + 1) int32) of a state maua_feat_hist_fwd filled (the layout of maua_hip.h)."""
    rec = state.view(torch.int32)[:c * (bins + 3)].reshape(c, bins + 3)
    ends = rec[:, :2].contiguous().view(torch.float32)
    return ends[:, 0], ends[:, 1], rec[:, 2:]


def _feat_hist_dims(who, f, table, bins):
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    if f.numel() != c * h * w or table.dim() != 2 or table.shape[0] != c:
        raise HipError(f"{who}: f is one (C, H, W) map and table is (C, knots)")
    knots = table.shape[1]
    if not feat_hist_supported(c, h, w, bins, knots):
        raise HipError(f"{who}: {c} channels, {h} x {w} pixels, {bins} bins, {knots} knots are not supported")
    return c, h, w, knots


def feat_hist_fwd(f, table, bins, state=None, loss=None, workspace=None):
    """f: (1,C,H,W) or (C,H,W); table: (C, knots).  Returns (loss (1,) float32 = mean (f - R)^2 with R the histogram-matched map, state):
    `state` (int32 words, feat_hist_state_bytes) holds lo, hi and the cumulative counts per channel - feat_hist_bwd reads it."""
    c, h, w, knots = _feat_hist_dims("feat_hist_fwd", f, table, bins)
    words = feat_hist_state_bytes(c, bins) // 4
    if state is None:
        state = torch.empty(words, dtype=torch.int32, device=f.device)
    elif state.dtype != torch.int32 or state.numel() < words or not state.is_contiguous() or not state.is_cuda:
        raise HipError("feat_hist_fwd: state is a contiguous int32 device tensor of feat_hist_state_bytes")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=f.device)
    workspace = _ws(workspace, feat_hist_workspace_bytes(c, h, w, bins, knots), f.device)
    _check(lib().maua_feat_hist_fwd(_ptr(_f32(f, "f")), _ptr(_f32(table, "table")), state.data_ptr(), _ptr(_f32(loss, "loss")), c, h, w,
                                    int(bins), knots, workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
           "maua_feat_hist_fwd")
    return loss, state


def feat_hist_bwd(f, table, state, bins, coef, gx, accumulate, upstream=None):
    """gx (+)= coef upstream (f - R); state: what feat_hist_fwd left for the same f and table; upstream: device float32 scalar or None (1)."""
    c, h, w, knots = _feat_hist_dims("feat_hist_bwd", f, table, bins)
    if gx.numel() != f.numel() or state.dtype != torch.int32 or state.numel() < feat_hist_state_bytes(c, bins) // 4 or not state.is_cuda \
            or (upstream is not None and upstream.numel() != 1):
        raise HipError("feat_hist_bwd: shapes of f, state, upstream and gx do not agree")
    _check(lib().maua_feat_hist_bwd(_ptr(_f32(f, "f")), _ptr(_f32(table, "table")), state.data_ptr(), _ptr(_f32(upstream, "upstream")),
                                    float(coef), _ptr(_f32(gx, "gx")), c, h, w, int(bins), knots, int(accumulate), _stream()),
           "maua_feat_hist_bwd")
    return gx


def mrf_supported(c, h, w, hs, ws, p):
    return bool(lib().maua_mrf_supported(int(c), int(h), int(w), int(hs), int(ws), int(p)))


def mrf_workspace_bytes(c, h, w, hs, ws, p):
    return lib().maua_mrf_workspace_bytes(int(c), int(h), int(w), int(hs), int(ws), int(p))


def mrf_state_bytes(h, w):
    return lib().maua_mrf_state_bytes(int(h), int(w))


def mrf_state_parts(state, h, w):
    """(nn (Q,) int32, best (Q,) float32) of a state maua_mrf_fwd filled, Q = (h - 2)(w - 2) (the layout of maua_hip.h)."""
    q = (h - 2) * (w - 2)
    return state[:q], state[q:2 * q].view(torch.float32)


def mrf_bank(s, origin):
    """The bank of one style map s (1,C,Hs,Ws) or (C,Hs,Ws) on the device: `origin` is a HOST int32 tensor (P,) of patch origins ys Ws + xs,
    checked here - every 3x3 patch inside the map - before it is uploaded.  Returns (origin on the device, inv (P,) float32 =
    1 / ||patch||).  Once per capture."""
    c, hs, ws = s.shape[-3], s.shape[-2], s.shape[-1]
    if s.numel() != c * hs * ws:
        raise HipError("mrf_bank: s is one (C, Hs, Ws) map")
    if origin.is_cuda or origin.dtype != torch.int32 or origin.dim() != 1:
        raise HipError("mrf_bank: origin is a host int32 tensor (P,): it is checked before the upload")
    p = origin.numel()
    if not mrf_supported(c, 3, 3, hs, ws, p):
        raise HipError(f"mrf_bank: {c} channels, a {hs} x {ws} style map, {p} patches are not supported")
    o = origin.long()
    if bool((o < 0).any()) or bool((o // ws > hs - 3).any()) or bool((o % ws > ws - 3).any()):
        raise HipError(f"mrf_bank: an origin whose 3 x 3 patch leaves the {hs} x {ws} map")
    od = origin.contiguous().to(s.device)
    inv = torch.empty(p, dtype=torch.float32, device=s.device)
    _check(lib().maua_mrf_bank(_ptr(_f32(s, "s")), od.data_ptr(), _ptr(inv), c, hs, ws, p, _stream()), "maua_mrf_bank")
    return od, inv


def _mrf_dims(who, f, s, origin, inv=None):
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    hs, ws = s.shape[-2], s.shape[-1]
    p = origin.numel()
    if f.numel() != c * h * w or s.numel() != c * hs * ws or origin.dtype != torch.int32 or not origin.is_cuda or not origin.is_contiguous() \
            or (inv is not None and inv.numel() != p):
        raise HipError(f"{who}: f is one (C, H, W) map, s one (C, Hs, Ws) map, origin a device int32 tensor (P,) and inv (P,)")
    if not mrf_supported(c, h, w, hs, ws, p):
        raise HipError(f"{who}: {c} channels, {h} x {w} pixels, a {hs} x {ws} style map, {p} patches are not supported")
    return c, h, w, hs, ws, p


def mrf_fwd(f, s, origin, inv, state=None, loss=None, workspace=None):
    """f: (1,C,H,W) or (C,H,W); the bank (s, origin, inv) of mrf_bank.  Returns (loss (1,) float32 = the mean squared distance of every 3x3
    patch to its nearest style patch, state): `state` (int32 words, mrf_state_bytes) holds nn[Q] and best[Q] - mrf_bwd reads nn."""
    c, h, w, hs, ws, p = _mrf_dims("mrf_fwd", f, s, origin, inv)
    words = mrf_state_bytes(h, w) // 4
    if state is None:
        state = torch.empty(words, dtype=torch.int32, device=f.device)
    elif state.dtype != torch.int32 or state.numel() < words or not state.is_contiguous() or not state.is_cuda:
        raise HipError("mrf_fwd: state is a contiguous int32 device tensor of mrf_state_bytes")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=f.device)
    workspace = _ws(workspace, mrf_workspace_bytes(c, h, w, hs, ws, p), f.device)
    _check(lib().maua_mrf_fwd(_ptr(_f32(f, "f")), _ptr(_f32(s, "s")), origin.data_ptr(), _ptr(_f32(inv, "inv")), state.data_ptr(),
                              _ptr(_f32(loss, "loss")), c, h, w, hs, ws, p, workspace.data_ptr(),
                              workspace.numel() * workspace.element_size(), _stream()), "maua_mrf_fwd")
    return loss, state


def mrf_bwd(f, s, origin, state, coef, gx, accumulate, upstream=None):
    """gx (+)= coef upstream times, per element, the sum over the query patches that cover it of (f - the nearest style patch's value there);
    state: what mrf_fwd left for the same f and bank; upstream: device float32 scalar or None (1)."""
    c, h, w, hs, ws, p = _mrf_dims("mrf_bwd", f, s, origin)
    if gx.numel() != f.numel() or state.dtype != torch.int32 or state.numel() < mrf_state_bytes(h, w) // 4 or not state.is_cuda \
            or (upstream is not None and upstream.numel() != 1):
        raise HipError("mrf_bwd: shapes of f, state, upstream and gx do not agree")
    _check(lib().maua_mrf_bwd(_ptr(_f32(f, "f")), _ptr(_f32(s, "s")), origin.data_ptr(), state.data_ptr(), _ptr(_f32(upstream, "upstream")),
                              float(coef), _ptr(_f32(gx, "gx")), c, h, w, hs, ws, p, int(accumulate), _stream()), "maua_mrf_bwd")
    return gx


def swd_supported(c, d, h, w, bins, knots):
    return bool(lib().maua_swd_supported(int(c), int(d), int(h), int(w), int(bins), int(knots)))


def swd_workspace_bytes(c, d, h, w, bins, knots):
    return lib().maua_swd_workspace_bytes(int(c), int(d), int(h), int(w), int(bins), int(knots))


def swd_state_bytes(d, bins):
    return lib().maua_swd_state_bytes(int(d), int(bins))


def _swd_dims(who, f, dirs):
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    if f.numel() != c * h * w or dirs.dim() != 2 or dirs.shape[1] != c:
        raise HipError(f"{who}: f is one (C, H, W) map and dirs is (D, C)")
    d = dirs.shape[0]
    if not swd_supported(c, d, h, w, 16, 2):
        raise HipError(f"{who}: {c} channels, {d} directions, {h} x {w} pixels are not supported")
    return c, d, h, w


def swd_project(f, dirs, bins=None, proj=None, state=None, workspace=None):
    """f: (1,C,H,W) or (C,H,W); dirs: (D, C), rows of unit length.  Returns (P (D, H, W) = dirs f, state, workspace).  bins None: the plain
    projection (state and workspace None) - the capture of a style map.  Otherwise `state` (int32 words, swd_state_bytes) has its counters
    zeroed and `workspace` holds the range slabs of P: both go to the swd_match that follows."""
    c, d, h, w = _swd_dims("swd_project", f, dirs)
    if proj is None:
        proj = torch.empty(d, h, w, dtype=torch.float32, device=f.device)
    elif proj.numel() != d * h * w:
        raise HipError("swd_project: proj is (D, H, W)")
    if bins is None:
        _check(lib().maua_swd_project(_ptr(_f32(f, "f")), _ptr(_f32(dirs, "dirs")), _ptr(_f32(proj, "proj")), None, c, d, h, w, 0, None, 0,
                                      _stream()), "maua_swd_project")
        return proj, None, None
    if not swd_supported(c, d, h, w, bins, 2):
        raise HipError(f"swd_project: {bins} bins are not supported")
    words = swd_state_bytes(d, bins) // 4
    if state is None:
        state = torch.empty(words, dtype=torch.int32, device=f.device)
    elif state.dtype != torch.int32 or state.numel() < words or not state.is_contiguous() or not state.is_cuda:
        raise HipError("swd_project: state is a contiguous int32 device tensor of swd_state_bytes")
    workspace = _ws(workspace, swd_workspace_bytes(c, d, h, w, bins, 2), f.device)
    _check(lib().maua_swd_project(_ptr(_f32(f, "f")), _ptr(_f32(dirs, "dirs")), _ptr(_f32(proj, "proj")), state.data_ptr(), c, d, h, w,
                                  int(bins), workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
           "maua_swd_project")
    return proj, state, workspace


def swd_match(proj, table, state, bins, workspace, loss=None):
    """proj: (D, H, W) = P, with `state` and `workspace` as swd_project left them; table: (D, knots).  Returns loss (1,) float32 = mean (P - R)^2
    with R the matched projections; fills `state` (the feature-histogram record of P) and leaves G = P - R in `proj`."""
    if proj.dim() != 3 or table.dim() != 2 or table.shape[0] != proj.shape[0]:
        raise HipError("swd_match: proj is (D, H, W) and table is (D, knots)")
    d, h, w = proj.shape
    knots = table.shape[1]
    if not swd_supported(1, d, h, w, bins, knots):
        raise HipError(f"swd_match: {d} directions, {h} x {w} pixels, {bins} bins, {knots} knots are not supported")
    if state.dtype != torch.int32 or state.numel() < swd_state_bytes(d, bins) // 4 or not state.is_contiguous() or not state.is_cuda:
        raise HipError("swd_match: state is a contiguous int32 device tensor of swd_state_bytes")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=proj.device)
    _check(lib().maua_swd_match(_ptr(_f32(proj, "proj")), _ptr(_f32(table, "table")), state.data_ptr(), _ptr(_f32(loss, "loss")), d, h, w,
                                int(bins), knots, workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
           "maua_swd_match")
    return loss


def swd_bwd(g, dirs_t, coef, gx, accumulate, upstream=None):
    """gx (C, H, W) (+)= coef upstream dirs_t g; g: (D, H, W) as swd_match left it, dirs_t: (C, D) the transposed directions; upstream: device
    float32 scalar or None (1)."""
    if g.dim() != 3 or dirs_t.dim() != 2 or dirs_t.shape[1] != g.shape[0]:
        raise HipError("swd_bwd: g is (D, H, W) and dirs_t is (C, D)")
    d, h, w = g.shape
    c = dirs_t.shape[0]
    if gx.numel() != c * h * w or (upstream is not None and upstream.numel() != 1) or not swd_supported(c, d, h, w, 16, 2):
        raise HipError("swd_bwd: shapes of g, dirs_t, upstream and gx do not agree")
    _check(lib().maua_swd_bwd(_ptr(_f32(g, "g")), _ptr(_f32(dirs_t, "dirs_t")), _ptr(_f32(upstream, "upstream")), float(coef),
                              _ptr(_f32(gx, "gx")), c, d, h, w, int(accumulate), _stream()), "maua_swd_bwd")
    return gx


def gram_guided_mse_ledger_supported(regions, c):
    """Do the partial sums of gram_guided_fwd_mse_ledger's finishing launch fit one ledger record?  (maua_hip.h states the bound.)"""
    return bool(lib().maua_guided_gram_mse_ledger_supported(int(regions), int(c)))


def gram_guided_fwd_mse_ledger(f, guides, scale, center, mass, out, mean_out, target, dmat, loss_scale, grad_scale, ledger, slot, workspace=None):
    """gram_guided_fwd into `out` (R,C,C) / `mean_out` (R,C) - the same bits - plus dmat[r] = grad_scale[r] (G_r - target[r]) (symmetric; zeros
    for a region with scale or grad_scale 0) and the layer's loss sum_r loss_scale[r] sum (G_r - target[r])^2 as record `slot` of `ledger`
    (one frame's records).  loss_scale, grad_scale: (R,) float32 device tensors."""
    c = f.shape[1] if f.dim() == 4 else f.shape[0]
    hw = f.numel() // c
    r = _guides_2d(guides, hw)
    if scale.numel() != r or loss_scale.numel() != r or grad_scale.numel() != r or \
            (center and (mass is None or mass.numel() != r or mass.dtype != torch.float64 or mean_out is None or mean_out.numel() != r * c)):
        raise HipError("gram_guided_fwd_mse_ledger: one scale, loss_scale, grad_scale (float32) and, to centre, one mass (float64) and C means per region")
    if out.numel() != r * c * c or target.numel() != r * c * c or dmat.numel() != r * c * c:
        raise HipError("gram_guided_fwd_mse_ledger: gram, target and dmat are (R, C, C)")
    workspace = _ws(workspace, gram_guided_workspace_bytes(r, c, hw), f.device)
    _check(lib().maua_guided_gram_fwd_mse_ledger(
        _ptr(_f32(f, "f")), _ptr(_f32(guides, "guides")), _ptr(_f32(scale, "scale")), _ptr(mass) if center else None, _ptr(_f32(out, "gram")),
        _ptr(_f32(mean_out, "mean")) if center else None, r, c, hw, int(center), _ptr(_f32(target, "target")), _ptr(_f32(loss_scale, "loss_scale")),
        _ptr(_f32(grad_scale, "grad_scale")), _ptr(_f32(dmat, "dmat")), ledger.data_ptr(), int(slot), workspace.data_ptr(),
        workspace.numel() * workspace.element_size(), _stream()), "maua_guided_gram_fwd_mse_ledger")
    return out, (mean_out if center else None)


def gram_guided_bwd_masked(d_sym, f, guides, coef, mean, gf, accumulate, relu_mask=None):
    """gram_guided_bwd whose result is written as 0 where relu_mask (shaped like gf) is <= 0; None: gram_guided_bwd's bits."""
    r, c = d_sym.shape[0], d_sym.shape[1]
    hw = f.numel() // c
    if _guides_2d(guides, hw) != r or coef.numel() != r or gf.numel() != f.numel() or (mean is not None and mean.numel() != r * c) or \
            (relu_mask is not None and relu_mask.numel() != gf.numel()):
        raise HipError("gram_guided_bwd_masked: shapes of d_sym, guides, coef, mean, relu_mask and gf do not agree")
    _check(lib().maua_guided_gram_bwd_masked(_ptr(_f32(d_sym, "d")), _ptr(_f32(f, "f")), _ptr(_f32(guides, "guides")), _ptr(_f32(coef, "coef")),
                                             _ptr(_f32(mean, "mean")), _ptr(_f32(relu_mask, "relu_mask")), _ptr(_f32(gf, "gf")), r, c, hw,
                                             int(accumulate), _stream()), "maua_guided_gram_bwd_masked")
    return gf


def _f64_args(name, n, *lists):
    """Host coefficient lists of n entries each -> ctypes double arrays."""
    for v in lists:
        if len(v) != n:
            raise HipError(f"{name}: {len(v)} coefficients for {n} terms")
    return [(ctypes.c_double * n)(*[float(x) for x in v]) for v in lists]


def gram_shift_mse_ledger_supported(shifts, c):
    """Do the partial sums of gram_shift_fwd_mse_ledger's finishing launch fit one ledger record?  (maua_hip.h states the bound.)"""
    return bool(lib().maua_shift_gram_mse_ledger_supported(int(shifts), int(c)))


def gram_shift_fwd_mse_ledger(f, shifts, scales, mean, out, target, dmat, loss_scales, grad_scales, ledger, slot, workspace=None):
    """gram_shift_fwd into `out` (S,C,C) - the same bits - plus dmat[s] = grad_scales[s] (G_s - target[s]) (as it is, not symmetrised; zeros
    where grad_scales[s] is 0) and sum_s loss_scales[s] sum (G_s - target[s])^2 as record `slot` of `ledger` (one frame's records).
    loss_scales, grad_scales: one host float per shift."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    n = len(shifts)
    if f.numel() != c * h * w or (mean is not None and mean.numel() != c):
        raise HipError("gram_shift_fwd_mse_ledger: f is one (C, H, W) map and mean holds C values")
    if out.numel() != n * c * c or target.numel() != n * c * c or dmat.numel() != n * c * c:
        raise HipError("gram_shift_fwd_mse_ledger: gram, target and dmat are (S, C, C)")
    axes, deltas, fac = _shift_args(shifts, scales)
    ls, gs = _f64_args("gram_shift_fwd_mse_ledger", n, loss_scales, grad_scales)
    workspace = _ws(workspace, gram_shift_workspace_bytes(n, c, h, w), f.device)
    _check(lib().maua_shift_gram_fwd_mse_ledger(
        _ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), axes, deltas, fac, _ptr(_f32(out, "gram")), n, c, h, w, _ptr(_f32(target, "target")), ls, gs,
        _ptr(_f32(dmat, "dmat")), ledger.data_ptr(), int(slot), workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
        "maua_shift_gram_fwd_mse_ledger")
    return out


def gram_shift_bwd_masked(d, f, shifts, coefs, mean, gx, accumulate, relu_mask=None):
    """gram_shift_bwd whose result is written as 0 where relu_mask (shaped like gx) is <= 0; None: gram_shift_bwd's bits."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    n = len(shifts)
    if f.numel() != c * h * w or d.numel() != n * c * c or gx.numel() != f.numel() or (mean is not None and mean.numel() != c) or \
            (relu_mask is not None and relu_mask.numel() != gx.numel()):
        raise HipError("gram_shift_bwd_masked: shapes of d, f, mean, relu_mask and gx do not agree")
    axes, deltas, fac = _shift_args(shifts, coefs)
    _check(lib().maua_shift_gram_bwd_masked(_ptr(_f32(d, "d")), _ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), axes, deltas, fac,
                                            _ptr(_f32(relu_mask, "relu_mask")), _ptr(_f32(gx, "gx")), n, c, h, w, int(accumulate), _stream()),
           "maua_shift_gram_bwd_masked")
    return gx


def gram_flip_mse_ledger_supported(mirrors, c):
    """Do the partial sums of gram_flip_fwd_mse_ledger's finishing launch fit one ledger record?  (maua_hip.h states the bound.)"""
    return bool(lib().maua_flip_gram_mse_ledger_supported(int(mirrors), int(c)))


def gram_flip_fwd_mse_ledger(f, kinds, scales, mean, out, target, dmat, loss_scales, grad_scales, ledger, slot, workspace=None):
    """gram_flip_fwd into `out` (M,C,C) - the same bits - plus dmat[m] = grad_scales[m] (G_m - target[m]) (bit-symmetric; zeros where
    grad_scales[m] is 0) and sum_m loss_scales[m] sum (G_m - target[m])^2 as record `slot` of `ledger` (one frame's records).
    loss_scales, grad_scales: one host float per mirror."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    n = len(kinds)
    if f.numel() != c * h * w or (mean is not None and mean.numel() != c):
        raise HipError("gram_flip_fwd_mse_ledger: f is one (C, H, W) map and mean holds C values")
    if out.numel() != n * c * c or target.numel() != n * c * c or dmat.numel() != n * c * c:
        raise HipError("gram_flip_fwd_mse_ledger: gram, target and dmat are (M, C, C)")
    kd, fac = _flip_args(kinds, scales)
    ls, gs = _f64_args("gram_flip_fwd_mse_ledger", n, loss_scales, grad_scales)
    workspace = _ws(workspace, gram_flip_workspace_bytes(n, c, h, w), f.device)
    _check(lib().maua_flip_gram_fwd_mse_ledger(
        _ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), kd, fac, _ptr(_f32(out, "gram")), n, c, h, w, _ptr(_f32(target, "target")), ls, gs,
        _ptr(_f32(dmat, "dmat")), ledger.data_ptr(), int(slot), workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
        "maua_flip_gram_fwd_mse_ledger")
    return out


def gram_flip_bwd_masked(d, f, kinds, coefs, mean, gx, accumulate, relu_mask=None):
    """gram_flip_bwd whose result is written as 0 where relu_mask (shaped like gx) is <= 0; None: gram_flip_bwd's bits."""
    c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
    n = len(kinds)
    if f.numel() != c * h * w or d.numel() != n * c * c or gx.numel() != f.numel() or (mean is not None and mean.numel() != c) or \
            (relu_mask is not None and relu_mask.numel() != gx.numel()):
        raise HipError("gram_flip_bwd_masked: shapes of d, f, mean, relu_mask and gx do not agree")
    kd, fac = _flip_args(kinds, coefs)
    _check(lib().maua_flip_gram_bwd_masked(_ptr(_f32(d, "d")), _ptr(_f32(f, "f")), _ptr(_f32(mean, "mean")), kd, fac,
                                           _ptr(_f32(relu_mask, "relu_mask")), _ptr(_f32(gx, "gx")), n, c, h, w, int(accumulate), _stream()),
           "maua_flip_gram_bwd_masked")
    return gx


def mse_fwd_bwd(x, target, grad, loss_scale, grad_scale, accumulate, loss_out, workspace=None, mask_grad_by_x=False):
    n = x.numel()
    workspace = _ws(workspace, reduce_workspace_bytes(n), x.device)
    _check(lib().maua_mse_fwd_bwd(_ptr(_f32(x, "x")), _ptr(_f32(target, "target")), _ptr(grad), n, float(loss_scale),
                                  float(grad_scale), int(accumulate), int(mask_grad_by_x), _ptr(loss_out),
                                  workspace.data_ptr(),
                                  workspace.numel() * workspace.element_size(), _stream()), "maua_mse_fwd_bwd")
    return loss_out


def mse_weighted_fwd_bwd(x, weights, target, grad, loss_scale, grad_scale, accumulate, loss_out, workspace=None):
    """Temporal ContentLoss: loss = loss_scale * sum((x*w - t)^2), grad (+)= grad_scale * w * (x*w - t)."""
    n, c, h, w = x.shape
    wplanes = weights.numel() // (h * w)
    workspace = _ws(workspace, reduce_workspace_bytes(x.numel()), x.device)
    _check(lib().maua_mse_weighted_fwd_bwd(_ptr(_f32(x, "x")), _ptr(_f32(weights, "weights")), _ptr(_f32(target, "target")),
                                           _ptr(grad), n * c, h * w, wplanes, float(loss_scale), float(grad_scale),
                                           int(accumulate), _ptr(loss_out), workspace.data_ptr(),
                                           workspace.numel() * workspace.element_size(), _stream()),
           "maua_mse_weighted_fwd_bwd")
    return grad


def tv_fwd_bwd(x, grad, strength, accumulate, loss_out, workspace=None):
    n, c, h, w = x.shape
    workspace = _ws(workspace, reduce_workspace_bytes(x.numel()), x.device)
    _check(lib().maua_tv_fwd_bwd(_ptr(_f32(x, "x")), _ptr(grad), n, c, h, w, float(strength), int(accumulate),
                                 _ptr(loss_out), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                 _stream()), "maua_tv_fwd_bwd")
    return loss_out


def fill_(x, value):
    _check(lib().maua_fill(_ptr(x), x.numel(), float(value), _stream()), "maua_fill")
    return x


def axpy_(y, x, alpha):
    _check(lib().maua_axpy(_ptr(y), _ptr(x), float(alpha), x.numel(), _stream()), "maua_axpy")
    return y


def sum_small(slots, out):
    _check(lib().maua_sum_small(_ptr(slots), slots.numel(), _ptr(out), _stream()), "maua_sum_small")
    return out


def adam_step(x, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    _check(lib().maua_adam_step(_ptr(x), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), x.numel(), int(step), float(lr),
                                beta1, beta2, eps, _stream()), "maua_adam_step")


# ------------------------------------------------------------------------------------------
# image-space steps between two optimisation runs (csrc/image.hip)
# ------------------------------------------------------------------------------------------
def conv_pack_filters_few_mfma(w):
    """OIHW weights (64, 1-3, 3, 3) -> the bank of conv3x3_few_mfma (bf16 triples in MFMA lane order)."""
    cout, cin = w.shape[:2]
    bank = torch.empty(lib().maua_conv_few_mfma_bank_bytes(), dtype=torch.uint8, device=w.device)
    _check(lib().maua_conv_pack_filters_few_mfma(_ptr(_f32(w, "w")), bank.data_ptr(), cout, cin, _stream()), "maua_conv_pack_filters_few_mfma")
    return bank


def conv_few_mfma_supported(n, cin, h, w, cout, pad):
    return bool(lib().maua_conv_few_mfma_supported(int(n), int(cin), int(h), int(w), int(cout), int(pad)))


def conv3x3_few_mfma(gy, bank, cin, out=None, tile=0):
    """Backward-data of the image layer on the matrix cores: gy (n, 64, h, w) -> (n, cin, h, w).  tile: 0 = the library's choice,
    1 / 2 / 3 = 4 / 8 / 14 output rows x 62 columns per workgroup."""
    n, cout, h, w = gy.shape
    if out is None:
        out = torch.empty(n, cin, h, w, device=gy.device, dtype=torch.float32)
    _check(lib().maua_conv3x3_few_mfma(_ptr(_f32(gy, "gy")), bank.data_ptr(), _ptr(out), n, cin, h, w, cout, int(tile), _stream()), "maua_conv3x3_few_mfma")
    return out


def space_to_depth(x, r, out):
    """out[n][(ry r + rx) C + c][qy][qx] = x[n][c][r qy + ry][r qx + rx] (0 beyond x), C = x.shape[1]."""
    n, c, h, w = x.shape
    assert out.shape[0] == n and out.shape[1] == r * r * c
    _check(lib().maua_space_to_depth(_ptr(_f32(x, "x")), _ptr(out), n, c, r, h, w, out.shape[2], out.shape[3], _stream()), "maua_space_to_depth")
    return out


def depth_to_space(x, r, out, accumulate=False):
    """out[n][c][r qy + ry][r qx + rx] (+)= x[n][(ry r + rx) C + c][qy][qx], C = out.shape[1]; pixels beyond the sites of x: 0."""
    n, cc, qh, qw = x.shape
    c_out = out.shape[1]
    assert cc == r * r * c_out and out.shape[0] == n
    _check(lib().maua_depth_to_space(_ptr(_f32(x, "x")), _ptr(out), n, c_out, r, qh, qw, out.shape[2], out.shape[3], int(accumulate), _stream()),
           "maua_depth_to_space")
    return out


ARRIVAL_COUNTER_BYTES = 4096 * 4
_ARMED = threading.local()


def conv_arm_workspace(workspace, counters=None, zero=True):
    """Arm `workspace` (a device tensor handed to the convolution launches of this host thread) for split channel loops that are finished
    inside the producing launch (maua_conv_arm_workspace): returns the counters tensor (16 KiB, zeroed by the library here and left zeroed
    by every launch) - keep it alive as long as the workspace is in use.  zero=False: only point this thread back at a workspace it armed
    before (nothing is enqueued).  workspace None: disarm."""
    if workspace is None:
        _check(lib().maua_conv_arm_workspace(None, None, 0, 0, _stream()), "maua_conv_arm_workspace")
        _ARMED.pair = None
        return None
    if counters is None:
        counters = torch.empty(ARRIVAL_COUNTER_BYTES, dtype=torch.uint8, device=workspace.device)
        zero = True
    _check(lib().maua_conv_arm_workspace(workspace.data_ptr(), counters.data_ptr(), counters.numel() * counters.element_size(), int(bool(zero)),
                                         _stream()), "maua_conv_arm_workspace")
    _ARMED.pair = (workspace, counters)  # (the library holds raw pointers: both tensors stay alive while this thread is armed with them)
    return counters


def set_split_batch_hint(frames):
    """Frames per launch the job plans with (split-K policy of the convolutions); returns the previous value."""
    prev = lib().maua_get_split_batch_hint()
    lib().maua_set_split_batch_hint(int(frames))
    return prev


def channel_stats(x, noise=None, noise_amp=1e-3, out=None, workspace=None):
    """Raw colour statistics of a batch x (B,3,H,W), optionally jittered by noise_amp * noise (laid out [B][W][H][3], the
    order the reference draws it in): out[B][9] doubles, one row per plane slot j of the reference's reshape (component k =
    plane k * B + j; for B = 1 the three channels): component sums (3) and the upper triangle of the product sums (6)."""
    b, c, h, w = x.shape
    if c != 3:
        raise HipError("channel_stats: 3-channel images")
    if out is None:
        out = torch.empty(b, 9, dtype=torch.float64, device=x.device)
    workspace = _ws(workspace, lib().maua_channel_stats_workspace_bytes(h, w), x.device)
    if noise is not None and noise.numel() != x.numel():
        raise HipError("channel_stats: noise must have the batch's element count")
    for j in range(b):
        _check(lib().maua_channel_stats(_ptr(_f32(x, "x")), _ptr(noise), float(noise_amp), b, j, h, w, _ptr(out[j]),
                                        workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
               "maua_channel_stats")
    return out


def color_match_solve(stats_t, pixels_t, stats_s, pixels_s, eps, coef_out):
    """coef_out (16 floats) = [M = cov_s^(1/2) cov_t^(-1/2) (9), mean_t (3), mean_s (3), ok]; no host sync."""
    _check(lib().maua_color_match_solve(_ptr(stats_t), stats_t.shape[0], int(pixels_t), _ptr(stats_s), int(pixels_s), float(eps),
                                        _ptr(coef_out), _stream()), "maua_color_match_solve")
    return coef_out


def color_match_apply(x, noise, noise_amp, coef, all_coef, weight, accumulate, out):
    b, c, h, w = x.shape
    for j in range(b):
        _check(lib().maua_color_match_apply(_ptr(_f32(x, "x")), _ptr(noise), float(noise_amp), _ptr(coef), _ptr(all_coef),
                                            all_coef.numel() // 16, float(weight), int(accumulate), b, j, h, w, _ptr(out), _stream()),
               "maua_color_match_apply")
    return out


def resize_bilinear(x, size=None, scale_factor=None):
    """F.interpolate(x, size | scale_factor=..., mode="bilinear", align_corners=False) for (N,C,H,W) device tensors, with
    ATen's conventions: scale_factor form -> output floor(in * s), source step float(1 / s); size form -> in / out."""
    import math
    import numpy as np
    n, c, h, w = x.shape
    if (size is None) == (scale_factor is None):
        raise HipError("resize_bilinear: give exactly one of size / scale_factor")
    if scale_factor is not None:
        oh, ow = int(math.floor(float(h) * scale_factor)), int(math.floor(float(w) * scale_factor))
        sh = sw = float(np.float32(1.0 / scale_factor))
    else:
        oh, ow = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        sh, sw = float(np.float32(h) / np.float32(oh)), float(np.float32(w) / np.float32(ow))
    if oh <= 0 or ow <= 0:
        raise HipError(f"resize_bilinear: output {oh}x{ow}")
    out = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
    _check(lib().maua_resize_bilinear(_ptr(_f32(x, "x")), _ptr(out), n * c, h, w, oh, ow, sh, sw, _stream()), "maua_resize_bilinear")
    return out


def deprocess_u8(x, mean_bgr):
    """(1,3,H,W) or (3,H,W) network-space BGR image -> (H,W,3) uint8 RGB device tensor (load.deprocess's arithmetic)."""
    x3 = x.reshape(3, x.shape[-2], x.shape[-1])
    _, h, w = x3.shape
    out = torch.empty(h, w, 3, dtype=torch.uint8, device=x.device)
    _check(lib().maua_deprocess_u8(_ptr(_f32(x3, "x")), out.data_ptr(), h, w, float(mean_bgr[0]), float(mean_bgr[1]),
                                   float(mean_bgr[2]), _stream()), "maua_deprocess_u8")
    return out


def flow_warp_grid(flo, size, workspace=None):
    """load.flow_warp_map from a device flow field (h, w, 2) in pixels, as a .flo file stores it: the (1, H, W, 2) sampling grid of
    F.grid_sample for size = (H, W)."""
    if flo.dim() != 3 or flo.shape[2] != 2:
        raise HipError(f"flow_warp_grid: flow of shape {tuple(flo.shape)}, expected (h, w, 2)")
    h, w = int(flo.shape[0]), int(flo.shape[1])
    oh, ow = int(size[0]), int(size[1])
    if oh <= 0 or ow <= 0:
        raise HipError(f"flow_warp_grid: output {oh}x{ow}")
    need = lib().maua_flow_warp_grid_workspace_bytes(h, w)
    if not need:
        raise HipError(f"flow_warp_grid: flow field {h}x{w}")
    grid = torch.empty(1, oh, ow, 2, device=flo.device, dtype=torch.float32)
    if workspace is None:  # allocated after the result and held until the launches are enqueued: it must not share memory with `grid`
        workspace = torch.empty(need, dtype=torch.uint8, device=flo.device)
    _check(lib().maua_flow_warp_grid(_ptr(_f32(flo, "flo")), _ptr(grid), h, w, oh, ow, workspace.data_ptr(),
                                     workspace.numel() * workspace.element_size(), _stream()), "maua_flow_warp_grid")
    return grid


def grid_sample_border(x, grid, blend=None, blend_a=0.0):
    """F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False) for x (N,C,h,w) and grid (N,H,W,2).
    With `blend` (shaped like x, h x w == H x W) returns (sampled, (1 - blend_a) * blend + blend_a * x): both from one pass over x."""
    if x.dim() != 4 or grid.dim() != 4 or grid.shape[0] != x.shape[0] or grid.shape[3] != 2:
        raise HipError(f"grid_sample_border: x {tuple(x.shape)}, grid {tuple(grid.shape)}")
    n, c, h, w = (int(v) for v in x.shape)
    oh, ow = int(grid.shape[1]), int(grid.shape[2])
    out = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
    init = None
    if blend is not None:
        if tuple(blend.shape) != tuple(x.shape) or (h, w) != (oh, ow):
            raise HipError(f"grid_sample_border: blend {tuple(blend.shape)} with x {tuple(x.shape)} sampled to {oh}x{ow}")
        init = torch.empty_like(out)
    _check(lib().maua_grid_sample_border(_ptr(_f32(x, "x")), _ptr(_f32(grid, "grid")), _ptr(out), n, c, h, w, oh, ow,
                                         _ptr(_f32(blend, "blend")), float(blend_a), _ptr(init), _stream()), "maua_grid_sample_border")
    return out if blend is None else (out, init)


def mask_u8_resize(mask, size):
    """load.reliable_flow_weighting + F.interpolate(size=size, mode="bilinear", align_corners=False): a uint8 device mask (h, w) or
    (h, w, c) -> (1, c, H, W) float in [0, 1]."""
    m = mask if mask.dim() == 3 else mask.unsqueeze(-1)
    if m.dim() != 3:
        raise HipError(f"mask_u8_resize: mask of shape {tuple(mask.shape)}")
    h, w, c = (int(v) for v in m.shape)
    oh, ow = int(size[0]), int(size[1])
    if oh <= 0 or ow <= 0:
        raise HipError(f"mask_u8_resize: output {oh}x{ow}")
    out = torch.empty(1, c, oh, ow, device=m.device, dtype=torch.float32)
    _check(lib().maua_mask_u8_resize(_u8(m, "mask"), _ptr(out), h, w, c, oh, ow, _stream()), "maua_mask_u8_resize")
    return out


def gauss_wrap(x, sigmas, roll=0, workspace=None, out=None):
    """scipy.ndimage.gaussian_filter(np.roll(x, -roll, axis=0), [sigmas[0], 0, sigmas[1], sigmas[2]], mode="wrap") for a (T,C,H,W) device
    clip: a new tensor (or `out`, which must not be x).  workspace: at least maua_gauss_wrap_workspace_bytes, else one is allocated."""
    if not x.is_cuda:
        raise HipError("gauss_wrap: needs a ROCm device tensor (got a CPU tensor): there is no CPU path")
    if x.dim() != 4:
        raise HipError(f"gauss_wrap: clip of shape {tuple(x.shape)}, expected (T, C, H, W)")
    if len(sigmas) != 3:
        raise HipError(f"gauss_wrap: sigmas {sigmas!r}, expected (sigma_t, sigma_h, sigma_w)")
    t, c, h, w = (int(v) for v in x.shape)
    st, sh, sw = (float(v) for v in sigmas)
    L = lib()
    if not L.maua_gauss_wrap_supported(t, c, h, w, st, sh, sw):
        raise HipError(f"gauss_wrap: unsupported clip {tuple(x.shape)} with sigmas {(st, sh, sw)}")
    need = L.maua_gauss_wrap_workspace_bytes(t, c, h, w, st, sh, sw)
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    elif tuple(out.shape) != tuple(x.shape):
        raise HipError(f"gauss_wrap: out {tuple(out.shape)} for a clip {tuple(x.shape)}")
    if workspace is None and need:  # allocated after the result and held until the launches are enqueued: it must not share memory with it
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    wp, wn = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if workspace is not None else (None, 0)
    _check(L.maua_gauss_wrap(_ptr(_f32(x, "x")), _ptr(_f32(out, "out")), t, c, h, w, st, sh, sw, int(roll) % t, wp, wn, _stream()), "maua_gauss_wrap")
    return out


class LbfgsState:
    """Device-resident L-BFGS state (history slab + bookkeeping) for one flat fp32 vector."""

    def __init__(self, count, history, device):
        self.count, self.history = int(count), int(history)
        if not 0 < self.history <= 254:
            raise HipError(f"--lbfgs_num_correction {history}: the device-side recursion holds at most 254 pairs")
        nbytes = lib().maua_lbfgs_state_bytes(self.count, self.history)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self._status = torch.zeros(5, dtype=torch.float32, device=device)
        _check(lib().maua_lbfgs_init(self.buf.data_ptr(), nbytes, self.count, self.history, _stream()), "maua_lbfgs_init")

    def reset(self):
        """Back to the state of a new object (no pairs, iteration 0) in the same memory: a captured graph that holds this state's
        address serves the next optimisation problem."""
        _check(lib().maua_lbfgs_init(self.buf.data_ptr(), self.buf.numel(), self.count, self.history, _stream()), "maua_lbfgs_init")

    def iterate(self, x, grad, lr=1.0, tolerance_change=-1.0, tolerance_grad=-1.0, loss=None):
        """One trip of LBFGS.step's loop; `loss` (device scalar of the evaluation that produced `grad`) feeds the
        |loss - prev_loss| < tolerance_change test and may be None."""
        _check(lib().maua_lbfgs_iterate(self.buf.data_ptr(), _ptr(x), _ptr(grad), _ptr(loss), self.count, self.history, float(lr),
                                        float(tolerance_change), float(tolerance_grad), _stream()), "maua_lbfgs_iterate")

    def status(self):
        """Host copy of {n_iter, history_len, stopped, g.d, t} - this one synchronises."""
        _check(lib().maua_lbfgs_status(self.buf.data_ptr(), self.count, self.history, _ptr(self._status), _stream()),
               "maua_lbfgs_status")
        n_iter, hlen, stopped, gtd, t = self._status.tolist()
        return dict(n_iter=int(n_iter), history_len=int(hlen), stopped=bool(stopped), gtd=gtd, t=t)


# ------------------------------------------------------------------------------------------
# optical flow (csrc/flow.hip): planes [component][h][w], fp32; frames (h, w, 3) uint8 RGB
# ------------------------------------------------------------------------------------------
FLOW_MAX_LEVELS = 8


def _flow_dims_ok(h, w):
    return 0 < h <= 1 << 16 and 0 < w <= 1 << 16 and h * w <= 1 << 28


def flow_levels(h, w, max_levels=5):
    """Pyramid levels for an h x w pair (maua_flow_levels, restated on the host): ceil halving while the coarser level's shorter
    side stays >= 16, at most `max_levels`."""
    if not _flow_dims_ok(h, w) or max_levels < 1:
        return 0
    n = 1
    while n < max_levels and (h + 1) // 2 >= 16 and (w + 1) // 2 >= 16:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def flow_tvl1_workspace_bytes(h, w, levels):
    """Bytes of maua_flow_tvl1's workspace (the library's own formula, restated on the host): both grey pyramids, two solver states
    (6 planes) and the fields (3 planes) at the finest size, a 2-plane scratch; every region 256-byte aligned.  0 = invalid."""
    if not _flow_dims_ok(h, w) or not 1 <= levels <= FLOW_MAX_LEVELS or levels > flow_levels(h, w, levels):
        return 0
    a = lambda b: (b + 255) & ~255
    total, lh, lw = 0, h, w
    for _ in range(levels):
        total += 2 * a(lh * lw * 4)
        lh, lw = (lh + 1) // 2, (lw + 1) // 2
    return total + 2 * a(6 * h * w * 4) + a(3 * h * w * 4) + a(2 * h * w * 4)


def _u8(t, name, shape=None):
    if not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous():
        raise HipError(f"{name}: expected a contiguous uint8 device tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise HipError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.data_ptr()


def flow_grey(rgb):
    """(h, w, 3) uint8 RGB -> (h, w) fp32 grey, (0.299 R + 0.587 G) + 0.114 B."""
    h, w = rgb.shape[:2]
    out = torch.empty(h, w, dtype=torch.float32, device=rgb.device)
    _check(lib().maua_flow_grey_u8(_u8(rgb, "rgb", (h, w, 3)), out.data_ptr(), h, w, _stream()), "maua_flow_grey_u8")
    return out


def flow_pyr_down(img):
    """(h, w) -> (ceil(h/2), ceil(w/2)): Gaussian smoothing and 2x decimation."""
    h, w = img.shape
    out = torch.empty((h + 1) // 2, (w + 1) // 2, dtype=torch.float32, device=img.device)
    _check(lib().maua_flow_pyr_down(_ptr(_f32(img, "img")), out.data_ptr(), h, w, _stream()), "maua_flow_pyr_down")
    return out


def flow_warp_prep(i0, i1, u, fields=None):
    """Fields [I1wx][I1wy][rho_c] (3, h, w) of one warp at the flow u (2, h, w)."""
    h, w = i0.shape
    if tuple(i1.shape) != (h, w) or tuple(u.shape) != (2, h, w):
        raise HipError("flow_warp_prep: shapes")
    if fields is None:
        fields = torch.empty(3, h, w, dtype=torch.float32, device=i0.device)
    _check(lib().maua_flow_warp_prep(_ptr(_f32(i0, "i0")), _ptr(_f32(i1, "i1")), _ptr(_f32(u, "u")), _ptr(fields), h, w, _stream()),
           "maua_flow_warp_prep")
    return fields


def flow_tvl1_step(fields, state, out=None, k=0):
    """TV-L1 iterations on the state (6, h, w) = [u1, u2, p11, p12, p21, p22]: k = 0 one single-step launch, k >= 1 one launch of the
    temporally blocked kernel running k iterations.  Returns the new state (a different tensor)."""
    _, h, w = state.shape
    if tuple(state.shape) != (6, h, w) or tuple(fields.shape) != (3, h, w):
        raise HipError("flow_tvl1_step: shapes")
    if out is None:
        out = torch.empty_like(state)
    if k == 0:
        _check(lib().maua_flow_tvl1_step(_ptr(_f32(fields, "fields")), _ptr(_f32(state, "state")), _ptr(out), h, w, _stream()),
               "maua_flow_tvl1_step")
    else:
        _check(lib().maua_flow_tvl1_blocked(_ptr(_f32(fields, "fields")), _ptr(_f32(state, "state")), _ptr(out), h, w, int(k), _stream()),
               "maua_flow_tvl1_blocked")
    return out


def flow_median5(x):
    """5 x 5 median of every plane of (p, h, w), edge pixels replicated."""
    p, h, w = x.shape
    out = torch.empty_like(x)
    _check(lib().maua_flow_median5(_ptr(_f32(x, "x")), _ptr(out), h, w, p, _stream()), "maua_flow_median5")
    return out


def flow_upsample(x, h, w, scale=2.0):
    """(p, ch, cw) -> (p, h, w): bilinear with half-pixel centres, values x scale."""
    p, ch, cw = x.shape
    out = torch.empty(p, h, w, dtype=torch.float32, device=x.device)
    _check(lib().maua_flow_upsample(_ptr(_f32(x, "x")), ch, cw, _ptr(out), h, w, p, float(scale), _stream()), "maua_flow_upsample")
    return out


def flow_consistency(flow1, flow2):
    """The reference's check_consistency(flow1, flow2) as the bytes of its PNG, (1 - r) * 255: flows as (2, h, w) planes [u][v]."""
    _, h, w = flow1.shape
    if tuple(flow1.shape) != (2, h, w) or tuple(flow2.shape) != (2, h, w):
        raise HipError("flow_consistency: shapes")
    need = lib().maua_flow_consistency_workspace_bytes(h, w)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=flow1.device)
    out = torch.empty(h, w, dtype=torch.uint8, device=flow1.device)
    _check(lib().maua_flow_consistency(_ptr(_f32(flow1, "flow1")), _ptr(_f32(flow2, "flow2")), out.data_ptr(), h, w, ws.data_ptr(), need,
                                       _stream()), "maua_flow_consistency")
    return out


def flow_tvl1(rgb1, rgb2, levels, warps, iters, block_k, out=None, workspace=None):
    """The whole TV-L1 estimate of one pair of (h, w, 3) uint8 RGB frames -> (2, h, w) flow [u][v] with rgb1(x) ~ rgb2(x + flow(x))."""
    h, w = rgb1.shape[:2]
    need = flow_tvl1_workspace_bytes(h, w, levels)
    if need == 0:
        raise HipError(f"flow_tvl1: {levels} levels for {h}x{w}")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=rgb1.device)
    if workspace.numel() < need:
        raise HipError("flow_tvl1: workspace too small")
    if out is None:
        out = torch.empty(2, h, w, dtype=torch.float32, device=rgb1.device)
    _check(lib().maua_flow_tvl1(_u8(rgb1, "rgb1", (h, w, 3)), _u8(rgb2, "rgb2", (h, w, 3)), _ptr(_f32(out, "out")), h, w, int(levels),
                                int(warps), int(iters), int(block_k), workspace.data_ptr(), workspace.numel(), _stream()), "maua_flow_tvl1")
    return out


# ------------------------------------------------------------------------------------------
# neural cellular automaton (csrc/nca.hip): state (n, chn, h, w) fp32, params flat [w1][b1][w2]
# ------------------------------------------------------------------------------------------
def nca_supported(n, chn, hidden, h, w):
    return bool(lib().maua_nca_supported(int(n), int(chn), int(hidden), int(h), int(w)))


def nca_param_count(chn, hidden):
    return int(lib().maua_nca_param_count(int(chn), int(hidden)))


def _nca_mask_args(x, rate_map, mask):
    n, _, h, w = x.shape
    if rate_map is not None and tuple(rate_map.shape) != (h, w):
        raise HipError(f"nca: rate_map shape {tuple(rate_map.shape)}, expected {(h, w)}")
    if mask is not None and tuple(mask.shape) not in ((n, h, w), (n, 1, h, w)):
        raise HipError(f"nca: mask shape {tuple(mask.shape)}, expected {(n, 1, h, w)}")
    return _ptr(_f32(rate_map, "rate_map")), _ptr(_f32(mask, "mask"))


def _nca_mask(mask):
    """Explicit masks may come as uint8 / bool; the kernel reads fp32."""
    return mask.float() if mask is not None and mask.dtype in (torch.uint8, torch.bool) else mask


def _nca_shape(x, params, chn, hidden):
    n, c, h, w = x.shape
    if c != chn:
        raise HipError(f"nca: state has {c} channels, the model {chn}")
    if params.numel() != nca_param_count(chn, hidden) or not nca_supported(n, chn, hidden, h, w):
        raise HipError(f"nca: unsupported chn/hidden {chn}/{hidden} for a {tuple(x.shape)} state")
    return n, h, w


def nca_step(x, params, chn, hidden, rate=0.5, rate_map=None, mask=None, seed=0, step=0, out=None):
    """One CA step: out = x + mask * W2 relu(W1 perception(x) + b1).  mask: explicit fp32 / uint8 (n, [1,] h, w), or None for the
    in-kernel mask floor(u(seed, step, b, y, x) + rate) with rate = rate_map[y][x] when given."""
    n, h, w = _nca_shape(x, params, chn, hidden)
    if out is None:
        out = torch.empty_like(x)
    mask = _nca_mask(mask)
    rp, mp = _nca_mask_args(x, rate_map, mask)
    _check(lib().maua_nca_step(_ptr(_f32(x, "x")), _ptr(_f32(out, "out")), _ptr(_f32(params, "params")), n, chn, hidden, h, w,
                               float(rate), rp, mp, int(seed) & (2 ** 64 - 1), int(step), _stream()), "maua_nca_step")
    return out


def nca_bwd_workspace(n, chn, hidden, h, w, device):
    need = lib().maua_nca_bwd_workspace_bytes(int(n), int(chn), int(hidden), int(h), int(w))
    if need == 0:
        raise HipError(f"nca: unsupported backward shape n={n} chn={chn} hidden={hidden} {h}x{w}")
    return torch.empty(need, dtype=torch.uint8, device=device)


def nca_step_bwd(x, g, params, chn, hidden, workspace, first, rate=0.5, rate_map=None, mask=None, seed=0, step=0, dx=None):
    """Backward of nca_step(x, ...) for the incoming gradient g: returns dx (may be g itself) and adds this step's parameter gradient
    to the partial slots in `workspace` (first=True clears them)."""
    n, h, w = _nca_shape(x, params, chn, hidden)
    if dx is None:
        dx = torch.empty_like(x)
    mask = _nca_mask(mask)
    rp, mp = _nca_mask_args(x, rate_map, mask)
    _check(lib().maua_nca_step_bwd(_ptr(_f32(x, "x")), _ptr(_f32(g, "g")), _ptr(_f32(dx, "dx")), _ptr(_f32(params, "params")), n, chn,
                                   hidden, h, w, float(rate), rp, mp, int(seed) & (2 ** 64 - 1), int(step), int(bool(first)),
                                   workspace.data_ptr(), workspace.numel(), _stream()), "maua_nca_step_bwd")
    return dx


def nca_grad_finish(shape, chn, hidden, workspace, normalize=False, out=None):
    """The parameter gradient (flat, params layout) summed from the partial slots; normalize: each tensor / (its norm + 1e-8)."""
    n, _, h, w = shape
    if out is None:
        out = torch.empty(nca_param_count(chn, hidden), dtype=torch.float32, device=workspace.device)
    _check(lib().maua_nca_grad_finish(_ptr(_f32(out, "grad")), n, chn, hidden, h, w, workspace.data_ptr(), workspace.numel(),
                                      int(bool(normalize)), _stream()), "maua_nca_grad_finish")
    return out
