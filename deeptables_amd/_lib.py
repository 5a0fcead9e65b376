# -*- coding:utf-8 -*-
"""ctypes binding of libdt_hip.so (the C-ABI declared in include/dt_hip.h).

This is the stub a DeepTables maintainer would add next to deeptables/models/layers.py to call
the MI355X kernels.  `import torch` MUST come first: the library's
NEEDED libamdhip64.so.7 then binds to the HIP runtime torch already loaded, so
`tensor.data_ptr()` and `torch.cuda.current_stream().cuda_stream` are valid in our launches.

There is no CPU fallback: `lib()` raises if the shared object is missing.
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported before the CDLL below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdt_hip.so')

_c_int = ctypes.c_int
_c_i64 = ctypes.c_int64
_c_f32 = ctypes.c_float
_ptr = ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/dt_hip.h one to one
SIGNATURES = {
    'dt_version': (_c_int, []),
    'dt_last_error': (ctypes.c_char_p, []),
    'dt_build_arch': (ctypes.c_char_p, []),
    'dt_source_hash': (ctypes.c_char_p, []),
    'dt_graph_upload': (_c_int, [_ptr, _ptr]),
    'dt_step_trace': (_c_int, [_c_int]),
    'dt_step_trace_read': (_c_int, [_ptr, _c_int, _ptr]),
    'dt_embedding_fwd': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr,
                                  _ptr, _ptr]),
    'dt_embedding_bwd_dense': (_c_int, [_ptr, _ptr, _c_int, _c_int, _ptr, _ptr]),
    'dt_embedding_drop_pass_units': (_c_i64, []),
    'dt_embedding_drop_fwd': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_f32, _ptr, ctypes.c_uint32,
                                       _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_embedding_drop_bwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _c_f32, _ptr, ctypes.c_uint32, _ptr, _ptr, _ptr,
                                       _ptr]),
    'dt_fm_fwd': (_c_int, [_ptr, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_fm_bwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_embed_fm_linear_fwd': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int,
                                        _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_embed_fm_linear_bwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _ptr, _ptr, _c_int, _c_int, _c_int,
                                        _ptr, _ptr]),
    'dt_bn_workspace_bytes': (_c_i64, [_c_int, _c_int]),
    'dt_bn_train_fwd': (_c_int, [_ptr, _c_int, _c_int, _ptr, _ptr, _c_f32, _c_f32, _c_f32, _ptr, _ptr, _ptr,
                                 _ptr, _ptr, _ptr, _ptr]),
    'dt_bn_infer_fwd': (_c_int, [_ptr, _c_int, _c_int, _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _ptr]),
    'dt_bn_train_bwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                 _ptr]),
    'dt_cross_workspace_bytes': (_c_i64, [_c_int, _c_int, _c_int]),
    'dt_cross_fwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr]),
    'dt_cross_bwd': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr,
                              _ptr, _ptr]),
    'dt_inner_product_fwd': (_c_int, [_ptr, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_inner_product_bwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_outer_product_fwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_outer_product_bwd': (_c_int, [_ptr, _ptr, _c_int, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr,
                                      _ptr]),
    'dt_cin_layer_fwd': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                  _c_int, _c_i64, _c_i64, _ptr, _ptr]),
    'dt_cin_layer_bwd': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                  _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_cin_bwd_workspace_bytes': (_c_i64, [_c_int] * 5),
    'dt_cin_pool': (_c_int, [_ptr, _c_i64, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_cin_pool_bwd': (_c_int, [_ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_cin_layer_bwd_ws': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                     _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_cin_bf16_workspace_bytes': (_c_i64, [_c_int, _c_int, _c_int]),
    'dt_cin_layer_fwd_bf16': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                       _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr]),
    'dt_cin_layer_bwd_bf16': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                       _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_cin_bf16x3_workspace_bytes': (_c_i64, [_c_int, _c_int, _c_int]),
    'dt_cin_layer_fwd_bf16x3': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                         _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr]),
    'dt_cin_layer_bwd_bf16x3': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                         _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_mha_core_fwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int, _c_f32, ctypes.c_uint32, _ptr,
                                 _ptr, _ptr, _ptr]),
    'dt_mha_core_bwd': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                 _c_f32, ctypes.c_uint32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_autoint_supported': (_c_int, [_c_int, _c_int, _c_int]),
    'dt_mha_core_supported': (_c_int, [_c_int, _c_int, _c_int, _c_int]),
    'dt_autoint_dropout_hash': (ctypes.c_uint32, [ctypes.c_uint32] * 5),
    'dt_autoint_dropout_threshold': (ctypes.c_uint32, [_c_f32]),
    'dt_autoint_fwd': (_c_int, [_ptr] * 9 + [_c_i64, _c_int, _c_int, _c_int, _c_f32, ctypes.c_uint32] + [_ptr] * 6 + [_c_int, _ptr]),
    'dt_autoint_bwd': (_c_int, [_ptr] * 11 + [_c_i64, _c_int, _c_int, _c_int, _c_f32, ctypes.c_uint32] + [_ptr] * 14 + [_c_int, _ptr]),
    'dt_autoint_fwd_bn': (_c_int, [_ptr] * 9 + [_c_i64, _c_int, _c_int, _c_int, _c_f32, ctypes.c_uint32, _ptr, _ptr, _c_f32, _c_f32]
                          + [_ptr] * 12 + [_c_int, _ptr]),
    'dt_autoint_fwd_bn_workspace_bytes': (_c_i64, [_c_i64, _c_int]),
    'dt_autoint_bwd_w': (_c_int, [_ptr] * 11 + [_c_i64, _c_int, _c_int, _c_int, _c_f32, ctypes.c_uint32] + [_ptr] * 19 + [_c_int, _ptr]),
    'dt_autoint_head_workspace_bytes': (_c_i64, [_c_i64, _c_int]),
    'dt_autoint_head_fwd': (_c_int, [_ptr] * 7 + [_c_i64, _c_int, _c_int, _ptr, _ptr]),
    'dt_autoint_head_bwd': (_c_int, [_ptr] * 7 + [_c_i64, _c_int, _c_int] + [_ptr] * 5),
    'dt_autoint_bwd_workspace_bytes': (_c_i64, [_c_i64, _c_int]),
    'dt_bn_train_bwd_stats': (_c_int, [_ptr, _ptr, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_adam_state_init': (_c_int, [_ptr, _c_f32, _c_f32, _c_f32, _c_int, _ptr]),
    'dt_adam_advance': (_c_int, [_ptr, _c_f32, _c_f32, _c_f32, _ptr]),
    'dt_adam_dense_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_f32, _c_f32, _c_f32, _c_f32,
                                    _ptr, _c_int, _c_f32, _ptr]),
    'dt_adam_multi_step': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _c_f32, _c_f32, _ptr, _c_int,
                                    _c_f32, _ptr]),
    'dt_adam_rows_slots': (_c_i64, [_c_i64]),
    'dt_adam_rows_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr, _c_i64, _ptr, _c_f32,
                                   _c_f32, _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32,
                                   _ptr]),
    'dt_adam_rows_step_seg': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr, _c_i64, _ptr, _c_f32,
                                   _c_f32, _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _ptr]),
    'dt_rows_merge_segments': (_c_int, [_ptr, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _ptr]),
    'dt_rows_compact': (_c_int, [_ptr, _ptr, _c_i64, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_f32, _c_i64,
                                 _ptr, _ptr, _ptr, _ptr]),
    'dt_bce_logits': (_c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    'dt_sgd_dense_step': (_c_int, [_ptr, _ptr, _c_i64, _c_f32, _ptr]),
    'dt_sgd_rows_step': (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32, _ptr]),
    # Adagrad / RMSprop: one slot per element; the rows forms take dt_adam_rows_step's merge arguments (csrc/optim_slots.hip)
    'dt_adagrad_dense_step': (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_f32, _c_f32, _ptr, _c_int, _ptr]),
    'dt_rmsprop_dense_step': (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_f32, _c_f32, _c_f32, _ptr, _c_int, _ptr]),
    'dt_adagrad_multi_step': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _ptr, _c_int, _ptr]),
    'dt_rmsprop_multi_step': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _c_f32, _ptr, _c_int, _ptr]),
    'dt_adagrad_rows_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr, _c_i64, _ptr, _c_f32, _c_f32,
                                      _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr]),
    'dt_rmsprop_rows_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr, _c_i64, _ptr, _c_f32,
                                      _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _ptr]),
    'dt_rmsprop_rows_materialize': (_c_int, [_ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_f32, _ptr, _ptr]),
    # momentum SGD / Adamax / Ftrl (csrc/optim_slots.hip): dt_adagrad_*'s arguments, the second slot behind the first, the
    # hyperparameters in place of (lr, eps): (lr, momentum, nesterov) / (lr, beta1, beta2, eps) / (lr, lr_power, l1, l2, l2_shrinkage)
    'dt_sgdm_dense_step': (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_f32, _c_f32, _c_int, _ptr, _c_int, _ptr]),
    'dt_sgdm_multi_step': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _c_int, _ptr, _c_int, _ptr]),
    'dt_sgdm_rows_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr, _c_i64, _ptr, _c_f32, _c_f32, _c_int,
                                   _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr]),
    'dt_adamax_dense_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_f32, _c_f32, _c_f32, _c_f32, _ptr, _c_int, _ptr]),
    'dt_adamax_multi_step': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _c_f32, _c_f32, _ptr, _c_int,
                                      _ptr]),
    'dt_adamax_rows_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr, _c_i64, _ptr, _c_f32, _c_f32,
                                     _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr]),
    'dt_ftrl_dense_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_f32, _c_f32, _c_f32, _c_f32, _c_f32, _ptr, _c_int,
                                    _ptr]),
    'dt_ftrl_multi_step': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _c_f32, _c_f32, _c_f32, _ptr, _c_int,
                                    _ptr]),
    'dt_ftrl_rows_step': (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr, _c_i64, _ptr, _c_f32, _c_f32,
                                   _c_f32, _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _ptr]),
    'dt_dense_supported': (_c_int, [_c_int] * 3),
    'dt_dense_workspace_bytes': (_c_i64, [_c_int] * 3),
    'dt_dense_geometry': (_c_int, [_c_int] * 4 + [_ptr]),       # N, K, M, product, int out[8]
    'dt_dense_fwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_dense_bwd': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr]),
    # the same Dense on K- and M-independent tiles, for the shapes dt_dense_supported refuses (csrc/dense_tiled.hip)
    'dt_dense_tiled_supported': (_c_int, [_c_int] * 3),
    'dt_dense_tiled_workspace_bytes': (_c_i64, [_c_int] * 3),
    'dt_dense_tiled_geometry': (_c_int, [_c_int] * 4 + [_ptr] * 3),
    'dt_dense_tiled_fwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_dense_tiled_bwd': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr]),
    # the tiled Dense on the bf16 matrix cores, operands split while they are staged (csrc/dense_tiled_x3.hip); mode: DT_DENSE_*
    'dt_dense_x3_supported': (_c_int, [_c_int] * 4),
    'dt_dense_x3_workspace_bytes': (_c_i64, [_c_int] * 4),
    'dt_dense_x3_geometry': (_c_int, [_c_int] * 5 + [_ptr] * 4),
    'dt_dense_x3_fwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _c_int, _ptr, _ptr]),
    'dt_dense_x3_bwd': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr, _c_int, _ptr,
                                 _ptr]),
    # FGCNN block for training: convolution + activation + max pooling, taps read from the map in LDS (csrc/fgcnn_train.hip)
    'dt_fg_conv_pool_supported': (_c_int, [_c_int] * 7),
    'dt_fg_conv_pool_workspace_bytes': (_c_i64, [_c_i64] + [_c_int] * 6),
    'dt_fg_conv_pool_geometry': (_c_int, [_c_int] * 7 + [_ptr, _ptr]),
    'dt_fg_conv_pool_fwd': (_c_int, [_ptr, _ptr, _ptr, _c_i64] + [_c_int] * 7 + [_ptr, _ptr, _ptr]),
    'dt_fg_conv_pool_bwd': (_c_int, [_ptr] * 5 + [_c_i64] + [_c_int] * 7 + [_ptr] * 5),
    'dt_afm_fwd': (_c_int, [_ptr] * 4 + [_c_int] * 5 + [_ptr] * 3),
    'dt_afm_bwd': (_c_int, [_ptr] * 6 + [_c_int] * 5 + [_ptr] * 5),
    'dt_bilinear_fwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_bilinear_bwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr]),
    'dt_field_pool_fwd': (_c_int, [_ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr]),
    'dt_field_pool_bwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_field_scale_fwd': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_field_scale_bwd': (_c_int, [_ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr]),
    'dt_deepfm_supported': (_c_int, [_c_int] * 6),
    'dt_deepfm_workspace_bytes': (_c_i64, [_c_int] * 4),
    'dt_deepfm_accum_floats': (_c_i64, [_c_int] * 3),
    'dt_deepfm_stamps_offset_floats': (_c_i64, [_c_int] * 4),
    'dt_deepfm_accum_offsets': (_c_int, [_c_int, _c_int, _c_int, _ptr]),
    'dt_deepfm_train_step': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int,
                                      _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr,
                                      _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_f32, _c_int, _c_int,
                                      _c_f32, _ptr, _c_f32, _ptr, _ptr]),
    'dt_deepfm_train_step_adam': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int,
                                           _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr,
                                           _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int,
                                           _c_f32, _ptr, _c_f32, _ptr, _ptr, _ptr, _c_int, _ptr, _c_f32, _c_f32, _c_f32, _c_f32,
                                           _ptr, _ptr, _ptr, _c_i64, _c_f32, _ptr, _ptr, _ptr, _ptr]),
    'dt_deepfm_step_chains': (_c_int, [_c_int] * 5),
    'dt_deepfm_dropout_hash': (ctypes.c_uint32, [ctypes.c_uint32] * 3),
    'dt_feed_gather': (_c_int, [_ptr, _c_i64, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_embedding_gather_owned': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int,
                                           _c_int, _ptr, _ptr, _ptr, _ptr]),
    'dt_deepfm_preelect': (_c_int, [_ptr, _c_int, _ptr, _ptr, _c_int, _c_int, _ptr, _ptr, _c_i64, _ptr]),
    'dt_deepfm_dedupe_slots': (_c_i64, [_c_int, _c_int]),
    'dt_deepfm_dedupe_bytes': (_c_i64, [_c_int, _c_int]),
    'dt_deepfm_dedupe_segments': (_c_int, [_c_int, _c_int, _ptr]),
    'dt_deepfm_dedupe_overflow_offset': (_c_i64, [_c_int, _c_int]),
    'dt_dcn_supported': (_c_int, [_c_int] * 7),
    'dt_dcn_workspace_bytes': (_c_i64, [_c_int] * 5),
    'dt_dcn_stamps_offset_floats': (_c_i64, [_c_int] * 5),
    'dt_dcn_accum_floats': (_c_i64, [_c_int] * 4),
    'dt_dcn_accum_offsets': (_c_int, [_c_int, _c_int, _c_int, _c_int, _ptr]),
    'dt_dcn_train_step': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int,
                                   _ptr, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32, _ptr, _c_f32, _ptr, _ptr]),
    'dt_dcn_train_step_adam': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int,
                                        _ptr, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _c_f32,
                                        _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                        _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32, _ptr, _c_f32, _ptr,
                                        _ptr, _ptr, _c_int, _ptr, _c_f32, _c_f32, _c_f32, _c_f32,
                                        _ptr, _ptr, _ptr, _c_i64, _c_f32, _ptr, _ptr, _ptr, _ptr]),
    # fused DeepFM / DCN inference (csrc/infer_x3.h)
    'dt_deepfm_infer_supported': (_c_int, [_c_int] * 6),
    'dt_dcn_infer_supported': (_c_int, [_c_int] * 7),
    'dt_deepfm_infer_workspace_bytes': (_c_i64, [_c_int] * 3),
    'dt_dcn_infer_workspace_bytes': (_c_i64, [_c_int] * 4),
    'dt_deepfm_infer_prepare': (_c_int, [_c_int, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _c_int, _c_int,
                                         _ptr, _ptr, _c_int, _c_int, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr,
                                         _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_dcn_infer_prepare': (_c_int, [_c_int, _c_int, _c_int, _ptr, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _c_int,
                                      _c_int, _ptr, _ptr, _c_int, _c_int, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr,
                                      _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_deepfm_infer': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr,
                                 _c_int, _ptr]),
    'dt_dcn_infer': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr,
                              _ptr, _c_int, _ptr]),
    # ... for every subset of {linear, fm_nets, dnn_nets}: dt_deepfm_infer*'s arguments with the DT_NET_* mask after Nd
    'dt_stack_infer_supported': (_c_int, [_c_int] * 7),
    'dt_stack_infer_workspace_bytes': (_c_i64, [_c_int] * 4),
    'dt_stack_infer_prepare': (_c_int, [_c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _c_int,
                                        _c_int, _ptr, _ptr, _c_int, _c_int, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr,
                                        _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_stack_infer': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr,
                                _ptr, _c_int, _ptr]),
    # one CIN layer's forward on a filter packed once (mode = DT_CIN_*)
    'dt_cin_fwd_supported': (_c_int, [_c_int] * 6),
    'dt_cin_packed_bytes': (_c_i64, [_c_int] * 4),
    'dt_cin_pack': (_c_int, [_c_int, _ptr, _c_int, _c_int, _c_int, _ptr, _ptr]),
    'dt_cin_layer_fwd_packed': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                         _c_i64, _c_i64, _ptr, _ptr]),
    # xDeepFM inference: prepare once, then tower / one call per CIN layer / head per batch (layer_sizes, cin_W, y: host arrays)
    'dt_xdeepfm_infer_supported': (_c_int, [_c_int] * 7 + [_ptr] + [_c_int] * 5),
    'dt_xdeepfm_infer_workspace_bytes': (_c_i64, [_c_int] * 4 + [_ptr, _c_int, _c_int]),
    'dt_xdeepfm_infer_prepare': (_c_int, [_c_int, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _c_int, _c_int,
                                          _ptr, _ptr, _c_int, _c_int, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr,
                                          _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _c_int, _ptr, _c_int, _c_int, _ptr, _ptr, _ptr,
                                          _ptr, _ptr]),
    'dt_xdeepfm_infer_tower': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr,
                                        _ptr, _c_int, _ptr]),
    'dt_xdeepfm_infer_cin': (_c_int, [_c_int, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _ptr, _c_int,
                                      _c_int, _ptr, _ptr, _ptr]),
    'dt_xdeepfm_infer_head': (_c_int, [_ptr, _ptr, _c_int, _c_int, _c_int, _c_int, _c_int, _ptr, _c_int, _c_int, _ptr, _ptr,
                                       _ptr, _c_int, _ptr]),
    # AutoInt inference: prepare once (per-layer HOST arrays of device pointers), then one launch per batch
    'dt_autoint_infer_supported': (_c_int, [_c_int] * 6),
    'dt_autoint_infer_workspace_bytes': (_c_i64, [_c_int] * 3),
    'dt_autoint_infer_prepare': (_c_int, [_c_int] * 3 + [_ptr] * 12 + [_c_f32, _ptr, _ptr, _ptr, _ptr]),
    'dt_autoint_infer': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr,
                                  _ptr, _ptr, _c_int, _c_int, _ptr]),
    # AFM inference ('afm_nets' alone or with 'linear' / 'fm_nets'): prepare once, then one launch per batch
    'dt_afm_infer_supported': (_c_int, [_c_int] * 6),
    'dt_afm_infer_workspace_bytes': (_c_i64, [_c_int] * 5),
    'dt_afm_infer_prepare': (_c_int, [_c_int] * 5 + [_ptr] * 9),
    'dt_afm_infer': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                              _ptr, _ptr, _ptr, _ptr, _c_int, _ptr]),
    # fused PNN inference (csrc/pnn_infer.hip): products = DT_PNN_* mask, kernel_type = DT_OP_KERNEL_*
    'dt_pnn_infer_supported': (_c_int, [_c_int] * 8),
    'dt_pnn_infer_workspace_bytes': (_c_i64, [_c_int] * 5),
    'dt_pnn_infer_prepare': (_c_int, [_c_int] * 5 + [_ptr] * 5 + [_c_f32, _ptr, _c_int, _c_int, _ptr, _ptr, _c_int, _c_int,
                                      _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr,
                                      _ptr, _ptr, _ptr]),
    'dt_pnn_infer': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _ptr, _ptr,
                              _ptr, _ptr, _c_int, _ptr]),
    # fused FiBiNet inference (csrc/fibi_infer.hip): bilinear_type = DT_BILINEAR_*, pooling_op = DT_FIBI_POOL_*
    'dt_fibi_infer_supported': (_c_int, [_c_int] * 9),
    'dt_fibi_infer_workspace_bytes': (_c_i64, [_c_int] * 5),
    'dt_fibi_infer_prepare': (_c_int, [_c_int] * 5 + [_ptr] * 6 + [_ptr, _c_int, _c_int, _ptr, _ptr, _c_int, _c_int, _ptr,
                                       _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr,
                                       _ptr, _ptr]),
    'dt_fibi_infer': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                               _ptr, _ptr, _ptr, _ptr, _c_int, _ptr]),
    # fused FGCNN inference (csrc/fgcnn_infer.hip): depth, then the blocks' filters / heights / pools / new_filters as HOST int
    # arrays; prepare takes HOST arrays of the blocks' device pointers; per batch conv / recomb per block, then tower
    'dt_fgcnn_infer_supported': (_c_int, [_c_int] * 7 + [_ptr] * 4),
    'dt_fgcnn_infer_workspace_bytes': (_c_i64, [_c_int] * 4 + [_ptr] * 4),
    'dt_fgcnn_infer_prepare': (_c_int, [_c_int] * 4 + [_ptr] * 8 + [_ptr, _c_int, _c_int, _ptr, _ptr, _c_int, _c_int, _ptr,
                                        _c_int, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr,
                                        _ptr, _ptr]),
    'dt_fgcnn_infer_conv': (_c_int, [_c_int, _ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_int]
                            + [_ptr] * 4 + [_ptr, _ptr, _ptr]),
    'dt_fgcnn_infer_recomb': (_c_int, [_c_int, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_int] + [_ptr] * 4 + [_ptr, _ptr, _ptr]),
    'dt_fgcnn_infer_tower': (_c_int, [_ptr, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_int, _c_int, _c_int]
                             + [_ptr] * 4 + [_ptr, _ptr, _ptr, _ptr, _c_int, _ptr]),
    # epoch metrics on the device (csrc/metrics.hip): stable radix sort, exact AUC counts, accuracy / MSE / MAE sums
    'dt_metric_sort_tile': (_c_int, []),
    'dt_metric_sort_workspace_bytes': (_c_i64, [_c_i64]),
    'dt_metric_sort_pairs': (_c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr]),
    'dt_metric_auc_workspace_bytes': (_c_i64, [_c_i64]),
    'dt_metric_auc': (_c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    'dt_metric_sums': (_c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr]),
    'dt_metric_argmax_hits': (_c_int, [_ptr, _ptr, _c_int, _c_i64, _c_int, _ptr, _ptr]),
    # ... log loss + precision / recall counts, MSLE / MAPE sums, top-k hits + categorical cross-entropy, AUC + average precision
    'dt_score_binary': (_c_int, [_ptr, _ptr, _c_int, _c_i64, _c_int, _ptr, _ptr]),
    'dt_score_regression': (_c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr]),
    'dt_score_categorical': (_c_int, [_ptr, _ptr, _c_int, _c_i64, _c_int, _c_int, _ptr, _ptr]),
    'dt_score_ranking_workspace_bytes': (_c_i64, [_c_i64]),
    'dt_score_ranking': (_c_int, [_ptr, _ptr, _c_i64, _ptr, _ptr, _ptr]),
    # keras.regularizers.L1L2 (csrc/regularizer.hip): HOST arrays of device pointers / sizes / coefficients, one per tensor
    'dt_reg_chunk': (_c_int, []),
    'dt_reg_penalty_workspace_bytes': (_c_i64, [_c_int, _ptr]),
    'dt_reg_penalty': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_reg_grad': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _ptr]),
    # the losses of a train step from the logits (csrc/loss.hip): kind = DT_LOSS_*, z, t, w (or NULL), rows, classes, gamma,
    # alpha, loss [1], dz (or NULL: value only), workspace, stream
    'dt_loss_workspace_bytes': (_c_i64, [_c_i64, _c_int]),
    'dt_loss': (_c_int, [_c_int, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr]),
    # Keras' regression losses from the model output (csrc/loss_reg.hip): kind = DT_LOSS_HUBER .. DT_LOSS_POISSON, p, t, w (or
    # NULL), rows, classes, delta, loss [1], dz (or NULL), workspace, stream
    'dt_loss_reg_workspace_bytes': (_c_i64, [_c_i64, _c_int]),
    'dt_loss_reg': (_c_int, [_c_int, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32, _ptr, _ptr, _ptr, _ptr]),
    # GHMCLoss.calc (csrc/loss_reg.hip): z, t, mask (or NULL), n, bins, momentum, float32(1 - momentum), acc_sum [bins] (updated
    # in place; NULL at momentum 0), loss [1], dz (or NULL), workspace, stream
    'dt_ghmc_workspace_bytes': (_c_i64, [_c_i64, _c_int]),
    'dt_ghmc': (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32, _c_f32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    # Activation -> (Dropout) of a tower cell in one launch each way (csrc/cell.hip): x, N, C, act (CELL_ACT_CODES), rate, the
    # DEVICE seed word, salt, out, stream / g, saved, saved_is_input, N, C, act, rate, seed, salt, dx, stream
    'dt_cell_dropout_hash': (ctypes.c_uint32, [ctypes.c_uint32] * 4),
    'dt_cell_dropout_threshold': (ctypes.c_uint32, [_c_f32]),
    'dt_cell_pass_elems': (_c_i64, []),
    'dt_cell_saves_input': (_c_int, [_c_int]),
    'dt_cell_fwd': (_c_int, [_ptr, _c_i64, _c_int, _c_int, _c_f32, _ptr, ctypes.c_uint32, _ptr, _ptr]),
    'dt_cell_bwd': (_c_int, [_ptr, _ptr, _c_int, _c_i64, _c_int, _c_int, _c_f32, _ptr, ctypes.c_uint32, _ptr, _ptr]),
    # gradient clipping (csrc/gradclip.hip): rows, values, n, D, V, out_rows, out_vals, count, ws, stream / count, g[], n[], sums,
    # ws, stream / out_rows, out_vals, n, D, count, row_offset, F, V, sums, ws, stream / mode (DT_CLIP_*), c, count, g[], n[],
    # sum_index[], sums, n_sums, norm_out, stream / mode, c, out_rows, out_vals, n, D, count, row_offset, F, V, sums, sum_base,
    # n_sums, norm_out, stream.  g / n / sum_index: HOST arrays
    'dt_rows_coalesce_chunk': (_c_int, []),
    'dt_rows_coalesce_workspace_bytes': (_c_i64, [_c_i64, _c_int]),
    'dt_rows_coalesce': (_c_int, [_ptr, _ptr, _c_i64, _c_int, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_grad_sumsq_workspace_bytes': (_c_i64, [_c_int, _ptr]),
    'dt_grad_sumsq': (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _ptr]),
    'dt_rows_field_sumsq': (_c_int, [_ptr, _ptr, _c_i64, _c_int, _ptr, _ptr, _c_int, _c_i64, _ptr, _ptr, _ptr]),
    'dt_grad_clip': (_c_int, [_c_int, _c_f32, _c_int, _ptr, _ptr, _ptr, _ptr, _c_int, _ptr, _ptr]),
    'dt_rows_clip': (_c_int, [_c_int, _c_f32, _ptr, _ptr, _c_i64, _c_int, _ptr, _ptr, _c_int, _c_i64, _ptr, _c_int, _c_int,
                              _ptr, _ptr]),
    # weight decay and the weights' moving average around any optimizer step (csrc/optim_stages.hip): state, steps_done, stream /
    # state, stream / count, p[], n[], weight_decay, lr, stream / count, p[], avg[], n[], momentum, state, stream (p / avg / n:
    # HOST arrays) / table, avg, stamp, rows, n, D, V, row_offset, field_on, F, decay, weight_decay, lr, momentum, state, stream /
    # table, avg, stamp, rows, n, D, V, momentum, state, stream / table, avg, stamp, V, D, momentum, state, stream
    'dt_stage_state_init': (_c_int, [_ptr, _c_int, _ptr]),
    'dt_stage_advance': (_c_int, [_ptr, _ptr]),
    'dt_decay_multi': (_c_int, [_c_int, _ptr, _ptr, _c_f32, _c_f32, _ptr]),
    'dt_ema_multi': (_c_int, [_c_int, _ptr, _ptr, _ptr, _c_f32, _ptr, _ptr]),
    'dt_rows_stage_pre': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_i64, _ptr, _ptr, _c_int, _c_int, _c_f32, _c_f32,
                                   _c_f32, _ptr, _ptr]),
    'dt_rows_stage_post': (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_i64, _c_f32, _ptr, _ptr]),
    'dt_ema_rows_materialize': (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_int, _c_f32, _ptr, _ptr]),
    # Keras' dense Adam result on a row-sparse table through per-row stamps (csrc/adam_exact.hip): table, m, v, slot_stride,
    # stamp, idx, idx_kind, row_offset, vocab, B, F, D, V, lr, beta1, beta2, eps, state, stream / table, m, v, slot_stride, stamp,
    # V, D, lr, beta1, beta2, eps, state, stream / stamp, rows, n, V, state, stream
    'dt_adam_exact_supported': (_c_int, [_c_int]),
    'dt_adam_rows_catchup': (_c_int, [_ptr, _ptr, _ptr, _c_int, _ptr, _ptr, _c_int, _ptr, _ptr, _c_int, _c_int, _c_int, _c_i64,
                                      _c_f32, _c_f32, _c_f32, _c_f32, _ptr, _ptr]),
    'dt_adam_rows_materialize': (_c_int, [_ptr, _ptr, _ptr, _c_int, _ptr, _c_i64, _c_int, _c_f32, _c_f32, _c_f32, _c_f32, _ptr,
                                          _ptr]),
    'dt_adam_rows_stamp': (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _ptr, _ptr]),
    # columns of a resident feed block permuted in place (csrc/feed_columns.hip): block, N, C, col0, width, perm, out, stream /
    # block, N, C, col0, width, buf, stream
    'dt_column_gather': (_c_int, [_ptr, _c_i64, _c_int, _c_int, _c_int, _ptr, _ptr, _ptr]),
    'dt_column_swap': (_c_int, [_ptr, _c_i64, _c_int, _c_int, _c_int, _ptr, _ptr]),
    # KernelSHAP on a resident feed (csrc/coalition.hip): x, bg, Nb, C, masks, S, M, s0, s1, group, group_host, out, stream /
    # out, nseg, Nb, O, ey, stream / P, masks, S, M, ey, fx, e0, R, O, phi, stream
    'dt_coalition_fill': (_c_int, [_ptr, _ptr, _c_i64, _c_int, _ptr, _c_i64, _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr]),
    'dt_coalition_mean': (_c_int, [_ptr, _c_i64, _c_i64, _c_int, _ptr, _ptr]),
    'dt_shap_solve': (_c_int, [_ptr, _ptr, _c_i64, _c_int, _ptr, _ptr, _ptr, _c_i64, _c_int, _ptr, _ptr]),
    # rows of a resident feed block gathered / scattered, the mean of K output buffers (csrc/feed_rows.hip): block, N, C, idx, n,
    # out, stream / block, N, C, idx, n, src, stream / parts_host, K, total, mode, out, stream
    'dt_rows_take': (_c_int, [_ptr, _c_i64, _c_int, _ptr, _c_i64, _ptr, _ptr]),
    'dt_rows_put': (_c_int, [_ptr, _c_i64, _c_int, _ptr, _c_i64, _ptr, _ptr]),
    'dt_ensemble_mean': (_c_int, [_ptr, _c_int, _c_i64, _c_int, _ptr, _ptr]),
    # the fitted preprocessor's transform on the device (csrc/prep_transform.hip): N, cols, cols_host, C, out_kind, out, stream
    'dt_prep_transform': (_c_int, [_c_i64, _ptr, _ptr, _c_int, _c_int, _ptr, _ptr]),
}

DT_IDX_F32, DT_IDX_I32 = 0, 1
DT_AI_F32, DT_AI_BF16, DT_AI_BF16X2 = 0, 1, 2
DT_STEP_LOSS_MSE = 0x10
DT_STEP_SKIP_FINISH, DT_STEP_FINISH_ONLY = 0x20, 0x40
DT_STEP_TOWER_X3 = 0x80
DT_STEP_PREELECTED = 0x100
DT_STEP_TOWER_BF16 = 0x200
DT_STEP_STAMPS = 0x400
DT_STEP_PREPARED = 0x800
DT_INFER_SIGMOID, DT_INFER_TOWER_BF16 = 0x1, 0x2
DT_NET_LINEAR, DT_NET_FM, DT_NET_DNN = 0x1, 0x2, 0x4
DT_NET_AFM = 0x8
DT_AFM_INFER_ROWS, DT_AFM_INFER_MAX_BLOCKS = 4, 1024
DT_PNN_INNER, DT_PNN_OUTER = 0x1, 0x2
DT_PNN_INFER_MAX_BLOCKS = 512
DT_BILINEAR_FIELD_INTERACTION, DT_BILINEAR_FIELD_EACH, DT_BILINEAR_FIELD_ALL = 0, 1, 2      # ops.BILINEAR_TYPES' codes
DT_FIBI_POOL_MEAN, DT_FIBI_POOL_MAX = 0, 1
DT_FIBI_INFER_MAX_BLOCKS = 512
DT_FGCNN_INFER_MAX_BLOCKS, DT_FGCNN_INFER_MAX_DEPTH = 512, 3
DT_CIN_F32, DT_CIN_BF16, DT_CIN_BF16X3 = 0, 1, 2
DT_XDEEPFM_MAX_LAYERS = 8
DT_AUTOINT_INFER_MAX_LAYERS, DT_AUTOINT_INFER_MAX_BLOCKS = 8, 256
DT_FEED_CURSOR_WORDS = 528          # 16 (1 + 32 ticket groups), csrc/embedding.hip kFeedGroups
DT_ACT_LINEAR, DT_ACT_RELU = 0, 1
DT_DENSE_X3, DT_DENSE_BF16 = 1, 2      # dt_dense_x3_*: split-bf16 (fp32 bars forward) / plain bf16
DT_METRIC_Y_LABELS, DT_METRIC_Y_ONEHOT = 0, 1
DT_METRIC_SUMS_BLOCKS, DT_METRIC_SUMS_WORDS = 256, 771      # dt_metric_sums' out: 3 result words + 3 per block
# dt_score_*' out: result words + that many per block; a thread per row up to DT_SCORE_THREAD_ROW_MAX_C classes
DT_SCORE_BLOCKS, DT_SCORE_THREAD_ROW_MAX_C = 256, 32
DT_SCORE_BINARY_WORDS, DT_SCORE_REGRESSION_WORDS, DT_SCORE_CATEGORICAL_WORDS, DT_SCORE_RANKING_WORDS = 1285, 514, 514, 262
DT_LOSS_BCE, DT_LOSS_CCE, DT_LOSS_MSE, DT_LOSS_MAE, DT_LOSS_BINARY_FOCAL, DT_LOSS_CATEGORICAL_FOCAL = 0, 1, 2, 3, 4, 5
DT_LOSS_HUBER, DT_LOSS_LOG_COSH, DT_LOSS_MSLE, DT_LOSS_MAPE, DT_LOSS_POISSON = 6, 7, 8, 9, 10     # dt_loss_reg's kinds
DT_LOSS_MAX_CLASSES = 4096
DT_GHMC_MAX_BINS = 256
DT_CLIP_VALUE, DT_CLIP_NORM, DT_CLIP_GLOBAL_NORM = 0, 1, 2
DT_FIELD_SUMSQ_PARTS = 32
# dt_prep_transform: source dtype codes, operations, flags, output kinds and the kernel's tile geometry (include/dt_hip.h)
DT_PREP_BOOL, DT_PREP_I8, DT_PREP_I16, DT_PREP_I32, DT_PREP_I64 = 0, 1, 2, 3, 4
DT_PREP_U8, DT_PREP_U16, DT_PREP_U32, DT_PREP_U64, DT_PREP_F32, DT_PREP_F64, DT_PREP_DTYPE_COUNT = 5, 6, 7, 8, 9, 10, 11
DT_PREP_LOOKUP, DT_PREP_CONT, DT_PREP_BIN, DT_PREP_COPY = 0, 1, 2, 3
DT_PREP_IMPUTE, DT_PREP_SCALE = 0x1, 0x2
DT_PREP_OUT_I32, DT_PREP_OUT_F32 = 0, 1
DT_PREP_TILE_ROWS, DT_PREP_CHUNK_COLS, DT_PREP_MAX_BLOCKS, DT_PREP_COL_BYTES = 256, 32, 1024, 80
# keras.activations names the CIN / AFM kernels fuse (include/dt_hip.h DT_ACT_*)
ACT_CODES = {None: 0, 'linear': 0, 'relu': 1, 'sigmoid': 2, 'tanh': 3, 'elu': 4, 'selu': 5, 'softplus': 6, 'softsign': 7,
             'exponential': 8}


# ... and the names dt_cell_fwd / dt_cell_bwd take (include/dt_hip.h DT_CELL_ACT_*): the table above plus the rest of Keras 3's
# element-wise set; 'swish' / 'silu' and 'hard_swish' / 'hard_silu' are one function each.  softmax is a row operation: not here.
DT_CELL_ACT_RELU6, DT_CELL_ACT_LEAKY_RELU, DT_CELL_ACT_SILU, DT_CELL_ACT_GELU = 9, 10, 11, 12
DT_CELL_ACT_MISH, DT_CELL_ACT_HARD_SIGMOID, DT_CELL_ACT_HARD_SILU, DT_CELL_ACT_COUNT = 13, 14, 15, 16
CELL_ACT_CODES = dict(ACT_CODES, relu6=9, leaky_relu=10, silu=11, swish=11, gelu=12, mish=13, hard_sigmoid=14, hard_silu=15,
                      hard_swish=15)


def act_code(name, what):
    if name not in ACT_CODES:
        raise ValueError(f'{what} activation {name!r}: the HIP kernels fuse {sorted(k for k in ACT_CODES if k)}')
    return ACT_CODES[name]
DT_OP_KERNEL = {'mat': 0, 'vec': 1, 'num': 2}

_lib = None


class DtHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle.  Raises if the HIP library was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'(hipcc --offload-arch=gfx950). deeptables_amd has no CPU fallback for the layers hot path.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().dt_last_error().decode('utf-8', 'replace')
        raise DtHipError(f'{what} failed with code {rc}: {msg}')


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise DtHipError('deeptables_amd kernels run on the GPU only (got a CPU tensor); '
                             'there is deliberately no CPU fallback for the hot path.')
