"""ctypes binding of libicsg3d_hip.so (include/icsg3d.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C icsg3d_amd/csrc``.  There
is NO CPU fallback: if the shared object is missing or fails to load, importing a compute entry
point raises ``IcsLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ICSG3D_LIB_PATH: another build of the same library (kernel A/B experiments: scripts/variants.sh)
LIB_PATH = os.environ.get("ICSG3D_LIB_PATH") or os.path.join(_HERE, "libicsg3d_hip.so")


class IcsLibraryError(RuntimeError):
    pass


class IcsError(RuntimeError):
    pass


class UnetConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("num_classes", C.c_int), ("d", C.c_int),
                ("max_batch", C.c_int), ("lr", C.c_float), ("loss_weight", C.c_float),
                ("pool_ties_all", C.c_int), ("bn_unbias", C.c_int), ("bce_from_logits", C.c_int)]


class VaeConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("cond_shape", C.c_int), ("latent_dim", C.c_int),
                ("filters", C.c_int * 4), ("d", C.c_int), ("max_batch", C.c_int), ("lr", C.c_float),
                ("alpha", C.c_float), ("beta", C.c_float), ("pm_layer_weights", C.c_float * 4),
                ("bn_unbias", C.c_int)]


class Structures(C.Structure):
    """ics_structures: site arrays [count][max_sites] (rows >= nsites[i] are never read)."""
    _fields_ = [("count", C.c_int), ("max_sites", C.c_int), ("nsites", C.POINTER(C.c_int32)),
                ("xyz", C.POINTER(C.c_double)), ("z", C.POINTER(C.c_double)), ("sigma", C.POINTER(C.c_double)),
                ("abc", C.POINTER(C.c_double))]


class TsneConfig(C.Structure):
    _fields_ = [("dim", C.c_int), ("capacity", C.c_int), ("n_components", C.c_int), ("perplexity", C.c_double),
                ("early_exaggeration", C.c_double), ("exaggeration_iter", C.c_int), ("max_iter", C.c_int),
                ("n_iter_check", C.c_int), ("n_iter_without_progress", C.c_int), ("min_grad_norm", C.c_double),
                ("learning_rate", C.c_double)]


class FeedConfig(C.Structure):
    """ics_feed_config (include/icsg3d.h)."""
    _fields_ = [("slots", C.c_int), ("x_parts", C.c_int), ("x_channels", C.c_int * 2), ("x_dtype", C.c_int * 2),
                ("label_kind", C.c_int)]


_F = C.POINTER(C.c_float)


class ConvLayerSrc(C.Structure):
    _fields_ = [("x", _F), ("scale", _F), ("shift", _F), ("C", C.c_int), ("up", C.c_int), ("act", C.c_int), ("bcast", C.c_int),
                ("dx", _F)]


class ConvLayerArgs(C.Structure):
    """ics_conv_layer (include/icsg3d.h)."""
    _fields_ = [("B", C.c_int), ("max_batch", C.c_int), ("S", C.c_int), ("taps", C.c_int), ("Cout", C.c_int),
                ("pre_act", C.c_int), ("has_bn", C.c_int), ("post_act", C.c_int), ("pad_input", C.c_int), ("nsrc", C.c_int),
                ("src", ConvLayerSrc * 2), ("w", _F), ("bias", _F), ("gamma", _F), ("beta", _F), ("dout", _F), ("y", _F),
                ("mean", _F), ("rstd", _F), ("scale", _F), ("shift", _F), ("moving_mean", _F), ("moving_var", _F),
                ("rows_per_block", C.c_int), ("blocks", C.c_int), ("dw", _F), ("dbias", _F), ("dgamma", _F), ("dbeta", _F),
                ("kernels", C.c_void_p), ("kernels_cap", C.c_int), ("ranks", C.c_int)]


class VaeLatentArgs(C.Structure):
    """ics_vae_latent (include/icsg3d.h)."""
    _fields_ = [("B", C.c_int), ("max_batch", C.c_int), ("latent", C.c_int), ("ncond", C.c_int), ("beta", C.c_float),
                ("h", _F), ("w_mean", _F), ("w_lv", _F), ("b_mean", _F), ("b_lv", _F), ("eps", _F), ("cond", _F), ("dzc", _F),
                ("mulv", _F), ("z", _F), ("zc", _F), ("dmulv", _F), ("dw_mean", _F), ("dw_lv", _F), ("dbias", _F), ("dh", _F)]


class ConvLinkLayer(C.Structure):
    _fields_ = [("Cout", C.c_int), ("w", _F), ("bias", _F), ("gamma", _F), ("beta", _F), ("y", _F), ("mean", _F), ("rstd", _F),
                ("scale", _F), ("shift", _F), ("dw", _F), ("dbias", _F), ("dgamma", _F), ("dbeta", _F)]


class ConvLinkArgs(C.Structure):
    """ics_conv_link (include/icsg3d.h)."""
    _fields_ = [("link", C.c_int), ("form", C.c_int), ("B", C.c_int), ("max_batch", C.c_int), ("S", C.c_int), ("C0", C.c_int),
                ("Cq", C.c_int), ("pool_ties_all", C.c_int), ("x0", _F), ("q", _F), ("P", ConvLinkLayer), ("K", ConvLinkLayer),
                ("L", ConvLinkLayer), ("dout", _F), ("dout_l", _F), ("pooled", _F), ("dy_p", _F), ("dx0", _F),
                ("sites", C.c_void_p), ("sites_cap", C.c_int), ("ranks", C.c_int)]


_U8 = C.POINTER(C.c_uint8)


class HeadLinkArgs(C.Structure):
    """ics_head_link (include/icsg3d.h)."""
    _fields_ = [("B", C.c_int), ("max_batch", C.c_int), ("S", C.c_int), ("C0", C.c_int), ("ncls", C.c_int), ("x0", _F),
                ("w", _F), ("bias", _F), ("gamma", _F), ("beta", _F), ("wsoft", _F), ("bsoft", _F), ("wsig", _F), ("bsig", _F),
                ("labels", _U8), ("loss_weight", C.c_float), ("class_weights", _F), ("bce_from_logits", C.c_int),
                ("want_grad", C.c_int), ("y", _F), ("mean", _F), ("rstd", _F), ("scale", _F), ("shift", _F), ("dz", _F),
                ("metrics", _F), ("sums", C.POINTER(C.c_double)), ("dwsoft", _F), ("dwsig", _F), ("dbias_head", _F),
                ("dw", _F), ("dbias", _F), ("dgamma", _F), ("dbeta", _F), ("dy_p", _F), ("dx0", _F), ("dy_in_place", C.c_int),
                ("sites", C.c_void_p), ("sites_cap", C.c_int), ("ranks", C.c_int)]


_I32 = C.POINTER(C.c_int32)
_I64 = C.POINTER(C.c_int64)
_H = C.c_void_p
_D = C.POINTER(C.c_double)
_ST = C.POINTER(Structures)

# name -> (restype, argtypes); every symbol include/icsg3d.h declares
SIGNATURES = {
    "ics_last_error": (C.c_char_p, []),
    "ics_version": (C.c_char_p, []),
    "ics_kernel_launches": (C.c_longlong, []),
    "ics_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ics_set_device": (C.c_int, [C.c_int]),
    "ics_device_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "ics_unet_create": (C.c_int, [C.POINTER(UnetConfig), C.POINTER(_H)]),
    "ics_unet_predict": (C.c_int, [_H, _F, C.c_int, _F, _F]),
    "ics_unet_predict_labels": (C.c_int, [_H, _F, C.c_int, C.c_float, _U8, _U8]),
    "ics_unet_train_step": (C.c_int, [_H, _F, _U8, C.c_int, _F]),
    "ics_unet_test_step": (C.c_int, [_H, _F, _U8, C.c_int, _F]),
    "ics_unet_upload_batch": (C.c_int, [_H, _F, _U8, C.c_int]),
    "ics_unet_train_step_resident": (C.c_int, [_H, _F]),
    "ics_vae_create": (C.c_int, [C.POINTER(VaeConfig), _H, C.POINTER(_H)]),
    "ics_vae_encode": (C.c_int, [_H, _F, _F, _F, C.c_int, _F, _F, _F]),
    "ics_unet_predict_resident": (C.c_int, [_H, C.c_int, C.c_float]),
    "ics_net_share_stream": (C.c_int, [_H, _H]),
    "ics_net_timer_start": (C.c_int, [_H]),
    "ics_net_timer_stop": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "ics_unet_metric_sums": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "ics_vae_decode": (C.c_int, [_H, _F, _F, C.c_int, _F]),
    "ics_vae_train_step": (C.c_int, [_H, _F, _F, _F, C.c_int, _F]),
    "ics_vae_test_step": (C.c_int, [_H, _F, _F, _F, C.c_int, _F]),
    "ics_vae_upload_batch": (C.c_int, [_H, _F, _F, _F, C.c_int]),
    "ics_vae_train_step_resident": (C.c_int, [_H, _F]),
    "ics_vae_decode_to_unet_labels": (C.c_int, [_H, _H, _F, _F, C.c_int, C.c_float, _U8, _U8, _F, _F]),
    "ics_vae_decode_to_unet_atoms": (C.c_int, [_H, _H, _F, _F, C.c_int, C.c_float, C.c_int, C.c_int, _U8, _U8, _F, _F,
                                               _I32, _I32, _I32, _I64]),
    "ics_op_segment_atoms": (C.c_int, [_U8, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _I32, _I32, _I32, _I64]),
    "ics_release_caches": (C.c_int, []),
    "ics_op_label_boxes": (C.c_int, [_I32, _I32, C.c_int, C.c_int, C.c_int, _I32, _I32, _I32]),
    "ics_op_watershed_split": (C.c_int, [_I32, _I32, _I32, C.c_int, C.c_int, _I32]),
    "ics_op_component_bounds": (C.c_int, [_I32, _I32, C.c_int, _I32, _I32, C.c_int, C.c_int, C.c_double, _I64]),
    "ics_op_voxelise": (C.c_int, [_ST, _I32, C.c_int, C.c_int, C.c_double, C.c_double, _D, _D, _D]),
    "ics_unet_voxelise_batch": (C.c_int, [_H, _ST, _I32, C.c_int, C.c_double, C.c_double]),
    "ics_vae_voxelise_batch": (C.c_int, [_H, _ST, _I32, C.c_int, C.c_double, C.c_double, _F, _F]),
    "ics_vae_reconstruct_resident_to_unet_atoms": (C.c_int, [_H, _H, C.c_float, C.c_int, C.c_int, _U8, _U8, _F, _F,
                                                            _I32, _I32, _I32, _I64]),
    "ics_op_match_emd": (C.c_int, [_D, _I32, _D, _I32, C.c_int, _D, _I32]),
    "ics_op_structure_screen": (C.c_int, [_I32, _I32, _D, _D, _D, C.c_int, C.c_double, _D, _D, _D, _D, _I32, _I32, _I32,
                                          _I32, _D, _I32]),
    "ics_op_structure_match": (C.c_int, [_I32, _I32, _D, _D, _I32, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                         _I32, _D, _I32, _I32, _D, _I32, _I32]),
    "ics_op_structure_symmetry": (C.c_int, [_I32, _I32, _D, _D, _I32, C.c_int, C.c_double, C.c_double, C.c_int,
                                            _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _D, _D, _I32, _I32, _D, _D, _D,
                                            _D]),
    "ics_op_structure_fingerprint": (C.c_int, [_I32, _I32, _D, _D, _I32, C.c_int, C.c_double, C.c_int, C.c_double,
                                               C.c_double, _D, _D, _I64, _D, _I32, _I32]),
    "ics_op_fingerprint_nearest": (C.c_int, [_D, _I32, C.c_int, C.c_int, C.c_int, _I32, _D, _I32, _D, _I32, _D, _D, _I64]),
    "ics_op_render_density": (C.c_int, [_F, C.c_int, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_float, C.c_float, _D,
                                        C.c_int, C.c_int, _F]),
    "ics_op_render_labels": (C.c_int, [_I32, C.c_int, C.c_int, _F, C.c_int, C.c_float, _D, C.c_int, C.c_int, _F]),
    "ics_op_render_atoms": (C.c_int, [_I32, _I32, _D, C.c_int, C.c_int, C.c_double, _F, C.c_int, _D, C.c_int, C.c_int, _F]),
    "ics_vae_render_resident": (C.c_int, [_H, C.c_int, C.c_int, C.c_float, C.c_float, _F, _D, C.c_int, C.c_int, _F]),
    "ics_op_render_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F,
                                      C.c_int, _F]),
    "ics_vae_render_slice_resident": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, C.c_int, _F]),
    "ics_unet_render_slice_resident": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, C.c_int, _F]),
    "ics_op_kde_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_H)]),
    "ics_op_kde_destroy": (C.c_int, [_H]),
    "ics_op_kde_append": (C.c_int, [_H, _F, C.c_int]),
    "ics_op_kde_append_vae": (C.c_int, [_H, _H, C.c_int, C.c_int]),
    "ics_op_kde_evaluate": (C.c_int, [_H, _D, C.c_int, _D, _D, _I32, C.POINTER(C.c_int)]),
    "ics_op_render_lines": (C.c_int, [_D, C.c_int, C.c_int, _D, _F, C.c_int, C.c_double, C.c_float, C.c_int, C.c_int, _F]),
    "ics_op_latent_path": (C.c_int, [_F, _F, C.c_int, C.c_int, _D, C.c_int, C.c_int, _F]),
    "ics_vae_interpolate": (C.c_int, [_H, _F, _F, _F, _F, _F, C.c_int, _D, C.c_int, C.c_int, _F, _F, _F]),
    "ics_vae_interpolate_to_unet_atoms": (C.c_int, [_H, _H, _F, _F, _F, _F, _F, C.c_int, _D, C.c_int, C.c_int, C.c_float,
                                                    C.c_int, C.c_int, _F, _F, _U8, _U8, _F, _F, _I32, _I32, _I32, _I64]),
    "ics_op_tsne_knn": (C.c_int, [_F, C.c_int, C.c_int, C.c_int, _I32, _D]),
    "ics_op_tsne_affinities": (C.c_int, [_D, C.c_int, C.c_int, C.c_double, _D]),
    "ics_op_tsne_create": (C.c_int, [C.POINTER(TsneConfig), C.POINTER(_H)]),
    "ics_op_tsne_destroy": (C.c_int, [_H]),
    "ics_op_tsne_append": (C.c_int, [_H, _F, C.c_int]),
    "ics_op_tsne_append_vae": (C.c_int, [_H, _H, C.c_int]),
    "ics_op_tsne_get_codes": (C.c_int, [_H, _F, C.c_int]),
    "ics_op_tsne_prepare": (C.c_int, [_H, _F, C.c_int, C.c_int, _D]),
    "ics_op_tsne_set_graph": (C.c_int, [_H, C.c_int, _I64, _I32, _D, _F, C.c_int, C.c_int]),
    "ics_op_tsne_get_graph": (C.c_int, [_H, _I64, _I32, _D, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ics_op_tsne_gradient": (C.c_int, [_H, _F, C.c_double, _F, _D]),
    "ics_op_tsne_run": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int)]),
    "ics_op_tsne_read": (C.c_int, [_H, _F, _D, _D, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ics_op_region_stats": (C.c_int, [_I32, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _I32]),
    "ics_net_destroy": (C.c_int, [_H]),
    "ics_net_sync": (C.c_int, [_H]),
    "ics_net_num_tensors": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "ics_net_tensor_info": (C.c_int, [_H, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "ics_net_set_tensor": (C.c_int, [_H, C.c_char_p, _F, C.c_size_t]),
    "ics_net_get_tensor": (C.c_int, [_H, C.c_char_p, _F, C.c_size_t]),
    "ics_net_get_grad": (C.c_int, [_H, C.c_char_p, _F, C.c_size_t]),
    "ics_net_get_activation": (C.c_int, [_H, C.c_char_p, _F, C.c_size_t]),
    "ics_net_get_bn_affine": (C.c_int, [_H, C.c_char_p, _F, _F, C.c_size_t]),
    "ics_net_check_canaries": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "ics_net_set_lr": (C.c_int, [_H, C.c_float]),
    "ics_net_reset_optimizer": (C.c_int, [_H]),
    "ics_net_num_params": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "ics_net_get_optimizer_state": (C.c_int, [_H, _F, _F, C.c_size_t, C.POINTER(C.c_int)]),
    "ics_net_set_optimizer_state": (C.c_int, [_H, _F, _F, C.c_size_t, C.c_int]),
    "ics_net_graph_probe": (C.c_int, [_H, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "ics_net_profile_enable": (C.c_int, [_H, C.c_int]),
    "ics_net_profile_filter": (C.c_int, [_H, C.c_char_p]),
    "ics_net_profile_count": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "ics_net_profile_row": (C.c_int, [_H, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ics_comm_unique_id": (C.c_int, [C.c_char_p]),
    "ics_net_comm_init": (C.c_int, [_H, C.c_int, C.c_int, C.c_char_p]),
    "ics_net_comm_allreduce_max": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "ics_net_comm_broadcast_state": (C.c_int, [_H, C.c_int]),
    "ics_net_set_sync_bn": (C.c_int, [_H, C.c_int]),
    "ics_net_comm_info": (C.c_int, [_H, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ics_op_unet_head": (C.c_int, [_F, _F, _F, _F, _F, _U8, C.c_size_t, C.c_int, C.c_float, C.c_int, C.c_int, _F, _F,
                                  C.POINTER(C.c_double)]),
    "ics_op_unet_metrics_from_sums": (C.c_int, [_D, _F]),
    "ics_op_unet_head_weighted": (C.c_int, [_F, _F, _F, _F, _F, _U8, C.c_size_t, C.c_int, C.c_float, C.c_int, C.c_int, _F,
                                           _F, C.POINTER(C.c_double), _F]),
    "ics_unet_set_class_weights": (C.c_int, [_H, _F, C.c_int]),
    "ics_unet_get_class_weights": (C.c_int, [_H, _F, C.c_int, C.POINTER(C.c_int)]),
    "ics_op_label_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_int, _I64, _I64]),
    "ics_op_confusion": (C.c_int, [C.c_void_p, C.c_int, _U8, _U8, C.c_size_t, C.c_int, _I64, _I64, _I64]),
    "ics_op_confusion_grid": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ics_unet_confusion_open": (C.c_int, [_H]),
    "ics_unet_confusion_reset": (C.c_int, [_H]),
    "ics_unet_confusion_step": (C.c_int, [_H, C.c_float]),
    "ics_unet_confusion_batch": (C.c_int, [_H, _F, _U8, C.c_int, C.c_float]),
    "ics_unet_confusion_read": (C.c_int, [_H, _I64, _I64, _I64, _I64]),
    "ics_op_atom_score": (C.c_int, [_D, _I32, _I32, _D, _I32, _I32, C.c_int, C.c_int, C.c_double, _I64, _I64, _I64, _I64,
                                    _I64, _I64, _I64, _I32, _I32, _D]),
    "ics_op_atom_score_volumes": (C.c_int, [_U8, _U8, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _I64,
                                            _I64, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _D]),
    "ics_op_atom_score_limits": (C.c_int, [C.POINTER(C.c_int)] * 4),
    "ics_unet_atom_score_open": (C.c_int, [_H, C.c_double, C.c_int, C.c_int]),
    "ics_unet_atom_score_reset": (C.c_int, [_H]),
    "ics_unet_atom_score_step": (C.c_int, [_H, C.c_float, C.c_int]),
    "ics_unet_atom_score_batch": (C.c_int, [_H, _F, _U8, C.c_int, C.c_float, C.c_int]),
    "ics_unet_atom_score_read": (C.c_int, [_H, _I64, _I64, _I64, _I64, _I64, _I64, _I64]),
    "ics_op_vae_loss": (C.c_int, [_F, C.c_int, C.c_int, _D, C.c_int, C.c_double, _D, C.POINTER(C.c_int), _D, _F, C.c_float,
                                  C.c_float, C.c_int, _D, _F]),
    "ics_op_vae_latent": (C.c_int, [C.POINTER(VaeLatentArgs)]),
    "ics_op_sqdiff": (C.c_int, [_F, _F, C.c_int, C.c_size_t, C.c_int, C.c_float, C.c_int, _F, _D]),
    "ics_op_up125_pool": (C.c_int, [_F, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    "ics_op_conv_layer": (C.c_int, [C.POINTER(ConvLayerArgs)]),
    "ics_op_conv_link": (C.c_int, [C.POINTER(ConvLinkArgs)]),
    "ics_op_head_link": (C.c_int, [C.POINTER(HeadLinkArgs)]),
    "ics_op_conv3d_forward": (C.c_int, [_F, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    "ics_op_conv3d_bench": (C.c_int, [C.c_int] * 8 + [_F]),
    "ics_op_conv3d_backward": (C.c_int, [_F, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F]),
    "ics_net_feed_open": (C.c_int, [_H, C.POINTER(FeedConfig)]),
    "ics_net_feed_close": (C.c_int, [_H]),
    "ics_net_feed_slot": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "ics_net_feed_submit": (C.c_int, [_H, C.c_int, C.c_int]),
    "ics_unet_train_step_fed": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int)]),
    "ics_unet_test_step_fed": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int)]),
    "ics_vae_train_step_fed": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int)]),
    "ics_vae_test_step_fed": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int)]),
    "ics_net_feed_metrics": (C.c_int, [_H, C.c_int, _F]),
    "ics_op_feed_pack": (C.c_int, [C.POINTER(FeedConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   _F, _U8]),
    "ics_net_feed_submit_rot": (C.c_int, [_H, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "ics_op_feed_pack_rot": (C.c_int, [C.POINTER(FeedConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32),
                                       C.c_int, C.c_int, C.c_int, _F, _U8]),
}

_lib = None


def load():
    """Load the shared library (once) and attach prototypes.  Raises IcsLibraryError loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IcsLibraryError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C icsg3d_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    # The engines run up to five HIP streams at once in one process (U-Net: compute + RCCL; DFC-VAE: compute + second stream +
    # RCCL).  The ROCm runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); two of OUR streams on
    # one queue serialise and the two-stream schedule of the DFC-VAE step loses 10 % instead of gaining 7 % (measured,
    # DESIGN.md section 10).  Read by the runtime when HIP initialises, i.e. at the first HIP call -- which this library makes.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)
    except OSError as e:  # pragma: no cover
        raise IcsLibraryError("failed to load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise IcsLibraryError("libicsg3d_hip.so does not export %s" % name) from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().ics_last_error()
        raise IcsError(msg.decode() if msg else "icsg3d call failed (%d)" % rc)


def fptr(a):
    return a.ctypes.data_as(_F) if a is not None else None


def u8ptr(a):
    return a.ctypes.data_as(_U8) if a is not None else None


def i32ptr(a):
    return a.ctypes.data_as(_I32) if a is not None else None


def f64ptr(a):
    return a.ctypes.data_as(_D) if a is not None else None


def i64ptr(a):
    return a.ctypes.data_as(_I64) if a is not None else None


def device_count():
    n = C.c_int(0)
    lib = load()
    if lib.ics_device_count(C.byref(n)) != 0:
        return 0
    return n.value
