"""The C ABI of libgeoadv.so (include/geoadv.h) as Python sees it, written once: the signature of every function, the mirrors of
the header's structs and the header's constants that the package uses.  tests/test_abi.py parses the header and holds all three to
it (and the argument count of every call site in the package to the table); _lib.lib() applies the signatures to the loaded
library, so that a call converts its arguments by the header's types, and one with an argument missing or a ctypes value of the
wrong width raises before it reaches C.

Signatures are "<return>:<arguments>", one letter per type:
    i int    f float    d double    q long long    Q unsigned long long    z size_t
    p any pointer or array parameter (handles, T *, T **, int plan[N]) -> c_void_p: it takes None, a Python int of any size,
      c_void_p, byref(...), ctypes arrays and typed pointers alike
    return only:  s const char *    v void"""
import ctypes as C

_TYPES = {"i": C.c_int, "f": C.c_float, "d": C.c_double, "q": C.c_longlong, "Q": C.c_ulonglong, "z": C.c_size_t, "p": C.c_void_p,
          "s": C.c_char_p, "v": None}

SIGNATURES = {      # in the header's order
    "geoadv_version": "i:",
    "geoadv_last_error": "s:",
    "geoadv_nn_distance": "i:iipipppppp",
    "geoadv_nn_distance_sym_workspace_floats": "z:iii",
    "geoadv_nn_distance_sym_is_screened": "i:iii",
    "geoadv_set_chamfer_screen": "i:i",
    "geoadv_nn_distance_sym": "i:iipippppppzp",
    "geoadv_nn_distance_lists_workspace_bytes": "z:iiii",
    "geoadv_nn_distance_lists": "i:iiipppppippppppppzp",
    "geoadv_chamfer_per_pc": "i:iiipppp",
    "geoadv_nn_distance_paired": "i:iippppppp",
    "geoadv_nn_distance_grad": "i:iipipppppppp",
    "geoadv_chamfer_matrix_workspace_floats": "z:iiii",
    "geoadv_chamfer_matrix": "i:iiiippppzp",
    "geoadv_approx_match_temp_floats": "z:iii",
    "geoadv_approx_match": "i:iiippppp",
    "geoadv_approx_match_mode": "i:iiiippppp",
    "geoadv_emd_sparse_levels": "i:i",
    "geoadv_match_cost": "i:iiippppp",
    "geoadv_match_cost_workspace_floats": "z:iii",
    "geoadv_match_cost_ws": "i:iiipppppzp",
    "geoadv_emd_cost_grad1_temp_floats": "z:iii",
    "geoadv_emd_cost_grad1": "i:iiipppppp",
    "geoadv_emd_cost_grad1_mode": "i:iiiipppppp",
    "geoadv_match_cost_grad": "i:iiipppppp",
    "geoadv_query_ball_point": "i:iiifippppp",
    "geoadv_selection_sort": "i:iiiipppp",
    "geoadv_group_point": "i:iiiiipppp",
    "geoadv_group_point_grad": "i:iiiiipppp",
    "geoadv_group_point_grad_workspace_bytes": "z:iiiii",
    "geoadv_group_point_grad_ws": "i:iiiiippppzp",
    "geoadv_knn_point": "i:iiiippppp",
    "geoadv_knn_dists": "i:iiippp",
    "geoadv_knn_workspace_bytes": "z:iiii",
    "geoadv_knn_point_ws": "i:iiiiipppppzp",
    "geoadv_knn_dists_ws": "i:iiiipppzp",
    "geoadv_knn_grid_mode": "i:i",
    "geoadv_farthest_point_sample": "i:iipipipppp",
    "geoadv_farthest_point_sample_plan": "i:iippp",
    "geoadv_outlier_filter": "i:iippiifppppp",
    "geoadv_sor_filter": "i:iippiidpppppp",
    "geoadv_random_drop": "i:iipiQQQppp",
    "geoadv_knn_outlier_loss_workspace_bytes": "z:iii",
    "geoadv_knn_outlier_loss": "i:iiiidppppppppzp",
    "geoadv_debug_knn_outlier_loss_launch": "i:iiidppppzp",
    "geoadv_critical_split": "i:iiippppppppp",
    "geoadv_sort_axes": "i:iipppip",
    "geoadv_batch_gather": "i:iipqpppppp",
    "geoadv_normalize_clouds": "i:iiippp",
    "geoadv_augment_batch": "i:iipqipppppp",
    "geoadv_latent_dist_matrix": "i:iiipppp",
    "geoadv_ae_create": "i:pp",
    "geoadv_ae_destroy": "v:p",
    "geoadv_set_default_encoder_arith": "i:i",
    "geoadv_ae_set_encoder_arith": "i:pi",
    "geoadv_ae_encoder_arith": "i:p",
    "geoadv_ae_status": "i:pp",
    "geoadv_ae_workspace_bytes": "z:pi",
    "geoadv_ae_critical": "i:pippppp",
    "geoadv_ae_forward": "i:pippppp",
    "geoadv_ae_decode": "i:pipppp",
    "geoadv_cls_create": "i:pp",
    "geoadv_cls_destroy": "v:p",
    "geoadv_cls_workspace_bytes": "z:pii",
    "geoadv_cls_forward": "i:piippppppp",
    "geoadv_cls_input_grad_workspace_bytes": "z:pii",
    "geoadv_cls_input_grad": "i:piippifpppppp",
    "geoadv_rotate_y": "i:iipddpp",
    "geoadv_cls_evaluate_workspace_bytes": "z:pii",
    "geoadv_cls_evaluate": "i:piippippppppp",
    "geoadv_cls_trainer_create": "i:ppp",
    "geoadv_cls_trainer_destroy": "v:p",
    "geoadv_cls_trainer_set_slots": "i:pppff",
    "geoadv_cls_trainer_step": "i:pppppp",
    "geoadv_cls_trainer_buffers": "i:pppp",
    "geoadv_cls_trainer_layout": "i:ppp",
    "geoadv_cls_trainer_counters": "i:pppp",
    "geoadv_cls_trainer_state": "i:piipp",
    "geoadv_atlas_create": "i:pppp",
    "geoadv_atlas_destroy": "v:p",
    "geoadv_atlas_workspace_bytes": "z:pii",
    "geoadv_atlas_forward": "i:piippppp",
    "geoadv_fold_create": "i:pp",
    "geoadv_fold_destroy": "v:p",
    "geoadv_fold_workspace_bytes": "z:pii",
    "geoadv_fold_graph": "i:piipppppp",
    "geoadv_fold_forward": "i:piipiQqppppppp",
    "geoadv_fold_trainer_create": "i:ppp",
    "geoadv_fold_trainer_destroy": "v:p",
    "geoadv_fold_trainer_set_slots": "i:ppp",
    "geoadv_fold_trainer_step": "i:ppipppp",
    "geoadv_fold_trainer_buffers": "i:pppp",
    "geoadv_fold_trainer_layout": "i:ppp",
    "geoadv_fold_trainer_counters": "i:ppp",
    "geoadv_fold_trainer_state": "i:piipp",
    "geoadv_fold_train_pool": "i:iiippppp",
    "geoadv_fold_train_pool_grad": "i:iiippppppp",
    "geoadv_fold_train_gmax": "i:iiipppppp",
    "geoadv_atlas_trainer_create": "i:pppp",
    "geoadv_atlas_trainer_destroy": "v:p",
    "geoadv_atlas_trainer_set_slots": "i:ppp",
    "geoadv_atlas_trainer_set_learning_rate": "i:pfi",
    "geoadv_atlas_trainer_step": "i:ppippp",
    "geoadv_atlas_trainer_buffers": "i:pppp",
    "geoadv_atlas_trainer_layout": "i:ppp",
    "geoadv_atlas_trainer_counters": "i:ppp",
    "geoadv_atlas_trainer_state": "i:piipp",
    "geoadv_train_gemm_partial_floats": "z:",
    "geoadv_train_gemm": "i:ipqqqpqqqpqqpqiiiipzpp",
    "geoadv_attack_create": "i:ppp",
    "geoadv_attack_destroy": "v:p",
    "geoadv_attack_set_inputs": "i:pppppp",
    "geoadv_attack_init_pert": "i:ppip",
    "geoadv_attack_run": "i:piiipp",
    "geoadv_attack_get_best": "i:pppppp",
    "geoadv_attack_set_source_search": "i:pi",
    "geoadv_attack_status": "i:pp",
    "geoadv_attack_peek": "i:ppppppppppp",
    "geoadv_attack_test_loss_form": "i:pi",
    "geoadv_attack_test_loss_state": "i:ppppppp",
    "geoadv_attack_test_plan": "i:pppp",
    "geoadv_debug_chamfer_sym_plan": "i:pp",
    "geoadv_debug_chamfer_sym_workspace_floats": "z:iiii",
    "geoadv_debug_h2_split": "i:pipppp",
    "geoadv_debug_emd_sparse_state": "i:iiiippp",
    "geoadv_attack_search_state": "i:pppp",
    "geoadv_attack_set_recon_lists": "i:pi",
    "geoadv_attack_list_state": "i:ppp",
    "geoadv_trainer_create": "i:ppp",
    "geoadv_trainer_destroy": "v:p",
    "geoadv_trainer_step": "i:pppppp",
    "geoadv_trainer_forward_backward": "i:pppppp",
    "geoadv_trainer_apply": "i:pfp",
    "geoadv_trainer_set_world": "i:pi",
    "geoadv_trainer_num_phases": "i:",
    "geoadv_trainer_run_phase": "i:pippp",
    "geoadv_trainer_exchange": "i:pipp",
    "geoadv_trainer_fetch": "i:pppp",
    "geoadv_trainer_buffers": "i:pppp",
    "geoadv_trainer_layout": "i:pp",
    "geoadv_trainer_state": "i:piipp",
    "geoadv_trainer_export": "i:ppp",
    "geoadv_attack_profile": "i:pi",
    "geoadv_attack_profile_read": "i:pipp",
    "geoadv_attack_markers": "i:pi",
    "geoadv_attack_profile_stride": "i:pi",
}


def ctypes_signature(name):
    """(restype, argtypes) of one function of the table."""
    ret, _, args = SIGNATURES[name].partition(":")
    return _TYPES[ret], tuple(_TYPES[a] for a in args)


# ---- constants (the header's names and values) ------------------------------------------------------------------------------------
GEOADV_OK, GEOADV_EINVAL = 0, 1
GEOADV_EMD_FAST, GEOADV_EMD_REFERENCE, GEOADV_EMD_DENSE_LEVELS = 0, 1, 0x100
GEOADV_KNN_AUTO, GEOADV_KNN_ALL_POINTS, GEOADV_KNN_GRID, GEOADV_KNN_GRID_SHELLS = 0, 1, 2, 3
GEOADV_KNN_LOSS_SURFACE = 0x100
GEOADV_FPS_AUTO, GEOADV_FPS_WORKGROUP, GEOADV_FPS_WAVE = 0, 1, 2
GEOADV_NORMALIZE_IDENTITY, GEOADV_NORMALIZE_UNIT_BALL, GEOADV_NORMALIZE_BOUNDING_BOX = 0, 1, 2
GEOADV_AUGMENT_RECORD = 45
GEOADV_ENC_LAYERS, GEOADV_DEC_LAYERS = 5, 3
GEOADV_ENC_ARITH_AUTO, GEOADV_ENC_ARITH_F32, GEOADV_ENC_ARITH_BF16X3, GEOADV_ENC_ARITH_F16X2 = -1, 0, 1, 2
GEOADV_CLS_LAYERS = 20
GEOADV_CLS_LOSS_XENT, GEOADV_CLS_LOSS_CW_TARGETED, GEOADV_CLS_LOSS_CW_UNTARGETED = 0, 1, 2
GEOADV_CLS_OPT_ADAM, GEOADV_CLS_OPT_MOMENTUM = 0, 1
(GEOADV_CLS_STATE_BN_MEAN, GEOADV_CLS_STATE_BN_VAR, GEOADV_CLS_STATE_MOVING_MEAN, GEOADV_CLS_STATE_MOVING_VAR,
 GEOADV_CLS_STATE_DROPOUT_MASK, GEOADV_CLS_STATE_POOL_ARGMAX, GEOADV_CLS_STATE_T1, GEOADV_CLS_STATE_T2, GEOADV_CLS_STATE_LOGITS,
 GEOADV_CLS_STATE_SLOT1, GEOADV_CLS_STATE_SLOT2, GEOADV_CLS_STATE_PRE_BN, GEOADV_CLS_STATE_BN_INV, GEOADV_CLS_STATE_BN_SHIFT) = range(14)
GEOADV_ATLAS_ENC_LAYERS, GEOADV_ATLAS_MAX_DEC_LAYERS = 5, 7
GEOADV_FOLD_ENC_LAYERS, GEOADV_FOLD_DEC_LAYERS = 7, 6
GEOADV_FOLD_PICKS_GIVEN, GEOADV_FOLD_PICKS_DEVICE = 0, 1
(GEOADV_FOLD_STATE_BN_MEAN, GEOADV_FOLD_STATE_BN_VAR, GEOADV_FOLD_STATE_RUNNING_MEAN, GEOADV_FOLD_STATE_RUNNING_VAR,
 GEOADV_FOLD_STATE_BN_INV, GEOADV_FOLD_STATE_BN_SHIFT, GEOADV_FOLD_STATE_PRE_BN, GEOADV_FOLD_STATE_POOL_WINNER,
 GEOADV_FOLD_STATE_GMAX_ROW, GEOADV_FOLD_STATE_HIDDEN, GEOADV_FOLD_STATE_PICKS, GEOADV_FOLD_STATE_COLS, GEOADV_FOLD_STATE_COV,
 GEOADV_FOLD_STATE_CODE, GEOADV_FOLD_STATE_MID, GEOADV_FOLD_STATE_RECON, GEOADV_FOLD_STATE_CHAMFER_IDX, GEOADV_FOLD_STATE_SLOT1,
 GEOADV_FOLD_STATE_SLOT2) = range(19)
(GEOADV_ATLAS_STATE_BN_MEAN, GEOADV_ATLAS_STATE_BN_VAR, GEOADV_ATLAS_STATE_RUNNING_MEAN, GEOADV_ATLAS_STATE_RUNNING_VAR,
 GEOADV_ATLAS_STATE_BN_INV, GEOADV_ATLAS_STATE_BN_SHIFT, GEOADV_ATLAS_STATE_PRE_BN, GEOADV_ATLAS_STATE_GMAX_ROW,
 GEOADV_ATLAS_STATE_TEMPLATE, GEOADV_ATLAS_STATE_LATENT, GEOADV_ATLAS_STATE_RECON, GEOADV_ATLAS_STATE_CHAMFER_IDX,
 GEOADV_ATLAS_STATE_SLOT1, GEOADV_ATLAS_STATE_SLOT2) = range(14)
GEOADV_LOSS_ADV_CHAMFER, GEOADV_LOSS_ADV_LATENT = 0, 1
GEOADV_LOSS_DIST_CHAMFER, GEOADV_LOSS_DIST_PERT = 0, 1
GEOADV_ENC_BWD_AUTO, GEOADV_ENC_BWD_MASKED, GEOADV_ENC_BWD_JACOBIAN = 0, 1, 2
GEOADV_CHAMFER_AUTO, GEOADV_CHAMFER_TWO_SCAN, GEOADV_CHAMFER_SYMMETRIC = 0, 1, 2
GEOADV_RECON_LISTS_ADAPTIVE, GEOADV_RECON_LISTS_OFF, GEOADV_RECON_LISTS_PINNED = 0, 1, 2
(GEOADV_LIST_STATE_ON, GEOADV_LIST_STATE_ANCHORS, GEOADV_LIST_STATE_LIST_ITERATIONS, GEOADV_LIST_STATE_CERTIFIED,
 GEOADV_LIST_STATE_REFUSED, GEOADV_LIST_STATE_UNLISTED, GEOADV_LIST_STATE_HANDED_BACK, GEOADV_LIST_STATE_FLAGGED,
 GEOADV_LIST_STATE_PERIOD, GEOADV_LIST_STATE_COUNT) = range(10)
GEOADV_PLAN_COUNT = 9
GEOADV_TRAIN_LOSS_CHAMFER, GEOADV_TRAIN_LOSS_EMD = 0, 1
(GEOADV_TRAIN_STATE_ACT, GEOADV_TRAIN_STATE_BN_MEAN, GEOADV_TRAIN_STATE_BN_INV_STD, GEOADV_TRAIN_STATE_BN_SCALE,
 GEOADV_TRAIN_STATE_BN_SHIFT, GEOADV_TRAIN_STATE_IDX1, GEOADV_TRAIN_STATE_IDX2, GEOADV_TRAIN_STATE_POOL_MAX,
 GEOADV_TRAIN_STATE_POOL_TIES, GEOADV_TRAIN_STATE_DEC1, GEOADV_TRAIN_STATE_DEC2) = range(11)
(GEOADV_PROF_ENCODER_FWD, GEOADV_PROF_DECODER_FWD, GEOADV_PROF_CHAMFER_FWD, GEOADV_PROF_LOSS_GRAD, GEOADV_PROF_DECODER_BWD,
 GEOADV_PROF_ENCODER_BWD, GEOADV_PROF_ADAM, GEOADV_PROF_COUNT) = range(8)


# ---- struct mirrors: the header's members, in order -------------------------------------------------------------------------------
def _ptrs(count, *names):
    return [(n, C.c_void_p * count) for n in names]


class BatchAugment(C.Structure):
    """geoadv_batch_augment (include/geoadv.h): the noise generator's key (seed, counter, slot_offset), the noise (mu, sigma,
    clip; sigma 0 = none, clip <= 0 = unclamped) and the order of noise and rotation.  rot_count is filled in by batch_gather."""
    _fields_ = [("seed", C.c_ulonglong), ("counter", C.c_ulonglong), ("slot_offset", C.c_int), ("noise_mu", C.c_float),
                ("noise_sigma", C.c_float), ("noise_clip", C.c_float), ("rot_count", C.c_int), ("rotate_first", C.c_int)]


class CloudAugment(C.Structure):
    """geoadv_cloud_augment (include/geoadv.h): the generator's key (seed, counter, slot_offset), sample (points drawn with
    replacement) and the Augmenter's operators: rot_axes / flip_axes are bit sets of the axes, rot_3d / scale / translate
    switches.  The ranges default to the reference's: range_rot 360, scale 0.75 .. 1.25, translate_scale 0.03."""
    _fields_ = [("seed", C.c_ulonglong), ("counter", C.c_ulonglong), ("slot_offset", C.c_int), ("sample", C.c_int),
                ("rot_axes", C.c_int), ("range_rot", C.c_float), ("rot_3d", C.c_int), ("scale", C.c_int), ("scale_min", C.c_float),
                ("scale_max", C.c_float), ("flip_axes", C.c_int), ("translate", C.c_int), ("translate_scale", C.c_float)]
    DEFAULTS = dict(range_rot=360.0, scale_min=0.75, scale_max=1.25, translate_scale=0.03)


class AEWeights(C.Structure):
    _fields_ = [("n_points", C.c_int), ("enc_dims", C.c_int * (GEOADV_ENC_LAYERS + 1)), ("dec_dims", C.c_int * (GEOADV_DEC_LAYERS + 1))] + \
               _ptrs(GEOADV_ENC_LAYERS, "enc_w", "enc_b", "bn_gamma", "bn_beta", "bn_mean", "bn_var") + \
               _ptrs(GEOADV_DEC_LAYERS, "dec_w", "dec_b")


class ClsWeights(C.Structure):
    """geoadv_cls_weights: HOST pointers (NULL where a layer has no such array)."""
    _fields_ = [("num_classes", C.c_int)] + _ptrs(GEOADV_CLS_LAYERS, "w", "b", "gamma", "beta", "mean", "var")


class ClsTrainConfig(C.Structure):
    _fields_ = [("batch", C.c_int), ("n_points", C.c_int), ("optimizer", C.c_int), ("learning_rate", C.c_float),
                ("momentum", C.c_float), ("decay_step", C.c_int), ("decay_rate", C.c_float), ("initial_step", C.c_int),
                ("dropout_seed", C.c_int)]


class AtlasConfig(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("nb_primitives", "points_per_primitive", "dim_template", "bottleneck_size",
                                       "hidden_neurons", "num_layers", "activation", "decoder_bn")]


class AtlasWeights(C.Structure):
    _fields_ = _ptrs(GEOADV_ATLAS_ENC_LAYERS, "enc_w", "enc_b", "enc_gamma", "enc_beta", "enc_mean", "enc_var") + \
               _ptrs(GEOADV_ATLAS_MAX_DEC_LAYERS, "dec_w", "dec_b", "dec_gamma", "dec_beta", "dec_mean", "dec_var")


class FoldWeights(C.Structure):
    _fields_ = _ptrs(GEOADV_FOLD_ENC_LAYERS, "enc_w", "enc_b", "enc_gamma", "enc_beta", "enc_mean", "enc_var") + \
               _ptrs(GEOADV_FOLD_DEC_LAYERS, "dec_w", "dec_b")


class FoldTrainConfig(C.Structure):
    _fields_ = [("batch", C.c_int), ("n_points", C.c_int), ("learning_rate", C.c_float), ("weight_decay", C.c_float),
                ("seed", C.c_longlong), ("initial_step", C.c_longlong), ("initial_ordinal", C.c_longlong)]


class AtlasTrainConfig(C.Structure):
    _fields_ = [("batch", C.c_int), ("n_points", C.c_int), ("points_per_primitive", C.c_int), ("learning_rate", C.c_float),
                ("seed", C.c_longlong), ("initial_step", C.c_longlong), ("initial_tracked", C.c_longlong)]


class AttackConfig(C.Structure):
    _fields_ = [("batch", C.c_int), ("loss_adv_type", C.c_int), ("loss_dist_type", C.c_int),
                ("max_point_pert_weight", C.c_float), ("max_point_dist_weight", C.c_float),
                ("learning_rate", C.c_float), ("emd_weight", C.c_float), ("all_pairs_source_dist", C.c_int),
                ("emd_weight_mode", C.c_int), ("recompute_backward", C.c_int), ("encoder_backward", C.c_int),
                ("separate_adam", C.c_int), ("chamfer_kernel", C.c_int), ("recon_lists", C.c_int),
                ("knn_rule", C.c_int), ("knn_thresh", C.c_float),
                ("knn_weight", C.c_float), ("knn_k", C.c_int), ("knn_alpha", C.c_float), ("loss_in_scan", C.c_int)]


class TrainConfig(C.Structure):
    _fields_ = [("batch", C.c_int), ("learning_rate", C.c_float), ("bn_decay", C.c_float), ("loss", C.c_int),
                ("max_workgroups", C.c_int)]


STRUCTS = {"geoadv_batch_augment": BatchAugment, "geoadv_cloud_augment": CloudAugment, "geoadv_ae_weights": AEWeights,
           "geoadv_cls_weights": ClsWeights, "geoadv_cls_train_config": ClsTrainConfig, "geoadv_atlas_config": AtlasConfig,
           "geoadv_atlas_weights": AtlasWeights, "geoadv_fold_weights": FoldWeights, "geoadv_fold_train_config": FoldTrainConfig,
           "geoadv_atlas_train_config": AtlasTrainConfig, "geoadv_attack_config": AttackConfig, "geoadv_train_config": TrainConfig}
