"""ctypes binding of the C ABI declared in include/nint.h.

The HIP library is the product: if ``libnint_hip.so`` is missing or cannot be loaded this
module raises -- there is no CPU or eager-PyTorch fallback anywhere in the package."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnint_hip.so")     # the one product library; nothing in the environment can swap it

NINT_F32, NINT_BF16 = 0, 1
NINT_OK, NINT_E_ARG, NINT_E_SHAPE, NINT_E_LDS, NINT_E_ALIGN = 0, -1, -2, -3, -4
NINT_MAX_LAYERS = 8
NINT_VERSION = 113     # include/nint.h NINT_VERSION: the library this binding was written against
NINT_LOSS_SCRATCH_FLOATS = 8194
NINT_LOSS_SPEC_SCRATCH_FLOATS = 10242     # the _spec loss entries: five doubles per workgroup
NINT_LOSS_STATS = 8
NINT_SKILL_PIX, NINT_SKILL_SAMPLE, NINT_SKILL_MAX_N = 5, 8, 64
NINT_ENS_PIX, NINT_ENS_SAMPLE, NINT_ENS_MAX_N, NINT_ENS_MAX_M = 7, 8, 64, 64
NINT_ENS_LOSS_OUT = 4     # nint_ens_loss's ens_out: SA, SD, SV, cnt
NINT_SPEC_PLANES, NINT_SPEC_MAX_W, NINT_SPEC_MAX_N = 5, 512, 64     # nint_spec_accum: YY, PP, CR, CI, SS per (slot, output, k)
NINT_GRAD_NORM_BLOCKS = 256
NINT_OPT_STATE = 16
NINT_MAX_OPT_GROUPS = 2 * NINT_MAX_LAYERS + 2
# nint_adam_flat_guarded's state (include/nint.h): counters, running norm figures, then this call's scalars
(NINT_OPT_APPLIED, NINT_OPT_SKIPPED, NINT_OPT_CLIPPED, NINT_OPT_CALLS, NINT_OPT_SUM_NORM, NINT_OPT_FINITE, NINT_OPT_MAX_NORM,
 NINT_OPT_S, NINT_OPT_NORM, NINT_OPT_COEF, NINT_OPT_SCALE, NINT_OPT_STEP_SIZE, NINT_OPT_SQRT_BC2, NINT_OPT_APPLY) = range(14)

vp = C.c_void_p


class NintGeom(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("P", C.c_int32), ("Hh", C.c_int32), ("Wh", C.c_int32)]


class NintLayer(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cxp", C.c_int32), ("Ch", C.c_int32), ("Ch16", C.c_int32), ("Chp", C.c_int32),
                ("k", C.c_int32), ("tile_rows", C.c_int32), ("xfold", C.c_int32), ("wide", C.c_int32),
                ("Wf", vp), ("Wd", vp), ("bias_p", vp)]


class NintSeq(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("L", C.c_int32),
                ("need_dx", C.c_int32), ("has_init_state", C.c_int32), ("n_cu", C.c_int32), ("zero_dstate", C.c_int32),
                ("g", NintGeom), ("train_from", C.c_int32), ("layer", NintLayer * NINT_MAX_LAYERS),
                ("xs", vp), ("h", vp * NINT_MAX_LAYERS), ("c", vp * NINT_MAX_LAYERS),
                ("gates", vp * NINT_MAX_LAYERS), ("dG", vp * NINT_MAX_LAYERS), ("dh", vp * NINT_MAX_LAYERS),
                ("dc", vp * NINT_MAX_LAYERS), ("dx", vp), ("dW", vp * NINT_MAX_LAYERS), ("db", vp * NINT_MAX_LAYERS),
                ("wg_partial", vp), ("wg_partial_bytes", C.c_size_t), ("fuse_bwd", C.c_int32),
                ("probe_mask", C.c_int32), ("lon_cyclic", C.c_int32), ("probe", vp), ("probe_slots", C.c_int32),
                ("wave", C.c_int32), ("bwd_parts", C.c_int32), ("accumulate", C.c_int32), ("dh_seq", vp)]


class NintFeedback(C.Structure):
    """nint_feedback: the closed-loop part of a forward pass (nint_seq_fwd_closed): the head (w, b), its outputs O (0 = open
    loop) and the first fed step"""
    _fields_ = [("w", vp), ("b", vp), ("O", C.c_int32), ("from_step", C.c_int32)]


class NintFeedbackGrad(C.Structure):
    """nint_feedback_grad: what the roll-out backward (nint_seq_bwd_rollout) takes beside them: the f32 slab of the per-step
    head cotangents (T*B, O, H, W), in l_t and out g_t, and a one-step ET d/dx scratch for need_dx = 0"""
    _fields_ = [("dpred", vp), ("dx_step", vp)]


class NintFeedbackMask(C.Structure):
    """nint_feedback_mask: scheduled sampling (the _sampled entries) -- T*B HOST bytes, index t*B + b, 1 = that image runs that
    step on the fed-back prediction; NULL: use nint_feedback.from"""
    _fields_ = [("fed", vp)]


class NintFeedbackNoise(C.Structure):
    """nint_feedback_noise: noise on the fed-back value (nint_seq_fwd_stochastic, nint_head_feedback_noise) -- O DEVICE sigmas
    (NULL: off) and the generator's key and offsets, as nint_input_noise takes them"""
    _fields_ = [("sigma", vp), ("seed", C.c_uint32), ("draw", C.c_uint32), ("step0", C.c_uint32), ("lane0", C.c_uint32)]


class NintHeadBase(C.Structure):
    """nint_head_base: the residual head's base operand (the _res head entries) -- the input halo slab, the image that pairs with
    the first head image, and where the feedback channels lie in a pixel; xs NULL: no base"""
    _fields_ = [("xs", vp), ("x_n0", C.c_int32), ("Cx", C.c_int32), ("Cxp", C.c_int32), ("c0", C.c_int32), ("xfold_k", C.c_int32)]


class NintLaunchRec(C.Structure):
    """nint_launch_rec: one conv / pointwise problem of a planned pass (nint_debug_seq_plan)"""
    _fields_ = [(n, C.c_int32) for n in ("index", "bwd", "op", "layer", "t", "kernel", "dtype", "epi", "wn", "wk", "ntw", "mt",
                                         "strip", "gx", "gy", "nt_begin")]


class NintWgradSrcRec(C.Structure):
    """nint_wgrad_src_rec: one source (x or h) of a planned weight-gradient launch"""
    _fields_ = [(n, C.c_int32) for n in ("CB", "JG", "TG", "nblk", "ntiles", "tiles_per_split", "want_db", "is_h")] + [("off", C.c_int64)]


class NintWgradLaunchRec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("family", "KS", "NTC", "JW", "KX", "nparts", "gx", "gy", "block", "lds")] + [
        ("src", NintWgradSrcRec * 2)]


class NintWgradFoldRec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("blk_begin", "splits", "waves")]


class NintWgradPlanRec(C.Structure):
    """nint_wgrad_plan_rec: the weight-gradient launches and the fold of one layer (nint_debug_wgrad_plan)"""
    _fields_ = [(n, C.c_int32) for n in ("n_launch", "n_fold", "fold_grid", "fold_block")] + [
        ("launch", NintWgradLaunchRec * 2), ("fold", NintWgradFoldRec * 2)]


class NintOptGroup(C.Structure):
    """nint_opt_group: one range of the flat buffer with its learning rate and decoupled weight decay (nint_adam_flat_groups)"""
    _fields_ = [("begin", C.c_uint64), ("end", C.c_uint64), ("lr", C.c_double), ("weight_decay", C.c_double)]


class NintLossSpec(C.Structure):
    """nint_loss_spec: the configurable loss of the _spec entries (coefficients, Huber threshold, output weights)"""
    _fields_ = [("mse", C.c_double), ("l1", C.c_double), ("huber", C.c_double), ("delta", C.c_double), ("ow", vp),
                ("now", C.c_int32), ("osum", C.c_double)]


class NintEnsLossSpec(C.Structure):
    """nint_ens_loss_spec: the almost-fair CRPS of nint_ens_loss (alpha, the normaliser, the output-weight table and the HOST
    array that picks each sample's row)"""
    _fields_ = [("alpha", C.c_double), ("cnt", C.c_double), ("ow", vp), ("ow_row", C.POINTER(C.c_int32)), ("nrows", C.c_int32)]


# every symbol include/nint.h declares: name -> (restype, argtypes)
_I, _SZ, _F, _D, _U = C.c_int, C.c_size_t, C.c_float, C.c_double, C.c_uint32
_PG, _PL, _PS, _PLS = C.POINTER(NintGeom), C.POINTER(NintLayer), C.POINTER(NintSeq), C.POINTER(NintLossSpec)
_POG = C.POINTER(NintOptGroup)
_PFB = C.POINTER(NintFeedback)
_PFG = C.POINTER(NintFeedbackGrad)
_PFM = C.POINTER(NintFeedbackMask)
_PHB = C.POINTER(NintHeadBase)
_PFN = C.POINTER(NintFeedbackNoise)
SIGNATURES = {
    "nint_version": (_I, []),
    "nint_error_string": (C.c_char_p, [_I]),
    "nint_device_info": (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.c_char_p, _I]),
    "nint_selftest": (_I, [vp, vp]),
    "nint_kc": (_I, [_I]),
    "nint_geom_make": (_I, [_PG, _I, _I, _I]),
    "nint_pack_btchw": (_I, [vp, vp, _I, _I, _I, _I, _PG, _I, vp]),
    "nint_unpack_halo": (_I, [vp, vp, _I, _I, _I, _I, _PG, _I, vp]),
    "nint_pack_compact": (_I, [vp, vp, _I, _I, _I, _I, _I, _I, vp]),
    "nint_unpack_compact": (_I, [vp, vp, _I, _I, _I, _I, _I, _I, vp]),
    "nint_pack_compact_add": (_I, [vp, vp, _I, _I, _I, _I, _I, _I, vp]),
    "nint_state_copy": (_I, [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int32), _I, _I, _I,
                             C.POINTER(C.c_int32), _PG, _I, vp]),
    "nint_packed_weight_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "nint_xfold_pays": (_I, [_I, _I, _I]),
    "nint_pack_weights": (_I, [vp, vp, vp, vp, vp, _I, _I, _I, _I, _I, vp]),
    "nint_pack_weights_layers": (_I, [C.POINTER(vp), C.POINTER(vp), C.POINTER(NintLayer), _I, _I, vp]),
    "nint_pack_btchw_xfold": (_I, [vp, vp, _I, _I, _I, _I, _I, _PG, _I, vp]),
    "nint_unfold_dx": (_I, [vp, vp, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_pack_btchw_xfold_cyclic": (_I, [vp, vp, _I, _I, _I, _I, _I, _PG, _I, vp]),
    "nint_unfold_dx_cyclic": (_I, [vp, vp, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_stencil_holds": (_I, [_PL]),
    "nint_cell_fwd": (_I, [_PL, _PG, _I, _I, vp, vp, vp, vp, vp, vp, vp]),
    "nint_cell_bwd_pointwise": (_I, [_PL, _PG, _I, _I, vp, vp, vp, vp, vp, vp, vp]),
    "nint_conv_dgrad": (_I, [_PL, _PG, _I, _I, vp, vp, vp, vp]),
    "nint_cell_bwd_fused": (_I, [_PL, _PG, _I, _I, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "nint_wgrad_workspace_bytes": (_SZ, [_PL, _I, _I]),
    "nint_conv_wgrad": (_I, [_PL, _PG, _I, _I, vp, vp, vp, vp, vp, vp, _SZ, _I, vp]),
    "nint_seq_fwd": (_I, [_PS, vp]),
    "nint_seq_bwd": (_I, [_PS, vp]),
    "nint_debug_seq_plan": (_I, [_PS, _I, C.POINTER(NintLaunchRec), _I]),
    "nint_seq_fwd_closed": (_I, [_PS, _PFB, vp]),
    "nint_seq_bwd_closed": (_I, [_PS, _PFB, vp]),
    "nint_debug_seq_plan_closed": (_I, [_PS, _PFB, _I, C.POINTER(NintLaunchRec), _I]),
    "nint_seq_bwd_rollout": (_I, [_PS, _PFB, _PFG, vp]),
    "nint_debug_seq_plan_rollout": (_I, [_PS, _PFB, C.POINTER(NintLaunchRec), _I]),
    "nint_seq_fwd_sampled": (_I, [_PS, _PFB, _PFM, vp]),
    "nint_seq_bwd_rollout_sampled": (_I, [_PS, _PFB, _PFM, _PFG, vp]),
    "nint_seq_fwd_residual": (_I, [_PS, _PFB, _PFM, vp]),
    "nint_seq_bwd_rollout_residual": (_I, [_PS, _PFB, _PFM, _PFG, vp]),
    "nint_seq_fwd_stochastic": (_I, [_PS, _PFB, _PFM, _I, _PFN, vp]),
    "nint_debug_seq_plan_sampled": (_I, [_PS, _PFB, _PFM, _I, C.POINTER(NintLaunchRec), _I]),
    "nint_debug_multi_carrier": (_I, [C.POINTER(C.c_int32), _I, _I]),
    "nint_debug_wgrad_plan": (_I, [_PL, _PG, _I, _I, _I, _I, C.POINTER(NintWgradPlanRec)]),
    "nint_head_fwd": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _PG, _I, vp]),
    "nint_head_feedback": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _I, _I, _I, _I, _I, _I, _PG, _I, vp]),
    "nint_head_feedback_bwd": (_I, [vp, _I, vp, _I, vp, _I, _I, _I, _I, _I, vp, _I, _I, _I, _I, _I, _PG, _I, vp]),
    "nint_head_feedback_sel": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _I, _I, _I, _I, _I, _I, vp, _PG, _I, vp]),
    "nint_head_feedback_bwd_sel": (_I, [vp, _I, vp, _I, vp, _I, _I, _I, _I, _I, vp, _I, _I, _I, _I, _I, vp, _PG, _I, vp]),
    "nint_head_fwd_res": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _PG, _I, _PHB, vp]),
    "nint_head_fwd_seq_res": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _PG, _I, _PHB, vp]),
    "nint_head_feedback_res": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _I, _I, _I, _I, _I, _I, _I, vp, _PG, _I, vp]),
    "nint_head_feedback_noise": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _I, _I, _I, _I, _I, _I, _I, vp, _PG, _I, vp, _PFN, _U]),
    "nint_head_feedback_bwd_res": (_I, [vp, _I, vp, _I, vp, _I, _I, _I, _I, _I, vp, _I, _I, _I, _I, _I, _I, vp, _PG, _I, vp]),
    "nint_input_noise": (_I, [vp, _I, _I, _I, _I, _I, _I, _I, vp, _I, _I, _U, _U, _U, _U, _PG, _I, vp]),
    "nint_noise_normal": (_I, [vp, _I, _I, _I, _U, _U, _U, _U, _PG, vp]),
    "nint_head_bwd": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, vp, _PG, _I, vp, _SZ, vp]),
    "nint_head_bwd_acc": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, vp, _I, _PG, _I, vp, _SZ, vp]),
    "nint_head_fwd_seq": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, _PG, _I, vp]),
    "nint_head_bwd_seq": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, vp, vp, _PG, _I, vp, _SZ, vp]),
    "nint_head_bwd_seq_acc": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, vp, vp, _I, _PG, _I, vp, _SZ, vp]),
    "nint_loss_mse_l1_crop": (_I, [vp, vp, vp, vp, vp, _I, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_head_loss_fused": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, vp]),
    "nint_head_loss_seq_fused": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, vp]),
    "nint_loss_mse_l1_crop_weighted": (_I, [vp, vp, vp, _D, vp, vp, vp, _I, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_head_loss_fused_weighted": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, _D, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, vp]),
    "nint_head_loss_seq_fused_weighted": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, _D, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, vp]),
    "nint_loss_crop_spec": (_I, [vp, vp, vp, _D, _PLS, vp, vp, vp, _I, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_head_loss_fused_spec": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, _D, _PLS, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, vp]),
    "nint_head_loss_seq_fused_spec": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, _D, _PLS, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, vp]),
    "nint_head_loss_fused_res": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, _D, _PLS, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, _PHB, vp]),
    "nint_head_loss_seq_fused_res": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, vp, _D, _PLS, vp, vp, vp, vp, _PG, _I, _I, _I, _I, _I, _PHB, vp]),
    "nint_skill_scratch_bytes": (_SZ, [_I, _I, _I, _I]),
    "nint_skill_accum": (_I, [vp, vp, C.POINTER(C.c_int32), _I, vp, vp, vp, vp, _SZ, _I, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_head_skill_accum": (_I, [vp, _I, _I, _I, _I, _I, vp, vp, vp, C.POINTER(C.c_int32), _I, vp, vp, vp, vp, vp, _SZ, _PG,
                                   _I, _I, _I, _I, _I, vp]),
    "nint_ens_scratch_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "nint_ens_accum": (_I, [vp, C.POINTER(C.c_int64), C.c_int64, _I, vp, C.POINTER(C.c_int32), _I, vp, vp, vp, vp, vp, vp, _SZ,
                            _I, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_ens_loss_scratch_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "nint_ens_loss": (_I, [vp, C.POINTER(C.c_int64), C.c_int64, vp, C.POINTER(C.c_int64), C.c_int64, _I, vp, vp, _D,
                           C.POINTER(NintEnsLossSpec), vp, vp, vp, vp, _SZ, _I, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_spec_scratch_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "nint_spec_twiddles": (_I, [_I, C.POINTER(C.c_double)]),
    "nint_spec_accum": (_I, [vp, C.POINTER(C.c_int64), C.c_int64, _I, vp, C.POINTER(C.c_int32), _I, vp, vp, vp, vp, _SZ,
                             _I, _I, _I, _I, _I, _I, _I, _I, vp]),
    "nint_adam_flat": (_I, [vp, vp, vp, vp, _SZ, C.c_double, C.c_double, C.c_double, C.c_double, _I, _F, vp]),
    "nint_grad_norm_scratch_bytes": (_SZ, []),
    "nint_grad_norm_flat": (_I, [vp, _SZ, _F, vp, vp, _SZ, vp]),
    "nint_adam_flat_guarded": (_I, [vp, vp, vp, vp, _SZ, _D, _D, _D, _D, _F, _D, _I, vp, vp, _SZ, vp]),
    "nint_adam_flat_groups": (_I, [vp, vp, vp, vp, _POG, _I, _D, _D, _D, _I, _F, vp]),
    "nint_adam_flat_groups_guarded": (_I, [vp, vp, vp, vp, _POG, _I, _D, _D, _D, _F, _D, _I, vp, vp, vp, _SZ, vp]),
    "nint_preproc_fuse_pad": (_I, [C.POINTER(vp), C.POINTER(_I), _I, vp, vp, vp, _I, _I, _I, _I, _I, _I, vp]),
    "nint_preproc_fuse_pad_batch": (_I, [C.POINTER(vp), C.POINTER(_I), _I, vp, vp, C.POINTER(_I), _I, vp, _I, _I, _I, _I, _I, _I, vp]),
    "nint_preproc_fuse_pad_slab": (_I, [C.POINTER(vp), C.POINTER(_I), _I, vp, vp, C.POINTER(_I), _I, vp, _I, _I, _I, _I, _I, _PG, _I, _I, vp]),
    "nint_preproc_fuse_pad_static": (_I, [C.POINTER(vp), C.POINTER(_I), _I, _I, vp, vp, vp, _I, _I, _I, _I, _I, _I, vp]),
    "nint_preproc_fuse_pad_static_batch": (_I, [C.POINTER(vp), C.POINTER(_I), _I, _I, vp, vp, C.POINTER(_I), _I, vp, _I, _I, _I, _I, _I,
                                                _I, vp]),
    "nint_preproc_fuse_pad_static_slab": (_I, [C.POINTER(vp), C.POINTER(_I), _I, _I, vp, vp, C.POINTER(_I), _I, vp, _I, _I, _I, _I, _I,
                                               _PG, _I, _I, vp]),
    "nint_preproc_fuse_pad_slab_cyclic": (_I, [C.POINTER(vp), C.POINTER(_I), _I, vp, vp, C.POINTER(_I), _I, vp, _I, _I, _I, _I, _I, _PG,
                                               _I, _I, vp]),
    "nint_preproc_fuse_pad_static_slab_cyclic": (_I, [C.POINTER(vp), C.POINTER(_I), _I, _I, vp, vp, C.POINTER(_I), _I, vp, _I, _I, _I, _I,
                                                      _I, _PG, _I, _I, vp]),
}

_lib = None


class NintError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load the HIP library (after torch, so that both share one HIP runtime) and bind signatures.
    ``path`` is the only way to pick another build (diagnostic tools load a -DNINT_STAMP build this way, before
    anything else touches the package); the first successful call wins for the life of the process."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NintError(f"{path} not found: build it with `python nasa-niswan_amd/build.py` "
                        "(the HIP extension is mandatory; there is no fallback path)")
    import torch  # noqa: F401  -- loads torch's bundled libamdhip64.so.7 first; ours binds to the same SONAME
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.nint_version() != NINT_VERSION:
        raise NintError("libnint_hip.so version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().nint_error_string(rc).decode()
        raise NintError(f"{what or 'nint call'} failed: {msg} (code {rc})")


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
