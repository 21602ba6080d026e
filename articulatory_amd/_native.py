"""ctypes binding of libhificar.so (C ABI: include/hificar.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  The CPU oracle under ``oracle/`` is test infrastructure and is never
imported from here.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIFICAR_LIB: developer override (A/B runs of two builds of the same ABI inside one gpurun call)
LIB_PATH = os.environ.get("HIFICAR_LIB") or os.path.join(_HERE, "libhificar.so")

MAX_STAGES = 8
MAX_BLOCKS = 4
MAX_DILATIONS = 4

PREC_F32 = 0
PREC_BF16X3 = 1
PREC_BF16X3W = 2
PREC_BF16X3A = 3
PREC_BF16X3WA = 4
PREC_BF16X3WAC = 6
PREC_BF16X3WACK = 8
PRECISIONS = {"f32": PREC_F32, "bf16x3": PREC_BF16X3}  # the inference arithmetics (``precision=``)
# ... and the Transformer's training arithmetics (``train_precision=``): bf16x3w = bf16x3 with the one-tap weight gradients in it too
TRAIN_PRECISIONS = dict(PRECISIONS, bf16x3w=PREC_BF16X3W)
# the Transformer's inference arithmetics: bf16x3a is bf16x3 with the attention's products on bf16 MFMAs too (no other model takes it)
XFMR_PRECISIONS = dict(PRECISIONS, bf16x3a=PREC_BF16X3A)
# the Transformer's training arithmetics with bf16x3wa: bf16x3w with the attention's query-tiled kernels (forward, backward-q) on bf16 MFMAs too
XFMR_TRAIN_PRECISIONS = dict(TRAIN_PRECISIONS, bf16x3wa=PREC_BF16X3WA)
# ... and with bf16x3wac: bf16x3wa with the weight gradients of the wide k = 3 ResBlock convs on bf16 MFMAs too (what ``train_precision=`` accepted before bf16x3wack)
XFMR_TRAIN_PRECISIONS_ALL = dict(XFMR_TRAIN_PRECISIONS, bf16x3wac=PREC_BF16X3WAC)
# ... and with bf16x3wack: bf16x3wac with the attention's key-tiled backward (dK, dV, the tables' gradient) on bf16 MFMAs too: every value
# ``train_precision=`` accepts (the three mappings above stay as they are: they are what their arithmetics' tests pin)
XFMR_TRAIN_PRECISIONS_K = dict(XFMR_TRAIN_PRECISIONS_ALL, bf16x3wack=PREC_BF16X3WACK)

# every symbol include/hificar.h declares (tests/test_cabi.py checks the .so exports each one)
SYMBOLS = (
    "hificar_create",
    "hificar_gblock_create",
    "hificar_set_weight",
    "hificar_finalize",
    "hificar_set_precision",
    "hificar_workspace_bytes",
    "hificar_forward",
    "hificar_ar_loop",
    "hificar_forward_ragged",
    "hificar_forward_cond",
    "hificar_ar_loop_ragged",
    "hificar_ar_loop_packed",
    "hificar_ar_step",
    "hificar_ar_loop_cond",
    "hificar_ar_loop_packed_cond",
    "hificar_ar_step_cond",
    "hificar_macs",
    "hificar_pcm16",
    "hificar_engine_of",
    "hificar_profile_begin",
    "hificar_profile_end",
    "hificar_debug_tap",
    "hificar_debug_force_tile",
    "hificar_set_weight_device",
    "hificar_set_parameters_device",
    "hificar_raw_grad_floats",
    "hificar_weight_norm_backward",
    "hificar_disc_create",
    "hificar_disc_destroy",
    "hificar_disc_engine",
    "hificar_disc_param_count",
    "hificar_disc_param_info",
    "hificar_disc_grad_floats",
    "hificar_disc_raw_grad_floats",
    "hificar_disc_set_parameters_device",
    "hificar_disc_weight_norm_backward",
    "hificar_disc_tape_bytes",
    "hificar_disc_macs",
    "hificar_disc_backward_workspace_bytes",
    "hificar_disc_output_count",
    "hificar_disc_output_info",
    "hificar_disc_forward",
    "hificar_disc_backward",
    "hificar_disc_dout_floats",
    "hificar_disc_loss",
    "hificar_disc_backward_flat",
    "hificar_mel_create",
    "hificar_mel_destroy",
    "hificar_mel_workspace_bytes",
    "hificar_mel_loss",
    "hificar_stft_loss_forward",
    "hificar_stft_loss_backward",
    "hificar_feat_create",
    "hificar_feat_destroy",
    "hificar_feat_engine",
    "hificar_feat_frames",
    "hificar_feat_workspace_bytes",
    "hificar_feat_forward",
    "hificar_tape_bytes",
    "hificar_forward_train",
    "hificar_backward_workspace_bytes",
    "hificar_grad_count",
    "hificar_grad_info",
    "hificar_grad_floats",
    "hificar_backward",
    "hificar_forward_train_cond",
    "hificar_backward_cond",
    "hificar_grad_bucket_count",
    "hificar_raw_param_bucket",
    "hificar_set_bucket_callback",
    "hificar_weight_norm_backward_bucket",
    "hificar_disc_grad_bucket_count",
    "hificar_disc_raw_param_bucket",
    "hificar_disc_bucket_folded_range",
    "hificar_disc_set_bucket_callback",
    "hificar_disc_weight_norm_backward_bucket",
    "hificar_disc_set_grad_accumulate",
    "hificar_disc_set_grad_scale",
    "hificar_bigru_create",
    "hificar_bigru_set_weight",
    "hificar_bigru_finalize",
    "hificar_bigru_workspace_bytes",
    "hificar_bigru_forward",
    "hificar_bigru_workspace_bytes_lowrate",
    "hificar_bigru_forward_lowrate",
    "hificar_bigru_engine",
    "hificar_bigru_destroy",
    "hificar_bigru_set_parameters_device",
    "hificar_bigru_grad_count",
    "hificar_bigru_grad_info",
    "hificar_bigru_grad_floats",
    "hificar_bigru_tape_bytes",
    "hificar_bigru_train_workspace_bytes",
    "hificar_bigru_forward_train",
    "hificar_bigru_forward_train_ragged",
    "hificar_bigru_backward",
    "hificar_bigru_tape_bytes_lowrate",
    "hificar_bigru_train_workspace_bytes_lowrate",
    "hificar_bigru_forward_train_lowrate",
    "hificar_bigru_backward_lowrate",
    "hificar_xfmr_create",
    "hificar_xfmr_set_weight",
    "hificar_xfmr_set_precision",
    "hificar_xfmr_finalize",
    "hificar_xfmr_workspace_bytes",
    "hificar_xfmr_forward",
    "hificar_xfmr_workspace_bytes_lowrate",
    "hificar_xfmr_forward_lowrate",
    "hificar_xfmr_debug_tap",
    "hificar_xfmr_engine",
    "hificar_xfmr_destroy",
    "hificar_xfmr_set_train_precision",
    "hificar_debug_pack16",
    "hificar_debug_split_rows_t",
    "hificar_debug_split_taps_t",
    "hificar_xfmr_set_parameters_device",
    "hificar_xfmr_grad_count",
    "hificar_xfmr_grad_info",
    "hificar_xfmr_grad_floats",
    "hificar_xfmr_tape_bytes",
    "hificar_xfmr_train_workspace_bytes",
    "hificar_xfmr_forward_train",
    "hificar_xfmr_forward_train_ragged",
    "hificar_xfmr_backward",
    "hificar_xfmr_packed_rows",
    "hificar_xfmr_tape_bytes_packed",
    "hificar_xfmr_train_workspace_bytes_packed",
    "hificar_xfmr_forward_train_packed",
    "hificar_xfmr_backward_packed",
    "hificar_destroy",
    "hificar_last_error",
    "hificar_version",
)


class HificarConfig(ctypes.Structure):
    _fields_ = [
        ("in_channels", ctypes.c_int32),
        ("out_channels", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("kernel_size", ctypes.c_int32),
        ("n_stages", ctypes.c_int32),
        ("upsample_scales", ctypes.c_int32 * MAX_STAGES),
        ("upsample_kernel_sizes", ctypes.c_int32 * MAX_STAGES),
        ("n_blocks", ctypes.c_int32),
        ("resblock_kernel_sizes", ctypes.c_int32 * MAX_BLOCKS),
        ("n_dilations", ctypes.c_int32 * MAX_BLOCKS),
        ("resblock_dilations", (ctypes.c_int32 * MAX_DILATIONS) * MAX_BLOCKS),
        ("use_additional_convs", ctypes.c_int32),
        ("bias", ctypes.c_int32),
        ("lrelu_slope", ctypes.c_float),
        ("use_tanh", ctypes.c_int32),
        ("use_ar", ctypes.c_int32),
        ("ar_input", ctypes.c_int32),
        ("ar_hidden", ctypes.c_int32),
        ("ar_output", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("use_spk_id", ctypes.c_int32),
        ("num_spk", ctypes.c_int32),
        ("spk_emb_size", ctypes.c_int32),
        ("use_ph", ctypes.c_int32),
        ("num_ph", ctypes.c_int32),
        ("ph_emb_size", ctypes.c_int32),
        ("use_ph_loss", ctypes.c_int32),
    ]


MAX_GBLOCKS = 10


class HificarGBlockConfig(ctypes.Structure):
    """hificar_gblock_config (include/hificar.h): the keyword arguments of the reference's GBlockGenerator.__init__ (gblock_gen.py:17-31)."""

    _fields_ = [
        ("in_channels", ctypes.c_int32),
        ("out_channels", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("kernel_size", ctypes.c_int32),
        ("n_blocks", ctypes.c_int32),
        ("g_scales", ctypes.c_int32 * MAX_GBLOCKS),
        ("g_kernel_sizes", ctypes.c_int32 * MAX_GBLOCKS),
        ("use_tanh", ctypes.c_int32),
        ("use_ar", ctypes.c_int32),
        ("ar_input", ctypes.c_int32),
        ("ar_hidden", ctypes.c_int32),
        ("ar_output", ctypes.c_int32),
        ("use_spk_id", ctypes.c_int32),
        ("num_spk", ctypes.c_int32),
        ("spk_emb_size", ctypes.c_int32),
        ("precision", ctypes.c_int32),
    ]


class HificarBigruConfig(ctypes.Structure):
    """hificar_bigru_config (include/hificar.h): the keyword arguments of the reference's BiGRU.__init__ (pytorch_models.py:23-25) that
    affect eval-mode inference."""

    _fields_ = [
        ("in_channels", ctypes.c_int32),
        ("hidden_size", ctypes.c_int32),
        ("out_channels", ctypes.c_int32),
        ("use_tanh", ctypes.c_int32),
    ]


class HificarXfmrConfig(ctypes.Structure):
    """hificar_xfmr_config (include/hificar.h): the keyword arguments of the reference's Transformer.__init__ (transformer.py:22-24) that
    shape eval-mode inference."""

    _fields_ = [
        ("in_channels", ctypes.c_int32),
        ("out_channels", ctypes.c_int32),
        ("elayers", ctypes.c_int32),
        ("hidden_dim", ctypes.c_int32),
    ]


DISC_MAX_SUBS = 8
DISC_MAX_LAYERS = 12
_LAY = ctypes.c_int32 * DISC_MAX_LAYERS


class HificarDiscConfig(ctypes.Structure):
    """hificar_disc_config (include/hificar.h)."""

    _fields_ = [
        ("n_scales", ctypes.c_int32),
        ("pool_kernel", ctypes.c_int32),
        ("pool_stride", ctypes.c_int32),
        ("pool_pad", ctypes.c_int32),
        ("s_n_layers", ctypes.c_int32),
        ("s_cin", _LAY),
        ("s_cout", _LAY),
        ("s_k", _LAY),
        ("s_stride", _LAY),
        ("s_pad", _LAY),
        ("s_groups", _LAY),
        ("s_bias", ctypes.c_int32),
        ("s_slope", ctypes.c_float),
        ("n_periods", ctypes.c_int32),
        ("periods", ctypes.c_int32 * DISC_MAX_SUBS),
        ("p_n_layers", ctypes.c_int32),
        ("p_cin", _LAY),
        ("p_cout", _LAY),
        ("p_k", _LAY),
        ("p_stride", _LAY),
        ("p_pad", _LAY),
        ("p_slope", ctypes.c_float),
    ]


class HificarGanLossConfig(ctypes.Structure):
    _fields_ = [
        ("loss_type", ctypes.c_int32),
        ("average_by_discriminators", ctypes.c_int32),
        ("fm_average_by_layers", ctypes.c_int32),
        ("fm_average_by_discriminators", ctypes.c_int32),
        ("fm_include_final_outputs", ctypes.c_int32),
        ("lambda_adv", ctypes.c_float),
        ("lambda_feat_match", ctypes.c_float),
    ]


class HificarMelConfig(ctypes.Structure):
    _fields_ = [
        ("fft_size", ctypes.c_int32),
        ("hop_size", ctypes.c_int32),
        ("win_length", ctypes.c_int32),
        ("num_mels", ctypes.c_int32),
        ("eps", ctypes.c_float),
        ("log_base", ctypes.c_int32),
        ("mode", ctypes.c_int32),
    ]


FEAT_LOGMEL = 0
FEAT_MFCC = 1
FEAT_MAX_MELS = 128


class HificarFeatConfig(ctypes.Structure):
    """hificar_feat_config (include/hificar.h)."""

    _fields_ = [
        ("kind", ctypes.c_int32),
        ("fft_size", ctypes.c_int32),
        ("hop_size", ctypes.c_int32),
        ("win_length", ctypes.c_int32),
        ("num_mels", ctypes.c_int32),
        ("n_mfcc", ctypes.c_int32),
        ("amin", ctypes.c_float),
        ("top_db", ctypes.c_float),
        ("log_base", ctypes.c_int32),
    ]


class HificarDiscOutput(ctypes.Structure):
    _fields_ = [
        ("sub", ctypes.c_int32),
        ("layer", ctypes.c_int32),
        ("group", ctypes.c_int32),
        ("n_groups", ctypes.c_int32),
        ("period", ctypes.c_int32),
        ("offset_bytes", ctypes.c_int64),
        ("nseq", ctypes.c_int32),
        ("rows", ctypes.c_int32),
        ("pitch", ctypes.c_int32),
        ("channels", ctypes.c_int32),
    ]


# hificar_bucket_fn (include/hificar.h): void (*)(int bucket, void* stream, void* user)
BUCKET_FN = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)


class HificarKernelStat(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * 96),
        ("launches", ctypes.c_int64),
        ("total_ms", ctypes.c_double),
        ("flops", ctypes.c_double),
        ("bytes", ctypes.c_double),
    ]


_lib = None


def load_library():
    """Load libhificar.so (once) and declare the prototypes.  Raises RuntimeError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C articulatory_amd/csrc`). "
            "There is no CPU fallback for the generator forward pass."
        )
    lib = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    lib.hificar_create.argtypes = [ctypes.POINTER(HificarConfig), ctypes.POINTER(vp)]
    lib.hificar_create.restype = ctypes.c_int
    lib.hificar_gblock_create.argtypes = [ctypes.POINTER(HificarGBlockConfig), ctypes.POINTER(vp)]
    lib.hificar_gblock_create.restype = ctypes.c_int
    lib.hificar_set_weight.argtypes = [vp, ctypes.c_char_p, vp, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    lib.hificar_set_weight.restype = ctypes.c_int
    lib.hificar_finalize.argtypes = [vp]
    lib.hificar_finalize.restype = ctypes.c_int
    lib.hificar_set_precision.argtypes = [vp, ctypes.c_int]
    lib.hificar_set_precision.restype = ctypes.c_int
    lib.hificar_workspace_bytes.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.hificar_workspace_bytes.restype = ctypes.c_size_t
    lib.hificar_forward.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.hificar_forward.restype = ctypes.c_int
    lib.hificar_ar_loop.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.hificar_ar_loop.restype = ctypes.c_int
    lib.hificar_forward_ragged.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.hificar_forward_ragged.restype = ctypes.c_int
    lib.hificar_forward_cond.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.hificar_forward_cond.restype = ctypes.c_int
    lib.hificar_ar_loop_ragged.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.hificar_ar_loop_ragged.restype = ctypes.c_int
    lib.hificar_ar_loop_packed.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.hificar_ar_loop_packed.restype = ctypes.c_int
    lib.hificar_ar_step.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp,
                                    ctypes.c_size_t, vp]
    lib.hificar_ar_step.restype = ctypes.c_int
    lib.hificar_ar_loop_cond.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.hificar_ar_loop_cond.restype = ctypes.c_int
    lib.hificar_ar_loop_packed_cond.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp,
                                                ctypes.c_size_t, vp]
    lib.hificar_ar_loop_packed_cond.restype = ctypes.c_int
    lib.hificar_ar_step_cond.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, ctypes.c_int, ctypes.c_int, vp,
                                         ctypes.c_int, vp, vp, ctypes.c_size_t, vp]
    lib.hificar_ar_step_cond.restype = ctypes.c_int
    lib.hificar_macs.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.hificar_macs.restype = ctypes.c_double
    lib.hificar_pcm16.argtypes = [vp, vp, ctypes.c_size_t, vp]
    lib.hificar_pcm16.restype = ctypes.c_int
    lib.hificar_engine_of.argtypes = [vp]
    lib.hificar_engine_of.restype = vp
    lib.hificar_profile_begin.argtypes = [vp]
    lib.hificar_profile_begin.restype = ctypes.c_int
    lib.hificar_profile_end.argtypes = [vp, ctypes.POINTER(HificarKernelStat), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.hificar_profile_end.restype = ctypes.c_int
    lib.hificar_debug_tap.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_size_t]
    lib.hificar_debug_tap.restype = ctypes.c_int
    lib.hificar_debug_force_tile.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.hificar_debug_force_tile.restype = ctypes.c_int
    lib.hificar_set_weight_device.argtypes = [vp, ctypes.c_char_p, vp, vp]
    lib.hificar_set_weight_device.restype = ctypes.c_int
    lib.hificar_set_parameters_device.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, vp]
    lib.hificar_set_parameters_device.restype = ctypes.c_int
    lib.hificar_raw_grad_floats.argtypes = [vp]
    lib.hificar_raw_grad_floats.restype = ctypes.c_int64
    lib.hificar_weight_norm_backward.argtypes = [vp, vp, vp, vp]
    lib.hificar_weight_norm_backward.restype = ctypes.c_int
    ci, cs, c64 = ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
    lib.hificar_disc_create.argtypes = [ctypes.POINTER(HificarDiscConfig), ctypes.POINTER(vp)]
    lib.hificar_disc_create.restype = ci
    lib.hificar_disc_destroy.argtypes = [vp]
    lib.hificar_disc_destroy.restype = None
    lib.hificar_disc_engine.argtypes = [vp]
    lib.hificar_disc_engine.restype = vp
    lib.hificar_disc_param_count.argtypes = [vp]
    lib.hificar_disc_param_count.restype = ci
    lib.hificar_disc_param_info.argtypes = [vp, ci, ctypes.c_char_p, ctypes.POINTER(c64), ctypes.POINTER(ci), ctypes.POINTER(c64)]
    lib.hificar_disc_param_info.restype = ci
    lib.hificar_disc_grad_floats.argtypes = [vp]
    lib.hificar_disc_grad_floats.restype = c64
    lib.hificar_disc_raw_grad_floats.argtypes = [vp]
    lib.hificar_disc_raw_grad_floats.restype = c64
    lib.hificar_disc_set_parameters_device.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp), ci, vp]
    lib.hificar_disc_set_parameters_device.restype = ci
    lib.hificar_disc_weight_norm_backward.argtypes = [vp, vp, vp, vp]
    lib.hificar_disc_weight_norm_backward.restype = ci
    lib.hificar_disc_tape_bytes.argtypes = [vp, ci, ci]
    lib.hificar_disc_tape_bytes.restype = cs
    lib.hificar_disc_macs.argtypes = [vp, ci, ci]
    lib.hificar_disc_macs.restype = ctypes.c_double
    lib.hificar_disc_backward_workspace_bytes.argtypes = [vp, ci, ci]
    lib.hificar_disc_backward_workspace_bytes.restype = cs
    lib.hificar_disc_output_count.argtypes = [vp]
    lib.hificar_disc_output_count.restype = ci
    lib.hificar_disc_output_info.argtypes = [vp, ci, ci, ci, ctypes.POINTER(HificarDiscOutput)]
    lib.hificar_disc_output_info.restype = ci
    lib.hificar_disc_forward.argtypes = [vp, vp, ci, ci, vp, cs, vp]
    lib.hificar_disc_forward.restype = ci
    lib.hificar_disc_backward.argtypes = [vp, ctypes.POINTER(vp), ci, ci, vp, cs, vp, vp, vp, cs, vp]
    lib.hificar_disc_backward.restype = ci
    lib.hificar_disc_dout_floats.argtypes = [vp, ci, ci]
    lib.hificar_disc_dout_floats.restype = cs
    lib.hificar_disc_loss.argtypes = [vp, ctypes.POINTER(HificarGanLossConfig), ci, vp, vp, ci, ci, vp, vp, vp]
    lib.hificar_disc_loss.restype = ci
    lib.hificar_disc_backward_flat.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, cs, vp, vp, vp, cs, vp]
    lib.hificar_disc_backward_flat.restype = ci
    lib.hificar_mel_create.argtypes = [ctypes.POINTER(HificarMelConfig), vp, ctypes.POINTER(vp)]
    lib.hificar_mel_create.restype = ci
    lib.hificar_mel_destroy.argtypes = [vp]
    lib.hificar_mel_destroy.restype = None
    lib.hificar_mel_workspace_bytes.argtypes = [vp, ci, ci]
    lib.hificar_mel_workspace_bytes.restype = cs
    lib.hificar_mel_loss.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, cs, vp]
    lib.hificar_mel_loss.restype = ci
    lib.hificar_stft_loss_forward.argtypes = [vp, vp, vp, ci, ci, vp, vp, cs, vp]
    lib.hificar_stft_loss_forward.restype = ci
    lib.hificar_stft_loss_backward.argtypes = [vp, ci, ci, vp, vp, vp, cs, vp]
    lib.hificar_stft_loss_backward.restype = ci
    lib.hificar_feat_create.argtypes = [ctypes.POINTER(HificarFeatConfig), vp, ctypes.POINTER(vp)]
    lib.hificar_feat_create.restype = ci
    lib.hificar_feat_destroy.argtypes = [vp]
    lib.hificar_feat_destroy.restype = None
    lib.hificar_feat_engine.argtypes = [vp]
    lib.hificar_feat_engine.restype = vp
    lib.hificar_feat_frames.argtypes = [vp, ci]
    lib.hificar_feat_frames.restype = ci
    lib.hificar_feat_workspace_bytes.argtypes = [vp, ci, ci]
    lib.hificar_feat_workspace_bytes.restype = cs
    lib.hificar_feat_forward.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, cs, vp]
    lib.hificar_feat_forward.restype = ci
    lib.hificar_tape_bytes.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.hificar_tape_bytes.restype = ctypes.c_size_t
    lib.hificar_forward_train.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    lib.hificar_forward_train.restype = ctypes.c_int
    lib.hificar_backward_workspace_bytes.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.hificar_backward_workspace_bytes.restype = ctypes.c_size_t
    lib.hificar_grad_count.argtypes = [vp]
    lib.hificar_grad_count.restype = ctypes.c_int
    lib.hificar_grad_info.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    lib.hificar_grad_info.restype = ctypes.c_int
    lib.hificar_grad_floats.argtypes = [vp]
    lib.hificar_grad_floats.restype = ctypes.c_int64
    lib.hificar_backward.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp, vp, vp, vp, ctypes.c_size_t, vp]
    lib.hificar_backward.restype = ctypes.c_int
    lib.hificar_forward_train_cond.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    lib.hificar_forward_train_cond.restype = ctypes.c_int
    lib.hificar_backward_cond.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp, vp, vp, vp, ctypes.c_size_t, vp]
    lib.hificar_backward_cond.restype = ctypes.c_int
    lib.hificar_grad_bucket_count.argtypes = [vp]
    lib.hificar_grad_bucket_count.restype = ctypes.c_int
    lib.hificar_raw_param_bucket.argtypes = [vp, ctypes.c_int]
    lib.hificar_raw_param_bucket.restype = ctypes.c_int
    lib.hificar_set_bucket_callback.argtypes = [vp, BUCKET_FN, vp]
    lib.hificar_set_bucket_callback.restype = ctypes.c_int
    lib.hificar_weight_norm_backward_bucket.argtypes = [vp, vp, vp, ctypes.c_int, vp]
    lib.hificar_weight_norm_backward_bucket.restype = ctypes.c_int
    lib.hificar_disc_grad_bucket_count.argtypes = [vp]
    lib.hificar_disc_grad_bucket_count.restype = ctypes.c_int
    lib.hificar_disc_raw_param_bucket.argtypes = [vp, ctypes.c_int]
    lib.hificar_disc_raw_param_bucket.restype = ctypes.c_int
    lib.hificar_disc_bucket_folded_range.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    lib.hificar_disc_bucket_folded_range.restype = ctypes.c_int
    lib.hificar_disc_set_bucket_callback.argtypes = [vp, BUCKET_FN, vp]
    lib.hificar_disc_set_bucket_callback.restype = ctypes.c_int
    lib.hificar_disc_weight_norm_backward_bucket.argtypes = [vp, vp, vp, ctypes.c_int, vp]
    lib.hificar_disc_weight_norm_backward_bucket.restype = ctypes.c_int
    lib.hificar_disc_set_grad_accumulate.argtypes = [vp, ctypes.c_int]
    lib.hificar_disc_set_grad_accumulate.restype = ctypes.c_int
    lib.hificar_disc_set_grad_scale.argtypes = [vp, vp]
    lib.hificar_disc_set_grad_scale.restype = ctypes.c_int
    lib.hificar_bigru_create.argtypes = [ctypes.POINTER(HificarBigruConfig), ctypes.POINTER(vp)]
    lib.hificar_bigru_create.restype = ci
    lib.hificar_bigru_set_weight.argtypes = [vp, ctypes.c_char_p, vp, ctypes.POINTER(c64), ci]
    lib.hificar_bigru_set_weight.restype = ci
    lib.hificar_bigru_finalize.argtypes = [vp]
    lib.hificar_bigru_finalize.restype = ci
    lib.hificar_bigru_workspace_bytes.argtypes = [vp, ci, ci]
    lib.hificar_bigru_workspace_bytes.restype = cs
    lib.hificar_bigru_forward.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, cs, vp]
    lib.hificar_bigru_forward.restype = ci
    lib.hificar_bigru_workspace_bytes_lowrate.argtypes = [vp, ci, ci, ci]
    lib.hificar_bigru_workspace_bytes_lowrate.restype = cs
    lib.hificar_bigru_forward_lowrate.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, cs, vp]
    lib.hificar_bigru_forward_lowrate.restype = ci
    lib.hificar_bigru_engine.argtypes = [vp]
    lib.hificar_bigru_engine.restype = vp
    lib.hificar_bigru_destroy.argtypes = [vp]
    lib.hificar_bigru_destroy.restype = None
    lib.hificar_bigru_set_parameters_device.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp), ci, vp]
    lib.hificar_bigru_set_parameters_device.restype = ci
    lib.hificar_bigru_grad_count.argtypes = [vp]
    lib.hificar_bigru_grad_count.restype = ci
    lib.hificar_bigru_grad_info.argtypes = [vp, ci, ctypes.c_char_p, ctypes.POINTER(c64), ctypes.POINTER(c64)]
    lib.hificar_bigru_grad_info.restype = ci
    lib.hificar_bigru_grad_floats.argtypes = [vp]
    lib.hificar_bigru_grad_floats.restype = c64
    lib.hificar_bigru_tape_bytes.argtypes = [vp, ci, ci]
    lib.hificar_bigru_tape_bytes.restype = cs
    lib.hificar_bigru_train_workspace_bytes.argtypes = [vp, ci, ci]
    lib.hificar_bigru_train_workspace_bytes.restype = cs
    lib.hificar_bigru_forward_train.argtypes = [vp, vp, vp, vp, ci, ci, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, vp, cs, vp, cs, vp]
    lib.hificar_bigru_forward_train.restype = ci
    lib.hificar_bigru_forward_train_ragged.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, vp, cs, vp,
                                                       cs, vp]
    lib.hificar_bigru_forward_train_ragged.restype = ci
    lib.hificar_bigru_backward.argtypes = [vp, vp, ci, ci, vp, cs, vp, vp, vp, cs, vp]
    lib.hificar_bigru_backward.restype = ci
    lib.hificar_bigru_tape_bytes_lowrate.argtypes = [vp, ci, ci, ci]
    lib.hificar_bigru_tape_bytes_lowrate.restype = cs
    lib.hificar_bigru_train_workspace_bytes_lowrate.argtypes = [vp, ci, ci, ci]
    lib.hificar_bigru_train_workspace_bytes_lowrate.restype = cs
    lib.hificar_bigru_forward_train_lowrate.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, vp, cs,
                                                        vp, cs, vp]
    lib.hificar_bigru_forward_train_lowrate.restype = ci
    lib.hificar_bigru_backward_lowrate.argtypes = [vp, vp, ci, ci, ci, ci, vp, cs, vp, vp, vp, cs, vp]
    lib.hificar_bigru_backward_lowrate.restype = ci
    lib.hificar_xfmr_create.argtypes = [ctypes.POINTER(HificarXfmrConfig), ctypes.POINTER(vp)]
    lib.hificar_xfmr_create.restype = ci
    lib.hificar_xfmr_set_weight.argtypes = [vp, ctypes.c_char_p, vp, ctypes.POINTER(c64), ci]
    lib.hificar_xfmr_set_weight.restype = ci
    lib.hificar_xfmr_set_precision.argtypes = [vp, ci]
    lib.hificar_xfmr_set_precision.restype = ci
    lib.hificar_xfmr_finalize.argtypes = [vp]
    lib.hificar_xfmr_finalize.restype = ci
    lib.hificar_xfmr_set_train_precision.argtypes = [vp, ci]
    lib.hificar_xfmr_set_train_precision.restype = ci
    lib.hificar_debug_pack16.argtypes = [ci, ci, ci, ci, ci, ci, vp, vp, cs, ctypes.POINTER(cs)]
    lib.hificar_debug_pack16.restype = ci
    lib.hificar_debug_split_rows_t.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp, cs, ctypes.POINTER(cs)]
    lib.hificar_debug_split_rows_t.restype = ci
    lib.hificar_debug_split_taps_t.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp, cs, ctypes.POINTER(cs)]
    lib.hificar_debug_split_taps_t.restype = ci
    lib.hificar_xfmr_workspace_bytes.argtypes = [vp, ci, ci]
    lib.hificar_xfmr_workspace_bytes.restype = cs
    lib.hificar_xfmr_forward.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, cs, vp]
    lib.hificar_xfmr_forward.restype = ci
    lib.hificar_xfmr_workspace_bytes_lowrate.argtypes = [vp, ci, ci, ci]
    lib.hificar_xfmr_workspace_bytes_lowrate.restype = cs
    lib.hificar_xfmr_forward_lowrate.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, cs, vp]
    lib.hificar_xfmr_forward_lowrate.restype = ci
    lib.hificar_xfmr_debug_tap.argtypes = [vp, ctypes.c_char_p, vp, cs]
    lib.hificar_xfmr_debug_tap.restype = ci
    lib.hificar_xfmr_engine.argtypes = [vp]
    lib.hificar_xfmr_engine.restype = vp
    lib.hificar_xfmr_destroy.argtypes = [vp]
    lib.hificar_xfmr_destroy.restype = None
    lib.hificar_xfmr_set_parameters_device.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp), ci, vp]
    lib.hificar_xfmr_set_parameters_device.restype = ci
    lib.hificar_xfmr_grad_count.argtypes = [vp]
    lib.hificar_xfmr_grad_count.restype = ci
    lib.hificar_xfmr_grad_info.argtypes = [vp, ci, ctypes.c_char_p, ctypes.POINTER(c64), ctypes.POINTER(c64)]
    lib.hificar_xfmr_grad_info.restype = ci
    lib.hificar_xfmr_grad_floats.argtypes = [vp]
    lib.hificar_xfmr_grad_floats.restype = c64
    lib.hificar_xfmr_tape_bytes.argtypes = [vp, ci, ci]
    lib.hificar_xfmr_tape_bytes.restype = cs
    lib.hificar_xfmr_train_workspace_bytes.argtypes = [vp, ci, ci]
    lib.hificar_xfmr_train_workspace_bytes.restype = cs
    lib.hificar_xfmr_forward_train.argtypes = [vp, vp, vp, vp, ci, ci, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, vp, cs, vp, cs, vp]
    lib.hificar_xfmr_forward_train.restype = ci
    lib.hificar_xfmr_forward_train_ragged.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, vp, cs, vp,
                                                      cs, vp]
    lib.hificar_xfmr_forward_train_ragged.restype = ci
    lib.hificar_xfmr_backward.argtypes = [vp, vp, ci, ci, vp, cs, vp, vp, vp, cs, vp]
    lib.hificar_xfmr_backward.restype = ci
    lib.hificar_xfmr_packed_rows.argtypes = [ci, ci, vp]
    lib.hificar_xfmr_packed_rows.restype = ci
    lib.hificar_xfmr_tape_bytes_packed.argtypes = [vp, ci, ci]
    lib.hificar_xfmr_tape_bytes_packed.restype = cs
    lib.hificar_xfmr_train_workspace_bytes_packed.argtypes = [vp, ci, ci]
    lib.hificar_xfmr_train_workspace_bytes_packed.restype = cs
    lib.hificar_xfmr_forward_train_packed.argtypes = list(lib.hificar_xfmr_forward_train_ragged.argtypes)
    lib.hificar_xfmr_forward_train_packed.restype = ci
    lib.hificar_xfmr_backward_packed.argtypes = [vp, vp, vp, ci, ci, vp, cs, vp, vp, vp, cs, vp]
    lib.hificar_xfmr_backward_packed.restype = ci
    lib.hificar_destroy.argtypes = [vp]
    lib.hificar_destroy.restype = None
    lib.hificar_last_error.argtypes = []
    lib.hificar_last_error.restype = ctypes.c_char_p
    lib.hificar_version.argtypes = []
    lib.hificar_version.restype = ctypes.c_char_p
    _lib = lib
    return lib


LOWRATE_MAX_FACTOR = 16  # HIFICAR_LOWRATE_MAX_FACTOR (include/hificar.h)


def check_interp_factor(interp_factor) -> int:
    """``interp_factor`` of ``forward_lowrate`` as hificar_*_forward_lowrate takes it: an integer in 1 .. 16 (ValueError otherwise, before any
    device work)."""
    import numbers

    if isinstance(interp_factor, bool) or not isinstance(interp_factor, numbers.Integral):
        raise ValueError(f"interp_factor must be an integer in 1 .. {LOWRATE_MAX_FACTOR}, got {interp_factor!r}")
    if not 1 <= int(interp_factor) <= LOWRATE_MAX_FACTOR:
        raise ValueError(f"interp_factor must lie in 1 .. {LOWRATE_MAX_FACTOR}, got {interp_factor}")
    return int(interp_factor)


def check(rc, what):
    if rc != 0:
        msg = load_library().hificar_last_error().decode("utf-8", "replace")
        exc = ValueError if rc == -1 else RuntimeError
        raise exc(f"{what}: {msg} (hificar error {rc})")


def make_config(params: dict, precision: int) -> HificarConfig:
    """generator_params (reference YAML keys) -> hificar_config."""
    cfg = HificarConfig()
    scales = list(params["upsample_scales"])
    ksizes = list(params["upsample_kernel_sizes"])
    rks = list(params["resblock_kernel_sizes"])
    rds = [list(d) for d in params["resblock_dilations"]]
    if len(scales) > MAX_STAGES or len(rks) > MAX_BLOCKS or any(len(d) > MAX_DILATIONS for d in rds):
        raise ValueError("generator is larger than the C ABI's fixed-size config arrays")
    cfg.in_channels = params["in_channels"]
    cfg.out_channels = params["out_channels"]
    cfg.channels = params["channels"]
    cfg.kernel_size = params["kernel_size"]
    cfg.n_stages = len(scales)
    for i, (s, k) in enumerate(zip(scales, ksizes)):
        cfg.upsample_scales[i] = s
        cfg.upsample_kernel_sizes[i] = k
    cfg.n_blocks = len(rks)
    for j, k in enumerate(rks):
        cfg.resblock_kernel_sizes[j] = k
        cfg.n_dilations[j] = len(rds[j])
        for d, v in enumerate(rds[j]):
            cfg.resblock_dilations[j][d] = v
    cfg.use_additional_convs = int(params["use_additional_convs"])
    cfg.bias = int(params["bias"])
    cfg.lrelu_slope = float(params["nonlinear_activation_params"].get("negative_slope", 0.01))
    cfg.use_tanh = int(params["use_tanh"])
    cfg.use_ar = int(params["use_ar"])
    cfg.ar_input = params["ar_input"]
    cfg.ar_hidden = params["ar_hidden"]
    cfg.ar_output = params["ar_output"]
    cfg.precision = precision
    cfg.use_spk_id = int(params.get("use_spk_id", False))
    cfg.num_spk = int(params.get("num_spk") or 0)
    cfg.spk_emb_size = int(params.get("spk_emb_size") or 0)
    cfg.use_ph = int(params.get("use_ph", False))
    cfg.num_ph = int(params.get("num_ph") or 0)
    cfg.ph_emb_size = int(params.get("ph_emb_size") or 0)
    cfg.use_ph_loss = int(params.get("use_ph_loss", False))
    return cfg


# what hificar_gblock_create accepts (csrc/hificar_gblock.hip.inc); GBlockGenerator.__init__ checks the same numbers so that an unsupported
# configuration fails at construction, not at the first forward on the device
GBLOCK_MAX_KERNEL = 11   # odd g_kernel_sizes up to this (the dilation-27 conv's halo against the LDS)
GBLOCK_MAX_SCALE = 64
GBLOCK_MAX_CONV_KERNEL = 16  # input / output conv kernel_size (kMaxTaps)


def check_gblock_params(params: dict):
    """ValueError for a configuration libhificar's GBlock engine rejects (the reference's own limits are checked by the class)."""
    if params["out_channels"] != 1:
        raise ValueError(f"out_channels={params['out_channels']} unsupported (1 only)")
    if params["kernel_size"] > GBLOCK_MAX_CONV_KERNEL:
        raise ValueError(f"kernel_size={params['kernel_size']} > {GBLOCK_MAX_CONV_KERNEL}")
    if params["channels"] // 8 < 1:
        raise ValueError(f"channels={params['channels']} leaves no channels for the last GBlocks")
    for i, (s, k) in enumerate(zip(params["g_scales"], params["g_kernel_sizes"])):
        if k > GBLOCK_MAX_KERNEL:
            raise ValueError(f"g_kernel_sizes[{i}]={k} > {GBLOCK_MAX_KERNEL} (the dilation-27 conv's halo must fit the LDS tiles)")
        if not 1 <= s <= GBLOCK_MAX_SCALE:
            raise ValueError(f"g_scales[{i}]={s} out of range (1 .. {GBLOCK_MAX_SCALE})")
    if params.get("use_ar"):
        if params["ar_input"] < 1 or params["ar_input"] > 1024 or params["ar_hidden"] > 512 or params["ar_output"] > 512:
            raise ValueError("PastFCEncoder: ar_input must be 1 .. 1024, ar_hidden / ar_output <= 512")
        if params["ar_hidden"] % 4 or params["ar_output"] % 4:
            raise ValueError("PastFCEncoder hidden / output dims must be multiples of 4")
    if params.get("use_spk_id") and (not params.get("num_spk") or (params.get("spk_emb_size") or 0) < 1 or params["in_channels"] > 1024):
        raise ValueError("use_spk_id needs num_spk and spk_emb_size (and in_channels <= 1024)")


def make_gblock_config(params: dict, precision: int) -> HificarGBlockConfig:
    """generator_params of a GBlockGenerator (reference keyword names) -> hificar_gblock_config."""
    cfg = HificarGBlockConfig()
    scales, ksizes = list(params["g_scales"]), list(params["g_kernel_sizes"])
    if len(scales) > MAX_GBLOCKS:
        raise ValueError(f"{len(scales)} GBlocks: the reference's channel plan has {MAX_GBLOCKS} entries (gblock_gen.py:63-64)")
    cfg.in_channels = params["in_channels"]
    cfg.out_channels = params["out_channels"]
    cfg.channels = params["channels"]
    cfg.kernel_size = params["kernel_size"]
    cfg.n_blocks = len(scales)
    for i, (s, k) in enumerate(zip(scales, ksizes)):
        cfg.g_scales[i] = s
        cfg.g_kernel_sizes[i] = k
    cfg.use_tanh = int(params["use_tanh"])
    cfg.use_ar = int(params["use_ar"])
    cfg.ar_input = params["ar_input"]
    cfg.ar_hidden = params["ar_hidden"]
    cfg.ar_output = params["ar_output"]
    cfg.use_spk_id = int(params.get("use_spk_id", False))
    cfg.num_spk = int(params.get("num_spk") or 0)
    cfg.spk_emb_size = int(params.get("spk_emb_size") or 0)
    cfg.precision = precision
    return cfg


# what hificar_bigru_create accepts (csrc/hificar_bigru.hip.inc; HIFICAR_BIGRU_MAX_* of include/hificar.h); BiGRU.__init__ checks the same
# numbers so that an unsupported configuration fails at construction, not at the first forward on the device
BIGRU_MAX_IN = 4096
BIGRU_MAX_HIDDEN = 256   # one workgroup holds one direction's W_hh in registers + LDS + a streamed remainder
BIGRU_MAX_OUT = 32       # fc2's rows in the head kernel's LDS


def check_bigru_params(params: dict):
    """ValueError for a BiGRU configuration libhificar's engine rejects."""
    h = params["hidden_size"]
    if not 1 <= params["in_channels"] <= BIGRU_MAX_IN:
        raise ValueError(f"in_channels={params['in_channels']} out of range (1 .. {BIGRU_MAX_IN})")
    if h < 64 or h > BIGRU_MAX_HIDDEN or h % 64:
        raise ValueError(f"hidden_size={h} unsupported (multiples of 64 up to {BIGRU_MAX_HIDDEN}: one workgroup holds a direction's W_hh)")
    if not 1 <= params["out_channels"] <= BIGRU_MAX_OUT:
        raise ValueError(f"out_channels={params['out_channels']} out of range (1 .. {BIGRU_MAX_OUT})")


def make_bigru_config(params: dict) -> HificarBigruConfig:
    """BiGRU keyword arguments (reference names) -> hificar_bigru_config."""
    cfg = HificarBigruConfig()
    cfg.in_channels = params["in_channels"]
    cfg.hidden_size = params["hidden_size"]
    cfg.out_channels = params["out_channels"]
    cfg.use_tanh = int(params["use_tanh"])
    return cfg


# what hificar_xfmr_create accepts (csrc/hificar_xfmr.hip.inc; HIFICAR_XFMR_MAX_* of include/hificar.h); Transformer.__init__ checks the same
# numbers so that an unsupported configuration fails at construction, before any device work
XFMR_MAX_IN = 4096
XFMR_MAX_OUT = 1024      # w_out's rows share the feed-forward buffer
XFMR_MAX_HIDDEN = 1024   # head size hidden_dim / 8 up to 128: the attention kernel's instantiations
XFMR_MAX_LAYERS = 24
XFMR_HEADS = 8           # nhead, dim_feedforward, relative_positional_distance: the reference constructor's constants (transformer.py:43)
XFMR_FF = 3072
XFMR_REL = 100


def check_xfmr_params(params: dict):
    """ValueError for a Transformer configuration libhificar's engine rejects."""
    f = params["hidden_dim"]
    if not 1 <= params["in_channels"] <= XFMR_MAX_IN:
        raise ValueError(f"in_channels={params['in_channels']} out of range (1 .. {XFMR_MAX_IN})")
    if not 1 <= params["out_channels"] <= XFMR_MAX_OUT:
        raise ValueError(f"out_channels={params['out_channels']} out of range (1 .. {XFMR_MAX_OUT})")
    if not 1 <= params["elayers"] <= XFMR_MAX_LAYERS:
        raise ValueError(f"elayers={params['elayers']} out of range (1 .. {XFMR_MAX_LAYERS})")
    if f < 128 or f > XFMR_MAX_HIDDEN or f % 128:
        raise ValueError(f"hidden_dim={f} unsupported (multiples of 128 up to {XFMR_MAX_HIDDEN}: the attention kernel is built for head sizes 16 .. 128)")


def make_xfmr_config(params: dict) -> HificarXfmrConfig:
    """Transformer keyword arguments (reference names) -> hificar_xfmr_config."""
    cfg = HificarXfmrConfig()
    cfg.in_channels = params["in_channels"]
    cfg.out_channels = params["out_channels"]
    cfg.elayers = params["elayers"]
    cfg.hidden_dim = params["hidden_dim"]
    return cfg
