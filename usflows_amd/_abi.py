"""Declarations of the C ABI of ``libusflows_hip.so`` for ctypes: constants, structs and the (restype, argtypes) of every
entry point, to be read next to ``include/usflows_hip.h`` (public) and ``include/usflows_hip_internal.h``.  Nothing here
loads the library or launches anything; ``_ext.py`` does, and re-exports every name."""
import ctypes as C

USF_ABI_VERSION = 36          # include/usflows_hip.h
USF_INTERNAL_VERSION = 6      # include/usflows_hip_internal.h
USF_MAX_HIDDEN = 4

ACT_NONE, ACT_LEAKY_RELU, ACT_GATE = 0, 1, 2
BASE_LAPLACE, BASE_NORMAL, BASE_LPNORM1, BASE_LPNORM2, BASE_LPNORMINF, BASE_ROWSUM = 0, 1, 2, 3, 4, 5
NORM_LOGNORMAL, NORM_GAMMA, NORM_RAW_PARAMS = 0, 1, 0x100
NORM_WEIBULL, NORM_HALFNORMAL, NORM_CHI = 2, 3, 4
RADIAL_MAX_K = 64
OP_LINEAR, OP_COUPLING, OP_PACK_PLANES, OP_GEMM_PLANES, OP_COUPLING_PLANES, OP_GATED_NORM, OP_CALL = 1, 2, 5, 6, 7, 9, 10
PLANES_BF16X3, PLANES_F16X2 = 0, 1
# entry points that have a USF_OP_CALL form (a layer loop's calls as ONE op list): name -> function id
CALL_FNS = {"usf_scale_f32": 1, "usf_channel_affine_f32": 2, "usf_layernorm_channels_f32": 3, "usf_gated_residual_f32": 4,
            "usf_masked_residual_f32": 5, "usf_pointwise_conv_f32": 6, "usf_conv2d_same_f32": 7, "usf_conv2d_same_res_f32": 8,
            "usf_base_logprob_f32": 9, "usf_radial_logprob_f32": 10, "usf_gated_tail_f32": 11, "usf_conv2d_same_ctx_f32": 12}

FN_COUPLING_PLANES_CTX = 64   # internal USF_OP_CALL id: the context arguments of the USF_OP_COUPLING_PLANES op behind it
FN_COUPLING_VCTX = 65         # internal USF_OP_CALL id: the vector context of the USF_OP_COUPLING op behind it
FN_GEMM_PLANES_SIDE = 66      # internal USF_OP_CALL id: the fp32 side output of the USF_OP_GEMM_PLANES op behind it
FN_COUPLING_PLANES_SIDE = 67  # internal USF_OP_CALL id: the fp32 residual buffer of the USF_OP_COUPLING_PLANES op behind it
VCTX_MAX = 32                # USF_VCTX_MAX: widest context usf_coupling_additive_vctx_f32 takes

_fp = C.c_void_p  # device pointers travel as integers


class LinearDesc(C.Structure):
    _fields_ = [
        ("A", _fp), ("lda", C.c_int64),
        ("W", _fp), ("ldw", C.c_int64),
        ("bias", _fp), ("pre_div", _fp), ("pre_sub", _fp),
        ("residual", _fp), ("ldr", C.c_int64),
        ("addend", _fp), ("ldadd", C.c_int64),
        ("post_mul", _fp),
        ("C", _fp), ("ldc", C.c_int64),
        ("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64),
        ("res_sign", C.c_float), ("slope", C.c_float),
        ("act", C.c_int32), ("reserved", C.c_int32),
        ("W_split", _fp), ("ldw_split", C.c_int64), ("split_plane_stride", C.c_int64),
        ("A_planes_out", _fp), ("ldp_out", C.c_int64), ("planes_out_stride", C.c_int64),
    ]


class CouplingDesc(C.Structure):
    _fields_ = [
        ("z", _fp), ("ldz", C.c_int64),
        ("out", _fp), ("ldo", C.c_int64),
        ("M", C.c_int64),
        ("off_pass", C.c_int64), ("n_pass", C.c_int64),
        ("off_trans", C.c_int64), ("n_trans", C.c_int64),
        ("n_hidden", C.c_int32), ("hidden", C.c_int32 * USF_MAX_HIDDEN),
        ("W_in", _fp), ("ldw_in", C.c_int64), ("b_in", _fp),
        ("W_hid", _fp * USF_MAX_HIDDEN), ("b_hid", _fp * USF_MAX_HIDDEN), ("ldw_hid", C.c_int64 * USF_MAX_HIDDEN),
        ("W_out", _fp), ("ldw_out", C.c_int64), ("b_out", _fp),
        ("context", _fp), ("W_ctx", _fp), ("b_ctx", _fp),
        ("post_sub", _fp),
        ("sign", C.c_float), ("slope", C.c_float),
        ("act", C.c_int32), ("reserved", C.c_int32),
        ("split_in", _fp), ("split_in_ld", C.c_int64), ("split_in_plane", C.c_int64),
        ("split_hid", _fp * USF_MAX_HIDDEN), ("split_hid_ld", C.c_int64), ("split_hid_plane", C.c_int64),
        ("split_out", _fp), ("split_out_ld", C.c_int64), ("split_out_plane", C.c_int64),
        ("hidden_out", _fp * USF_MAX_HIDDEN), ("ld_hidden_out", C.c_int64),
        ("gate", _fp * USF_MAX_HIDDEN), ("ld_gate", C.c_int64),
    ]


class PackPlanesDesc(C.Structure):
    _fields_ = [("src", _fp), ("ld", C.c_int64), ("M", C.c_int64), ("nkb", C.c_int64), ("idx", _fp),
                ("pre_div", _fp), ("pre_sub", _fp), ("planes", _fp), ("format", C.c_int32), ("reserved", C.c_int32), ("range_flag", _fp),
                ("src_cols", C.c_int64), ("row_weight", _fp), ("loc", _fp), ("scale", _fp), ("grad_base", C.c_int32),
                ("reserved2", C.c_int32)]


class GemmPlanesDesc(C.Structure):
    _fields_ = [("A", _fp), ("a_nkb", C.c_int64), ("a_kb0", C.c_int64), ("nk", C.c_int64),
                ("W_planes", _fp), ("ldw", C.c_int64), ("w_plane_stride", C.c_int64), ("w_rows", C.c_int64),
                ("bias", _fp), ("post_mul", _fp), ("residual", _fp),
                ("C_planes", _fp), ("c_nkb", C.c_int64), ("c_kb0", C.c_int64), ("c_kbn", C.c_int64),
                ("C_f32", _fp), ("ldc", C.c_int64), ("N", C.c_int64), ("M", C.c_int64),
                ("res_sign", C.c_float), ("slope", C.c_float), ("act", C.c_int32), ("format", C.c_int32), ("range_flag", _fp),
                ("base_tab", _fp), ("base_tab_stride", C.c_int64), ("base_part", _fp), ("base", C.c_int32), ("reserved", C.c_int32)]


class CouplingPlanesDesc(C.Structure):
    _fields_ = [("z", _fp), ("z_nkb", C.c_int64), ("M", C.c_int64),
                ("kb_p0", C.c_int64), ("nk_p", C.c_int64), ("kb_t0", C.c_int64), ("nk_t", C.c_int64),
                ("n_hidden", C.c_int32), ("hidden_padded", C.c_int32),
                ("W_in", _fp), ("ldw_in", C.c_int64), ("w_in_plane", C.c_int64), ("b_in", _fp),
                ("W_hid", _fp * 2), ("b_hid", _fp * 2), ("ldw_hid", C.c_int64), ("w_hid_plane", C.c_int64),
                ("W_out", _fp), ("ldw_out", C.c_int64), ("w_out_plane", C.c_int64), ("b_out", _fp),
                ("sign", C.c_float), ("slope", C.c_float), ("act", C.c_int32), ("format", C.c_int32),
                ("range_flag", _fp), ("hidden_out", _fp * 2), ("gate", _fp * 2)]


class MtChunk(C.Structure):
    """usf_mt_chunk: one block's share of one parameter tensor (SophiaG multi-tensor kernels)"""
    _fields_ = [("p", _fp), ("g", _fp), ("m", _fp), ("h", _fp), ("n", C.c_int32), ("reserved", C.c_int32)]


class AdamChunk(C.Structure):
    """usf_adam_chunk: one block's share of one parameter tensor (usf_adam_step_f32); slot: its device step counter"""
    _fields_ = [("p", _fp), ("g", _fp), ("m", _fp), ("v", _fp), ("vmax", _fp), ("n", C.c_int32), ("slot", C.c_int32)]


class GradChunk(C.Structure):
    """usf_grad_chunk: one block's share of one gradient tensor (usf_grad_sqnorm_partials_f32 / usf_grad_clip_scale_f32)"""
    _fields_ = [("g", _fp), ("n", C.c_int32), ("reserved", C.c_int32)]


class ConvVariantQuery(C.Structure):
    """usf_conv_variant_query: one call of the "same" convolution's entry points, as usf_conv2d_same_variant is asked about it"""
    _fields_ = [("entry", C.c_int32), ("aligned", C.c_int32), ("B", C.c_int64), ("cin", C.c_int64), ("cout", C.c_int64),
                ("H", C.c_int64), ("W", C.c_int64), ("ks", C.c_int64), ("cus", C.c_int32), ("reserved", C.c_int32)]


class ConvVariant(C.Structure):
    """usf_conv_variant: the kernel, group size, grid and instantiation / patch shapes such a call launches"""
    _fields_ = [("kernel", C.c_int32), ("S", C.c_int32), ("grid", C.c_int64), ("groups", C.c_int64), ("lds_bytes", C.c_int64),
                ("NB", C.c_int32), ("CP", C.c_int32), ("NCT", C.c_int32), ("CTX", C.c_int32),
                ("PC_full", C.c_int32), ("PR_full", C.c_int32), ("PC_last", C.c_int32), ("PR_last", C.c_int32),
                ("max_mHW", C.c_int32), ("max_mW", C.c_int32), ("max_mSE", C.c_int32), ("max_mSO", C.c_int32)]


class ConvWgradQuery(C.Structure):
    """usf_conv_wgrad_query: one call of usf_conv_wgrad_f32, as usf_conv_wgrad_variant is asked about it"""
    _fields_ = [("B", C.c_int64), ("cin", C.c_int64), ("cout", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("ks", C.c_int64),
                ("masked", C.c_int32), ("cus", C.c_int32), ("blocks_per_cu", C.c_int32), ("reserved", C.c_int32)]


class ConvWgradInfo(C.Structure):
    """usf_conv_wgrad_info: the kernel, instantiation, grid, staging geometry and reduction such a call launches"""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "CIT", "COT", "T", "rsplit", "blocks", "lds_bytes", "S", "base", "q0", "CS", "nch",
                                         "nacc", "tab_floats", "slots", "rounds", "per", "rows_used", "max_samples_per_wave",
                                         "blocks_per_cu", "cus", "reserved")]


class LnBwdInfo(C.Structure):
    """usf_ln_bwd_info: the kernel, its width (CMAX or CPT), grid and reduction usf_layernorm_channels_bwd_f32 launches"""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "width", "blocks", "slots", "rounds", "per", "rows_used", "reserved")]


class ConvWgradWideInfo(C.Structure):
    """usf_conv_wgrad_wide_info: the instantiation, grid, staging geometry and reduction usf_conv_wgrad_wide_f32 launches"""
    _fields_ = [(n, C.c_int32) for n in ("served", "CIT", "COT", "T", "tiles", "tiles_per_wave", "wave_groups", "position_parts",
                                         "blocks", "lds_bytes", "S", "q0", "CSx", "CSy", "nch", "nacc", "slots", "rounds", "per",
                                         "rows_used", "max_samples_per_block", "blocks_per_cu", "cus", "reserved")]


class ChannelAffineBwdQuery(C.Structure):
    """usf_channel_affine_bwd_query: one call of usf_channel_affine_bwd_f32, as usf_channel_affine_bwd_variant is asked about it"""
    _fields_ = [("B", C.c_int64), ("C", C.c_int64), ("P", C.c_int64),
                ("aligned16", C.c_int32), ("want_bias", C.c_int32), ("grid_cap", C.c_int32), ("reserved", C.c_int32)]


class ChannelAffineBwdInfo(C.Structure):
    """usf_channel_affine_bwd_info: the instantiation (padded width, 16-byte or scalar form), grid, loop trips and reduction
    usf_channel_affine_bwd_f32 launches"""
    _fields_ = [(n, C.c_int32) for n in ("served", "width", "vec", "blocks", "trips", "slot_floats", "slots", "rounds", "per",
                                         "rows_used", "grid_cap", "reserved")]


class ConvBandQuery(C.Structure):
    """usf_conv_band_query: one call of usf_conv2d_same_band_f32, as usf_conv2d_same_band_variant is asked about it"""
    _fields_ = [("B", C.c_int64), ("cin", C.c_int64), ("cout", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("ks", C.c_int64),
                ("ctx", C.c_int32), ("band_rows", C.c_int32), ("cus", C.c_int32), ("reserved", C.c_int32)]


class ConvBandInfo(C.Structure):
    """usf_conv_band_info: the band height, bands per sample, grid, LDS bytes, staging iterations and patch shapes such a call launches"""
    _fields_ = [("served", C.c_int32), ("band_rows", C.c_int32), ("bands", C.c_int32), ("last_rows", C.c_int32),
                ("groups", C.c_int64), ("grid", C.c_int64), ("lds_bytes", C.c_int64), ("weight_bytes", C.c_int64)] + \
               [(n, C.c_int32) for n in ("stage_iters", "CTX", "PC_full", "PR_full", "PC_last", "PR_last", "best_rows", "reserved")]


class ConvWgradBandQuery(C.Structure):
    """usf_conv_wgrad_band_query: one call of usf_conv_wgrad_band_f32, as usf_conv_wgrad_band_variant is asked about it"""
    _fields_ = [("B", C.c_int64), ("cin", C.c_int64), ("cout", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("ks", C.c_int64),
                ("band_rows", C.c_int32), ("cus", C.c_int32), ("blocks_per_cu", C.c_int32), ("reserved", C.c_int32)]


class ConvWgradBandInfo(C.Structure):
    """usf_conv_wgrad_band_info: the whole plan usf_conv_wgrad_band_f32 launches from -- the band, the grid, the instantiation, the
    reduction, the LDS geometry and the staging loops' multiply-high divisions"""
    _fields_ = [(n, C.c_int32) for n in ("served", "band_rows", "best_rows", "fit_rows", "bands", "last_rows", "staged_rows", "groups",
                                         "grid", "lds_bytes", "CIT", "COT", "T", "tiles", "tiles_per_wave", "wave_groups",
                                         "position_parts", "slots", "rounds", "per", "rows_used", "max_groups_per_block",
                                         "blocks_per_cu", "cus", "S", "q0", "CSx", "CSy", "nch", "nacc", "max_dividend", "reserved")] + \
               [(n, C.c_uint32) for n in ("m_x", "m_y", "m_w", "reserved2")]


CONV_ENTRIES = {"plain": 0, "ctx": 1, "res": 2, "gate_mul": 3, "gate_add": 4, "gated": 5}   # USF_CONV_ENTRY_*


class GatedNormDesc(C.Structure):
    """usf_gated_norm_desc: row pass of the vector ConvNet conditioner (gate, layer norm, activation)"""
    _fields_ = [("skip", _fp), ("ld_skip", C.c_int64), ("vg", _fp), ("ld_vg", C.c_int64), ("gate_off", C.c_int64),
                ("gamma", _fp), ("beta", _fp), ("out", _fp), ("ld_out", C.c_int64), ("out_act", _fp), ("ld_act", C.c_int64),
                ("M", C.c_int64), ("C", C.c_int64), ("c_pad", C.c_int64), ("eps", C.c_float), ("slope", C.c_float),
                ("act", C.c_int32), ("reserved", C.c_int32)]


class GatedNormBwdDesc(C.Structure):
    """usf_gated_norm_bwd_desc: the backward twin of the row pass"""
    _fields_ = [("skip", _fp), ("ld_skip", C.c_int64), ("vg", _fp), ("ld_vg", C.c_int64), ("gate_off", C.c_int64),
                ("gamma", _fp), ("dy", _fp), ("ld_dy", C.c_int64), ("d_skip", _fp), ("ld_d_skip", C.c_int64),
                ("d_vg", _fp), ("ld_d_vg", C.c_int64), ("dy_xh", _fp), ("ld_dy_xh", C.c_int64),
                ("M", C.c_int64), ("C", C.c_int64), ("c_pad", C.c_int64), ("eps", C.c_float), ("reserved", C.c_float)]


class CallDesc(C.Structure):
    """usf_call_desc: one entry-point call inside an op list, arguments as 64-bit words"""
    _fields_ = [("fn", C.c_int32), ("n_args", C.c_int32), ("a", C.c_uint64 * 20)]


class _OpUnion(C.Union):
    _fields_ = [("linear", LinearDesc), ("coupling", CouplingDesc), ("pack_planes", PackPlanesDesc),
                ("gemm_planes", GemmPlanesDesc), ("coupling_planes", CouplingPlanesDesc), ("gated_norm", GatedNormDesc),
                ("call", CallDesc)]


class Op(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("u", _OpUnion)]


class LuPrepDesc(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("D", C.c_int64),
        ("L_raw", C.POINTER(C.c_void_p)), ("U_raw", C.POINTER(C.c_void_p)),
        ("tri", _fp), ("tri_inv", _fp), ("work", _fp), ("M", _fp), ("Minv", _fp), ("ladj", _fp),
    ]


class PackJob(C.Structure):
    _fields_ = [
        ("src", _fp), ("out_idx", _fp), ("in_idx", _fp), ("W", _fp), ("planes", _fp),
        ("ld_src", C.c_int64), ("n_out", C.c_int64), ("n_in", C.c_int64), ("ldw", C.c_int64),
        ("ld_planes", C.c_int64), ("plane_stride", C.c_int64),
        ("src_is_f32", C.c_int32), ("transpose", C.c_int32),
    ]


class PsumJob(C.Structure):
    """usf_psum_job: one deferred sum of per-wave partial slots (usf_conv_wgrad_deferred_f32 / usf_partial_sum_jobs_f32)"""
    _fields_ = [("part", _fp), ("out", _fp), ("out2", _fp),
                ("nparts", C.c_int32), ("n", C.c_int32), ("mode", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
                ("CIT", C.c_int32), ("T", C.c_int32), ("ntile", C.c_int32), ("first_block", C.c_int32), ("per", C.c_int32),
                ("rows", C.c_int32), ("vec4", C.c_int32)]


class WgradJob(C.Structure):
    """usf_wgrad_job: one queued weight-gradient launch (usf_conv_wgrad_plan_f32 / usf_conv_wgrad_jobs_f32)"""
    _fields_ = [("args", C.c_ubyte * 192), ("CIT", C.c_int32), ("COT", C.c_int32), ("T", C.c_int32), ("blocks", C.c_int32),
                ("lds_bytes", C.c_int32), ("first_block", C.c_int32)]


class WReduceJob(C.Structure):
    """usf_wreduce_job: one queued reduction of usf_wgrad_blocked_plan_f32 (usf_wgrad_reduce_jobs_f32)"""
    _fields_ = [("part", _fp), ("out", _fp), ("cs_part", _fp), ("cs_out", _fp), ("rows", C.c_int64), ("cols", C.c_int64),
                ("ldo", C.c_int64), ("alpha", C.c_float), ("beta", C.c_float), ("cs_alpha", C.c_float), ("cs_beta", C.c_float),
                ("first_block", C.c_int32), ("blocks", C.c_int32), ("sched", C.c_ubyte * 64)]


class WPlanesJob(C.Structure):
    """usf_wplanes_job"""
    _fields_ = [("w", C.c_void_p), ("out_off", C.c_int64), ("cin", C.c_int32), ("cout", C.c_int32), ("ks", C.c_int32),
                ("first_block", C.c_int32)]


class GradJob(C.Structure):
    _fields_ = [
        ("Y", _fp), ("A", _fp), ("G", _fp),
        ("ldy", C.c_int64), ("lda", C.c_int64), ("ldg", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("first_block", C.c_int32),
        ("alpha", C.c_float), ("beta", C.c_float),
    ]

# usf_sizeof_desc kind -> the struct whose size it reports: every Structure above (load() compares each one with C)
SIZEOF_KINDS = {OP_LINEAR: LinearDesc, OP_COUPLING: CouplingDesc, 0: Op, 3: LuPrepDesc, 4: PackJob, OP_PACK_PLANES: PackPlanesDesc,
                OP_GEMM_PLANES: GemmPlanesDesc, OP_COUPLING_PLANES: CouplingPlanesDesc, 8: MtChunk, OP_GATED_NORM: GatedNormDesc,
                OP_CALL: CallDesc, 11: GradJob, 12: PsumJob, 13: GatedNormBwdDesc, 14: WgradJob, 15: WReduceJob, 16: WPlanesJob, 17: AdamChunk, 18: GradChunk,
                19: ConvVariantQuery, 20: ConvVariant, 21: ConvWgradQuery, 22: ConvWgradInfo, 23: LnBwdInfo, 24: ConvWgradWideInfo,
                25: ChannelAffineBwdQuery, 26: ChannelAffineBwdInfo, 27: ConvBandQuery, 28: ConvBandInfo,
                29: ConvWgradBandQuery, 30: ConvWgradBandInfo}


# every symbol include/usflows_hip.h declares (the stable public ABI): (restype, argtypes)
PUBLIC_SYMBOLS = {
    "usf_abi_version": (C.c_int, []),
    "usf_sizeof_desc": (C.c_int, [C.c_int32]),
    "usf_last_error": (C.c_char_p, []),
    "usf_build_info": (C.c_char_p, []),
    "usf_linear_f32": (C.c_int, [C.POINTER(LinearDesc), C.c_void_p]),
    "usf_pack_planes_f32": (C.c_int, [C.POINTER(PackPlanesDesc), C.c_void_p]),
    "usf_gemm_planes_bf16x3": (C.c_int, [C.POINTER(GemmPlanesDesc), C.c_void_p]),
    "usf_coupling_planes": (C.c_int, [C.POINTER(CouplingPlanesDesc), C.c_void_p]),
    "usf_coupling_additive_f32": (C.c_int, [C.POINTER(CouplingDesc), C.c_void_p]),
    "usf_coupling_max_width": (C.c_int, []),
    "usf_coupling_padded_width": (C.c_int, [C.c_int]),
    "usf_base_logprob_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _fp, _fp, C.c_float,
                                       _fp, _fp, _fp, C.c_void_p]),
    "usf_base_tables_f32": (C.c_int, [C.c_int32, _fp, _fp, C.c_int64, _fp, C.c_int64, C.c_void_p]),
    "usf_base_sample_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _fp, _fp, C.c_uint64,
                                      C.c_uint64, C.c_int64, C.c_void_p]),
    "usf_radial_sample_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _fp, _fp, C.c_uint64,
                                        C.c_uint64, C.c_int64, C.c_void_p]),
    "usf_radial_logprob_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp,
                                         C.c_double, C.c_float, _fp, _fp, _fp, _fp, C.c_void_p]),
    "usf_variates_from_bits_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, C.c_void_p]),
    "usf_scale_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_int32, C.c_void_p]),
    "usf_affine_coupling_apply_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64,
                                                C.c_float, C.c_int32, _fp, C.c_void_p]),
    "usf_channel_affine_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, _fp, C.c_void_p]),
    "usf_layernorm_channels_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, C.c_float, C.c_int32,
                                             C.c_float, C.c_void_p]),
    "usf_gated_residual_f32": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_int64, C.c_void_p]),
    "usf_gated_norm_rows_f32": (C.c_int, [C.POINTER(GatedNormDesc), C.c_void_p]),
    "usf_pointwise_conv_supported": (C.c_int, [C.c_int64, C.c_int64, C.c_int32]),
    "usf_pointwise_conv_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, C.c_int32, C.c_float,
                                         C.c_int32, C.c_float, _fp, _fp, _fp, C.c_float, C.c_void_p]),
    "usf_conv2d_weight_elems": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "usf_conv2d_same_fits": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "usf_conv2d_same_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, _fp,
                                      C.c_int32, C.c_float, C.c_int32, C.c_float, _fp, C.c_int64, C.c_void_p]),
    "usf_conv2d_same_ctx_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, _fp,
                                          C.c_int32, C.c_float, C.c_int32, C.c_float, _fp, C.c_int64, _fp, C.c_void_p]),
    "usf_conv2d_same_res_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, _fp,
                                          C.c_int32, C.c_float, _fp, _fp, C.c_float, C.c_void_p]),
    "usf_masked_residual_f32": (C.c_int, [_fp, _fp, _fp, C.c_float, _fp, C.c_int64, C.c_int64, C.c_void_p]),
    "usf_gated_tail_supported": (C.c_int, [C.c_int64]),
    "usf_gated_tail_f32": (C.c_int, [_fp, _fp, _fp] + [C.c_int64] * 3 + [_fp, _fp, C.c_int32, C.c_float, C.c_int32, C.c_float, _fp, _fp,
                                     C.c_float, C.c_void_p]),
    "usf_conv2d_weight_planes_f32": (C.c_int, [_fp, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "usf_gather_cols_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_void_p]),
    "usf_run_ops": (C.c_int, [C.POINTER(Op), C.c_int32, C.c_void_p]),
    "usf_lu_prepare_f64": (C.c_int, [C.POINTER(LuPrepDesc), C.c_void_p]),
    "usf_gemm_f64": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int64, C.c_int64, C.c_int32,
                               _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                               C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "usf_householder_f64": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, _fp, C.c_void_p]),
    "usf_pack_weight_f32": (C.c_int, [_fp, C.c_int32, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, C.c_int64,
                                      _fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_void_p]),
    "usf_pack_weights_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "usf_pack_weights_t_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "usf_affine_prep_f32": (C.c_int, [_fp, _fp, _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp,
                                      C.c_void_p]),
    "usf_matvec_f64": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, C.c_int64, _fp, C.c_double, _fp, _fp, C.c_void_p]),
}
# every symbol include/usflows_hip_internal.h declares (the engine's own plumbing, no stability promise)
INTERNAL_SYMBOLS = {
    "usf_internal_version": (C.c_int, []),
    "usf_set_tuning": (C.c_int, [C.c_char_p, C.c_int64]),
    "usf_get_tuning": (C.c_int64, [C.c_char_p, C.c_int64]),
    "usf_linear_variant": (C.c_int, [C.POINTER(LinearDesc)]),
    "usf_gemm_planes_variant": (C.c_int, [C.POINTER(GemmPlanesDesc)]),
    "usf_coupling_variant": (C.c_int, [C.POINTER(CouplingDesc)]),
    "usf_coupling_planes_variant": (C.c_int, [C.POINTER(CouplingPlanesDesc), C.c_int32, C.c_int32]),
    "usf_radial_logprob_grad_workspace": (C.c_int64, [C.c_int64, C.c_int64]),
    "usf_radial_logprob_grad_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int32, C.c_int32,
                                              _fp, _fp, _fp, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, C.c_int64, C.c_void_p]),
    "usf_radial_sample_norm_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp,
                                             _fp, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p]),
    "usf_gated_norm_rows_bwd_f32": (C.c_int, [C.POINTER(GatedNormBwdDesc), C.c_void_p]),
    "usf_coupling_planes_ctx": (C.c_int, [C.POINTER(CouplingPlanesDesc), _fp, C.c_int64, _fp, _fp, C.c_void_p]),
    "usf_gemm_planes_side": (C.c_int, [C.POINTER(GemmPlanesDesc), _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "usf_coupling_planes_side": (C.c_int, [C.POINTER(CouplingPlanesDesc), _fp, C.c_int64, C.c_void_p]),
    "usf_coupling_additive_vctx_f32": (C.c_int, [C.POINTER(CouplingDesc), _fp, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, C.c_void_p]),
    "usf_coupling_additive_vctx_variant": (C.c_int, [C.POINTER(CouplingDesc), C.c_int32]),
    "usf_conv_ctx_wgrad_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_void_p]),
    "usf_conv2d_same_gate_f32": (C.c_int, [_fp, _fp] + [C.c_int64] * 6 + [C.c_void_p, _fp, C.c_float, _fp, _fp, C.c_void_p]),
    "usf_conv2d_same_variant": (C.c_int, [C.POINTER(ConvVariantQuery), C.POINTER(ConvVariant)]),
    "usf_conv_wgrad_variant": (C.c_int, [C.POINTER(ConvWgradQuery), C.POINTER(ConvWgradInfo)]),
    "usf_layernorm_channels_bwd_variant": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(LnBwdInfo)]),
    "usf_conv_wgrad_workspace": (C.c_int64, [C.c_int64] * 6),
    "usf_conv2d_same_pad_fits": (C.c_int, [C.c_int64] * 6),
    "usf_conv2d_same_band_fits": (C.c_int, [C.c_int64] * 5),
    "usf_conv2d_same_band_f32": (C.c_int, [_fp, _fp] + [C.c_int64] * 6 + [_fp, _fp, _fp, C.c_int32, C.c_float, C.c_int32, C.c_float, _fp,
                                           C.c_int64, _fp, C.c_int64, C.c_void_p]),
    "usf_conv2d_same_band_variant": (C.c_int, [C.POINTER(ConvBandQuery), C.POINTER(ConvBandInfo)]),
    "usf_conv2d_same_pad_f32": (C.c_int, [_fp, _fp] + [C.c_int64] * 7 + [_fp, _fp, _fp, C.c_int32, C.c_float, C.c_int32, C.c_float, _fp,
                                          C.c_int64, C.c_void_p]),
    "usf_conv_wgrad_f32": (C.c_int, [_fp, _fp] + [C.c_int64] * 6 + [_fp, _fp, C.c_int32, C.c_float, _fp, _fp, _fp, C.c_int64,
                                     C.c_void_p]),
    "usf_conv_wgrad_deferred_f32": (C.c_int, [_fp, _fp] + [C.c_int64] * 6 + [_fp, _fp, C.c_int32, C.c_float, _fp, _fp, _fp, C.c_int64,
                                              C.POINTER(PsumJob), C.c_void_p]),
    "usf_conv_wgrad_plan_f32": (C.c_int, [_fp, _fp] + [C.c_int64] * 6 + [_fp, _fp, C.c_int32, C.c_float, _fp, _fp, _fp, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "usf_conv_wgrad_jobs_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),      # (job: two entries)
    "usf_partial_sum_jobs_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_void_p]),
    "usf_layernorm_channels_bwd_workspace": (C.c_int64, [C.c_int64] * 3),
    "usf_layernorm_channels_bwd_f32": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_float, C.c_int32, C.c_float,
                                                 _fp, _fp, C.c_int64, C.c_void_p]),
    "usf_gated_residual_bwd_f32": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_int64, C.c_void_p]),
    "usf_conv2d_weight_planes_batch_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "usf_gated_tail_workspace": (C.c_int64, [C.c_int64] * 3),
    "usf_channel_affine_bwd_workspace": (C.c_int64, [C.c_int64] * 3),
    "usf_channel_affine_bwd_f32": (C.c_int, [_fp, _fp, _fp] + [C.c_int64] * 3 + [_fp, _fp, _fp, _fp, _fp, C.c_int64, C.c_void_p, C.c_void_p]),
    "usf_channel_affine_bwd_variant": (C.c_int, [C.POINTER(ChannelAffineBwdQuery), C.POINTER(ChannelAffineBwdInfo)]),
    "usf_gated_tail_bwd_f32": (C.c_int, [_fp] * 6 + [C.c_int64] * 3 + [_fp, _fp, C.c_int32, C.c_float, C.c_int32, C.c_float, _fp, _fp,
                                         C.c_float, _fp, _fp, C.c_int64, C.c_void_p, C.c_void_p]),
    "usf_lu_grad_finish_f64": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, C.c_int64, C.c_int64, _fp, _fp, C.c_void_p]),
    "usf_wgrad_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_int64,
                                C.c_float, C.c_float, C.c_int32, _fp, C.c_int64, C.c_void_p]),
    "usf_wgrad_workspace_floats": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "usf_wgrad_bias_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_int64,
                                     C.c_float, C.c_float, C.c_int32, _fp, C.c_float, C.c_float, _fp, C.c_int64, _fp]),
    "usf_wgrad_bias_ok": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    "usf_wgrad_planes_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                       C.c_int64, C.c_int64, _fp, C.c_int64, C.c_float, C.c_float, _fp, C.c_float, C.c_float,
                                       _fp, C.c_int64, _fp]),
    "usf_wgrad_blocked_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp,
                                        C.c_int64, C.c_float, C.c_float, _fp, C.c_float, C.c_float, _fp, C.c_int64, _fp]),
    "usf_wgrad_blocked_plan_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _fp,
                                             C.c_int64, C.c_float, C.c_float, _fp, C.c_float, C.c_float, _fp, C.c_int64, C.c_void_p, _fp]),
    "usf_wgrad_reduce_jobs_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "usf_base_param_grad_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int32, _fp, _fp, _fp, _fp, C.c_int64, C.c_void_p]),
    "usf_mfma_probe": (C.c_int, [_fp, _fp, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_void_p]),
    "usf_set_clock_buffer": (C.c_int, [_fp]),
    "usf_wgrad_planes_colsum_ok": (C.c_int, [C.c_int64, C.c_int64, C.c_int64]),
    "usf_wgrad_planes_workspace_floats": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "usf_wgrad_planes_ok": (C.c_int, [C.c_int64, C.c_int64, C.c_int64]),
    "usf_split_planes_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_int64, C.c_int64, _fp]),
    "usf_wgrad_variant": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    "usf_wgrad_plan": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32]),
    "usf_wgrad_planes_plan": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32]),
    "usf_sophiag_step_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                                       C.c_void_p]),
    "usf_sophiag_hessian_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p]),
    "usf_adam_step_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                    C.c_double, C.c_int32, C.c_void_p]),
    "usf_grad_sqnorm_partials_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "usf_grad_clip_scale_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p]),
    "usf_colsum_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_float, C.c_float, _fp, C.c_int64,
                                 C.c_void_p]),
    "usf_act_grad_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_float,
                                   C.c_void_p]),
    "usf_base_logprob_grad_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, C.c_int32, _fp, _fp, _fp,
                                            C.c_int64, C.c_void_p]),
    "usf_grad_jobs_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_void_p]),
    "usf_affine_prep_bwd_f32": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int64, C.c_int32,
                                          C.c_int32, _fp, _fp, _fp, _fp, C.c_void_p]),
}
for _stem in ("usf_conv_wgrad_wide", "usf_conv_wgrad_k5", "usf_conv_wgrad_k4"):      # the stream-ordered weight-gradient kernels: one block of signatures
    INTERNAL_SYMBOLS.update({
        _stem + "_workspace": (C.c_int64, [C.c_int64] * 6),
        _stem + "_f32": INTERNAL_SYMBOLS["usf_conv_wgrad_f32"],
        _stem + "_variant": (C.c_int, [C.POINTER(ConvWgradQuery), C.POINTER(ConvWgradWideInfo)]),
        _stem + "_instances": (C.c_int, [C.POINTER(C.c_int32), C.c_int32])})
_wide = INTERNAL_SYMBOLS["usf_conv_wgrad_wide_f32"]
INTERNAL_SYMBOLS.update({                                                                # the same contract + band_rows in front of the stream
    "usf_conv_wgrad_band_workspace": (C.c_int64, [C.c_int64] * 7),
    "usf_conv_wgrad_band_f32": (_wide[0], _wide[1][:-1] + [C.c_int64] + _wide[1][-1:]),
    "usf_conv_wgrad_band_variant": (C.c_int, [C.POINTER(ConvWgradBandQuery), C.POINTER(ConvWgradBandInfo)]),
    "usf_conv_wgrad_band_instances": (C.c_int, [C.POINTER(C.c_int32), C.c_int32])})
SYMBOLS = {**PUBLIC_SYMBOLS, **INTERNAL_SYMBOLS}
