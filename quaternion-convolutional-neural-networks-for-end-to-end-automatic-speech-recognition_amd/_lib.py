"""ctypes binding of libqk_hip.so -- the C-ABI declared in include/qk.h.

The product path has NO fallback: if the library is missing or a call fails, a RuntimeError
is raised.  (The CPU oracle under oracle/ is test infrastructure and is never imported here.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.realpath(__file__))
# QK_LIB: diagnostic override (A/B runs of two builds of the library on one GPU box, tools/ab_layers.py)
LIB_PATH = os.environ.get('QK_LIB') or os.path.join(_HERE, 'libqk_hip.so')

QK_F32, QK_BF16, QK_F16 = 0, 1, 2
QK_CH_LAST, QK_CH_FIRST = 0, 1
QK_ACT_LINEAR, QK_ACT_RELU = 0, 1
QK_OP_FWD, QK_OP_BWD_DATA, QK_OP_BWD_WEIGHT, QK_OP_BWD = 0, 1, 2, 3
QK_KERNEL_TAPS_MAJOR, QK_KERNEL_CHANNEL_MAJOR = 0, 1            # qk_conv_desc_t.kernel_order
QK_BWD_MASK_DX, QK_BWD_DY_PREMASKED, QK_BWD_ACCUMULATE = 1, 2, 4      # flags of qk_*_bwd_chain
QK_DBG_NO_MFMA16, QK_DBG_NO_BAND16, QK_DBG_NO_BAND32, QK_DBG_WGRAD16_ONE_TAP, QK_DBG_BAND16_8WAVES = 1, 2, 4, 8, 16   # qk_set_debug_flags
QK_DBG_NO_WGRAD_BAND = 32
QK_DBG_NO_POINT16 = 64
QK_DBG_CTC_TWO_SWEEPS = 128
QK_DBG_DETERMINISTIC = 0x10000
QK_DBG_WGRAD_BAND_V1 = 0x20000
QK_DBG_NO_SMALL16 = 0x40000
# graph-level A/B switches (include/qk.h): kept in the library's mask, acted on by models/interspeech_model.py and layers.py
QK_DBG_NO_CONV_CHAIN, QK_DBG_NO_FUSED_PRELU, QK_DBG_NO_FUSED_DROPOUT, QK_DBG_NO_FUSED_CTC = 0x100000, 0x200000, 0x400000, 0x800000
QK_DBG_NO_FUSED_FIRST, QK_DBG_NO_DENSE_IN_CHAIN, QK_DBG_NO_FUSED_SOFTMAX = 0x1000000, 0x2000000, 0x4000000
QK_DBG_NO_MASK_BITS = 0x8000000        # relu + dropout chains: the next layer's backward-data re-reads y instead of its bit-packed mask (functional._ConvChainFn)
QK_WAVE_F32, QK_WAVE_I16 = 0, 1                                  # acoustic front end (qk_fbank_quaternion)
QK_WINDOW_RECT, QK_WINDOW_HAMMING = 0, 1
QK_FBANK_NORM_NONE, QK_FBANK_NORM_UTTERANCE = 0, 1
QK_FBANK_MAX_FILT = 128
QK_SPECAUG_MAX_MASKS, QK_SPECAUG_PLAN_WORDS = 8, 36             # SpecAugment (qk_spec_augment)
QK_SPEED_MAX_SPEEDS, QK_SPEED_MAX_DEN, QK_SPEED_MAX_TAPS, QK_SPEED_PLAN_WORDS = 8, 32, 64, 4       # qk_speed_perturb
QK_REVERB_MAX_TAPS, QK_NOISE_REVERB_PLAN_WORDS = 8192, 8                                          # qk_noise_reverb
QK_ERR_INVALID_ARG, QK_ERR_UNSUPPORTED, QK_ERR_WORKSPACE, QK_ERR_LAUNCH = -1, -2, -3, -4
QK_PATH_NAMES = {0: 'none', 1: 'mfma16', 2: 'mfma16_band', 3: 'fp32_mfma', 4: 'mfma16_point', 5: 'mfma16_small'}               # qk_last_path

I32 = ctypes.c_int32


class ConvDesc(ctypes.Structure):
    _fields_ = [('rank', I32), ('batch', I32), ('in_spatial', I32 * 3), ('out_spatial', I32 * 3),
                ('cq', I32), ('fq', I32), ('kernel', I32 * 3), ('stride', I32 * 3),
                ('dilation', I32 * 3), ('pad_lo', I32 * 3), ('layout', I32), ('dtype', I32),
                ('activation', I32), ('has_bias', I32), ('conj', I32), ('ws_has_kernel', I32), ('kernel_order', I32)]


class DenseDesc(ctypes.Structure):
    _fields_ = [('rows', I32), ('in_q', I32), ('q_units', I32), ('dtype', I32),
                ('activation', I32), ('has_bias', I32), ('ws_has_kernel', I32)]


# every symbol include/qk.h declares: name -> (restype, argtypes)
_VP, _FP, _SZ = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t
_CD, _DD = ctypes.POINTER(ConvDesc), ctypes.POINTER(DenseDesc)
class PoolDesc(ctypes.Structure):
    """qk_pool_desc_t (include/qk.h)."""
    _fields_ = [('batch', ctypes.c_int32), ('in_h', ctypes.c_int32), ('in_w', ctypes.c_int32),
                ('channels', ctypes.c_int32), ('win_h', ctypes.c_int32), ('win_w', ctypes.c_int32),
                ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32), ('dtype', ctypes.c_int32)]


_PD = ctypes.POINTER(PoolDesc)


class PostOp(ctypes.Structure):
    """qk_postop_t (include/qk.h): PReLU (+ Dropout) behind a layer."""
    _fields_ = [('alpha_axis', ctypes.c_int32), ('alpha_len', ctypes.c_int32), ('alpha', ctypes.c_void_p),
                ('drop_rate', ctypes.c_float), ('drop_seed', ctypes.c_uint32), ('drop_seed_dev', ctypes.c_void_p)]


_PO = ctypes.POINTER(PostOp)

class ProfRec(ctypes.Structure):
    """qk_prof_rec_t (include/qk.h)"""
    _fields_ = [('op', I32), ('dtype', I32), ('path', I32), ('rows', ctypes.c_int64), ('n', I32), ('k', I32),
                ('ms', ctypes.c_float)]


class GradGuardConfig(ctypes.Structure):
    """qk_grad_guard_config_t (include/qk.h)"""
    _fields_ = [('clipnorm', ctypes.c_float), ('clipvalue', ctypes.c_float), ('dynamic', I32),
                ('growth_factor', ctypes.c_float), ('backoff_factor', ctypes.c_float), ('growth_interval', I32),
                ('min_scale', ctypes.c_float), ('max_scale', ctypes.c_float)]


class SpecAugPolicy(ctypes.Structure):
    """qk_specaug_t (include/qk.h)"""
    _fields_ = [('time_warp', I32), ('freq_masks', I32), ('freq_width', I32), ('time_masks', I32), ('time_width', I32),
                ('time_ratio', ctypes.c_float), ('fill', ctypes.c_float), ('seed', ctypes.c_uint32)]


class SpeedPerturbPolicy(ctypes.Structure):
    """qk_speed_perturb_t (include/qk.h)"""
    _fields_ = [('n_speeds', I32), ('num', I32 * 8), ('den', I32 * 8), ('half_width', I32 * 8), ('table_offset', I32 * 8),
                ('gain_lo', ctypes.c_float), ('gain_hi', ctypes.c_float), ('seed', ctypes.c_uint32)]


class NoiseReverbPolicy(ctypes.Structure):
    """qk_noise_reverb_t (include/qk.h)"""
    _fields_ = [('n_rirs', I32), ('rir_stride', I32), ('n_noises', I32), ('noise_stride', I32), ('rir_prob_q24', I32),
                ('noise_prob_q24', I32), ('snr_lo', ctypes.c_float), ('snr_hi', ctypes.c_float), ('seed', ctypes.c_uint32)]


# qk_grad_guard_state_t: eight 4-byte fields in device memory; (name, is_float) in order
GRAD_GUARD_STATE = (('scale', True), ('good_steps', False), ('skipped_steps', False), ('last_skipped', False),
                    ('last_norm', True), ('last_coef', True), ('last_unscale', True), ('nonfinite_count', False))
_GC = ctypes.POINTER(GradGuardConfig)

SYMBOLS = {
    'qk_version': (ctypes.c_int, []),
    'qk_prof_enable': (ctypes.c_int, [ctypes.c_int]),
    'qk_prof_count': (ctypes.c_int, []),
    'qk_prof_get': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ProfRec)]),
    'qk_last_error': (ctypes.c_char_p, []),
    'qk_set_debug_flags': (ctypes.c_uint, [ctypes.c_uint]),
    'qk_get_debug_flags': (ctypes.c_uint, []),
    'qk_set_debug_buffer': (None, [_VP, _SZ]),
    'qk_last_path': (ctypes.c_int, []),
    'qk_conv_workspace_bytes': (_SZ, [_CD, ctypes.c_int]),
    'qk_dense_workspace_bytes': (_SZ, [_DD, ctypes.c_int]),
    'qk_conv_fwd': (ctypes.c_int, [_CD, _VP, _FP, _FP, _VP, _VP, _SZ, _VP]),
    'qk_conv_bwd_data': (ctypes.c_int, [_CD, _VP, _VP, _FP, _VP, _VP, _SZ, _VP]),
    'qk_conv_fwd_post': (ctypes.c_int, [_CD, _PO, _VP, _FP, _FP, _VP, _VP, _VP, _SZ, _VP]),
    'qk_conv_bwd_post': (ctypes.c_int, [_CD, _VP, _VP, _FP, _VP, _FP, _FP, _PO, _VP, _FP, I32, _VP, _SZ, _VP]),
    'qk_conv_mask_bits_bytes': (_SZ, [_CD]),
    'qk_conv_bwd_reads_mask_bits': (ctypes.c_int, [_CD]),
    'qk_conv_fwd_post_bits': (ctypes.c_int, [_CD, _PO, _VP, _FP, _FP, _VP, _VP, _VP, _VP, _SZ, _VP]),
    'qk_conv_bwd_post_bits': (ctypes.c_int, [_CD, _VP, _VP, _VP, _FP, _VP, _FP, _FP, _PO, I32, _VP, _SZ, _VP]),
    'qk_postop_fwd': (ctypes.c_int, [_CD, _PO, _VP, _VP, _VP]),
    'qk_postop_bwd': (ctypes.c_int, [_CD, _PO, _VP, _VP, _VP, _FP, _VP]),
    'qk_conv_bwd_weight': (ctypes.c_int, [_CD, _VP, _VP, _VP, _FP, _FP, _VP, _SZ, _VP]),
    'qk_conv_bwd_chain': (ctypes.c_int, [_CD, _VP, _VP, _VP, _FP, _VP, _FP, _FP, I32, _VP, _SZ, _VP]),
    'qk_dense_bwd_chain': (ctypes.c_int, [_DD, _VP, _VP, _VP, _FP, _VP, _FP, _FP, I32, _VP, _SZ, _VP]),
    'qk_conv_bwd_weight_acc': (ctypes.c_int, [_CD, _VP, _VP, _VP, _FP, _FP, _VP, _SZ, _VP]),
    'qk_dense_bwd_weight_acc': (ctypes.c_int, [_DD, _VP, _VP, _VP, _FP, _FP, _VP, _SZ, _VP]),
    'qk_conv_bwd': (ctypes.c_int, [_CD, _VP, _VP, _VP, _FP, _VP, _FP, _FP, _VP, _SZ, _VP]),
    'qk_dense_bwd': (ctypes.c_int, [_DD, _VP, _VP, _VP, _FP, _VP, _FP, _FP, _VP, _SZ, _VP]),
    'qk_conv_fold_taps': (ctypes.c_int, [_CD, _VP, _VP, I32, _VP]),
    'qk_conv_relu_pool_aux_bytes': (_SZ, [_CD, I32]),
    'qk_conv_relu_pool_fwd': (ctypes.c_int, [_CD, I32, _VP, _FP, _FP, _VP, _VP, _VP]),
    'qk_conv_relu_pool_bwd': (ctypes.c_int, [_CD, I32, _VP, _VP, _VP, _FP, _FP, I32, _VP]),
    'qk_conv_prelu_pool_fwd': (ctypes.c_int, [_CD, I32, _PO, _VP, _FP, _FP, _VP, _VP, _VP, _VP]),
    'qk_conv_prelu_pool_bwd': (ctypes.c_int, [_CD, I32, _PO, _VP, _VP, _VP, _VP, _FP, _FP, _FP, I32, _VP]),
    'qk_dense_fwd': (ctypes.c_int, [_DD, _VP, _FP, _FP, _VP, _VP, _SZ, _VP]),
    'qk_dense_bwd_data': (ctypes.c_int, [_DD, _VP, _VP, _FP, _VP, _VP, _SZ, _VP]),
    'qk_dense_bwd_weight': (ctypes.c_int, [_DD, _VP, _VP, _VP, _FP, _FP, _VP, _SZ, _VP]),
    'qk_adam_step_zero_grad': (ctypes.c_int, [_FP, _FP, _FP, _FP, _SZ, ctypes.c_float, ctypes.c_float,
                                              ctypes.c_float, ctypes.c_float, I32, ctypes.c_float, _VP]),
    'qk_ctc_workspace_bytes': (_SZ, [I32, I32, I32]),
    'qk_ctc_batch_cost': (ctypes.c_int, [I32, I32, I32, I32, _VP, _VP, I32, _VP, _VP, _FP, _VP, _VP, _SZ, _VP]),
    'qk_conv_prep_kernels': (ctypes.c_int, [I32, ctypes.POINTER(_CD), ctypes.POINTER(I32), ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_void_p), _VP]),
    'qk_adam_step_l2': (ctypes.c_int, [_FP, _FP, _FP, _FP, _FP, _SZ, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_float, I32, ctypes.c_float, I32, _VP]),
    'qk_adam_step_dev': (ctypes.c_int, [_FP, _FP, _FP, _FP, _FP, _SZ, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_float, ctypes.c_float, _VP, ctypes.c_float, I32, _VP]),
    'qk_ctc_greedy_decode': (ctypes.c_int, [I32, I32, I32, I32, _VP, _VP, _VP, _VP, _FP, _VP]),
    'qk_ctc_beam_workspace_bytes': (_SZ, [I32, I32, I32]),
    'qk_ctc_beam_search_decode': (ctypes.c_int, [I32, I32, I32, I32, _VP, _VP, I32, I32, I32, _VP, _VP, _FP, _VP, _SZ, _VP]),
    'qk_ctc_beam_search_decode_lm': (ctypes.c_int, [I32, I32, I32, I32, _VP, _VP, I32, I32, I32, I32, _FP, ctypes.c_float,
                                                    ctypes.c_float, I32, _VP, _VP, _FP, _FP, _VP, _SZ, _VP]),
    'qk_edit_distance': (ctypes.c_int, [I32, _VP, I32, _VP, _VP, I32, _VP, _VP, I32, _VP, _VP, _VP]),
    'qk_edit_align_workspace_bytes': (_SZ, [I32, I32, I32]),
    'qk_edit_align': (ctypes.c_int, [I32, _VP, I32, _VP, _VP, I32, _VP, _VP, I32, _VP, _VP, _VP, _VP, _VP, I32, _VP, _SZ, _VP]),
    'qk_ctc_align_workspace_bytes': (_SZ, [I32, I32, I32]),
    'qk_ctc_forced_align': (ctypes.c_int, [I32, I32, I32, I32, _VP, _VP, I32, _VP, _VP, _VP, _VP, _VP, _FP, _VP, _SZ, _VP]),
    'qk_fbank_num_frames': (I32, [ctypes.c_int64, I32, I32]),
    'qk_fbank_workspace_bytes': (_SZ, [I32, I32, I32, I32]),
    'qk_fbank_quaternion': (ctypes.c_int, [I32, I32, ctypes.c_int64, _VP, _VP, I32, I32, I32, I32, ctypes.c_float, I32, I32,
                                           ctypes.POINTER(I32), I32, I32, I32, I32, _VP, _VP, _VP, _SZ, _VP]),
    'qk_spec_augment': (ctypes.c_int, [I32, I32, I32, I32, I32, I32, _VP, _VP, ctypes.POINTER(SpecAugPolicy), _VP, _VP, _VP, _VP]),
    'qk_speed_perturb_out_samples': (ctypes.c_int64, [ctypes.c_int64, ctypes.POINTER(SpeedPerturbPolicy)]),
    'qk_speed_perturb': (ctypes.c_int, [I32, I32, ctypes.c_int64, _VP, _VP, ctypes.POINTER(SpeedPerturbPolicy), _VP, _VP, ctypes.c_int64,
                                        _VP, _VP, _VP, _VP]),
    'qk_noise_reverb_workspace_bytes': (ctypes.c_int64, [I32, ctypes.c_int64]),
    'qk_noise_reverb': (ctypes.c_int, [I32, I32, ctypes.c_int64, _VP, _VP, ctypes.POINTER(NoiseReverbPolicy), _VP, _VP, _VP, _VP, _VP, _VP,
                                       _VP, _VP, _VP, ctypes.c_int64, _VP]),
    'qk_softmax_rows_fwd': (ctypes.c_int, [I32, ctypes.c_int64, I32, _VP, _VP, _VP, _VP]),
    'qk_softmax_rows_bwd': (ctypes.c_int, [I32, ctypes.c_int64, I32, _VP, _VP, _VP, _VP, _VP]),
    'qk_dense_softmax_supported': (ctypes.c_int, [I32, ctypes.c_int64, I32, I32]),
    'qk_dense_softmax_fwd': (ctypes.c_int, [I32, ctypes.c_int64, I32, I32, _VP, _VP, _VP, _VP, _VP]),
    'qk_dense_softmax_bwd_workspace_bytes': (ctypes.c_size_t, [I32, ctypes.c_int64, I32, I32]),
    'qk_dense_softmax_bwd': (ctypes.c_int, [I32, ctypes.c_int64, I32, I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, ctypes.c_float, _VP, _SZ, _VP]),
    'qk_weighted_sum': (ctypes.c_int, [I32, ctypes.c_int64, _VP, _VP, _VP, _VP]),
    'qk_maxpool2d_fwd': (ctypes.c_int, [_PD, _VP, _VP, _VP]),
    'qk_maxpool2d_bwd': (ctypes.c_int, [_PD, _VP, _VP, _VP, _VP]),
    'qk_adam_step': (ctypes.c_int, [_FP, _FP, _FP, _FP, _SZ, ctypes.c_float, ctypes.c_float,
                                    ctypes.c_float, ctypes.c_float, I32, ctypes.c_float, _VP]),
    'qk_grad_guard_workspace_bytes': (_SZ, [_SZ]),
    'qk_grad_guard_reduce': (ctypes.c_int, [_FP, _FP, _FP, _SZ, ctypes.c_float, _GC, _VP, _VP, _SZ, _VP]),
    'qk_adam_step_guarded': (ctypes.c_int, [_FP, _FP, _FP, _FP, _FP, _SZ, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                            ctypes.c_float, _VP, I32, _GC, _VP, _VP]),
}

# ---- include/qk_opt.h: the scheduled optimiser step (a second table: SYMBOLS stays the inventory of include/qk.h) ----
QK_LR_CONSTANT, QK_LR_INVERSE_TIME, QK_LR_EXPONENTIAL, QK_LR_COSINE, QK_LR_INV_SQRT = 0, 1, 2, 3, 4
QK_LR_KINDS = {'constant': QK_LR_CONSTANT, 'inverse-time': QK_LR_INVERSE_TIME, 'exponential': QK_LR_EXPONENTIAL,
               'cosine': QK_LR_COSINE, 'inv-sqrt': QK_LR_INV_SQRT}


class LRScheduleDesc(ctypes.Structure):
    """qk_lr_schedule_t (include/qk_opt.h)"""
    _fields_ = [('base_lr', ctypes.c_double), ('kind', I32), ('warmup_steps', I32), ('total_steps', I32), ('decay_steps', I32),
                ('rate', ctypes.c_double), ('floor', ctypes.c_double)]


# qk_opt_state_t: eight 4-byte words in device memory; (name, is_float) in order
OPT_STATE = (('lr_scale', True), ('last_lr', True), ('last_ema_decay', True), ('ema_updates', False),
             ('reserved0', False), ('reserved1', False), ('reserved2', False), ('reserved3', False))
_LS = ctypes.POINTER(LRScheduleDesc)

OPT_SYMBOLS = {
    'qk_adam_step_sched': (ctypes.c_int, [_FP, _FP, _FP, _FP, _FP, _FP, _SZ, _LS, ctypes.c_float, I32, ctypes.c_float, ctypes.c_float,
                                          ctypes.c_float, ctypes.c_float, _VP, I32, _GC, _VP, _VP, _VP]),
    'qk_swap_f32': (ctypes.c_int, [_FP, _FP, _SZ, _VP]),
    'qk_lr_schedule_value': (ctypes.c_int, [_LS, ctypes.c_int64, ctypes.c_float, ctypes.POINTER(ctypes.c_float)]),
}

# ---- include/qk_data.h: the device-resident corpus (a third table, for the same reason) ----
QK_CORPUS_PLAN_WORDS = 4
_I64 = ctypes.c_int64


class CorpusDesc(ctypes.Structure):
    """qk_corpus_t (include/qk_data.h)"""
    _fields_ = [('wave_pack', _VP), ('wave_off', _VP), ('wave_len', _VP), ('label_pack', _VP), ('label_off', _VP), ('label_len', _VP),
                ('aux_pack', _VP), ('wave_samples', _I64), ('label_words', _I64), ('num_utts', I32), ('reserved', I32)]


class BatchScheduleDesc(ctypes.Structure):
    """qk_batch_schedule_t (include/qk_data.h)"""
    _fields_ = [('batches', _VP), ('num_batches', I32), ('batch', I32), ('seed', ctypes.c_uint32), ('shuffle', I32)]


DATA_SYMBOLS = {
    'qk_corpus_batch': (ctypes.c_int, [ctypes.POINTER(CorpusDesc), ctypes.POINTER(BatchScheduleDesc), ctypes.c_uint32, _VP, I32, I32,
                                       _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    'qk_epoch_permutation': (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, I32, ctypes.POINTER(I32)]),
}

# ---- include/qk_rnn.h: the quaternion LSTM recurrence (a fourth table, for the same reason) ----
QK_QLSTM_REVERSE = 1
QK_QLSTM_PATH_GENERIC, QK_QLSTM_PATH_MFMA16 = 1, 2
QK_QLSTM_PATH_NAMES = {0: 'none', QK_QLSTM_PATH_GENERIC: 'generic', QK_QLSTM_PATH_MFMA16: 'mfma16'}


class QLSTMDesc(ctypes.Structure):
    """qk_qlstm_desc_t (include/qk_rnn.h)"""
    _fields_ = [('dtype', I32), ('batch', I32), ('steps', I32), ('q_units', I32), ('directions', I32), ('y_stride', I32), ('flags', I32)]


_QD = ctypes.POINTER(QLSTMDesc)

RNN_SYMBOLS = {
    'qk_qlstm_supported': (ctypes.c_int, [_QD]),
    'qk_qlstm_workspace_bytes': (_SZ, [_QD, I32]),
    'qk_qlstm_reserve_bytes': (_SZ, [_QD]),
    'qk_qlstm_fwd': (ctypes.c_int, [_QD, _VP, _FP, _VP, _VP, _FP, _VP, _VP, _FP, _VP, _VP, _SZ, _VP]),
    'qk_qlstm_bwd': (ctypes.c_int, [_QD, _VP, _VP, _FP, _FP, _VP, _VP, _FP, _VP, _VP, _VP, _VP, _VP, _FP, _VP, _SZ, _VP]),
}

# ---- include/qk_norm.h: quaternion layer normalisation (a fifth table, for the same reason) ----
QK_QLNORM_PATH_GENERIC, QK_QLNORM_PATH_VEC = 1, 2
QK_QLNORM_PATH_NAMES = {0: 'none', QK_QLNORM_PATH_GENERIC: 'generic', QK_QLNORM_PATH_VEC: 'vec'}


class QLNormDesc(ctypes.Structure):
    """qk_qlnorm_desc_t (include/qk_norm.h)"""
    _fields_ = [('dtype', I32), ('rows', I32), ('steps', I32), ('q', I32), ('x_stride', I32), ('y_stride', I32), ('flags', I32)]


_ND = ctypes.POINTER(QLNormDesc)

NORM_SYMBOLS = {
    'qk_qlnorm_supported': (ctypes.c_int, [_ND]),
    'qk_qlnorm_slab_rows': (ctypes.c_int, [_ND]),
    'qk_qlnorm_workspace_bytes': (_SZ, [_ND, I32]),
    'qk_qlnorm_fwd': (ctypes.c_int, [_ND, _VP, _FP, _FP, _VP, ctypes.c_float, _VP, _FP, _VP]),
    'qk_qlnorm_bwd': (ctypes.c_int, [_ND, _VP, _VP, _FP, _VP, _FP, _VP, _FP, _FP, _VP, _SZ, _VP]),
}

# ---- include/qk_attn.h: quaternion multi-head self-attention (a sixth table, for the same reason) ----
QK_QATTN_PATH_GENERIC, QK_QATTN_PATH_MFMA = 1, 2
QK_QATTN_PATH_NAMES = {0: 'none', QK_QATTN_PATH_GENERIC: 'generic', QK_QATTN_PATH_MFMA: 'mfma'}


class QAttnDesc(ctypes.Structure):
    """qk_qattn_desc_t (include/qk_attn.h)"""
    _fields_ = [('dtype', I32), ('batch', I32), ('steps', I32), ('heads', I32), ('dq', I32), ('q_row', I32), ('q_comp', I32),
                ('k_row', I32), ('k_comp', I32), ('v_row', I32), ('v_comp', I32), ('o_row', I32), ('o_comp', I32), ('flags', I32)]


_AD = ctypes.POINTER(QAttnDesc)

ATTN_SYMBOLS = {
    'qk_qattn_supported': (ctypes.c_int, [_AD]),
    'qk_qattn_workspace_bytes': (_SZ, [_AD, I32]),
    'qk_qattn_fwd': (ctypes.c_int, [_AD, _VP, _VP, _VP, _VP, ctypes.c_float, _VP, _FP, _VP]),
    'qk_qattn_bwd': (ctypes.c_int, [_AD, _VP, _VP, _VP, _VP, _VP, _FP, _VP, ctypes.c_float, _VP, _VP, _VP, _VP, _SZ, _VP]),
}

# ---- include/qk_dwconv.h: depthwise quaternion convolution with a fused GLU gate (a seventh table, for the same reason) ----
QK_QDWCONV_PATH_GENERIC, QK_QDWCONV_PATH_VEC = 1, 2
QK_QDWCONV_PATH_NAMES = {0: 'none', QK_QDWCONV_PATH_GENERIC: 'generic', QK_QDWCONV_PATH_VEC: 'vec'}


class QDWConvDesc(ctypes.Structure):
    """qk_qdwconv_desc_t (include/qk_dwconv.h)"""
    _fields_ = [('dtype', I32), ('batch', I32), ('steps', I32), ('units', I32), ('taps', I32), ('pad_lo', I32), ('x_row', I32),
                ('x_comp', I32), ('y_row', I32), ('y_comp', I32), ('flags', I32)]


_WD = ctypes.POINTER(QDWConvDesc)

DWCONV_SYMBOLS = {
    'qk_qdwconv_supported': (ctypes.c_int, [_WD]),
    'qk_qdwconv_workspace_bytes': (_SZ, [_WD, I32]),
    'qk_qdwconv_last_path': (ctypes.c_int, []),
    'qk_qdwconv_fwd': (ctypes.c_int, [_WD, _VP, _VP, _FP, _FP, _VP, _VP, _VP]),
    'qk_qdwconv_bwd': (ctypes.c_int, [_WD, _VP, _VP, _VP, _FP, _VP, _VP, _VP, _FP, _FP, _VP, _SZ, _VP]),
}

# ---- include/qk_rnnt.h: the transducer (RNN-T) loss (an eighth table, for the same reason) ----
QK_RNNT_MAX_CLASSES, QK_RNNT_MAX_U1 = 256, 128

RNNT_SYMBOLS = {
    'qk_rnnt_supported': (ctypes.c_int, [I32, I32, I32, I32, I32]),
    'qk_rnnt_workspace_bytes': (_SZ, [I32, I32, I32, I32]),
    'qk_rnnt_loss': (ctypes.c_int, [I32, I32, I32, I32, I32, _VP, _VP, _VP, _VP, _FP, _VP, _VP, _SZ, _VP]),
}

_lib = None


def lib():
    """The loaded library; raises RuntimeError (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'libqk_hip.so is not built (%s). Run `python -c "import __graft_entry__ as g; '
                'g.build()"` -- the quaternion layers have no CPU or eager fallback.' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for table in (SYMBOLS, OPT_SYMBOLS, DATA_SYMBOLS, RNN_SYMBOLS, NORM_SYMBOLS, ATTN_SYMBOLS, DWCONV_SYMBOLS, RNNT_SYMBOLS):
            for name, (res, args) in table.items():
                fn = getattr(handle, name)
                fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().qk_last_error()
        raise RuntimeError('%s failed (status %d): %s' % (what, rc, msg.decode() if msg else ''))


def dbg(bit):
    """True when diagnostic bit `bit` of the library's process-wide mask is set (qk_get_debug_flags: one relaxed atomic load; the
    mask's initial value was read from the environment ONCE, when the library initialised it)."""
    return bool(lib().qk_get_debug_flags() & bit)


class debug_flags(object):
    """`with debug_flags(QK_DBG_NO_MFMA16): ...` -- OR the given diagnostic bits into the library's process-wide
    mask (qk_set_debug_flags) for the duration of the block.  Tests and profiling only."""

    def __init__(self, bits, ablate=0):
        self.bits = int(bits) | (int(ablate) << 8)

    def __enter__(self):
        self.prev = lib().qk_get_debug_flags()
        lib().qk_set_debug_flags(self.prev | self.bits)
        return self

    def __exit__(self, *exc):
        lib().qk_set_debug_flags(self.prev)
        return False


class profile(object):
    """`with profile() as p: step()` then `p.records()`: every forward / backward-data / backward-weight call made
    inside the block (any thread, any stream) with its GEMM view and the milliseconds its launches took on their
    stream (qk_prof_*, HIP events recorded by the library).  records() synchronises."""

    OPS = {QK_OP_FWD: 'fwd', QK_OP_BWD_DATA: 'bwd_data', QK_OP_BWD_WEIGHT: 'bwd_weight'}

    def __enter__(self):
        lib().qk_prof_enable(1)
        return self

    def __exit__(self, *exc):
        lib().qk_prof_enable(0)
        return False

    def records(self):
        out = []
        rec = ProfRec()
        for i in range(lib().qk_prof_count()):
            check(lib().qk_prof_get(i, ctypes.byref(rec)), 'qk_prof_get')
            out.append(dict(op=self.OPS.get(rec.op, str(rec.op)), dtype=rec.dtype, path=QK_PATH_NAMES.get(rec.path, 'none'),
                            rows=int(rec.rows), n=int(rec.n), k=int(rec.k), ms=float(rec.ms)))
        return out


def last_path():
    """Kernel family that served this thread's most recent compute call: 'mfma16', 'mfma16_band', 'fp32_mfma'."""
    return QK_PATH_NAMES.get(lib().qk_last_path(), 'none')
