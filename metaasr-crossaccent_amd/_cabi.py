"""ctypes binding of libmasr.so (include/masr.h; the masr_test_* entries are include/masr_test.h).  No fallback: if the HIP library is missing the
import raises -- the product path never runs on the CPU oracle."""
import ctypes as C
import math
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MASR_LIB", _HERE / "lib" / "libmasr.so"))


class MasrConfig(C.Structure):
    _fields_ = [("idim", C.c_int32), ("odim", C.c_int32), ("d_model", C.c_int32), ("nheads", C.c_int32),
                ("d_inner", C.c_int32), ("enc_layers", C.c_int32), ("dec_layers", C.c_int32),
                ("tie_weights", C.c_int32), ("dropout", C.c_float), ("pos_dropout", C.c_float),
                ("label_smoothing", C.c_float)]


class MasrSpecaugPolicy(C.Structure):
    _fields_ = [("time_warp", C.c_int32), ("freq_masks", C.c_int32), ("freq_width", C.c_int32), ("freq_bins", C.c_int32),
                ("time_masks", C.c_int32), ("time_width", C.c_int32), ("time_ratio", C.c_float)]


class MasrChunkPolicy(C.Structure):
    _fields_ = [("size", C.c_int32), ("left", C.c_int32), ("dynamic", C.c_int32)]


vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
_SIGS = {
    "masr_version": (C.c_int, []),
    "masr_last_error": (C.c_char_p, []),
    "masr_create": (vp, [C.POINTER(MasrConfig)]),
    "masr_create_ctc": (vp, [C.POINTER(MasrConfig), f32]),
    "masr_destroy": (None, [vp]),
    "masr_param_numel": (i64, [vp]),
    "masr_param_count": (i32, [vp]),
    "masr_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]),
    "masr_workspace_bytes": (i64, [vp, i32, i32, i32]),
    "masr_bind": (i32, [vp, vp, vp, vp, vp, i64]),
    "masr_refresh": (i32, [vp, vp]),
    "masr_set_seed": (None, [vp, C.c_uint64]),
    "masr_set_concurrency": (None, [vp, i32]),
    "masr_dropout_state": (None, [vp, C.POINTER(C.c_uint64), i32]),
    "masr_run_batch": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "masr_set_step_graphs": (None, [vp, i32]),
    "masr_set_split_wgrad_launches": (None, [vp, i32]),
    "masr_set_ksplit": (None, [vp, i32]),
    "masr_set_drop_nan_grads": (None, [vp, i32]),
    "masr_step_counters": (None, [vp, C.POINTER(i64)]),
    "masr_read_stats": (i32, [vp, C.POINTER(f32), vp]),
    "masr_stats_post": (i64, [vp, vp]),
    "masr_stats_peek": (C.POINTER(C.c_uint32), [vp, i64]),
    "masr_stats_wait": (i32, [vp, i64, C.POINTER(f32)]),
    "masr_last_logits": (i32, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "masr_specaug": (i32, [vp, vp, vp, i32, i32, i32, C.POINTER(MasrSpecaugPolicy), C.c_uint64, C.c_uint64, vp]),
    "masr_set_specaug": (i32, [vp, C.POINTER(MasrSpecaugPolicy)]),
    "masr_specaug_last": (i32, [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "masr_set_chunk": (i32, [vp, C.POINTER(MasrChunkPolicy)]),
    "masr_chunk_draw": (i32, [C.c_uint64, C.c_uint64, i32]),
    "masr_chunk_last": (i32, [vp, C.POINTER(i32)]),
    "masr_grad_norm": (i32, [vp, vp]),
    "masr_clip_sgd_step": (i32, [vp, vp, f32, f32, f32, i32, i32, vp]),
    "masr_clip_grads": (i32, [vp, f32, vp]),
    "masr_clip_accumulate": (i32, [vp, vp, f32, vp]),
    "masr_clip_scale_flat": (i32, [vp, i64, vp, f32, vp]),
    "masr_adam_step": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i32, vp]),
    "masr_adam_step_guarded": (i32, [vp, vp, vp, vp, vp, i64, f32, i32, f32, i32, f32, f32, f32, f32, i32, i32, vp]),
    "masr_sum_n": (i32, [vp, vp, i32, f32, i64, vp]),
    "masr_adam_sum_step": (i32, [vp, vp, i32, f32, vp, vp, i64, f32, f32, f32, f32, i32, vp]),
    "masr_adamw_step": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, i32, vp]),
    "masr_radam_step": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, i32, vp]),
    "masr_sgd_step": (i32, [vp, vp, vp, i64, f32, f32, i32, i32, vp]),
    "masr_scale": (i32, [vp, i64, f32, vp]),
    "masr_axpy": (i32, [vp, vp, i64, f32, vp]),
    "masr_copy": (i32, [vp, vp, i64, vp]),
    "masr_allreduce_unique_id": (i32, [C.c_char_p]),
    "masr_allreduce_init": (vp, [i32, i32, C.c_char_p]),
    "masr_allreduce_destroy": (None, [vp]),
    "masr_allreduce": (i32, [vp, vp, i64, vp, f32, i32, vp]),
    "masr_allreduce_wait": (i32, [vp, vp]),
    "masr_allreduce_check": (i32, [vp, i32]),
    "masr_stats_device": (vp, [vp]),
    "masr_recog": (i32, [vp, vp, vp, i32, i32, vp, vp]),
    "masr_recog_full": (i32, [vp, vp, vp, i32, i32, vp, vp]),
    "masr_beam_workspace_bytes": (i64, [vp, i32, i32, i32, i32]),
    "masr_recog_beam": (i32, [vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp]),
    "masr_beam_ctc_workspace_bytes": (i64, [vp, i32, i32, i32, i32]),
    "masr_recog_beam_ctc": (i32, [vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp]),
    "masr_lm_create": (vp, [i32, i32, C.POINTER(i64), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "masr_lm_destroy": (None, [vp]),
    "masr_lm_bytes": (i64, [vp]),
    "masr_bias_create": (vp, [i32, i32, vp, vp]),
    "masr_bias_destroy": (None, [vp]),
    "masr_bias_bytes": (i64, [vp]),
    "masr_bias_nodes": (i32, [vp]),
    "masr_recog_ctc_beam_bias": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "masr_beam_bias_workspace_bytes": (i64, [vp, i32, i32, i32, i32]),
    "masr_recog_beam_bias": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp]),
    "masr_beam_ctc_bias_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32]),
    "masr_recog_beam_ctc_bias": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, f32, f32, vp, vp, vp, vp, vp]),
    "masr_recog_rescore_bias": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
    "masr_beam_lm_workspace_bytes": (i64, [vp, i32, i32, i32, i32]),
    "masr_recog_beam_lm": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp]),
    "masr_nlm_create": (vp, [i32, i32, i32, i32, i32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]),
    "masr_nlm_destroy": (None, [vp]),
    "masr_nlm_bytes": (i64, [vp]),
    "masr_beam_nlm_workspace_bytes": (i64, [vp, vp, i32, i32, i32, i32]),
    "masr_recog_beam_nlm": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp]),
    "masr_nlm_score_work_bytes": (i64, [vp, i32, i32]),
    "masr_nlm_score": (i32, [vp, vp, vp, i32, i32, vp, vp, i64, vp]),
    "masr_beam_ctc_lm_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32]),
    "masr_recog_beam_ctc_lm": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, f32, vp, vp, vp, vp]),
    "masr_beam_ctc_nlm_workspace_bytes": (i64, [vp, vp, i32, i32, i32, i32, i32]),
    "masr_recog_beam_ctc_nlm": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, f32, vp, vp, vp, vp]),
    "masr_ctc_beam_workspace_bytes": (i64, [vp, i32, i32, i32]),
    "masr_recog_ctc_beam": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "masr_recog_ctc_beam_lm": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp]),
    "masr_ctc_align_workspace_bytes": (i64, [vp, i32, i32, i32]),
    "masr_recog_ctc_align": (i32, [vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "masr_rescore_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32]),
    "masr_recog_rescore": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
    "masr_recog_rescore_lm": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
    "masr_ctc_beam_nlm_workspace_bytes": (i64, [vp, vp, i32, i32, i32]),
    "masr_recog_ctc_beam_nlm": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp]),
    "masr_rescore_nlm_workspace_bytes": (i64, [vp, vp, i32, i32, i32, i32, i32]),
    "masr_recog_rescore_nlm": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
    "masr_rescore_nbest": (i32, [vp, vp, vp, i32, i32, i32, vp, i64, vp, vp, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
    "masr_edit_distance": (i64, [vp, i32, vp, i32]),
    "masr_blstm_create": (vp, [vp]),
    "masr_blstm_destroy": (None, [vp]),
    "masr_blstm_param_numel": (i64, [vp]),
    "masr_blstm_param_count": (i32, [vp]),
    "masr_blstm_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]),
    "masr_blstm_workspace_bytes": (i64, [vp, i32, i32, i32]),
    "masr_blstm_bind": (i32, [vp, vp, vp, vp, i64]),
    "masr_blstm_refresh": (i32, [vp, vp]),
    "masr_blstm_run_batch": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "masr_blstm_forward": (i32, [vp, vp, vp, i32, i32, vp]),
    "masr_blstm_read_stats": (i32, [vp, C.POINTER(f32), vp]),
    "masr_blstm_set_resident_recurrence": (None, [vp, i32]),
    "masr_blstm_check": (i32, [vp, vp]),
    "masr_blstm_last_logits": (i32, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "masr_blstm_clip_grads": (i32, [vp, f32, vp]),
    "masr_blstm_clip_sgd_step": (i32, [vp, vp, f32, f32, f32, i32, i32, vp]),
    "masr_fbank": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "masr_fbank_pitch_work_bytes": (i64, [i64, i32, i32]),
    "masr_fbank_pitch": (i32, [vp, vp, vp, i64, i64, i32, i32, i32, vp, vp, i64, vp]),
    "masr_gather_pad": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "masr_ctc_work_floats": (i64, [i32, i32, i32]),
    "masr_ctc_status": (i32, [vp, i32, i32, i32, vp]),
    "masr_ctc_loss": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp]),
    "masr_ctc_beam_work_bytes": (i64, [i32, i32, i32, i32]),
    "masr_ctc_beam_search": (i32, [vp, i64, vp, i32, i32, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp]),
    "masr_ctc_beam_lm_work_bytes": (i64, [i32, i32, i32, i32]),
    "masr_ctc_beam_bias_work_bytes": (i64, [i32, i32, i32, i32]),
    "masr_ctc_beam_search_bias": (i32, [vp, i64, vp, i32, i32, i32, i32, i32, i32, i32, vp, f32, f32, vp, f32, vp, i64, vp, vp, vp, vp, vp, vp]),
    "masr_ctc_beam_search_lm": (i32, [vp, i64, vp, i32, i32, i32, i32, i32, i32, i32, vp, f32, f32, vp, i64, vp, vp, vp, vp, vp]),
    "masr_ctc_beam_run_work_bytes": (i64, [i32, i32, i32, i32]),
    "masr_ctc_beam_run_open": (vp, [vp, i64, vp, i32, i32, i32, i32, i32, i32, vp, f32, f32, vp, f32, vp, i64, vp]),
    "masr_ctc_beam_run_advance": (i32, [vp, i32, vp]),
    "masr_ctc_beam_run_result": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    "masr_ctc_beam_run_close": (None, [vp]),
    "masr_ctc_beam_nlm_work_bytes": (i64, [vp, i32, i32, i32, i32]),
    "masr_ctc_beam_search_nlm": (i32, [vp, i64, vp, i32, i32, i32, i32, i32, i32, i32, vp, f32, f32, vp, i64, vp, vp, vp, vp, vp]),
    "masr_ctc_align_work_bytes": (i64, [i32, i32, i32]),
    "masr_ctc_align": (i32, [vp, i64, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp]),
    "masr_profile_enable": (i32, [vp, i32]),
    "masr_profile_read": (i32, [vp, C.POINTER(f32), C.POINTER(i32)]),
    "masr_test_blstm_stall": (None, [vp, i32]),          # include/masr_test.h from here on
    "masr_test_gemm": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, vp, i32, vp, i64, vp]),
    "masr_test_dropout_mask": (i32, [C.c_uint32, C.c_uint32, i64, f32, vp, vp]),
    "masr_test_gemm_dropout": (i32, [vp, i64, vp, i64, i32, i32, i32, f32, C.c_uint32, C.c_uint32, vp, i64, vp]),
    "masr_test_attention_dropout": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, C.c_uint32, C.c_uint32, vp]),
    "masr_test_gemm_epi": (i32, [vp, i64, vp, i64, i32, i32, i32, vp, i32, f32, vp, vp, vp, vp, vp]),
    "masr_test_gemm_pe_acc": (i32, [vp, i64, vp, i64, i32, i32, i32, vp, vp, i32, i32, vp, i64, vp, i64, vp]),
    "masr_test_skinny_gemm": (i32, [vp, i64, vp, i64, i32, i32, i32, vp, i32, vp, vp, vp, vp]),
    "masr_test_ctc_prefix": (i32, [vp, i32, i32, i32, vp, f32, f32, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "masr_test_ctc_beam_logits": (i32, [vp, i32, i32, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp)]),
    "masr_test_ctc_align_logits": (i32, [vp, i32, i32, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp)]),
    "masr_test_ctc_align_no_trace": (i32, [vp, i64, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp]),
    "masr_test_rescore_score": (i32, [vp, i64, vp, i32, i32, i32, vp, vp, vp]),
    "masr_test_rescore_select": (i32, [vp, i64, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_rescore_logits": (i32, [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]),
    "masr_test_lm_score": (i32, [vp, vp, i32, vp, vp]),
    "masr_test_lm_max_probe": (i32, [vp]),
    "masr_test_bias_step": (i32, [vp, vp, vp, vp, i32, vp, vp, vp]),
    "masr_test_bias_max_probe": (i32, [vp]),
    "masr_test_beam_bias_rows": (i32, [vp, vp, f32, f32, i32, i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_beam_select_bias": (i32, [i32, i32, i32, i32, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_beam_select_nbest_bias": (i32, [i32, i32, i32, i32, i32, vp, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_beam_lm_topk": (i32, [vp, f32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
    "masr_test_joint_lm_prebeam": (i32, [vp, f32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_beam_nlm_rows": (i32, [vp, i64, f32, i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_ctc_prefix_lm": (i32, [vp, i32, i32, i32, vp, f32, f32, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "masr_test_beam_select_nbest": (i32, [i32, i32, i32, i32, i32, vp, f32] + [vp] * 15),
    "masr_test_attn_decode": (i32, [vp, i64, vp, vp, i64, i64, vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp, i64, i64, vp]),
    "masr_test_logits_f32": (i32, [vp, vp, vp, vp, i64, i32, i32, i32, vp]),
    "masr_test_recog_argmax_step": (i32, [vp, vp, i64, vp, i32, i32, vp]),
    "masr_test_beam_step": (i32, [i32, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_ls_ce": (i32, [vp, i64, vp, i32, i32, f32, f32, vp, f32, vp, vp, vp, vp, vp]),
    "masr_test_embed_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, C.c_uint32, C.c_uint32, vp, vp]),
    "masr_test_embed_bwd": (i32, [vp, i32, vp, vp, i32, i32, i32, f32, C.c_uint32, C.c_uint32, vp, vp]),
    "masr_test_cast_dropout": (i32, [vp, vp, i64, f32, C.c_uint32, C.c_uint32, vp, vp]),
    "masr_test_vgg2enc_grad_unpermute": (i32, [vp, vp, i32, i32, i32, vp]),
    "masr_test_recog_argmax": (i32, [vp, i64, vp, i32, i32, i32, vp]),
    "masr_test_linear_shadows": (i32, [vp, i64, i32, i32, i32, vp, vp, vp]),
    "masr_test_conv1_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "masr_test_conv3x3": (i32, [vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]),
    "masr_test_conv3x3_ex": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "masr_test_conv3x3_sign_bits": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "masr_test_conv3x3_pool_idx": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "masr_test_conv3x3_dgrad_pooled": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "masr_test_conv1_wgrad_fused_slab_floats": (i64, [i32, i32, i32]),
    "masr_test_conv1_wgrad_fused": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, vp]),
    "masr_test_conv3x3_wgrad": (i32, [vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp]),
    "masr_test_conv3x3_wgrad_slab_floats": (i64, [i32, i32, i32, i32, i32]),
    "masr_test_set_conv_grid_cap": (None, [i32]),
    "masr_test_wgrad_grouped": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, i32, i32, i32, vp]),
    "masr_test_ksplit_ln": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, f32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_wgrad_grouped_n": (i32, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, vp]),
    "masr_test_conv3x3_wgrad_pooled": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp]),
    "masr_test_layernorm_slab_floats": (i64, [i32, i32]),
    "masr_test_layernorm": (i32, [vp] * 13 + [i32, i32, f32, C.c_uint32, C.c_uint32, vp]),
    "masr_test_attention_dropout_bwd": (i32, [vp] * 10 + [i32] * 6 + [f32, C.c_uint32, C.c_uint32, vp]),
    "masr_test_attention_chunk": (i32, [vp] * 10 + [i32] * 6 + [f32, C.c_uint32, C.c_uint32, i32, i32, vp, vp]),
    "masr_test_attention": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "masr_test_attention_stream": (i32, [vp] * 7 + [i32] * 7 + [vp]),
    "masr_test_ctc_greedy_stream": (i32, [vp, i64, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp]),
    "masr_stream_workspace_bytes": (i64, [vp, i32, i32]),
    "masr_stream_begin": (i32, [vp, i32, i32, vp]),
    "masr_stream_feed": (i32, [vp, vp, i32, C.POINTER(C.c_int32), i32, C.POINTER(i32), vp]),
    "masr_stream_partial": (i32, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]),
    "masr_stream_logits": (i32, [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i32)]),
    "masr_stream_ctc_beam": (i32, [vp, i32, i32, vp, vp, vp, vp]),
    "masr_stream_beam_open": (i32, [vp, i32, vp, f32, f32, vp, f32, vp]),
    "masr_stream_beam_result": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    "masr_test_lstm_shadows": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "masr_test_lstm_unperm": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "masr_test_lstm_fwd": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_lstm_bwd": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "masr_test_lstm_hprev": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "masr_test_cast_rows_pad": (i32, [vp, vp, i64, i32, i32, vp]),
    "masr_test_tanh": (i32, [vp, vp, vp, vp, i64, vp]),
    "masr_test_mask_rows": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "masr_test_subsample_rows": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "masr_test_nlm_step": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp]),
    "masr_test_nlm_step_carry": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp]),
    "masr_test_sumsq": (i32, [vp, i64, vp, vp]),
    "masr_test_clip_sgd": (i32, [vp, vp, vp, i64, vp, f32, f32, f32, i32, i32, vp]),
    "masr_test_clip_axpy": (i32, [vp, vp, i64, vp, f32, i32, vp]),
    "masr_test_clip_scale": (i32, [vp, i64, vp, f32, i32, vp]),
    "masr_test_adam_guarded": (i32, [vp, vp, vp, vp, i64, f32, i32, f32, i32, f32, f32, f32, f32, i32, vp, vp, i32, vp]),
    "masr_test_shadow_jobs": (i32, [vp, i32, vp, vp, vp]),
    "masr_test_transpose_cast_bf16": (i32, [vp, vp, i32, i32, i64, vp]),
    "masr_test_cast_bf16": (i32, [vp, vp, i64, vp]),
    "masr_test_conv_weight_shadows": (i32, [vp, vp, vp, i32, i32, vp]),
    "masr_test_ctc_loss_layout": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, i32]),
    "masr_test_ctc_loss_joint": (i32, [vp, i64, vp, vp, vp, vp, i32, i32, i32, vp, vp, f32, vp, vp, i32, vp]),
}
EXPORTS = tuple(_SIGS)
PROF_NAMES = ("conv1_fwd", "conv2_fwd", "conv3_fwd", "conv4_fwd", "conv2_dgrad", "conv3_dgrad", "conv4_dgrad", "conv2_wgrad",
              "conv3_wgrad", "conv4_wgrad", "conv1_wgrad", "gemm_enc", "gemm_dec", "wgrad_enc", "wgrad_dec", "attn_enc", "attn_dec",
              "layernorm", "pool", "optim", "shadows", "misc")          # include/masr.h MASR_PROF_*

_lib = None


def lib():
    """Load libmasr.so (raises if it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"libmasr.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                               "There is no CPU fallback for the product path.")
        l = C.CDLL(str(LIB_PATH))
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


class MasrError(RuntimeError):
    pass


def nbest_lists(tok, lens, scores, *more):
    """device results of masr_ctc_beam_search (tokens [B][N][Tp], lens [B][N], scores [B][N] torch tensors) -> per utterance
    [(token list, score), ...] without the slots beyond the live entries (lens -1); of masr_ctc_beam_search_lm, with `more` = its acoustic
    scores [B][N]: [(token list, fused score, acoustic score), ...]"""
    tok, lens, *vals = (t.cpu() for t in (tok, lens, scores, *more))
    return [[(tok[b, i, :int(lens[b, i])].tolist(), *[float(v[b, i]) for v in vals]) for i in range(lens.size(1)) if int(lens[b, i]) >= 0]
            for b in range(lens.size(0))]


def align_lists(frames, start, end, score, ys, olens):
    """device results of masr_ctc_align (frames [B][Tp], start / end [B][maxL], score [B] torch tensors) and the targets (per-utterance token
    lists, lengths) -> per utterance (score, [(token, start, end), ...], frames list without the -2 tail); an infeasible or refused utterance
    has no segments and no frames"""
    frames, start, end, score = (t.cpu().tolist() for t in (frames, start, end, score))
    out = []
    for b, L in enumerate(olens):
        segs = list(zip(map(int, ys[b][:int(L)]), start[b], end[b])) if math.isfinite(score[b]) else []
        out.append((score[b], segs, [f for f in frames[b] if f != -2]))
    return out


def align_outputs(B, Tp, maxL, device):
    """device outputs of masr_ctc_align -> ((frames int32 [B, Tp], start int32 [B, maxL], end int32 [B, maxL], score fp32 [B]), their four
    pointers for the call).  An empty tensor's data_ptr() is null, which the operator refuses, so start and end are views of backing tensors
    of at least one element and the pointers are the backings': with maxL = 0 the views are [B, 0] and the pointers still point somewhere."""
    import torch
    i32 = dict(dtype=torch.int32, device=device)
    backing = [torch.empty(max(B * maxL, 1), **i32) for _ in range(2)]
    frames, score = torch.empty(B, Tp, **i32), torch.empty(B, dtype=torch.float32, device=device)
    st, en = (t[:B * maxL].view(B, maxL) for t in backing)
    return (frames, st, en, score), [C.c_void_p(t.data_ptr()) for t in (frames, *backing, score)]


def check_target_lengths(ys, olens):
    """what both engines' ctc_align vet on the Python side: one transcript per length, none shorter than its length says"""
    if len(ys) != len(olens):
        raise ValueError(f"ctc_align needs one transcript per utterance, got {len(ys)} for {len(olens)} lengths")
    for b, (y, n) in enumerate(zip(ys, olens)):
        if int(n) > len(y):
            raise ValueError(f"olens[{b}] = {int(n)} but ys[{b}] holds {len(y)} tokens")


def align_targets(ys, olens, device):
    """the device arrays masr_ctc_align takes for per-utterance token lists, each cut to its olens[b] (ValueError where it is shorter than
    that): (targets int32 [sum], tgt_off int32 [B], tgt_len int32 [B], maxL)"""
    import torch
    ol = [int(n) for n in olens]
    check_target_lengths(ys, ol)
    flat = [int(t) for y, n in zip(ys, ol) for t in list(y)[:max(n, 0)]]
    off = [sum(max(n, 0) for n in ol[:b]) for b in range(len(ol))]
    i32 = dict(dtype=torch.int32, device=device)
    return torch.tensor(flat or [0], **i32), torch.tensor(off, **i32), torch.tensor(ol, **i32), max(ol + [0])


def nbest_lists_bias(tok, lens, scores, am, nbias):
    """device results of masr_ctc_beam_search_bias -> per utterance [(token list, final score, acoustic score, credited tokens), ...]"""
    return [[(t, s, a, int(n)) for t, s, a, n in u] for u in nbest_lists(tok, lens, scores, am, nbias)]


nbest_lists_lm = nbest_lists                                   # (the name the LM-fused searches' callers know)


def stable_prefix(nbest_lists):
    """the longest common prefix of the token lists of all live entries of one utterance's partial K-best (stream_beam_result with
    nbest = beam_size): [(token list, ...), ...] -> token list.  Every entry of a later beam extends an entry of this one, so the prefix
    only grows from feed to feed and is a prefix of the final best hypothesis: the text a streaming front end can commit.  No live entry:
    the empty list."""
    toks = [list(e[0]) for e in nbest_lists]
    if not toks:
        return []
    n = 0
    while n < min(map(len, toks)) and all(t[n] == toks[0][n] for t in toks):
        n += 1
    return toks[0][:n]


def check_beam_args(beam_size, nbest=1):
    """the beam size and list length every beam decoder vets on the Python side -> (K, N) as ints; nbest None = beam_size"""
    K = int(beam_size)
    N = K if nbest is None else int(nbest)
    if not 1 <= K <= 64:
        raise ValueError(f"beam_size must be in [1, 64], got {beam_size}")
    if not 1 <= N <= K:
        raise ValueError(f"nbest must be in [1, beam_size], got {nbest}")
    return K, N


def check_lm_args(lm, lm_w, len_bonus):
    """what the LM-fused CTC searches vet on the Python side -> (lm_w, len_bonus) as floats"""
    lm_w, len_bonus = float(lm_w), float(len_bonus)
    if not (math.isfinite(lm_w) and lm_w >= 0.0):
        raise ValueError(f"lm_w must be finite and >= 0, got {lm_w}")
    if not math.isfinite(len_bonus):
        raise ValueError(f"len_bonus must be finite, got {len_bonus}")
    if getattr(lm, "h", None) is None:
        raise ValueError("lm must be a live NGramLM")
    return lm_w, len_bonus


def check_nlm_args(nlm, lm_w, len_bonus=None):
    """what the LSTM-LM-fused beams vet on the Python side -> lm_w as a float; with a len_bonus (the joint beam) -> (lm_w, len_bonus)"""
    lm_w = float(lm_w)
    if not (math.isfinite(lm_w) and lm_w >= 0.0):
        raise ValueError(f"lm_w must be finite and >= 0, got {lm_w}")
    if len_bonus is not None and not math.isfinite(float(len_bonus)):
        raise ValueError(f"len_bonus must be finite, got {float(len_bonus)}")
    if getattr(nlm, "h", None) is None or not hasattr(nlm, "score"):
        raise ValueError("lm must be a live LstmLM")
    return lm_w if len_bonus is None else (lm_w, float(len_bonus))


def check(rc, what=""):
    if rc != 0:
        raise MasrError(f"{what} failed ({rc}): {lib().masr_last_error().decode()}")
