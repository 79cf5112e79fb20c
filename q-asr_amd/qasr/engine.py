"""ctypes binding of libqasr_hip.so (include/qasr.h).  PyTorch is used only to own device
memory and streams.  There is no CPU fallback: a missing library or a failing call raises."""
import ctypes as C
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('QASR_LIB', os.path.join(HERE, 'libqasr_hip.so'))   # QASR_LIB: A/B builds in one run

SYMBOLS = ['qasr_blob_check', 'qasr_engine_create', 'qasr_engine_create_ex', 'qasr_engine_default_opts', 'qasr_engine_destroy', 'qasr_engine_forward', 'qasr_engine_forward_audio', 'qasr_engine_out_frames',
           'qasr_engine_num_ops', 'qasr_engine_num_launches', 'qasr_engine_read_acc', 'qasr_engine_read_tensor', 'qasr_engine_last_op_ms',
           'qasr_engine_time_ops', 'qasr_engine_run_op', 'qasr_engine_op_label', 'qasr_engine_op_paired', 'qasr_engine_op_halved', 'qasr_engine_pair_timeouts', 'qasr_engine_pair_flag_words',
           'qasr_sep_pair_workspace_bytes', 'qasr_sep_pair_timeout_offset',
           'qasr_frontend_mel', 'qasr_frontend_plan', 'qasr_frontend_mel_planned', 'qasr_frontend_frames',
           'qasr_frontend_workspace_bytes', 'qasr_pw_conv_acc',
           'qasr_dw_conv_acc', 'qasr_dense_conv_acc', 'qasr_requant', 'qasr_dyn_range', 'qasr_dyn_range_percentile', 'qasr_dyn_residue_codes', 'qasr_dyn_act_params', 'qasr_dyn_requant',
           'qasr_dyn_quant_in', 'qasr_dyn_conv_params', 'qasr_sep_layer', 'qasr_quantile2', 'qasr_quantile_workspace_bytes', 'qasr_debug_prof',
           'qasr_debug_timeline', 'qasr_ctc_collapse', 'qasr_engine_attach_ctc', 'qasr_ctc_topn', 'qasr_ctc_beam_workspace_bytes', 'qasr_ctc_beam',
           'qasr_lm_check', 'qasr_ctc_beam_lm', 'qasr_boost_check', 'qasr_ctc_beam_boost', 'qasr_ctc_align_workspace_bytes', 'qasr_ctc_align',
           'qasr_ctc_align_band_workspace_bytes', 'qasr_ctc_align_band', 'qasr_ctc_star', 'qasr_ctc_spot', 'qasr_ctc_post_workspace_bytes', 'qasr_ctc_post',
           'qasr_ctc_post_band_workspace_bytes', 'qasr_ctc_post_band',
           'qasr_engine_reserve', 'qasr_engine_forward_ragged', 'qasr_engine_forward_ragged_audio', 'qasr_engine_ragged_stats',
           'qasr_ragged_bucket_frames', 'qasr_ragged_envelope_frames',
           'qasr_resample_check', 'qasr_resample', 'qasr_resample_out_samples', 'qasr_longform_cut', 'qasr_longform_stitch',
           'qasr_stream_state_bytes', 'qasr_stream_push', 'qasr_stream_window', 'qasr_stream_emit',
           'qasr_stream_rs_state_bytes', 'qasr_stream_rs_work_bytes', 'qasr_stream_rs_push',
           'qasr_stream_beam_state_bytes', 'qasr_stream_beam', 'qasr_stream_ep_state_bytes', 'qasr_stream_endpoint',
           'qasr_stream_beam_boost_state_bytes', 'qasr_stream_beam_boost', 'qasr_stream_beam_ep',
           'qasr_stream_spot_state_bytes', 'qasr_stream_spot', 'qasr_edit_workspace_bytes', 'qasr_edit_distance',
           'qasr_edit_trace_workspace_bytes', 'qasr_edit_trace', 'qasr_mbr_workspace_bytes', 'qasr_ctc_mbr',
           'qasr_last_error', 'qasr_version']

_lib = None


class _SepOut(C.Structure):
    _fields_ = [('ptr', C.c_void_p), ('mtab', C.c_void_p), ('m', C.c_double), ('lo', C.c_int32), ('hi', C.c_int32),
                ('mode', C.c_int32), ('pad_', C.c_int32)]


class SepLayerArgs(C.Structure):
    """qasr_sep_layer_args (include/qasr.h)."""
    _fields_ = ([(n, C.c_int32) for n in ('B', 'T', 'Tp', 'cin', 'cout', 'K', 'dilation', 'tile', 'gen')] +
                [('flags', C.c_uint32), ('x', C.c_void_p)] +
                [(n, C.c_int32) for n in ('x_unsigned', 'dw_lo', 'dw_hi', 'n_outs')] +
                [(n, C.c_void_p) for n in ('wdw', 'wdw2', 'bias_dw', 'm_dw', 'w', 'bias', 'sb', 'm_main', 'lens', 'rx', 'rw',
                                           'rbias', 'rm', 'rsb')] +
                [(n, C.c_int32) for n in ('rcin', 'r_unsigned', 'qlo', 'qhi')] +
                [('outs', _SepOut * 3), ('dw_acc', C.c_void_p), ('acc', C.c_void_p), ('racc', C.c_void_p)] +
                [('pair', C.c_int32), ('pad_', C.c_int32), ('pair_ws', C.c_void_p), ('pair_ws_bytes', C.c_size_t)])


class EngineOpts(C.Structure):
    """qasr_engine_opts (include/qasr.h): the launch-plan choices of one engine."""
    _fields_ = ([('struct_size', C.c_uint32), ('debug', C.c_uint32)] +
                [(n, C.c_int32) for n in ('tile_frames', 'sep_gen', 'fuse_dw', 'fuse_stem', 'fuse_decoder', 'graph',
                                          'retired_whole_utterance', 'res_tile128', 'dense_tile128', 'retired_legacy_pw', 'retired_persistent', 'fuse_norm',
                                          'mask_skip', 'pair_split')])


class CtcOut(C.Structure):
    """qasr_ctc_out (include/qasr.h): caller-owned device buffers of k_ctc, row pitch T."""
    _fields_ = [('struct_size', C.c_uint32)] + [(n, C.c_void_p) for n in ('labels', 'n_labels', 'start', 'nframes', 'score',
                                                                         'utt_score')]


class ReserveOpts(C.Structure):
    """qasr_reserve_opts (include/qasr.h): the envelope of a reserved engine."""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('max_batch', 'max_samples', 'max_frames', 'n_mels', 'pad_to', 'want_logp', 'decode',
                                          'max_graphs')] + [('reserved', C.c_int32 * 3)])


class RaggedOut(C.Structure):
    """qasr_ragged_out (include/qasr.h): engine-owned buffers of the last ragged forward."""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('out_frames', 'bucket_frames', 'row_pitch', 'n_classes')] +
                [(n, C.c_void_p) for n in ('tokens', 'lens_out', 'logp', 'frame_score')] + [('ctc', CtcOut)] +
                [(n, C.c_void_p) for n in ('feats', 'feat_lens')])


class RaggedStats(C.Structure):
    """qasr_ragged_stats (include/qasr.h)"""
    _fields_ = [('struct_size', C.c_uint32), ('n_buckets', C.c_int32), ('device_allocs', C.c_uint64),
                ('device_frees', C.c_uint64), ('graphs_captured', C.c_uint64), ('graph_replays', C.c_uint64),
                ('eager_runs', C.c_uint64), ('bucket_frames', C.c_int32 * 64), ('bucket_calls', C.c_uint64 * 64)]


class QasrError(RuntimeError):
    pass


class _DeviceView:
    """Engine-owned device memory as a torch tensor without a copy (torch.as_tensor reads __cuda_array_interface__)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {'shape': tuple(int(x) for x in shape), 'typestr': typestr, 'data': (int(ptr), False),
                                         'version': 2, 'strides': None}


def _view(ptr, shape, dtype, device):
    if not ptr:
        return None
    return torch.as_tensor(_DeviceView(ptr, shape, '<f4' if dtype == torch.float32 else '<i4'), device=device)


def load_library():
    """Loads the HIP extension; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QasrError(f'{LIB_PATH} is missing: run `python __graft_entry__.py` (build()) first; '
                        'the quantised inference path has no CPU fallback')
    lib = C.CDLL(LIB_PATH)
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.qasr_blob_check.argtypes = [C.c_char_p, sz, C.c_char_p, sz]
    lib.qasr_engine_create.argtypes = [vp, sz, i32, i32, C.POINTER(vp)]
    lib.qasr_engine_create_ex.argtypes = [vp, sz, i32, C.POINTER(EngineOpts), C.POINTER(vp)]
    lib.qasr_engine_default_opts.argtypes = [C.POINTER(EngineOpts)]
    lib.qasr_engine_default_opts.restype = None
    lib.qasr_engine_destroy.argtypes = [vp]
    lib.qasr_engine_destroy.restype = None
    lib.qasr_engine_forward.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.qasr_engine_out_frames.argtypes = [vp, i32]
    lib.qasr_engine_num_ops.argtypes = [vp]
    lib.qasr_engine_num_launches.argtypes = [vp]
    lib.qasr_engine_read_acc.argtypes = [vp, i32, i32, vp, sz]
    lib.qasr_engine_read_tensor.argtypes = [vp, i32, vp, sz, C.POINTER(i32), C.POINTER(i32)]
    lib.qasr_engine_last_op_ms.argtypes = [vp, vp, i32]
    lib.qasr_engine_time_ops.argtypes = [vp, vp, i32, vp, i32]
    lib.qasr_engine_run_op.argtypes = [vp, vp, i32]
    lib.qasr_engine_op_label.argtypes = [vp, i32, C.c_char_p, sz]
    lib.qasr_engine_op_paired.argtypes = [vp, i32]
    if hasattr(lib, 'qasr_engine_op_halved'):   # (a QASR_LIB A/B build of an older tree lacks it)
        lib.qasr_engine_op_halved.argtypes = [vp, i32]
    lib.qasr_engine_pair_timeouts.argtypes = [vp]
    if hasattr(lib, 'qasr_engine_pair_flag_words'):   # (a QASR_LIB A/B build of an older tree lacks it)
        lib.qasr_engine_pair_flag_words.argtypes = [vp, vp, sz]
    lib.qasr_sep_pair_workspace_bytes.argtypes = [i32, i32]
    lib.qasr_sep_pair_workspace_bytes.restype = sz
    lib.qasr_sep_pair_timeout_offset.argtypes = [i32, i32]
    lib.qasr_sep_pair_timeout_offset.restype = sz
    lib.qasr_engine_forward_audio.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, i32, C.c_float, i32, vp, sz, vp, vp, vp, vp, vp]
    lib.qasr_frontend_mel.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, C.c_float, i32, vp, vp, vp, sz]
    lib.qasr_frontend_mel_planned.argtypes = lib.qasr_frontend_mel.argtypes
    lib.qasr_frontend_plan.argtypes = [vp, vp, i32, vp, sz]
    lib.qasr_frontend_frames.argtypes = [i32, i32]
    lib.qasr_frontend_workspace_bytes.argtypes = [i32, i32, i32]
    lib.qasr_frontend_workspace_bytes.restype = sz
    lib.qasr_pw_conv_acc.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.qasr_dw_conv_acc.argtypes = [vp, vp, i32, vp, vp] + [i32] * 11 + [vp]
    lib.qasr_dense_conv_acc.argtypes = [vp, vp, i32, vp, vp] + [i32] * 12 + [vp]
    lib.qasr_requant.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.qasr_dyn_range.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]
    lib.qasr_dyn_residue_codes.argtypes = [vp, vp, i32, vp, sz, vp, vp]
    lib.qasr_dyn_range_percentile.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, C.c_float, C.c_float, vp, vp, sz, vp]
    lib.qasr_dyn_act_params.argtypes = [vp, vp, i32, i32, vp, i32, vp, i32, vp, vp, vp]
    lib.qasr_dyn_requant.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.qasr_dyn_quant_in.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.qasr_dyn_conv_params.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp]
    if hasattr(lib, 'qasr_ctc_collapse'):       # (a QASR_LIB A/B build of an older tree lacks them: calling them raises there)
        lib.qasr_ctc_collapse.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.POINTER(CtcOut)]
        lib.qasr_engine_attach_ctc.argtypes = [vp, vp, C.POINTER(CtcOut), i32]
    if hasattr(lib, 'qasr_ctc_beam'):           # (likewise)
        lib.qasr_ctc_topn.argtypes = [vp, C.POINTER(TopnArgs)]
        lib.qasr_ctc_beam.argtypes = [vp, C.POINTER(BeamArgs)]
        lib.qasr_ctc_beam_workspace_bytes.argtypes = [i32, i32, i32]
        lib.qasr_ctc_beam_workspace_bytes.restype = sz
    if hasattr(lib, 'qasr_ctc_beam_lm'):        # (likewise)
        lib.qasr_lm_check.argtypes = [C.c_char_p, sz, i32]
        lib.qasr_ctc_beam_lm.argtypes = [vp, C.POINTER(BeamLmArgs)]
    if hasattr(lib, 'qasr_ctc_beam_boost'):     # (likewise)
        lib.qasr_boost_check.argtypes = [C.c_char_p, sz, i32]
        lib.qasr_ctc_beam_boost.argtypes = [vp, C.POINTER(BeamBoostArgs)]
    if hasattr(lib, 'qasr_ctc_align'):          # (likewise)
        lib.qasr_ctc_align.argtypes = [vp, C.POINTER(AlignArgs)]
        lib.qasr_ctc_align_workspace_bytes.argtypes = [i32, i32, i32]
        lib.qasr_ctc_align_workspace_bytes.restype = sz
    if hasattr(lib, 'qasr_ctc_align_band'):     # (likewise)
        lib.qasr_ctc_align_band.argtypes = [vp, C.POINTER(AlignBandArgs)]
        lib.qasr_ctc_align_band_workspace_bytes.argtypes = [i32, i32, i32]
        lib.qasr_ctc_align_band_workspace_bytes.restype = sz
    if hasattr(lib, 'qasr_ctc_star'):           # (likewise)
        lib.qasr_ctc_star.argtypes = [vp, C.POINTER(StarArgs)]
    if hasattr(lib, 'qasr_ctc_spot'):           # (likewise)
        lib.qasr_ctc_spot.argtypes = [vp, C.POINTER(SpotArgs)]
    if hasattr(lib, 'qasr_ctc_post'):           # (likewise)
        lib.qasr_ctc_post.argtypes = [vp, C.POINTER(PostArgs)]
        lib.qasr_ctc_post_workspace_bytes.argtypes = [i32, i32]
        lib.qasr_ctc_post_workspace_bytes.restype = sz
    if hasattr(lib, 'qasr_ctc_post_band'):      # (likewise)
        lib.qasr_ctc_post_band.argtypes = [vp, C.POINTER(PostBandArgs)]
        lib.qasr_ctc_post_band_workspace_bytes.argtypes = [i32, i32]
        lib.qasr_ctc_post_band_workspace_bytes.restype = sz
    if hasattr(lib, 'qasr_engine_reserve'):     # (likewise)
        lib.qasr_engine_reserve.argtypes = [vp, C.POINTER(ReserveOpts)]
        lib.qasr_engine_forward_ragged.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(RaggedOut)]
        lib.qasr_engine_forward_ragged_audio.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, i32, C.c_float, i32, vp, sz,
                                                         C.POINTER(RaggedOut)]
        lib.qasr_engine_ragged_stats.argtypes = [vp, C.POINTER(RaggedStats)]
        lib.qasr_ragged_bucket_frames.argtypes = [i32, i32, i32]
        lib.qasr_ragged_envelope_frames.argtypes = [i32, i32, i32]
    if hasattr(lib, 'qasr_resample'):           # (likewise)
        lib.qasr_resample_check.argtypes = [C.c_char_p, sz]
        lib.qasr_resample.argtypes = [vp, C.POINTER(ResampleArgs)]
        lib.qasr_resample_out_samples.argtypes = [i32, i32, i32]
    if hasattr(lib, 'qasr_longform_cut'):       # (likewise)
        lib.qasr_longform_cut.argtypes = [vp, C.POINTER(LongformCutArgs)]
        lib.qasr_longform_stitch.argtypes = [vp, C.POINTER(LongformStitchArgs)]
    if hasattr(lib, 'qasr_stream_push'):        # (likewise)
        lib.qasr_stream_state_bytes.argtypes = [i32, i32, i32]
        lib.qasr_stream_state_bytes.restype = sz
        lib.qasr_stream_push.argtypes = [vp, C.POINTER(StreamPushArgs)]
        lib.qasr_stream_window.argtypes = [vp, C.POINTER(StreamWindowArgs)]
        lib.qasr_stream_emit.argtypes = [vp, C.POINTER(StreamEmitArgs)]
    if hasattr(lib, 'qasr_stream_rs_push'):     # (likewise)
        lib.qasr_stream_rs_state_bytes.argtypes = [i32, i32]
        lib.qasr_stream_rs_state_bytes.restype = sz
        lib.qasr_stream_rs_work_bytes.argtypes = [i32]
        lib.qasr_stream_rs_work_bytes.restype = sz
        lib.qasr_stream_rs_push.argtypes = [vp, C.POINTER(StreamRsPushArgs)]
    if hasattr(lib, 'qasr_stream_beam'):        # (likewise)
        lib.qasr_stream_beam_state_bytes.argtypes = [i32, i32, i32]
        lib.qasr_stream_beam_state_bytes.restype = sz
        lib.qasr_stream_beam.argtypes = [vp, C.POINTER(StreamBeamArgs)]
    if hasattr(lib, 'qasr_stream_beam_boost'):  # (likewise)
        lib.qasr_stream_beam_boost_state_bytes.argtypes = [i32, i32, i32]
        lib.qasr_stream_beam_boost_state_bytes.restype = sz
        lib.qasr_stream_beam_boost.argtypes = [vp, C.POINTER(StreamBeamBoostArgs)]
    if hasattr(lib, 'qasr_stream_endpoint'):    # (likewise)
        lib.qasr_stream_ep_state_bytes.argtypes = [i32]
        lib.qasr_stream_ep_state_bytes.restype = sz
        lib.qasr_stream_endpoint.argtypes = [vp, C.POINTER(StreamEndpointArgs)]
    if hasattr(lib, 'qasr_stream_beam_ep'):     # (likewise)
        lib.qasr_stream_beam_ep.argtypes = [vp, C.POINTER(StreamBeamEpArgs)]
    if hasattr(lib, 'qasr_stream_spot'):        # (likewise)
        lib.qasr_stream_spot_state_bytes.argtypes = [i32, i32, i32]
        lib.qasr_stream_spot_state_bytes.restype = sz
        lib.qasr_stream_spot.argtypes = [vp, C.POINTER(StreamSpotArgs)]
    if hasattr(lib, 'qasr_edit_distance'):      # (likewise)
        lib.qasr_edit_workspace_bytes.argtypes = [i32, i32, i32, i32]
        lib.qasr_edit_workspace_bytes.restype = sz
        lib.qasr_edit_distance.argtypes = [vp, C.POINTER(EditArgs)]
    if hasattr(lib, 'qasr_edit_trace'):         # (likewise)
        lib.qasr_edit_trace_workspace_bytes.argtypes = [i32, i32, i32, i32]
        lib.qasr_edit_trace_workspace_bytes.restype = sz
        lib.qasr_edit_trace.argtypes = [vp, C.POINTER(EditTraceArgs)]
    if hasattr(lib, 'qasr_ctc_mbr'):            # (likewise)
        lib.qasr_mbr_workspace_bytes.argtypes = [i32, i32, i32, i32]
        lib.qasr_mbr_workspace_bytes.restype = sz
        lib.qasr_ctc_mbr.argtypes = [vp, C.POINTER(MbrArgs)]
    lib.qasr_debug_prof.argtypes = [vp]
    lib.qasr_debug_timeline.argtypes = [vp, sz]
    lib.qasr_sep_layer.argtypes = [vp, C.POINTER(SepLayerArgs), C.c_char_p, sz]
    lib.qasr_quantile2.argtypes = [vp, vp, sz, C.c_float, C.c_float, vp, vp, sz]
    lib.qasr_quantile_workspace_bytes.argtypes = []
    lib.qasr_quantile_workspace_bytes.restype = sz
    lib.qasr_last_error.restype = C.c_char_p
    lib.qasr_version.restype = C.c_char_p
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise QasrError(f'{what} failed ({rc}): {load_library().qasr_last_error().decode()}')


def blob_check(blob: bytes):
    """qasr_blob_check: raises QasrError naming the first malformed field of a packed model (host-only, no GPU needed)."""
    lib = load_library()
    why = C.create_string_buffer(256)
    if lib.qasr_blob_check(bytes(blob), len(blob), why, len(why)) != 0:
        raise QasrError('malformed blob: ' + why.value.decode())


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _ctc_out_struct(res):
    o = CtcOut()
    o.struct_size = C.sizeof(CtcOut)
    for n in ('labels', 'n_labels', 'start', 'nframes', 'score', 'utt_score'):
        t = getattr(res, n)
        if t is not None:
            assert t.is_cuda and t.is_contiguous() and t.dtype == (torch.float32 if 'score' in n else torch.int32), n
            setattr(o, n, t.data_ptr())
    return o


def ctc_buffers(B, T, device, scores=True, blank=-1):
    """Device buffers of one k_ctc call as a qasr.ctc.CtcResult of torch tensors (score / utt_score / frame_score only with
    `scores`)."""
    from .ctc import CtcResult
    i32 = dict(device=device, dtype=torch.int32)
    f32 = dict(device=device, dtype=torch.float32)
    return CtcResult(labels=torch.empty(B, T, **i32), n_labels=torch.empty(B, **i32), start=torch.empty(B, T, **i32),
                     nframes=torch.empty(B, T, **i32), score=torch.empty(B, T, **f32) if scores else None,
                     utt_score=torch.empty(B, **f32) if scores else None, blank=blank,
                     frame_score=torch.empty(B, T, **f32) if scores else None)


def ctc_collapse(tokens, frame_score=None, lens=None, blank=None, out=None, stream=None):
    """qasr_ctc_collapse: greedy CTC collapse of a cuda int32 token matrix [B, T] on the device (k_ctc, one launch on the
    current stream).  frame_score f32 [B, T] / lens int32 [B] optional (lens None: the padded row).  Returns a
    qasr.ctc.CtcResult of cuda tensors (`out`: caller-owned, any of its optional arrays may be None)."""
    lib = load_library()
    if blank is None:
        raise ValueError('ctc_collapse: blank is required (the decoder\'s last class)')
    assert tokens.is_cuda and tokens.dim() == 2, 'ctc_collapse: tokens must be a cuda tensor [B, T]'
    dev = tokens.device
    tok = tokens.to(torch.int32).contiguous()
    fs = None if frame_score is None else frame_score.to(device=dev, dtype=torch.float32).contiguous()
    ln = None if lens is None else lens.to(device=dev, dtype=torch.int32).contiguous()
    B, T = tok.shape
    if out is None:
        out = ctc_buffers(B, T, dev, scores=fs is not None, blank=int(blank))
        out.frame_score = fs
    o = _ctc_out_struct(out)
    with torch.cuda.device(dev):
        _check(lib.qasr_ctc_collapse(_stream_ptr(stream), _ptr(tok), _ptr(fs), _ptr(ln), B, T, int(blank), C.byref(o)),
               'qasr_ctc_collapse')
    out._keep = (tok, fs, ln)               # inputs stay alive until the stream has consumed them
    return out


class TopnArgs(C.Structure):
    """qasr_ctc_topn_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'T', 'C', 'N')] +
                [('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64)] +
                [(n, C.c_void_p) for n in ('log_probs', 'lens', 'cand_id', 'cand_q')])


class BeamArgs(C.Structure):
    """qasr_ctc_beam_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'T', 'N', 'beam_width', 'n_best', 'blank')] +
                [('lae_entries', C.c_uint32)] + [(n, C.c_void_p) for n in ('cand_id', 'cand_q', 'lens', 'lae_table', 'workspace')] +
                [('workspace_bytes', C.c_size_t)] + [(n, C.c_void_p) for n in ('labels', 'n_labels', 'score', 'n_hyps')])


class BeamLmArgs(C.Structure):
    """qasr_ctc_beam_lm_args (include/qasr.h): the fields of BeamArgs, then the model"""
    _fields_ = (BeamArgs._fields_ + [('lm', C.c_void_p), ('lm_bytes', C.c_size_t)] +
                [(n, C.c_int32) for n in ('alpha_q', 'beta_q', 'space', 'reserved')] + [('lm_score', C.c_void_p)])


class BeamBoostArgs(C.Structure):
    """qasr_ctc_beam_boost_args (include/qasr.h): the fields of BeamLmArgs with `reserved` become whole_words, then the set"""
    _fields_ = (BeamArgs._fields_ + [('lm', C.c_void_p), ('lm_bytes', C.c_size_t)] +
                [(n, C.c_int32) for n in ('alpha_q', 'beta_q', 'space', 'whole_words')] + [('lm_score', C.c_void_p)] +
                [('boost', C.c_void_p), ('boost_bytes', C.c_size_t), ('boost_score', C.c_void_p)])


_lae_tables = {}
_boost_blobs = {}                       # (id of the PhraseSet, device) -> (the set, its packed form on the device)
_lm_blobs = {}                          # (id of the NgramLM, device) -> (the model, its packed form on the device)


def lm_check(blob: bytes, n_labels: int):
    """qasr_lm_check: raises QasrError naming the first malformed field of a packed n-gram model (host-only, no GPU)"""
    lib = load_library()
    if lib.qasr_lm_check(bytes(blob), len(blob), int(n_labels)) != 0:
        raise QasrError('malformed language model: ' + lib.qasr_last_error().decode())


def lm_device(lm, device):
    """The packed form of a qasr.ngram.NgramLM on `device` as a uint8 tensor: packed, validated (qasr_lm_check) and uploaded
    once per (model, device) and kept, like the log-add-exp table.  The upload is a host-to-device copy: the first ctc_beam
    with a model must run outside a stream capture (or call this first); later calls only launch."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    key = (id(lm), dev)
    hit = _lm_blobs.get(key)
    if hit is None or hit[0] is not lm:
        blob = lm.pack()
        lm_check(blob, lm.n_labels)
        hit = _lm_blobs[key] = (lm, torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev))
    return hit[1]


def boost_check(blob: bytes, n_labels: int):
    """qasr_boost_check: raises QasrError naming the first malformed field of a packed phrase set (host-only, no GPU)"""
    lib = load_library()
    if lib.qasr_boost_check(bytes(blob), len(blob), int(n_labels)) != 0:
        raise QasrError('malformed phrase set: ' + lib.qasr_last_error().decode())


def boost_device(boost, device):
    """The packed form of a qasr.boost.PhraseSet on `device` as a uint8 tensor: packed, validated (qasr_boost_check) and
    uploaded once per (set, device) and kept, like lm_device.  A sweep of weights builds a new PhraseSet per weight, which
    packs and uploads again: nothing stale is reused.  The upload is a host-to-device copy: the first ctc_beam with a set
    must run outside a stream capture (or call this first); later calls only launch."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    key = (id(boost), dev)
    hit = _boost_blobs.get(key)
    if hit is None or hit[0] is not boost:
        blob = boost.pack()
        boost_check(blob, boost.n_labels)
        if len(_boost_blobs) >= 8:                          # per-request sets come and go: keep the cache small
            _boost_blobs.clear()
        hit = _boost_blobs[key] = (boost, torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev))
    return hit[1]


def lae_table_device(device):
    """qasr.beam.lae_table() on `device` (its 16384 u16 entries as an int16 tensor), uploaded once per device ('cuda' and
    'cuda:N' of the current device share one copy).  The upload is a host-to-device copy on the current stream: the first
    ctc_beam of a device must therefore run outside a stream capture (or call this first); later calls only launch."""
    from . import beam
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    t = _lae_tables.get(dev)
    if t is None:
        t = _lae_tables[dev] = torch.from_numpy(beam.lae_table().view(np.int16).copy()).to(dev)
    return t


def ctc_topn(log_probs, lens=None, n=40, out=None, stream=None):
    """qasr_ctc_topn: each frame's min(n, C) best classes of a cuda float32 tensor [B, T, C] (any utterance / frame pitch,
    classes contiguous) as (cand_id, cand_q), int32 [B, T, n], best first: k_topn, one launch on the current stream; equal
    to qasr.beam.topn_host byte for byte.  lens int32 [B] optional; `out`: a caller-owned (cand_id, cand_q) pair."""
    lib = load_library()
    assert log_probs.is_cuda and log_probs.dim() == 3 and log_probs.dtype == torch.float32, \
        'ctc_topn: log_probs must be a cuda float32 tensor [B, T, C]'
    dev = log_probs.device
    lp = log_probs if log_probs.stride(2) == 1 or log_probs.shape[2] == 1 else log_probs.contiguous()
    ln = None if lens is None else lens.to(device=dev, dtype=torch.int32).contiguous()
    B, T, Cn = lp.shape
    if out is None:
        out = (torch.empty(B, T, int(n), device=dev, dtype=torch.int32), torch.empty(B, T, int(n), device=dev, dtype=torch.int32))
    cid, cq = out
    for t in out:
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and tuple(t.shape) == (B, T, int(n)), 'ctc_topn: out'
    a = TopnArgs()
    a.struct_size = C.sizeof(TopnArgs)
    a.B, a.T, a.C, a.N = B, T, Cn, int(n)
    a.pitch_utt, a.pitch_frame = (lp.stride(0) if B > 1 else max(lp.stride(0), T * lp.stride(1))), lp.stride(1)
    a.log_probs, a.lens, a.cand_id, a.cand_q = lp.data_ptr(), 0 if ln is None else ln.data_ptr(), cid.data_ptr(), cq.data_ptr()
    with torch.cuda.device(dev):
        _check(lib.qasr_ctc_topn(_stream_ptr(stream), C.byref(a)), 'qasr_ctc_topn')
    cid._keep = (lp, ln)
    return cid, cq


def ctc_beam_workspace_bytes(B, T, beam_width):
    return int(load_library().qasr_ctc_beam_workspace_bytes(int(B), int(T), int(beam_width)))


def _lm_weights(who, lm, alpha, beta, blank):
    """The weights of a model in fixed point ((0, 0) without one); they and the model's vocabulary are checked here, under the
    call's name, before any launch."""
    if lm is None:
        return 0, 0
    from .ngram import fixed_weights
    alpha_q, beta_q = fixed_weights(alpha, beta)
    if lm.n_labels != int(blank):
        raise ValueError(f'{who}: the model was loaded for {lm.n_labels} labels, blank is {blank}')
    return alpha_q, beta_q


def _beam_args(cls, cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out, lm_score=False, boost_score=False):
    """What qasr_ctc_beam, _lm and _boost share: the candidates coerced, the BeamResult (with lm_score / boost_score where the
    call writes them) and the workspace unless the caller owns them, the table, and the fields every one of the three structs
    opens with.  Returns (the struct of type cls, out, what must stay alive)."""
    from .beam import BeamResult, TAB_ENTRIES
    assert cand_id.is_cuda and cand_id.dim() == 3 and cand_id.shape == cand_q.shape, 'ctc_beam: candidates must be cuda [B, T, N]'
    dev = cand_id.device
    cid, cq = cand_id.to(torch.int32).contiguous(), cand_q.to(device=dev, dtype=torch.int32).contiguous()
    ln = None if lens is None else lens.to(device=dev, dtype=torch.int32).contiguous()
    B, T, N = cid.shape
    W = int(beam_width)
    nb = W if n_best is None else int(n_best)
    if out is None:
        shape = (B, max(nb, 0))
        i64 = lambda on: torch.empty(*shape, device=dev, dtype=torch.int64) if on else None
        out = BeamResult(labels=torch.empty(*shape, T, device=dev, dtype=torch.int32),
                         n_labels=torch.empty(*shape, device=dev, dtype=torch.int32), score=i64(True),
                         n_hyps=torch.empty(B, device=dev, dtype=torch.int32), blank=int(blank), lm_score=i64(lm_score),
                         boost_score=i64(boost_score))
    if workspace is None:
        workspace = torch.empty(max(ctc_beam_workspace_bytes(B, T, W), 8), device=dev, dtype=torch.uint8)
    tab = lae_table_device(dev)
    a = cls()
    a.struct_size = C.sizeof(cls)
    a.B, a.T, a.N, a.beam_width, a.n_best, a.blank = B, T, N, W, nb, int(blank)
    a.lae_entries = TAB_ENTRIES
    a.cand_id, a.cand_q, a.lens, a.lae_table = cid.data_ptr(), cq.data_ptr(), 0 if ln is None else ln.data_ptr(), tab.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a.labels, a.n_labels, a.score, a.n_hyps = (out.labels.data_ptr(), out.n_labels.data_ptr(), out.score.data_ptr(),
                                               out.n_hyps.data_ptr())
    return a, out, (cid, cq, ln, workspace, tab)


def _beam_launch(symbol, a, out, keep, stream):
    with torch.cuda.device(keep[0].device):
        _check(getattr(load_library(), symbol)(_stream_ptr(stream), C.byref(a)), symbol)
    out._keep = keep
    return out


def ctc_beam(cand_id, cand_q, lens=None, blank=None, beam_width=16, n_best=None, workspace=None, out=None, stream=None,
             lm=None, alpha=0.0, beta=0.0, boost=None):
    """qasr_ctc_beam: CTC prefix beam search over the candidates of ctc_topn (cuda int32 [B, T, N]) on the device (k_beam,
    one launch on the current stream, no host synchronisation); equal to qasr.beam.beam_search_host byte for byte.  Returns
    a qasr.beam.BeamResult of cuda tensors.  workspace: a caller-owned uint8 tensor of ctc_beam_workspace_bytes(B, T, W)
    bytes (None: allocated by torch here); `out`: a caller-owned BeamResult.  lm: a qasr.ngram.NgramLM with its weights
    alpha (0 .. 16) and beta (|beta| <= 16): qasr_ctc_beam_lm (k_beam_lm) instead, and the result carries lm_score.
    boost: a qasr.boost.PhraseSet, with or without lm: qasr_ctc_beam_boost (k_beam_boost) instead, and the result carries
    boost_score; without one the calls above run exactly as they did."""
    if boost is not None:
        return _ctc_beam_boost(cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out, stream, lm, alpha, beta, boost)
    if lm is not None:
        return _ctc_beam_lm(cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out, stream, lm, alpha, beta)
    if blank is None:
        raise ValueError('ctc_beam: blank is required (the decoder\'s last class)')
    a, out, keep = _beam_args(BeamArgs, cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out)
    return _beam_launch('qasr_ctc_beam', a, out, keep, stream)


def _ctc_beam_lm(cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out, stream, lm, alpha, beta):
    """ctc_beam with a model: qasr_ctc_beam_lm.  The weights and the vocabulary are checked here, before any launch."""
    if blank is None:
        raise ValueError('ctc_beam: blank is required (the decoder\'s last class)')
    alpha_q, beta_q = _lm_weights('ctc_beam', lm, alpha, beta, blank)
    a, out, keep = _beam_args(BeamLmArgs, cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out, lm_score=True)
    blob = lm_device(lm, keep[0].device)
    a.lm, a.lm_bytes, a.alpha_q, a.beta_q, a.space = blob.data_ptr(), blob.numel(), alpha_q, beta_q, int(lm.space)
    a.lm_score = 0 if out.lm_score is None else out.lm_score.data_ptr()
    return _beam_launch('qasr_ctc_beam_lm', a, out, keep + (blob,), stream)


def _ctc_beam_boost(cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out, stream, lm, alpha, beta, boost):
    """ctc_beam with a phrase set: qasr_ctc_beam_boost.  Weights, vocabulary sizes and the set are checked here, before any
    launch."""
    if blank is None:
        raise ValueError('ctc_beam: blank is required (the decoder\'s last class)')
    alpha_q, beta_q = _lm_weights('ctc_beam', lm, alpha, beta, blank)
    if boost.n_labels != int(blank):
        raise ValueError(f'ctc_beam: the phrase set was compiled for {boost.n_labels} labels, blank is {blank}')
    a, out, keep = _beam_args(BeamBoostArgs, cand_id, cand_q, lens, blank, beam_width, n_best, workspace, out, lm_score=lm is not None,
                              boost_score=True)
    lm_blob = None if lm is None else lm_device(lm, keep[0].device)
    blob = boost_device(boost, keep[0].device)
    if lm is not None:
        a.lm, a.lm_bytes, a.alpha_q, a.beta_q = lm_blob.data_ptr(), lm_blob.numel(), alpha_q, beta_q
        a.lm_score = 0 if out.lm_score is None else out.lm_score.data_ptr()
    a.space = int(lm.space) if lm is not None else int(boost.space)
    a.whole_words = int(boost.whole_words)
    a.boost, a.boost_bytes = blob.data_ptr(), blob.numel()
    a.boost_score = 0 if out.boost_score is None else out.boost_score.data_ptr()
    return _beam_launch('qasr_ctc_beam_boost', a, out, keep + (lm_blob, blob), stream)


def ctc_beam_search(log_probs, lens=None, blank=None, beam_width=16, n_best=None, cutoff_top_n=40, stream=None, lm=None,
                    alpha=0.0, beta=0.0, boost=None):
    """k_topn + k_beam (k_beam_lm with a model, k_beam_boost with a phrase set) on the same stream: the device form of
    qasr.beam.search_host (blank None: the last class)"""
    blank = log_probs.shape[-1] - 1 if blank is None else blank
    if lm is not None:
        from .ngram import fixed_weights
        fixed_weights(alpha, beta)                              # refused before the first launch
    cid, cq = ctc_topn(log_probs, lens, cutoff_top_n, stream=stream)
    return ctc_beam(cid, cq, lens, blank, beam_width, n_best, stream=stream, lm=lm, alpha=alpha, beta=beta, boost=boost)


class AlignArgs(C.Structure):
    """qasr_ctc_align_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'T', 'C', 'P', 'K', 'blank', 'max_labels')] +
                [('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64)] +
                [(n, C.c_void_p) for n in ('log_probs', 'lens', 'targets', 'target_lens')] +
                [('lae_entries', C.c_uint32), ('reserved', C.c_uint32), ('lae_table', C.c_void_p), ('workspace', C.c_void_p),
                 ('workspace_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('start', 'nframes', 'score', 'path_score', 'total', 'ok')] +
                [('star_logp', C.c_void_p), ('star_pitch', C.c_int64)])


class StarArgs(C.Structure):
    """qasr_ctc_star_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'T', 'C')] +
                [('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64), ('log_probs', C.c_void_p), ('lens', C.c_void_p),
                 ('penalty', C.c_float), ('reserved', C.c_uint32), ('star', C.c_void_p), ('star_pitch', C.c_int64)])


def _row_pitch(t, T):
    """the row pitch of a plane [rows, T] whose frames are contiguous (a single row: at least T)"""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), T)


def _lattice_logp(who, cls, log_probs, lens, dims='[B, T, C]', struct_size=None):
    """What every CTC lattice binding opens with, under the call's name `who`: the library loaded, log_probs checked, it and lens
    coerced and written with the two pitches into a fresh struct of type cls.  Returns (the struct, lp, ln, (B, T, C))."""
    load_library()
    assert log_probs.is_cuda and log_probs.dim() == 3 and log_probs.dtype == torch.float32, \
        f'{who}: log_probs must be a cuda float32 tensor {dims}'
    lp = log_probs if log_probs.stride(2) == 1 or log_probs.shape[2] == 1 else log_probs.contiguous()
    B, T, _ = lp.shape
    a = cls()
    a.struct_size = C.sizeof(cls) if struct_size is None else struct_size
    a.log_probs, a.pitch_utt, a.pitch_frame = lp.data_ptr(), (lp.stride(0) if B > 1 else max(lp.stride(0), T * lp.stride(1))), lp.stride(1)
    ln = None
    if lens is not None:
        ln = lens.to(device=lp.device, dtype=torch.int32).contiguous()
        a.lens = ln.data_ptr()
    return a, lp, ln, tuple(lp.shape)


def _lattice_targets(who, a, targets, target_lens, dev, rows='P'):
    """targets / target_lens checked for their ranks, coerced and written into the struct; returns (tg, tl)"""
    assert targets.dim() == 2 and target_lens.dim() == 1, f'{who}: targets must be [{rows}, max_labels], target_lens [{rows}]'
    tg, tl = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (targets, target_lens))
    a.targets, a.target_lens = tg.data_ptr(), tl.data_ptr()
    return tg, tl


def _max_labels_error(who, cap, ML):
    return ValueError(f'{who}: max_labels (the row pitch of targets) must be 1 .. {cap}, got {ML}')


def _align_targets(who, a, targets, target_lens, dev):
    """the targets of ctc_align and ctc_post: P rows of at most MAX_LABELS labels, P lengths"""
    from .align import MAX_LABELS
    tg, tl = _lattice_targets(who, a, targets, target_lens, dev)
    P, ML = tg.shape
    if ML > MAX_LABELS:                                             # refused here: the kernel holds at most this many labels
        raise _max_labels_error(who, MAX_LABELS, ML)
    if tl.shape[0] != P:
        raise ValueError(f'{who}: {P} target rows but {tl.shape[0]} lengths')
    return tg, tl


def _band_targets(who, a, targets, target_lens, dev, P, T):
    """the targets of ctc_align_band and ctc_post_band: one row and one length per recording, and the two limits of the band"""
    from .align import BAND_MAX_FRAMES, BAND_MAX_LABELS
    tg, tl = _lattice_targets(who, a, targets, target_lens, dev)
    ML = tg.shape[1]
    if tg.shape[0] != P or tl.shape[0] != P:
        raise ValueError(f'{who}: {P} recordings but {tg.shape[0]} target rows and {tl.shape[0]} lengths')
    if not 1 <= ML <= BAND_MAX_LABELS:
        raise _max_labels_error(who, BAND_MAX_LABELS, ML)
    if T > BAND_MAX_FRAMES:
        raise ValueError(f'{who}: at most {BAND_MAX_FRAMES} frames, got {T}')
    return tg, tl


def _set_outputs(who, a, out, table):
    """Each (name, dtype, shape, optional) of the table: out.<name> is a contiguous cuda tensor of that dtype and shape, or None
    where optional; its pointer goes into the struct's field of the same name."""
    for n, dt, shape, optional in table:
        t = getattr(out, n)
        assert optional if t is None else (t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shape), f'{who}: out.{n}'
        setattr(a, n, 0 if t is None else t.data_ptr())


def _set_workspace(a, workspace, dev, query, *shape):
    """the caller's workspace, or query(*shape) bytes allocated by torch here, into the struct; returns the tensor"""
    if workspace is None:
        workspace = torch.empty(max(query(*shape), 8), device=dev, dtype=torch.uint8)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return workspace


def _set_star(who, a, star, B, T, dev):
    """the wildcard's plane, a cuda float32 [B, T] whose frames are contiguous, into the struct; returns the tensor to keep alive"""
    assert star.is_cuda and star.dtype == torch.float32 and tuple(star.shape) == (B, T), \
        f'{who}: star must be a cuda float32 plane [{B}, {T}]'
    st = star.to(dev) if T == 1 or star.stride(1) == 1 else star.contiguous()
    a.star_logp, a.star_pitch = st.data_ptr(), _row_pitch(st, T)
    return st


def _set_post(who, a, result, result_name, ins, out, P, T, ML, dev):
    """What ctc_post and ctc_post_band share behind their targets.  `ins`, (field, shape) rows: the alignment's outputs that the
    kernel reads, checked, coerced and written (result.ok is the struct's ok_in); the PostResult, allocated here unless the caller
    owns it, checked and written, frame_post with its row pitch; the table.  Returns (out, the coerced inputs, the table)."""
    from .align import PostResult
    from .beam import TAB_ENTRIES
    i32 = dict(device=dev, dtype=torch.int32)
    kept = []
    for n, shape in ins:
        t = getattr(result, n)
        assert t is not None and tuple(t.shape) == shape, f'{who}: {result_name}.{n} must be {list(shape)}'
        kept.append(t.to(**i32).contiguous())
        setattr(a, 'ok_in' if n == 'ok' else n, kept[-1].data_ptr())
    if out is None:
        out = PostResult(frame_post=torch.empty(P, T, **i32), label_post=torch.empty(P, ML, **i32),
                         total=torch.empty(P, device=dev, dtype=torch.int64), ok=torch.empty(P, **i32))
    fp = out.frame_post
    assert fp is not None and fp.is_cuda and fp.dtype == torch.int32 and tuple(fp.shape) == (P, T) and (T == 1 or fp.stride(1) == 1), \
        f'{who}: out.frame_post'
    _set_outputs(who, a, out, (('label_post', torch.int32, (P, ML), False), ('total', torch.int64, (P,), True), ('ok', torch.int32, (P,), False)))
    a.frame_post, a.post_pitch = fp.data_ptr(), _row_pitch(fp, T)
    tab = lae_table_device(dev)
    a.lae_entries, a.lae_table = TAB_ENTRIES, tab.data_ptr()
    return out, kept, tab


def _lattice_launch(symbol, a, dev, stream, out, keep):
    with torch.cuda.device(dev):
        _check(getattr(load_library(), symbol)(_stream_ptr(stream), C.byref(a)), symbol)
    out._keep = keep                                                # device memory the asynchronous launch reads
    return out


def ctc_star(log_probs, lens, penalty, out=None, stream=None):
    """qasr_ctc_star: the wildcard's emission plane on the device (k_star, one launch on the current stream, no host
    synchronisation); equal to qasr.align.star_host byte for byte.  log_probs: a cuda float32 tensor [B, T, C] (any utterance
    / frame pitch, classes contiguous); lens int32 [B] optional; penalty: nats per frame, finite, 0 .. 16 (refused by name
    otherwise).  Returns a cuda float32 tensor [B, T]; `out`: a caller-owned one (rows of any pitch >= T)."""
    from .align import check_star_penalty
    a, lp, ln, (B, T, Cn) = _lattice_logp('ctc_star', StarArgs, log_probs, lens)
    a.B, a.T, a.C, a.penalty = B, T, Cn, float(check_star_penalty(penalty, 'ctc_star'))
    if out is None:
        out = torch.empty(B, T, device=lp.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, T) and (T == 1 or out.stride(1) == 1), 'ctc_star: out'
    a.star, a.star_pitch = out.data_ptr(), _row_pitch(out, T)
    with torch.cuda.device(lp.device):
        _check(load_library().qasr_ctc_star(_stream_ptr(stream), C.byref(a)), 'qasr_ctc_star')
    return out


class SpotArgs(C.Structure):
    """qasr_ctc_spot_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('B', 'T', 'C', 'K', 'max_labels', 'blank', 'threshold_q', 'max_span', 'max_hits')] +
                [('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64), ('log_probs', C.c_void_p), ('lens', C.c_void_p),
                 ('star_logp', C.c_void_p), ('star_pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('targets', 'target_lens', 'hit_start', 'hit_end', 'hit_score', 'n_hits', 'ok',
                                           'trace_score', 'trace_start')] +
                [('trace_pitch', C.c_int64)])


def ctc_spot(log_probs, lens, star, targets, target_lens, blank, threshold, max_span, max_hits=16, want_trace=False, out=None,
             stream=None):
    """qasr_ctc_spot: keyword spotting on the device (k_spot, one launch on the current stream, no host synchronisation); equal
    to qasr.spot.spot_host byte for byte.  log_probs: a cuda float32 tensor [B, T, C] (any utterance / frame pitch, classes
    contiguous); lens int32 [B] optional; star: the cuda float32 plane [B, T] of ctc_star(log_probs, lens, 0.0); targets int32
    [K, max_labels] with target_lens int32 [K]: the keywords, shared by all utterances (problem p = u * K + k); threshold: nats
    per frame, -16 .. 0; max_span: frames, 1 .. 65536; max_hits: hits stored per problem.  Returns a qasr.spot.SpotResult of
    cuda tensors (want_trace: with trace_score / trace_start [B * K, T]); `out`: a caller-owned one."""
    from .spot import MAX_LABELS, SpotResult, check_max_span, check_threshold
    who, i32, i64 = 'ctc_spot', torch.int32, torch.int64
    a, lp, ln, (B, T, Cn) = _lattice_logp(who, SpotArgs, log_probs, lens)
    a.threshold_q, a.max_span, MH = check_threshold(threshold, who), check_max_span(max_span, who), int(max_hits)
    if MH < 1:
        raise ValueError(f'ctc_spot: max_hits must be at least 1, got {max_hits!r}')
    dev = lp.device
    tg, tl = _lattice_targets(who, a, targets, target_lens, dev, 'K')
    K, ML = tg.shape
    if not 1 <= ML <= MAX_LABELS:                                   # refused here: the kernel holds at most this many labels
        raise _max_labels_error(who, MAX_LABELS, ML)
    if tl.shape[0] != K or K < 1:
        raise ValueError(f'ctc_spot: {K} target rows but {tl.shape[0]} lengths')
    P = B * K
    if out is None:
        new = lambda dt, *shape: torch.empty(*shape, device=dev, dtype=dt)
        out = SpotResult(new(i32, P, MH), new(i32, P, MH), new(i64, P, MH), new(i32, P), new(i32, P),
                         new(i64, P, T) if want_trace else None, new(i32, P, T) if want_trace else None, K)
    _set_outputs(who, a, out, (('hit_start', i32, (P, MH), False), ('hit_end', i32, (P, MH), False), ('hit_score', i64, (P, MH), False),
                               ('n_hits', i32, (P,), False), ('ok', i32, (P,), False)))
    assert (out.trace_score is None) == (out.trace_start is None), 'ctc_spot: out.trace_score and out.trace_start go together'
    if out.trace_score is not None:                                 # the two planes: rows of any one pitch >= T
        ts, tb = out.trace_score, out.trace_start
        assert ts.is_cuda and ts.dtype == i64 and tuple(ts.shape) == (P, T) and (T == 1 or ts.stride(1) == 1), 'ctc_spot: out.trace_score'
        assert tb.is_cuda and tb.dtype == i32 and tuple(tb.shape) == (P, T) and (T == 1 or tb.stride(1) == 1), 'ctc_spot: out.trace_start'
        a.trace_score, a.trace_start, a.trace_pitch = ts.data_ptr(), tb.data_ptr(), _row_pitch(ts, T)
        assert P == 1 or tb.stride(0) == a.trace_pitch, 'ctc_spot: the two trace planes must share one row pitch'
    out.n_keywords = K
    st = _set_star(who, a, star, B, T, dev)
    a.B, a.T, a.C, a.K, a.max_labels, a.blank, a.max_hits = B, T, Cn, K, ML, int(blank), MH
    return _lattice_launch('qasr_ctc_spot', a, dev, stream, out, (lp, ln, st, tg, tl))


class EditArgs(C.Structure):
    """qasr_edit_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('mode', 'B', 'K', 'C', 'max_hyp', 'max_ref', 'pad_')] +
                [('hyp_pitch', C.c_int64), ('ref_pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('hyp', 'hyp_lens', 'ref', 'ref_lens', 'n_hyps', 'is_space', 'rows', 'totals',
                                           'workspace')] +
                [('workspace_bytes', C.c_size_t)])


def edit_workspace_bytes(P, max_hyp, max_ref, mode):
    """qasr_edit_workspace_bytes; mode: 'char' / 'word'"""
    from .edit import check_mode
    return int(load_library().qasr_edit_workspace_bytes(int(P), int(max_hyp), int(max_ref), check_mode(mode, 'edit_workspace_bytes')))


def _edit_rows(who, t, name):
    """an id matrix for k_edit: cuda int32 [rows, ids] with contiguous ids (rows of any pitch)"""
    assert t.is_cuda and t.dim() == 2, f'{who}: {name} must be a cuda matrix [rows, ids]'
    t = t if t.dtype == torch.int32 else t.to(torch.int32)
    return t if t.shape[1] == 1 or t.stride(1) == 1 else t.contiguous()


def _edit_fill(who, a, hyp, hyp_lens, ref, ref_lens, n_classes, mode, is_space, rows_per_ref, n_hyps):
    """What the two edit bindings share, under the call's name `who`: the rows, lengths and mask checked, coerced and written
    into the struct `a` with the shape and the pitches.  Returns (tensors to keep alive, device, P, max_hyp, max_ref, K)."""
    from .edit import check_mode, check_widths
    a.struct_size, a.mode = C.sizeof(type(a)), check_mode(mode, who)
    h, r = _edit_rows(who, hyp, 'hyp'), _edit_rows(who, ref, 'ref')
    dev = h.device
    (P, MH), (B, MR), K = h.shape, r.shape, int(rows_per_ref)
    if K < 1 or B < 1 or P != B * K:
        raise ValueError(f'{who}: {P} hypothesis rows are not {B} references * {K} rows per reference')
    if int(n_classes) < 1:
        raise ValueError(f'{who}: n_classes must be at least 1, got {n_classes}')
    check_widths(MH, MR, who)
    keep = [h, r]
    for name, v, n in (('hyp_lens', hyp_lens, P), ('ref_lens', ref_lens, B), ('n_hyps', n_hyps, B)):
        if v is not None:
            if tuple(v.shape) != (n,):
                raise ValueError(f'{who}: {name} must have {n} entries')
            v = v.to(device=dev, dtype=torch.int32).contiguous()
            keep.append(v)
            setattr(a, name, v.data_ptr())
    if a.mode == 1:
        if is_space is None:
            raise ValueError(f'{who}: word mode needs is_space')
        if tuple(is_space.shape) != (int(n_classes),):
            raise ValueError(f'{who}: is_space must have one entry per class ({int(n_classes)}), got shape {tuple(is_space.shape)}')
        sp = is_space.to(device=dev, dtype=torch.uint8).contiguous()
        keep.append(sp)
        a.is_space = sp.data_ptr()
    a.B, a.K, a.C, a.max_hyp, a.max_ref = B, K, int(n_classes), MH, MR
    a.hyp, a.hyp_pitch, a.ref, a.ref_pitch = h.data_ptr(), _row_pitch(h, MH), r.data_ptr(), _row_pitch(r, MR)
    return keep, dev, P, MH, MR, K


def edit_distance(hyp, hyp_lens, ref, ref_lens, n_classes, mode='char', is_space=None, rows_per_ref=1, n_hyps=None, totals=None,
                  workspace=None, out=None, stream=None):
    """qasr_edit_distance: word / character error counts on the device (k_edit_cut, k_edit, k_edit_totals: three launches on the
    current stream, no host synchronisation); equal to qasr.edit.edit_host byte for byte.  hyp: a cuda int32 matrix
    [B * rows_per_ref, max_hyp], ref [B, max_ref] (rows of any pitch), hyp_lens / ref_lens / n_hyps int32 vectors or None (None
    lengths: the padded rows); is_space: uint8 [n_classes] (word mode); totals: a cuda int64 [16] block the call adds to (None: a
    zeroed one); `out`: a caller-owned cuda int32 [B * rows_per_ref, 8].  Returns a qasr.edit.EditResult of cuda tensors."""
    from .edit import ROW_WORDS, TOTAL_WORDS, EditResult
    who = 'edit_distance'
    lib = load_library()
    a = EditArgs()
    keep, dev, P, MH, MR, K = _edit_fill(who, a, hyp, hyp_lens, ref, ref_lens, n_classes, mode, is_space, rows_per_ref, n_hyps)
    if totals is None:
        totals = torch.zeros(TOTAL_WORDS, device=dev, dtype=torch.int64)
    assert totals.is_cuda and totals.dtype == torch.int64 and tuple(totals.shape) == (TOTAL_WORDS,) and totals.is_contiguous(), \
        f'{who}: totals must be a cuda int64 [{TOTAL_WORDS}]'
    if out is None:
        out = torch.empty(P, ROW_WORDS, device=dev, dtype=torch.int32)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (P, ROW_WORDS) and out.is_contiguous(), \
        f'{who}: out must be a cuda int32 [{P}, {ROW_WORDS}]'
    a.rows, a.totals = out.data_ptr(), totals.data_ptr()
    keep.append(_set_workspace(a, workspace, dev, lib.qasr_edit_workspace_bytes, P, MH, MR, a.mode))
    res = EditResult(out, totals, K)
    return _lattice_launch('qasr_edit_distance', a, dev, stream, res, tuple(keep))


class MbrArgs(C.Structure):
    """qasr_mbr_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('mode', 'B', 'K', 'C', 'max_ids', 'scale_q')] +
                [('wtab_entries', C.c_uint32), ('label_pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('labels', 'n_labels', 'score', 'n_hyps', 'is_space', 'wtab', 'dist', 'weight', 'wsum',
                                           'risk', 'order', 'ok', 'workspace')] +
                [('workspace_bytes', C.c_size_t)])


_mbr_tables = {}


def mbr_table_device(device):
    """qasr.mbr.weight_table() on `device` (its 16384 u32 entries as an int32 tensor), uploaded once per device, as
    lae_table_device: the first mbr_rerank of a device must run outside a stream capture (or call this first)."""
    from . import mbr
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    t = _mbr_tables.get(dev)
    if t is None:
        t = _mbr_tables[dev] = torch.from_numpy(mbr.weight_table().view(np.int32).copy()).to(dev)
    return t


def mbr_workspace_bytes(B, K, max_ids, mode):
    """qasr_mbr_workspace_bytes; mode: 'char' / 'word'"""
    from .edit import check_mode
    return int(load_library().qasr_mbr_workspace_bytes(int(B), int(K), int(max_ids), check_mode(mode, 'mbr_workspace_bytes')))


def mbr_rerank(labels, n_labels, score, n_hyps, n_classes, mode='word', is_space=None, scale=1.0, wtab=None, dist=None,
               workspace=None, out=None, stream=None):
    """qasr_ctc_mbr: minimum Bayes risk order of n-best rows on the device (k_edit_cut, k_mbr_pair, k_mbr_pick: three launches on
    the current stream, no host synchronisation); equal to qasr.mbr.mbr_host byte for byte.  The beam's tensors as they lie, no
    copy: labels cuda int32 [B, K, L] (ids contiguous, rows of one pitch >= L, utterances K rows apart), n_labels int32 [B, K],
    score int64 [B, K], n_hyps int32 [B] or None; is_space uint8 [n_classes] (word mode); wtab: the weight table on the device
    (None: mbr_table_device); dist: True for the matrix [B, K, K] in the result (None: it stays in the workspace); `out`: a
    caller-owned qasr.mbr.MbrResult of cuda tensors.  Returns an MbrResult of cuda tensors."""
    from .edit import check_mode
    from .mbr import WTAB_ENTRIES, MbrResult, check_scale, check_shape
    who, i32, i64 = 'mbr_rerank', torch.int32, torch.int64
    lib = load_library()
    a = MbrArgs()
    a.struct_size, a.mode = C.sizeof(MbrArgs), check_mode(mode, who)
    assert labels.is_cuda and labels.dim() == 3 and labels.dtype == i32, f'{who}: labels must be a cuda int32 tensor [B, K, L]'
    B, K, L = labels.shape
    check_shape(B, K, L, who)
    if int(n_classes) < 1:
        raise ValueError(f'{who}: n_classes must be at least 1, got {n_classes}')
    pitch = labels.stride(1) if K > 1 else max(labels.stride(1), L)
    if not ((L == 1 or labels.stride(2) == 1) and pitch >= L and (B == 1 or labels.stride(0) == K * pitch)):
        labels = labels.contiguous()
        pitch = L
    dev = labels.device
    a.scale_q = check_scale(scale, who)
    keep = [labels]
    for name, v, shape, dt in (('n_labels', n_labels, (B, K), i32), ('score', score, (B, K), i64), ('n_hyps', n_hyps, (B,), i32)):
        if v is None and name == 'n_hyps':
            continue
        if v is None or tuple(v.shape) != shape:
            raise ValueError(f'{who}: {name} must be {list(shape)}')
        v = v.to(device=dev, dtype=dt).contiguous()
        keep.append(v)
        setattr(a, name, v.data_ptr())
    if a.mode == 1:
        if is_space is None:
            raise ValueError(f'{who}: word mode needs is_space')
        if tuple(is_space.shape) != (int(n_classes),):
            raise ValueError(f'{who}: is_space must have one entry per class ({int(n_classes)}), got shape {tuple(is_space.shape)}')
        sp = is_space.to(device=dev, dtype=torch.uint8).contiguous()
        keep.append(sp)
        a.is_space = sp.data_ptr()
    tab = mbr_table_device(dev) if wtab is None else wtab
    assert tab.is_cuda and tab.is_contiguous() and tab.numel() == WTAB_ENTRIES and tab.element_size() == 4, \
        f'{who}: wtab must be a cuda tensor of {WTAB_ENTRIES} 32-bit entries'
    keep.append(tab)
    if out is None:
        new = lambda dt, *shape: torch.empty(*shape, device=dev, dtype=dt)
        out = MbrResult(new(i32, B, K, K) if dist else None, new(i32, B, K), new(i64, B), new(i64, B, K), new(i32, B, K), new(i32, B, K))
    _set_outputs(who, a, out, (('dist', i32, (B, K, K), True), ('weight', i32, (B, K), False), ('wsum', i64, (B,), False),
                               ('risk', i64, (B, K), False), ('order', i32, (B, K), False), ('ok', i32, (B, K), False)))
    a.B, a.K, a.C, a.max_ids, a.label_pitch = B, K, int(n_classes), L, pitch
    a.labels, a.wtab, a.wtab_entries = labels.data_ptr(), tab.data_ptr(), WTAB_ENTRIES
    keep.append(_set_workspace(a, workspace, dev, lib.qasr_mbr_workspace_bytes, B, K, L, a.mode))
    return _lattice_launch('qasr_ctc_mbr', a, dev, stream, out, tuple(keep))


class EditTraceArgs(C.Structure):
    """qasr_edit_trace_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('mode', 'B', 'K', 'C', 'max_hyp', 'max_ref', 'pad_')] +
                [('hyp_pitch', C.c_int64), ('ref_pitch', C.c_int64), ('ops_pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('hyp', 'hyp_lens', 'ref', 'ref_lens', 'n_hyps', 'is_space', 'rows', 'ops', 'n_ops',
                                           'workspace')] +
                [('workspace_bytes', C.c_size_t)])


def edit_trace_workspace_bytes(P, max_hyp, max_ref, mode):
    """qasr_edit_trace_workspace_bytes; mode: 'char' / 'word'"""
    from .edit import check_mode
    return int(load_library().qasr_edit_trace_workspace_bytes(int(P), int(max_hyp), int(max_ref),
                                                              check_mode(mode, 'edit_trace_workspace_bytes')))


def edit_trace(hyp, hyp_lens, ref, ref_lens, n_classes, mode='char', is_space=None, rows_per_ref=1, n_hyps=None, ops=None,
               n_ops=None, workspace=None, out=None, stream=None, max_workspace_bytes=1 << 30):
    """qasr_edit_trace: the edit path on the device (k_edit_cut, k_edit_trace: two launches on the current stream, no host
    synchronisation); equal to qasr.edit.trace_host byte for byte.  The rows as for edit_distance; ops: a caller-owned cuda uint8
    [B * rows_per_ref, >= HU + RU] whose ids are contiguous (rows of any pitch), n_ops: a cuda int32 [B * rows_per_ref], `out`: a
    cuda int32 [B * rows_per_ref, 8].  A shape whose workspace exceeds max_workspace_bytes is refused by name before anything
    is allocated.  Returns a qasr.edit.TraceResult of cuda tensors."""
    from .edit import ROW_WORDS, TraceResult, check_trace_workspace, unit_bound
    who = 'edit_trace'
    lib = load_library()
    a = EditTraceArgs()
    keep, dev, P, MH, MR, K = _edit_fill(who, a, hyp, hyp_lens, ref, ref_lens, n_classes, mode, is_space, rows_per_ref, n_hyps)
    check_trace_workspace(P, MH, MR, mode, max_workspace_bytes, who)
    units = unit_bound(MH, a.mode) + unit_bound(MR, a.mode)
    if ops is None:
        ops = torch.zeros(P, units, device=dev, dtype=torch.uint8)
    if not (ops.is_cuda and ops.dtype == torch.uint8 and ops.dim() == 2 and ops.shape[0] == P and ops.shape[1] >= units
            and ops.stride(1) == 1):
        raise ValueError(f'{who}: ops must be a cuda uint8 [{P}, >= {units}] (the unit bounds of the two widths)')
    if n_ops is None:
        n_ops = torch.empty(P, device=dev, dtype=torch.int32)
    assert n_ops.is_cuda and n_ops.dtype == torch.int32 and tuple(n_ops.shape) == (P,) and n_ops.is_contiguous(), \
        f'{who}: n_ops must be a cuda int32 [{P}]'
    if out is None:
        out = torch.empty(P, ROW_WORDS, device=dev, dtype=torch.int32)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (P, ROW_WORDS) and out.is_contiguous(), \
        f'{who}: out must be a cuda int32 [{P}, {ROW_WORDS}]'
    a.rows, a.ops, a.n_ops, a.ops_pitch = out.data_ptr(), ops.data_ptr(), n_ops.data_ptr(), _row_pitch(ops, ops.shape[1])
    keep.append(_set_workspace(a, workspace, dev, lib.qasr_edit_trace_workspace_bytes, P, MH, MR, a.mode))
    res = TraceResult(out, ops, n_ops, K)
    return _lattice_launch('qasr_edit_trace', a, dev, stream, res, tuple(keep))


def ctc_align_workspace_bytes(P, T, max_labels):
    return int(load_library().qasr_ctc_align_workspace_bytes(int(P), int(T), int(max_labels)))


def ctc_align(log_probs, lens, targets, target_lens, blank, problems_per_utt=1, want_total=True, workspace=None, out=None,
              stream=None, star=None):
    """qasr_ctc_align: CTC forced alignment and scoring of given label sequences on the device (k_align, one launch on the
    current stream, no host synchronisation); equal to qasr.align.align_host byte for byte.  log_probs: a cuda float32
    tensor [B, T, C] (any utterance / frame pitch, classes contiguous); lens int32 [B] optional; targets cuda int32
    [P, max_labels] with target_lens int32 [P], P = B * problems_per_utt (problem p belongs to utterance
    p // problems_per_utt).  want_total=False skips the forward pass (total None).  Returns a qasr.align.AlignResult of cuda
    tensors.  workspace: a caller-owned uint8 tensor of ctc_align_workspace_bytes(P, T, max_labels) bytes (None: allocated by
    torch here); `out`: a caller-owned AlignResult whose start / nframes / score / path_score / total may each be None.
    star: the wildcard's plane, a cuda float32 tensor [B, T] (ctc_star); with it the label id C is a valid target label
    (qasr.align.STAR_RULES) and k_align<., true> runs."""
    from .align import AlignResult
    from .beam import TAB_ENTRIES
    who, i32, i64 = 'ctc_align', torch.int32, torch.int64
    v1 = None if star is not None else AlignArgs.star_logp.offset   # no plane: the shorter struct, the call every build takes
    a, lp, ln, (B, T, Cn) = _lattice_logp(who, AlignArgs, log_probs, lens, struct_size=v1)
    dev, K = lp.device, int(problems_per_utt)
    tg, tl = _align_targets(who, a, targets, target_lens, dev)
    P, ML = tg.shape
    if out is None:
        new = lambda dt, *shape: torch.empty(*shape, device=dev, dtype=dt)
        out = AlignResult(labels=tg, n_labels=tl, start=new(i32, P, ML), nframes=new(i32, P, ML), score=new(torch.float32, P, ML),
                          path_score=new(i64, P), total=new(i64, P) if want_total else None, ok=new(i32, P), blank=int(blank),
                          problems_per_utt=K)
    _set_outputs(who, a, out, (('start', i32, (P, ML), True), ('nframes', i32, (P, ML), True), ('score', torch.float32, (P, ML), True),
                               ('path_score', i64, (P,), True), ('total', i64, (P,), True), ('ok', i32, (P,), True)))
    assert out.ok is not None, 'ctc_align: out.ok is required'
    workspace = _set_workspace(a, workspace, dev, ctc_align_workspace_bytes, P, T, ML)
    tab = lae_table_device(dev) if out.total is not None else None  # the table is needed for total only
    a.lae_entries, a.lae_table = TAB_ENTRIES, 0 if tab is None else tab.data_ptr()
    a.B, a.T, a.C, a.P, a.K, a.blank, a.max_labels = B, T, Cn, P, K, int(blank), ML
    st = None if star is None else _set_star(who, a, star, B, T, dev)
    return _lattice_launch('qasr_ctc_align', a, dev, stream, out, (lp, ln, tg, tl, workspace, tab, st))


class PostArgs(C.Structure):
    """qasr_ctc_post_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'T', 'C', 'P', 'K', 'blank', 'max_labels')] +
                [('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64)] +
                [(n, C.c_void_p) for n in ('log_probs', 'lens', 'targets', 'target_lens')] +
                [('lae_entries', C.c_uint32), ('reserved', C.c_uint32), ('lae_table', C.c_void_p)] +
                [(n, C.c_void_p) for n in ('start', 'nframes', 'ok_in')] +
                [('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('frame_post', C.c_void_p), ('post_pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('label_post', 'total', 'ok')] +
                [('star_logp', C.c_void_p), ('star_pitch', C.c_int64)])


def ctc_post_workspace_bytes(P, T):
    return int(load_library().qasr_ctc_post_workspace_bytes(int(P), int(T)))


def ctc_post(log_probs, lens, targets, target_lens, blank, align_result, problems_per_utt=1, star=None, workspace=None, out=None,
             stream=None):
    """qasr_ctc_post: the log-posteriors of an alignment's own states on the device (k_post: forward-backward, one launch on
    the current stream, no host synchronisation); equal to qasr.align.post_host byte for byte.  The inputs are ctc_align's;
    align_result: the AlignResult of ctc_align for them (its start, nframes and ok are read on the device, so the call may
    follow ctc_align at once).  Returns a qasr.align.PostResult of cuda tensors: frame_post int32 [P, T], label_post int32
    [P, max_labels], total int64 [P], ok int32 [P].  workspace: a caller-owned uint8 tensor of ctc_post_workspace_bytes(P, T)
    bytes, 8-byte aligned (None: allocated by torch here); `out`: a caller-owned PostResult whose total may be None and whose
    frame_post rows may have any pitch >= T."""
    who = 'ctc_post'
    a, lp, ln, (B, T, Cn) = _lattice_logp(who, PostArgs, log_probs, lens)
    dev = lp.device
    tg, tl = _align_targets(who, a, targets, target_lens, dev)
    P, ML = tg.shape
    out, ins, tab = _set_post(who, a, align_result, 'align_result', (('start', (P, ML)), ('nframes', (P, ML)), ('ok', (P,))), out, P, T,
                              ML, dev)
    workspace = _set_workspace(a, workspace, dev, ctc_post_workspace_bytes, P, T)
    a.B, a.T, a.C, a.P, a.K, a.blank, a.max_labels = B, T, Cn, P, int(problems_per_utt), int(blank), ML
    st = None if star is None else _set_star(who, a, star, B, T, dev)
    return _lattice_launch('qasr_ctc_post', a, dev, stream, out, (lp, ln, tg, tl, ins, workspace, tab, st))


class AlignBandArgs(C.Structure):
    """qasr_ctc_align_band_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'T', 'C', 'blank', 'max_labels', 'band_states')] +
                [('reserved', C.c_uint32), ('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64)] +
                [(n, C.c_void_p) for n in ('log_probs', 'lens', 'targets', 'target_lens', 'workspace')] +
                [('workspace_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('start', 'nframes', 'score', 'path_score', 'frame_logp', 'band_base', 'ok')] +
                [('star_logp', C.c_void_p), ('star_pitch', C.c_int64)])


def ctc_align_band_workspace_bytes(P, T, band_states):
    return int(load_library().qasr_ctc_align_band_workspace_bytes(int(P), int(T), int(band_states)))


def ctc_align_band(log_probs, lens, targets, target_lens, blank, band_states=None, want_band_base=True, workspace=None, out=None,
                   stream=None, star=None):
    """qasr_ctc_align_band: banded CTC alignment of whole recordings against whole transcripts on the device (k_align_band,
    one launch on the current stream, no host synchronisation); equal to qasr.align.align_band_host byte for byte.
    log_probs: a cuda float32 tensor [P, T, C] (any recording / frame pitch, classes contiguous); lens int32 [P] optional;
    targets cuda int32 [P, max_labels] with target_lens int32 [P].  band_states: 256, 1024 or 4352 (None: the smallest that
    holds 2 * max_labels + 1 states, else 4352).  Returns a qasr.align.BandResult of cuda tensors.  workspace: a caller-owned
    uint8 tensor of ctc_align_band_workspace_bytes(P, T, band_states) bytes (None: allocated by torch here); `out`: a
    caller-owned BandResult whose start / nframes / score / path_score / frame_logp / band_base may each be None.
    star: the wildcard's plane, a cuda float32 tensor [P, T] (ctc_star), as in ctc_align."""
    from .align import BAND_BLOCK, BandResult, pick_band_states
    who, i32, f32 = 'ctc_align_band', torch.int32, torch.float32
    v1 = None if star is not None else AlignBandArgs.star_logp.offset   # (as ctc_align)
    a, lp, ln, (P, T, Cn) = _lattice_logp(who, AlignBandArgs, log_probs, lens, '[P, T, C]', struct_size=v1)
    dev = lp.device
    tg, tl = _band_targets(who, a, targets, target_lens, dev, P, T)
    ML = tg.shape[1]
    BW = pick_band_states(ML, band_states)
    NB = (T + BAND_BLOCK - 1) // BAND_BLOCK
    if out is None:
        new = lambda dt, *shape: torch.empty(*shape, device=dev, dtype=dt)
        out = BandResult(labels=tg, n_labels=tl, start=new(i32, P, ML), nframes=new(i32, P, ML), score=new(f32, P, ML),
                         path_score=new(torch.int64, P), total=None, ok=new(i32, P), blank=int(blank), problems_per_utt=1,
                         frame_logp=new(f32, P, T), band_base=new(i32, P, NB) if want_band_base else None)
    out.band_states = BW
    _set_outputs(who, a, out, (('start', i32, (P, ML), True), ('nframes', i32, (P, ML), True), ('score', f32, (P, ML), True),
                               ('path_score', torch.int64, (P,), True), ('frame_logp', f32, (P, T), True),
                               ('band_base', i32, (P, NB), True), ('ok', i32, (P,), True)))
    assert out.ok is not None, 'ctc_align_band: out.ok is required'
    workspace = _set_workspace(a, workspace, dev, ctc_align_band_workspace_bytes, P, T, BW)
    a.B, a.T, a.C, a.blank, a.max_labels, a.band_states = P, T, Cn, int(blank), ML, BW
    st = None if star is None else _set_star(who, a, star, P, T, dev)
    return _lattice_launch('qasr_ctc_align_band', a, dev, stream, out, (lp, ln, tg, tl, workspace, st))


class PostBandArgs(C.Structure):
    """qasr_ctc_post_band_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'T', 'C', 'blank', 'max_labels', 'band_states')] +
                [('reserved', C.c_uint32), ('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64)] +
                [(n, C.c_void_p) for n in ('log_probs', 'lens', 'targets', 'target_lens')] +
                [('lae_entries', C.c_uint32), ('reserved2', C.c_uint32), ('lae_table', C.c_void_p)] +
                [(n, C.c_void_p) for n in ('start', 'nframes', 'ok_in', 'band_base')] +
                [('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('frame_post', C.c_void_p), ('post_pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('label_post', 'total', 'ok')] +
                [('star_logp', C.c_void_p), ('star_pitch', C.c_int64)])


def ctc_post_band_workspace_bytes(P, T):
    return int(load_library().qasr_ctc_post_band_workspace_bytes(int(P), int(T)))


def ctc_post_band(log_probs, lens, targets, target_lens, blank, band_result, star=None, workspace=None, out=None, stream=None):
    """qasr_ctc_post_band: the log-posteriors of a banded alignment's own states, inside its band, on the device (k_post_band:
    forward-backward, one launch on the current stream, no host synchronisation); equal to qasr.align.post_band_host byte for
    byte.  The inputs are ctc_align_band's; band_result: the BandResult of ctc_align_band for them, made with
    want_band_base=True (its start, nframes, ok and band_base are read on the device, so the call may follow ctc_align_band at
    once; its band_states is the width).  Returns a qasr.align.PostResult of cuda tensors: frame_post int32 [P, T], label_post
    int32 [P, max_labels], total int64 [P], ok int32 [P].  workspace: a caller-owned uint8 tensor of
    ctc_post_band_workspace_bytes(P, T) bytes, 8-byte aligned (None: allocated by torch here); `out`: a caller-owned PostResult
    whose total may be None and whose frame_post rows may have any pitch >= T."""
    from .align import BAND_BLOCK, pick_band_states
    who = 'ctc_post_band'
    a, lp, ln, (P, T, Cn) = _lattice_logp(who, PostBandArgs, log_probs, lens, '[P, T, C]')
    dev = lp.device
    tg, tl = _band_targets(who, a, targets, target_lens, dev, P, T)
    ML = tg.shape[1]
    try:
        BW = pick_band_states(ML, band_result.band_states or None)
    except ValueError as e:
        raise ValueError(f'ctc_post_band: band_result.{e}') from None
    NB = (T + BAND_BLOCK - 1) // BAND_BLOCK
    out, ins, tab = _set_post(who, a, band_result, 'band_result',
                              (('start', (P, ML)), ('nframes', (P, ML)), ('ok', (P,)), ('band_base', (P, NB))), out, P, T, ML, dev)
    workspace = _set_workspace(a, workspace, dev, ctc_post_band_workspace_bytes, P, T)
    a.B, a.T, a.C, a.blank, a.max_labels, a.band_states = P, T, Cn, int(blank), ML, BW
    st = None if star is None else _set_star(who, a, star, P, T, dev)
    return _lattice_launch('qasr_ctc_post_band', a, dev, stream, out, (lp, ln, tg, tl, ins, workspace, tab, st))


class ResampleArgs(C.Structure):
    """qasr_resample_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('B', 'channels', 'dtype', 'L', 'M', 'W', 'reserved')] +
                [('blob', C.c_void_p), ('blob_bytes', C.c_size_t), ('in_', C.c_void_p), ('in_lens', C.c_void_p),
                 ('in_pitch', C.c_int64), ('out', C.c_void_p), ('out_pitch', C.c_int64), ('out_lens', C.c_void_p)])


PCM_S16, PCM_F32 = 0, 1
_resample_blobs = {}                    # (sr_in, sr_out, quality, device) -> the packed table on the device


def resample_check(blob: bytes):
    """qasr_resample_check: raises QasrError naming the first malformed field of a packed resampling table (host-only, no GPU)"""
    lib = load_library()
    if lib.qasr_resample_check(bytes(blob), len(blob)) != 0:
        raise QasrError('malformed resampling table: ' + lib.qasr_last_error().decode())


def resample_out_samples(in_samples, L, M):
    return int(load_library().qasr_resample_out_samples(int(in_samples), int(L), int(M)))


def resample_plan(plan, device):
    """The packed table of a qasr.resample.ResamplePlan on `device` as a uint8 tensor: packed, validated (qasr_resample_check)
    and uploaded once per (sr_in, sr_out, quality, device) and kept.  The upload is a host-to-device copy: the first resample
    of a rate must run outside a stream capture (or call this first); later calls only launch."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    key = (plan.sr_in, plan.sr_out, plan.quality, dev)
    t = _resample_blobs.get(key)
    if t is None:
        blob = plan.pack()
        resample_check(blob)
        t = _resample_blobs[key] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    return t


def resample(x, lens, plan, channels=1, out=None, out_lens=None, stream=None):
    """qasr_resample: int16 or float32 PCM [B, S * channels] (interleaved) at plan.sr_in with `lens` frames per utterance ->
    (float32 [B, plan.out_len(S)] at plan.sr_out, zeros behind each row's length, int32 lengths [B]): k_resample, one launch
    on the current stream, no host synchronisation; equal to qasr.resample.resample_host byte for byte.  `out` / `out_lens`:
    caller-owned cuda tensors (float32 [B, pitch], any pitch: a row is cut at it; int32 [B]).  A CPU tensor, or a build
    without the library, runs the NumPy twin (the results return on x's device)."""
    from . import resample as rs
    ch = int(channels)
    if x.dim() != 2 or x.dtype not in (torch.int16, torch.float32):
        raise ValueError(f'resample: samples must be an int16 or float32 tensor [B, S * channels], got {x.dtype} {tuple(x.shape)}')
    if not 1 <= ch <= rs.MAX_CHANNELS or x.shape[1] % ch:
        raise ValueError(f'resample: channels must be 1 .. {rs.MAX_CHANNELS} and divide the row of {x.shape[1]} samples, got {ch}')
    B, S = x.shape[0], x.shape[1] // ch
    if not x.is_cuda or not os.path.exists(LIB_PATH):
        o, ol = rs.resample_host(x.cpu().numpy(), lens.cpu().numpy(), plan, ch)
        o, ol = torch.from_numpy(o).to(x.device), torch.from_numpy(ol).to(x.device)
        if out is not None:
            w = min(out.shape[1], o.shape[1])
            out.zero_()
            out[:, :w] = o[:, :w]
            o, ol = out, ol.clamp(max=out.shape[1])
        if out_lens is not None:
            out_lens.copy_(ol)
            ol = out_lens
        return o, ol
    lib = load_library()
    dev = x.device
    blob = resample_plan(plan, dev)
    xc = x.contiguous()
    ln = lens.to(device=dev, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty(B, plan.out_len(S), device=dev, dtype=torch.float32)
    if out_lens is None:
        out_lens = torch.empty(B, device=dev, dtype=torch.int32)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == B and out.stride(1) == 1, 'resample: out'
    assert out_lens.is_cuda and out_lens.dtype == torch.int32 and out_lens.is_contiguous() and out_lens.numel() == B, \
        'resample: out_lens'
    if B == 0:
        return out, out_lens
    a = ResampleArgs()
    a.struct_size = C.sizeof(ResampleArgs)
    a.B, a.channels, a.dtype = B, ch, PCM_S16 if x.dtype == torch.int16 else PCM_F32
    a.L, a.M, a.W = plan.L, plan.M, plan.W
    a.blob, a.blob_bytes = blob.data_ptr(), blob.numel()
    a.in_, a.in_lens, a.in_pitch = xc.data_ptr(), ln.data_ptr(), S
    a.out, a.out_pitch, a.out_lens = out.data_ptr(), (out.stride(0) if B > 1 else out.shape[1]), out_lens.data_ptr()
    if B > 1 and out.stride(0) != out.shape[1]:
        raise ValueError('resample: out must have contiguous rows (zeros are written to the pitch)')
    with torch.cuda.device(dev):
        _check(lib.qasr_resample(_stream_ptr(stream), C.byref(a)), 'qasr_resample')
    return out, out_lens


class LongformCutArgs(C.Structure):
    """qasr_longform_cut_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('R', 'Wn', 'Wl')] +
                [('audio', C.c_void_p), ('pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('lens', 'table', 'windows', 'window_lens')])


class LongformPlane(C.Structure):
    """qasr_longform_plane (include/qasr.h)"""
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('bytes_per_frame', C.c_int64), ('fill', C.c_uint32),
                ('reserved', C.c_uint32)]


class LongformStitchArgs(C.Structure):
    """qasr_longform_stitch_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('R', 'Wn', 'Tw', 'Tmax', 'guard', 'hop_frames', 'blank', 'seam_mode', 'n_planes')] +
                [(n, C.c_void_p) for n in ('table', 'enc_lens', 'tokens', 'frame_score', 'total_frames', 'seams')] +
                [('planes', LongformPlane * 6)])


SEAM_MODES = {'blank': 0, 'middle': 1}


def longform_table(plan, device):
    """The window table of a qasr.longform.WindowPlan on `device` (int32 [Wn, 4]), uploaded once per (plan, device) and kept
    on the plan.  The upload is a host-to-device copy: the first longform_cut / longform_stitch of a plan must run outside
    a stream capture (or call this first); later calls only launch."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    tabs = plan.__dict__.setdefault('_device_tables', {})
    if dev not in tabs:
        tabs[dev] = torch.from_numpy(plan.table.copy()).to(dev)
    return tabs[dev]


def longform_cut(audio, lens, plan, out=None, stream=None):
    """qasr_longform_cut: float32 audio [R, S] (rows of any pitch) with `lens` samples per recording -> (windows float32
    [Wn, Wl], zeros behind each window's length; window_lens int32 [Wn]) under a qasr.longform.WindowPlan: k_cut, one launch
    on the current stream, nothing read back; equal to qasr.longform.cut_host byte for byte.  `out`: a caller-owned
    (windows, window_lens) pair.  A CPU tensor, or a build without the library, runs the NumPy twin."""
    from . import longform as lf
    if audio.dim() != 2 or audio.dtype != torch.float32 or audio.shape[0] != plan.R:
        raise ValueError(f'longform_cut: audio must be a float32 tensor [{plan.R}, S], got {audio.dtype} {tuple(audio.shape)}')
    if not audio.is_cuda or not os.path.exists(LIB_PATH):
        w, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
        w, wl = torch.from_numpy(w).to(audio.device), torch.from_numpy(wl).to(audio.device)
        if out is not None:
            out[0].copy_(w)
            out[1].copy_(wl)
            return out
        return w, wl
    lib = load_library()
    dev = audio.device
    x = audio if audio.stride(1) == 1 else audio.contiguous()
    ln = lens.to(device=dev, dtype=torch.int32).contiguous()
    tab = longform_table(plan, dev)
    if out is None:
        out = (torch.empty(plan.Wn, plan.Wl, device=dev, dtype=torch.float32), torch.empty(plan.Wn, device=dev, dtype=torch.int32))
    win, wl = out
    assert win.is_cuda and win.dtype == torch.float32 and win.is_contiguous() and tuple(win.shape) == (plan.Wn, plan.Wl), 'longform_cut: out'
    assert wl.is_cuda and wl.dtype == torch.int32 and wl.is_contiguous() and wl.numel() == plan.Wn, 'longform_cut: out'
    a = LongformCutArgs()
    a.struct_size = C.sizeof(LongformCutArgs)
    a.R, a.Wn, a.Wl = plan.R, plan.Wn, plan.Wl
    a.audio, a.pitch = x.data_ptr(), (x.stride(0) if plan.R > 1 else x.shape[1])
    a.lens, a.table, a.windows, a.window_lens = ln.data_ptr(), tab.data_ptr(), win.data_ptr(), wl.data_ptr()
    with torch.cuda.device(dev):
        _check(lib.qasr_longform_cut(_stream_ptr(stream), C.byref(a)), 'qasr_longform_cut')
    win._keep = (x, ln, tab)
    return win, wl


def longform_stitch(plan, enc_lens, tokens, frame_score=None, planes=(), blank=None, seam='blank', out=None, stream=None):
    """qasr_longform_stitch: the per-frame outputs of a plan's windows - tokens int32 [Wn, Tw], frame_score float32 [Wn, Tw]
    or None, planes: cuda tensors [Wn, Tw, ...] of a multiple of 4 bytes per frame - joined per recording at the seams of
    qasr.longform.SEAM_RULES: k_stitch, one launch on the current stream, nothing read back; equal to
    qasr.longform.stitch_host byte for byte.  Returns (out_planes, total_frames int32 [R], seams int32 [Wn]) with out_planes
    = [tokens, frame_score (if given), *planes] stitched, each [R, plan.Tmax, ...].  `out`: the same triple, caller-owned.
    CPU tensors, or a build without the library, run the NumPy twin."""
    from . import longform as lf
    if blank is None:
        raise ValueError('longform_stitch: blank is required (the decoder\'s last class)')
    if seam not in SEAM_MODES:
        raise ValueError(f"longform_stitch: seam must be 'blank' or 'middle', got {seam!r}")
    if not tokens.is_cuda or not os.path.exists(LIB_PATH):
        o, tot, sm = lf.stitch_host(plan, enc_lens.cpu().numpy(), tokens.cpu().numpy(),
                                    None if frame_score is None else frame_score.cpu().numpy(),
                                    [p.cpu().numpy() for p in planes], blank, seam)
        res = ([torch.from_numpy(x).to(tokens.device) for x in o], torch.from_numpy(tot).to(tokens.device),
               torch.from_numpy(sm).to(tokens.device))
        if out is not None:
            for d, s_ in zip(out[0], res[0]):
                d.copy_(s_)
            out[1].copy_(res[1])
            out[2].copy_(res[2])
            return out
        return res
    lib = load_library()
    dev = tokens.device
    tok = tokens.to(torch.int32).contiguous()
    if tok.dim() != 2 or tok.shape[0] != plan.Wn:
        raise ValueError(f'longform_stitch: tokens must be [{plan.Wn}, Tw], got {tuple(tok.shape)}')
    Tw = tok.shape[1]
    fs = None if frame_score is None else frame_score.to(device=dev, dtype=torch.float32).contiguous()
    if fs is not None and fs.shape != tok.shape:
        raise ValueError('longform_stitch: frame_score must have the shape of tokens')
    src = [tok] + ([fs] if fs is not None else []) + [p.contiguous() for p in planes]
    if len(src) > lf.MAX_PLANES:
        raise ValueError(f'longform_stitch: at most {lf.MAX_PLANES} planes, tokens and frame_score included, got {len(src)}')
    bpf = []
    for i, p in enumerate(src):
        nbytes = p.element_size() * int(np.prod(p.shape[2:], dtype=np.int64)) if p.dim() >= 2 else 0
        if not p.is_cuda or p.dim() < 2 or tuple(p.shape[:2]) != (plan.Wn, Tw) or nbytes < 4 or nbytes % 4:
            raise ValueError(f'longform_stitch: plane {i} must be a cuda tensor [{plan.Wn}, {Tw}, bytes_per_frame, a multiple of 4], '
                             f'got {tuple(p.shape)} {p.dtype}')
        bpf.append(nbytes)
    ln = enc_lens.to(device=dev, dtype=torch.int32).contiguous()
    if ln.numel() != plan.Wn:
        raise ValueError(f'longform_stitch: {plan.Wn} windows but {ln.numel()} encoded lengths')
    tab = longform_table(plan, dev)
    if out is None:
        out = ([torch.empty((plan.R, plan.Tmax) + tuple(p.shape[2:]), device=dev, dtype=p.dtype) for p in src],
               torch.empty(plan.R, device=dev, dtype=torch.int32), torch.empty(plan.Wn, device=dev, dtype=torch.int32))
    dst, total, seams = out
    assert len(dst) == len(src), 'longform_stitch: out'
    for d, p in zip(dst, src):
        assert d.is_cuda and d.is_contiguous() and d.dtype == p.dtype and tuple(d.shape) == (plan.R, plan.Tmax) + tuple(p.shape[2:]), \
            'longform_stitch: out'
    for t, n in ((total, plan.R), (seams, plan.Wn)):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n, 'longform_stitch: out'
    a = LongformStitchArgs()
    a.struct_size = C.sizeof(LongformStitchArgs)
    a.R, a.Wn, a.Tw, a.Tmax, a.guard, a.hop_frames = plan.R, plan.Wn, Tw, plan.Tmax, plan.guard, plan.hop_frames
    a.blank, a.seam_mode, a.n_planes = int(blank), SEAM_MODES[seam], len(src)
    a.table, a.enc_lens, a.tokens, a.frame_score = tab.data_ptr(), ln.data_ptr(), tok.data_ptr(), 0 if fs is None else fs.data_ptr()
    a.total_frames, a.seams = total.data_ptr(), seams.data_ptr()
    for i, (p, d) in enumerate(zip(src, dst)):
        a.planes[i].src, a.planes[i].dst, a.planes[i].bytes_per_frame = p.data_ptr(), d.data_ptr(), bpf[i]
        a.planes[i].fill = (int(blank) & 0xffffffff) if i == 0 else 0
    with torch.cuda.device(dev):
        _check(lib.qasr_longform_stitch(_stream_ptr(stream), C.byref(a)), 'qasr_longform_stitch')
    total._keep = (src, ln, tab)
    return dst, total, seams


class StreamPushArgs(C.Structure):
    """qasr_stream_push_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('S', 'B', 'Wl', 'C', 'samples_per_frame', 'dtype', 'reserved')] +
                [('state', C.c_void_p), ('state_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('slots', 'flags', 'n_new', 'chunk')] + [('pitch', C.c_int64)])


class StreamWindowArgs(C.Structure):
    """qasr_stream_window_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] + [(n, C.c_int32) for n in ('S', 'B', 'Wl', 'C', 'samples_per_frame')] +
                [('reserved', C.c_int32 * 2), ('state', C.c_void_p), ('state_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('slots', 'windows', 'window_lens', 'first_frame')])


class StreamEmitArgs(C.Structure):
    """qasr_stream_emit_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('S', 'B', 'Wl', 'C', 'Rr', 'samples_per_frame', 'Tw', 'P', 'Ptail', 'blank', 'reserved')] +
                [('state', C.c_void_p), ('state_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('slots', 'flags', 'tokens', 'frame_score', 'enc_lens', 'first_frame', 'labels', 'start',
                                           'nframes', 'score', 'n_new_labels', 'status', 'total_frames', 'utt_score', 'tail_labels',
                                           'tail_n')])


def stream_state(S, plan, device):
    """Zeroed device state of S fresh streams under a qasr.stream.StreamPlan: an int32 tensor of
    qasr_stream_state_bytes(S, Wl, C) / 4 words (S blocks of 80 words, then S rings).  `stream_block(state, S)` views the
    blocks as [S, 80]."""
    lib = load_library()
    n = int(lib.qasr_stream_state_bytes(int(S), plan.Wl, plan.C))
    if n == 0:
        raise ValueError(f'stream_state: S {S}, Wl {plan.Wl}, C {plan.C} out of range')
    return torch.zeros(n // 4, device=device, dtype=torch.int32)


def stream_block(state, S):
    from . import stream as qs
    return state[:int(S) * qs.STATE_WORDS].view(int(S), qs.STATE_WORDS)


def _i32dev(t, B, what):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B, what


def stream_push(state, S, plan, slots, flags, n_new, chunk, stream=None):
    """qasr_stream_push: chunk float32 or int16 [B, n] (rows of any pitch) appended to the slots' rings; slots / flags /
    n_new: cuda int32 [B].  k_stream_push, one launch on the current stream, nothing read back; equal to
    qasr.stream.push_host byte for byte."""
    lib = load_library()
    if chunk.dim() != 2 or chunk.dtype not in (torch.float32, torch.int16) or not chunk.is_cuda:
        raise ValueError(f'stream_push: chunk must be a cuda float32 or int16 tensor [B, n], got {chunk.dtype} {tuple(chunk.shape)}')
    B = chunk.shape[0]
    x = chunk if chunk.stride(1) == 1 else chunk.contiguous()
    for t, w in ((slots, 'slots'), (flags, 'flags'), (n_new, 'n_new')):
        _i32dev(t, B, 'stream_push: ' + w)
    a = StreamPushArgs()
    a.struct_size = C.sizeof(StreamPushArgs)
    a.S, a.B, a.Wl, a.C, a.samples_per_frame = int(S), B, plan.Wl, plan.C, plan.samples_per_frame
    a.dtype = PCM_S16 if x.dtype == torch.int16 else PCM_F32
    a.state, a.state_bytes = state.data_ptr(), state.numel() * state.element_size()
    a.slots, a.flags, a.n_new = slots.data_ptr(), flags.data_ptr(), n_new.data_ptr()
    a.chunk, a.pitch = x.data_ptr(), (x.stride(0) if B > 1 else x.shape[1])
    with torch.cuda.device(state.device):
        _check(lib.qasr_stream_push(_stream_ptr(stream), C.byref(a)), 'qasr_stream_push')


class StreamRsPushArgs(C.Structure):
    """qasr_stream_rs_push_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('S', 'B', 'Wl', 'C', 'samples_per_frame', 'dtype', 'channels', 'L', 'M', 'W', 'hcap')] +
                [('state', C.c_void_p), ('state_bytes', C.c_size_t), ('rs_state', C.c_void_p), ('rs_state_bytes', C.c_size_t),
                 ('work', C.c_void_p), ('work_bytes', C.c_size_t), ('blob', C.c_void_p), ('blob_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('slots', 'flags', 'n_in', 'out_limit', 'chunk')] + [('pitch', C.c_int64)] +
                [(n, C.c_void_p) for n in ('n_taken', 'n_out', 'status')])


def stream_rs_state(S, rs_plan, device):
    """Zeroed resampler state of S fresh streams under a qasr.stream_rs.StreamResamplePlan: an int32 tensor of
    qasr_stream_rs_state_bytes(S, hcap) / 4 words (S blocks of 16 words, then S histories of hcap 8-byte entries)."""
    lib = load_library()
    n = int(lib.qasr_stream_rs_state_bytes(int(S), rs_plan.hcap))
    if n == 0:
        raise ValueError(f'stream_rs_state: S {S}, hcap {rs_plan.hcap} out of range')
    return torch.zeros(n // 4, device=device, dtype=torch.int32)


def stream_rs_work(B, device):
    """the workspace of qasr_stream_rs_push for up to B rows (qasr_stream_rs_work_bytes)"""
    return torch.zeros(int(load_library().qasr_stream_rs_work_bytes(int(B))) // 4, device=device, dtype=torch.int32)


def stream_rs_args(state, rs_state, S, rs_plan, slots, flags, n_in, out_limit, chunk, work=None, out=None):
    """the filled qasr_stream_rs_push_args of stream_rs_push (the tensors it points to are kept alive on it)"""
    lib = load_library()
    plan, rp, ch = rs_plan.stream_plan, rs_plan.resample_plan, rs_plan.channels
    if chunk.dim() != 2 or chunk.dtype not in (torch.float32, torch.int16) or not chunk.is_cuda or chunk.shape[1] % ch:
        raise ValueError(f'stream_rs_push: chunk must be a cuda float32 or int16 tensor [B, n * {ch}], got {chunk.dtype} {tuple(chunk.shape)}')
    B, dev = chunk.shape[0], state.device
    x = chunk if chunk.stride(1) == 1 and (B == 1 or chunk.stride(0) % ch == 0) else chunk.contiguous()
    for t, w in ((slots, 'slots'), (flags, 'flags'), (n_in, 'n_in'), (out_limit, 'out_limit')):
        _i32dev(t, B, 'stream_rs_push: ' + w)
    if work is None:
        work = stream_rs_work(B, dev)
    if out is None:
        out = tuple(torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
    for t in out:
        _i32dev(t, B, 'stream_rs_push: out')
    blob = resample_plan(rp, dev)
    a = StreamRsPushArgs()
    a.struct_size = C.sizeof(StreamRsPushArgs)
    a.S, a.B, a.Wl, a.C, a.samples_per_frame = int(S), B, plan.Wl, plan.C, plan.samples_per_frame
    a.dtype, a.channels = (PCM_S16 if x.dtype == torch.int16 else PCM_F32), ch
    a.L, a.M, a.W, a.hcap = rp.L, rp.M, rp.W, rs_plan.hcap
    a.state, a.state_bytes = state.data_ptr(), state.numel() * state.element_size()
    a.rs_state, a.rs_state_bytes = rs_state.data_ptr(), rs_state.numel() * rs_state.element_size()
    a.work, a.work_bytes = work.data_ptr(), work.numel() * work.element_size()
    a.blob, a.blob_bytes = blob.data_ptr(), blob.numel()
    a.slots, a.flags, a.n_in, a.out_limit = slots.data_ptr(), flags.data_ptr(), n_in.data_ptr(), out_limit.data_ptr()
    a.chunk, a.pitch = x.data_ptr(), (x.stride(0) // ch if B > 1 else x.shape[1] // ch)
    a.n_taken, a.n_out, a.status = (t.data_ptr() for t in out)
    a._keep = (x, work, blob, out)
    return a


def stream_rs_push(state, rs_state, S, rs_plan, slots, flags, n_in, out_limit, chunk, work=None, out=None, stream=None):
    """qasr_stream_rs_push: chunk int16 or float32 [B, n * channels] (interleaved, at the source's rate) appended to the slots'
    histories, and the resampled samples that became final written to the slots' sample rings; slots / flags / n_in /
    out_limit: cuda int32 [B].  Returns (n_taken, n_out, status), cuda int32 [B] (`out`: the same triple, caller-owned).
    k_stream_rs_append and k_stream_rs_fir, two launches on the current stream, nothing read back; equal to
    qasr.stream_rs.push_rs_host byte for byte, both states included.  The table is uploaded by the first call of a rate
    (engine.resample_plan): make that call outside a capture."""
    a = stream_rs_args(state, rs_state, S, rs_plan, slots, flags, n_in, out_limit, chunk, work, out)
    with torch.cuda.device(state.device):
        _check(load_library().qasr_stream_rs_push(_stream_ptr(stream), C.byref(a)), 'qasr_stream_rs_push')
    return a._keep[3]


def stream_window(state, S, plan, slots, out=None, stream=None):
    """qasr_stream_window: -> (windows float32 [B, Wl], zeros behind each length; window_lens int32 [B]; first_frame int32
    [B]).  k_stream_window, one launch, nothing read back; equal to qasr.stream.window_host byte for byte.  `out`: the same
    triple, caller-owned."""
    lib = load_library()
    B, dev = slots.numel(), state.device
    _i32dev(slots, B, 'stream_window: slots')
    if out is None:
        out = (torch.empty(B, plan.Wl, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.int32),
               torch.empty(B, device=dev, dtype=torch.int32))
    win, wl, first = out
    assert win.is_cuda and win.dtype == torch.float32 and win.is_contiguous() and tuple(win.shape) == (B, plan.Wl), 'stream_window: out'
    _i32dev(wl, B, 'stream_window: out')
    _i32dev(first, B, 'stream_window: out')
    a = StreamWindowArgs()
    a.struct_size = C.sizeof(StreamWindowArgs)
    a.S, a.B, a.Wl, a.C, a.samples_per_frame = int(S), B, plan.Wl, plan.C, plan.samples_per_frame
    a.state, a.state_bytes, a.slots = state.data_ptr(), state.numel() * state.element_size(), slots.data_ptr()
    a.windows, a.window_lens, a.first_frame = win.data_ptr(), wl.data_ptr(), first.data_ptr()
    with torch.cuda.device(dev):
        _check(lib.qasr_stream_window(_stream_ptr(stream), C.byref(a)), 'qasr_stream_window')
    return win, wl, first


def stream_emit_buffers(B, plan, device, P=None, tail=True):
    """k_stream_emit's outputs as a qasr.stream.StepBatch of cuda tensors"""
    from . import stream as qs
    P = plan.emit_pitch if P is None else int(P)
    i = lambda *s: torch.empty(*s, device=device, dtype=torch.int32)
    f = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)
    return qs.StepBatch(i(B, P), i(B, P), i(B, P), f(B, P), i(B), i(B), i(B), f(B),
                        i(B, plan.tail_pitch) if tail else None, i(B) if tail else None)


def stream_emit(state, S, plan, slots, flags, tokens, frame_score, enc_lens, first_frame, blank, out=None, stream=None):
    """qasr_stream_emit: one step's final frames folded into the slots' state; tokens int32 [B, Tw], frame_score float32
    [B, Tw], enc_lens / first_frame / slots / flags cuda int32 [B] -> a qasr.stream.StepBatch of cuda tensors.
    k_stream_emit, one launch, nothing read back; equal to qasr.stream.emit_batch_host byte for byte, the state included."""
    lib = load_library()
    dev = state.device
    if tokens.dim() != 2 or tokens.dtype != torch.int32 or not tokens.is_contiguous() or not tokens.is_cuda:
        raise ValueError(f'stream_emit: tokens must be a contiguous cuda int32 tensor [B, Tw], got {tokens.dtype} {tuple(tokens.shape)}')
    B, Tw = tokens.shape
    if frame_score.dtype != torch.float32 or not frame_score.is_contiguous() or frame_score.shape != tokens.shape:
        raise ValueError('stream_emit: frame_score must be a contiguous float32 tensor of the shape of tokens')
    for t, w in ((slots, 'slots'), (flags, 'flags'), (enc_lens, 'enc_lens'), (first_frame, 'first_frame')):
        _i32dev(t, B, 'stream_emit: ' + w)
    if out is None:
        out = stream_emit_buffers(B, plan, dev)
    P = out.labels.shape[1]
    for t in (out.labels, out.start, out.nframes):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (B, P), 'stream_emit: out'
    assert out.score.dtype == torch.float32 and out.score.is_contiguous() and tuple(out.score.shape) == (B, P), 'stream_emit: out'
    for t in (out.n_new_labels, out.status, out.total_frames):
        _i32dev(t, B, 'stream_emit: out')
    assert out.utt_score.dtype == torch.float32 and out.utt_score.numel() == B and out.utt_score.is_contiguous(), 'stream_emit: out'
    a = StreamEmitArgs()
    a.struct_size = C.sizeof(StreamEmitArgs)
    a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame = int(S), B, plan.Wl, plan.C, plan.Rr, plan.samples_per_frame
    a.Tw, a.P, a.blank = Tw, P, int(blank)
    a.state, a.state_bytes = state.data_ptr(), state.numel() * state.element_size()
    a.slots, a.flags, a.tokens, a.frame_score = slots.data_ptr(), flags.data_ptr(), tokens.data_ptr(), frame_score.data_ptr()
    a.enc_lens, a.first_frame = enc_lens.data_ptr(), first_frame.data_ptr()
    for n in ('labels', 'start', 'nframes', 'score', 'n_new_labels', 'status', 'total_frames', 'utt_score'):
        setattr(a, n, getattr(out, n).data_ptr())
    if out.tail_labels is not None:
        assert out.tail_labels.dtype == torch.int32 and out.tail_labels.is_contiguous() and out.tail_labels.shape[0] == B, 'stream_emit: out'
        _i32dev(out.tail_n, B, 'stream_emit: out')
        a.Ptail, a.tail_labels, a.tail_n = out.tail_labels.shape[1], out.tail_labels.data_ptr(), out.tail_n.data_ptr()
    with torch.cuda.device(dev):
        _check(lib.qasr_stream_emit(_stream_ptr(stream), C.byref(a)), 'qasr_stream_emit')
    return out


class StreamBeamArgs(C.Structure):
    """qasr_stream_beam_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('S', 'B', 'Wl', 'C', 'Rr', 'samples_per_frame', 'Tw', 'N', 'beam_width', 'n_best', 'blank',
                                          'Lg', 'K', 'F', 'max_final_frames', 'P', 'Ptail', 'Pend')] +
                [('lae_entries', C.c_uint32), ('state', C.c_void_p), ('state_bytes', C.c_size_t), ('beam_state', C.c_void_p),
                 ('beam_state_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('slots', 'flags', 'cand_id', 'cand_q', 'enc_lens', 'first_frame', 'lae_table', 'labels',
                                           'frames', 'n_new_labels', 'commit_len', 'n_live', 'status', 'tail_labels', 'tail_n',
                                           'end_labels', 'end_n_labels', 'end_score', 'n_hyps', 'lm')] +
                [('lm_bytes', C.c_size_t)] + [(n, C.c_int32) for n in ('alpha_q', 'beta_q', 'space', 'reserved')] +
                [('end_lm_score', C.c_void_p)])


def stream_beam_state(S, bplan, device):
    """Zeroed beam state of S fresh streams under a qasr.stream_beam.StreamBeamPlan: an int32 tensor of
    qasr_stream_beam_state_bytes(S, W, F) / 4 words.  `stream_beam_block(state, S, bplan)` views it as [S, slot_words]."""
    n = int(load_library().qasr_stream_beam_state_bytes(int(S), bplan.W, bplan.F))
    if n == 0:
        raise ValueError(f'stream_beam_state: S {S}, width {bplan.W}, F {bplan.F} out of range')
    return torch.zeros(n // 4, device=device, dtype=torch.int32)


def stream_beam_block(bstate, S, bplan):
    """the S slots of a beam state as [S, slot_words] (header, entries, ring), as qasr.stream_beam.StreamBeamState.block"""
    return bstate[:int(S) * bplan.slot_words].view(int(S), bplan.slot_words)


def _stream_beam_pitches(bplan, P, Ptail, Pend):
    """the row pitches of a step's outputs: the plan's own unless given"""
    return (bplan.delta_pitch if P is None else int(P), bplan.tail_pitch if Ptail is None else int(Ptail),
            bplan.end_pitch if Pend is None else int(Pend))


def stream_beam_buffers(B, bplan, device, with_lm, P=None, Ptail=None, Pend=None):
    """k_stream_beam's outputs as a qasr.stream_beam.BeamStepBatch of cuda tensors"""
    from . import stream_beam as sb
    P, Ptail, Pend = _stream_beam_pitches(bplan, P, Ptail, Pend)
    i = lambda *s: torch.empty(*s, device=device, dtype=torch.int32)
    l = lambda *s: torch.empty(*s, device=device, dtype=torch.int64)
    nb = bplan.n_best
    return sb.BeamStepBatch(i(B, P), i(B, P), i(B), i(B), i(B), i(B), i(B, Ptail), i(B), i(B, nb, Pend), i(B, nb), l(B, nb),
                            l(B, nb) if with_lm else None, i(B))


def _stream_beam_rows(who, cand_id, cand_q, rows):
    """(B, Tw, N) of a step's candidates; they and `rows`, the step's int32 [B] tensors as (tensor, name), are checked under
    the call's name"""
    if cand_id.dim() != 3 or cand_id.dtype != torch.int32 or not cand_id.is_contiguous() or not cand_id.is_cuda:
        raise ValueError(f'{who}: cand_id must be a contiguous cuda int32 tensor [B, Tw, N], got {cand_id.dtype} {tuple(cand_id.shape)}')
    if cand_q.dtype != torch.int32 or not cand_q.is_contiguous() or cand_q.shape != cand_id.shape:
        raise ValueError(f'{who}: cand_q must be a contiguous int32 tensor of the shape of cand_id')
    for t, w in rows:
        _i32dev(t, cand_id.shape[0], f'{who}: {w}')
    return cand_id.shape


def _stream_beam_fill(a, who, state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, lm, alpha_q,
                      beta_q, out, outs, Pend):
    """Fills a qasr_stream_beam_args, stream_beam's own or the one embedded in stream_beam_ep's: the plans' numbers, the states,
    the step's inputs, the outputs `outs` of `out` (checked under the call's name) and the model.  Returns (the table, the
    model's blob): they must stay alive."""
    from .beam import TAB_ENTRIES
    B, Tw, N = cand_id.shape
    tab = lae_table_device(state.device)
    blob = None if lm is None else lm_device(lm, state.device)
    a.struct_size = C.sizeof(StreamBeamArgs)
    a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame, a.Tw = int(S), B, plan.Wl, plan.C, plan.Rr, plan.samples_per_frame, Tw
    a.N, a.beam_width, a.n_best, a.blank = N, bplan.W, bplan.n_best, int(blank)
    a.Lg, a.K, a.F, a.max_final_frames = bplan.Lg, bplan.K, bplan.F, bplan.max_final_frames
    a.P, a.Ptail, a.Pend = out.labels.shape[1], out.tail_labels.shape[1], Pend
    a.lae_entries = TAB_ENTRIES
    a.state, a.state_bytes = state.data_ptr(), state.numel() * state.element_size()
    a.beam_state, a.beam_state_bytes = bstate.data_ptr(), bstate.numel() * bstate.element_size()
    a.slots, a.flags, a.cand_id, a.cand_q = slots.data_ptr(), flags.data_ptr(), cand_id.data_ptr(), cand_q.data_ptr()
    a.enc_lens, a.first_frame, a.lae_table = enc_lens.data_ptr(), first_frame.data_ptr(), tab.data_ptr()
    for n in outs:
        t = getattr(out, n)
        assert t.is_cuda and t.is_contiguous() and t.dtype == (torch.int64 if n == 'end_score' else torch.int32), f'{who}: out.{n}'
        setattr(a, n, t.data_ptr())
    if lm is not None:
        a.lm, a.lm_bytes, a.alpha_q, a.beta_q, a.space = blob.data_ptr(), blob.numel(), alpha_q, beta_q, int(lm.space)
    return tab, blob


def _stream_beam_set_labels(who, sets, blank):
    for k, bs in enumerate(sets or []):
        if bs.n_labels != int(blank):
            raise ValueError(f'{who}: phrase set {k} was compiled for {bs.n_labels} labels, blank is {blank}')


def _stream_beam_sets(q, who, sets, blobs, boost_set, device, lm):
    """Fills the sets of a qasr_stream_beam_boost_args whose `beam` is filled (without a model the sets name the space label);
    returns the sets' blobs: boost_device's unless the caller holds them"""
    blobs = [boost_device(bs, device) for bs in sets] if blobs is None else list(blobs)
    assert len(blobs) == len(sets), f'{who}: one blob per set'
    q.struct_size, q.n_sets = C.sizeof(StreamBeamBoostArgs), len(sets)
    if lm is None:
        q.beam.space = int(sets[0].space)
    for k, (bs, blob) in enumerate(zip(sets, blobs)):
        q.sets[k], q.set_bytes[k], q.whole_words[k] = blob.data_ptr(), blob.numel(), int(bs.whole_words)
    q.boost_set = boost_set.data_ptr()
    return blobs


_STREAM_BEAM_STEP_OUTS = ('labels', 'frames', 'n_new_labels', 'commit_len', 'n_live', 'status', 'tail_labels', 'tail_n')


def stream_beam_args(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, lm=None,
                     alpha=0.0, beta=0.0, out=None):
    """the filled qasr_stream_beam_args of stream_beam (the tensors it points to are kept alive on it)"""
    B, _, _ = _stream_beam_rows('stream_beam', cand_id, cand_q,
                                ((slots, 'slots'), (flags, 'flags'), (enc_lens, 'enc_lens'), (first_frame, 'first_frame')))
    alpha_q, beta_q = _lm_weights('stream_beam', lm, alpha, beta, blank)
    if out is None:
        out = stream_beam_buffers(B, bplan, state.device, lm is not None)
    a = StreamBeamArgs()
    tab, blob = _stream_beam_fill(a, 'stream_beam', state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame,
                                  blank, lm, alpha_q, beta_q, out,
                                  _STREAM_BEAM_STEP_OUTS + ('end_labels', 'end_n_labels', 'end_score', 'n_hyps'), out.end_labels.shape[2])
    if lm is not None:
        a.end_lm_score = 0 if out.end_lm_score is None else out.end_lm_score.data_ptr()
    a._keep = (tab, blob, out)
    return a


def stream_beam(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, lm=None, alpha=0.0,
                beta=0.0, out=None, stream=None):
    """qasr_stream_beam: one step's final frames searched from the slots' beams; cand_id / cand_q cuda int32 [B, Tw, N]
    (ctc_topn over the windows' log-probabilities), enc_lens / first_frame / slots / flags cuda int32 [B]; state: the stream
    state (read-only: call this BEFORE stream_emit), bstate: stream_beam_state.  Returns a qasr.stream_beam.BeamStepBatch of
    cuda tensors.  k_stream_beam, one launch, nothing read back; equal to qasr.stream_beam.step_batch_host byte for byte,
    the beam state included.  The table and the model are uploaded by the first call: make that one outside a capture."""
    a = stream_beam_args(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, lm, alpha,
                         beta, out)
    with torch.cuda.device(state.device):
        _check(load_library().qasr_stream_beam(_stream_ptr(stream), C.byref(a)), 'qasr_stream_beam')
    return a._keep[2]


MAX_STREAM_SETS = 8                     # QASR_STREAM_BEAM_MAX_SETS


class StreamBeamBoostArgs(C.Structure):
    """qasr_stream_beam_boost_args (include/qasr.h)"""
    _fields_ = [('struct_size', C.c_uint32), ('n_sets', C.c_int32), ('beam', StreamBeamArgs),
                ('sets', C.c_void_p * MAX_STREAM_SETS), ('set_bytes', C.c_size_t * MAX_STREAM_SETS),
                ('whole_words', C.c_int32 * MAX_STREAM_SETS), ('boost_set', C.c_void_p), ('end_boost_score', C.c_void_p)]


def stream_beam_boost_state(S, bplan, device):
    """stream_beam_state for a boosted plan (StreamBeamPlan(boost=True)): qasr_stream_beam_boost_state_bytes(S, W, F) / 4
    zeroed words; `stream_beam_block` views it."""
    if not bplan.boost:
        raise ValueError('stream_beam_boost_state: the plan was built without boost')
    n = int(load_library().qasr_stream_beam_boost_state_bytes(int(S), bplan.W, bplan.F))
    if n == 0:
        raise ValueError(f'stream_beam_boost_state: S {S}, width {bplan.W}, F {bplan.F} out of range')
    return torch.zeros(n // 4, device=device, dtype=torch.int32)


def stream_beam_boost_buffers(B, bplan, device, with_lm, P=None, Ptail=None, Pend=None):
    """k_stream_beam_boost's outputs: stream_beam_buffers with end_boost_score"""
    out = stream_beam_buffers(B, bplan, device, with_lm, P, Ptail, Pend)
    out.end_boost_score = torch.empty(B, bplan.n_best, device=device, dtype=torch.int64)
    return out


def stream_beam_boost_args(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, sets,
                           boost_set, lm=None, alpha=0.0, beta=0.0, out=None, blobs=None):
    """the filled qasr_stream_beam_boost_args of stream_beam_boost.  sets: 1 .. 8 qasr.boost.PhraseSet of the model's
    vocabulary; each is packed, checked (qasr_boost_check) and uploaded by boost_device, once
    (blobs: what boost_device gave for each, for a caller that holds them itself)."""
    from . import stream_beam as sb
    sets = sb.as_sets(sets)
    if sets is None or not bplan.boost:
        raise ValueError('stream_beam_boost: needs phrase sets and a plan built with boost=True')
    _stream_beam_set_labels('stream_beam_boost', sets, blank)
    B = cand_id.shape[0] if cand_id.dim() == 3 else 0
    _i32dev(boost_set, B, 'stream_beam_boost: boost_set')
    if out is None:
        out = stream_beam_boost_buffers(B, bplan, state.device, lm is not None)
    t = out.end_boost_score
    assert t is not None and t.is_cuda and t.is_contiguous() and t.dtype == torch.int64, 'stream_beam_boost: out.end_boost_score'
    inner = stream_beam_args(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, lm, alpha,
                             beta, out)
    a = StreamBeamBoostArgs()
    C.memmove(C.byref(a.beam), C.byref(inner), C.sizeof(StreamBeamArgs))
    blobs = _stream_beam_sets(a, 'stream_beam_boost', sets, blobs, boost_set, state.device, lm)
    a.end_boost_score = t.data_ptr()
    a._keep = inner._keep + (blobs, boost_set)
    return a


def stream_beam_boost(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, sets,
                      boost_set, lm=None, alpha=0.0, beta=0.0, out=None, stream=None, blobs=None):
    """qasr_stream_beam_boost: stream_beam with phrase boosting across steps.  sets: the session's phrase sets, boost_set cuda
    int32 [B]: the set of each BEGIN row (-1: none); bstate: stream_beam_boost_state.  Returns a BeamStepBatch with
    end_boost_score.  k_stream_beam_boost, one launch, nothing read back; equal to qasr.stream_beam.step_batch_host(boost=)
    byte for byte, the beam state included.  The sets are uploaded by the first call: make that one outside a capture."""
    a = stream_beam_boost_args(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, sets,
                               boost_set, lm, alpha, beta, out, blobs)
    with torch.cuda.device(state.device):
        _check(load_library().qasr_stream_beam_boost(_stream_ptr(stream), C.byref(a)), 'qasr_stream_beam_boost')
    return a._keep[2]


class StreamBeamEpArgs(C.Structure):
    """qasr_stream_beam_ep_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32), ('E', C.c_int32), ('boost', StreamBeamBoostArgs)] +
                [(n, C.c_void_p) for n in ('records', 'n_records', 'ep_status', 'n_cuts', 'cut_n_hyps', 'cut_delta_end', 'cut_labels',
                                           'cut_n_labels', 'cut_score', 'cut_lm_score', 'cut_boost_score')])


def stream_beam_ep_buffers(B, bplan, E, device, with_lm, P=None, Ptail=None, Pend=None):
    """k_stream_beam_ep's outputs as a qasr.stream_beam.BeamEpStepBatch of cuda tensors (E: the records' row pitch,
    EndpointPlan.max_records)"""
    from . import stream_beam as sb
    P, Ptail, Pend = _stream_beam_pitches(bplan, P, Ptail, Pend)
    i = lambda *s: torch.empty(*s, device=device, dtype=torch.int32)
    l = lambda *s: torch.empty(*s, device=device, dtype=torch.int64)
    nb, E = bplan.n_best, int(E)
    return sb.BeamEpStepBatch(i(B, P), i(B, P), i(B), i(B), i(B), i(B), i(B, Ptail), i(B), i(B), i(B, E), i(B, E), i(B, E, nb, Pend),
                              i(B, E, nb), l(B, E, nb), l(B, E, nb) if with_lm else None, l(B, E, nb) if bplan.boost else None)


def stream_beam_ep_args(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, ep, sets=None,
                        boost_set=None, lm=None, alpha=0.0, beta=0.0, out=None, blobs=None):
    """the filled qasr_stream_beam_ep_args of stream_beam_ep (the tensors it points to are kept alive on it)"""
    from . import stream_beam as sb, stream_ep as qe
    who, dev = 'stream_beam_ep', state.device
    sets = sb.as_sets(sets)
    if (sets is not None) != bplan.boost:
        raise ValueError('stream_beam_ep: phrase sets go with a plan built with boost=True')
    _stream_beam_set_labels(who, sets, blank)
    B, _, _ = _stream_beam_rows(who, cand_id, cand_q,
                                ((slots, 'slots'), (flags, 'flags'), (enc_lens, 'enc_lens'), (first_frame, 'first_frame'),
                                 (ep.n_records, 'ep.n_records'), (ep.status, 'ep.status')) + (((boost_set, 'boost_set'),) if sets is not None else ()))
    E = ep.records.shape[1] if ep.records.dim() == 3 else 0
    assert ep.records.is_cuda and ep.records.dtype == torch.int32 and ep.records.is_contiguous() and \
        tuple(ep.records.shape) == (B, E, qe.REC_WORDS), 'stream_beam_ep: ep.records'
    alpha_q, beta_q = _lm_weights(who, lm, alpha, beta, blank)
    if out is None:
        out = stream_beam_ep_buffers(B, bplan, E, dev, lm is not None)
    assert out.cut_labels.dim() == 4 and tuple(out.cut_labels.shape[:3]) == (B, E, bplan.n_best), 'stream_beam_ep: out.cut_labels'
    x = StreamBeamEpArgs()
    x.struct_size, x.E = C.sizeof(StreamBeamEpArgs), E
    x.boost.struct_size = C.sizeof(StreamBeamBoostArgs)
    tab, blob = _stream_beam_fill(x.boost.beam, who, state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame,
                                  blank, lm, alpha_q, beta_q, out, _STREAM_BEAM_STEP_OUTS, out.cut_labels.shape[3])
    for n in ('n_cuts', 'cut_n_hyps', 'cut_delta_end', 'cut_labels', 'cut_n_labels', 'cut_score', 'cut_lm_score', 'cut_boost_score'):
        t = getattr(out, n)
        if t is None:
            assert (n == 'cut_lm_score' and lm is None) or (n == 'cut_boost_score' and sets is None), 'stream_beam_ep: out.' + n
            continue
        assert t.is_cuda and t.is_contiguous() and t.dtype == (torch.int64 if n.endswith('score') else torch.int32), 'stream_beam_ep: out.' + n
        setattr(x, n, t.data_ptr())
    x.records, x.n_records, x.ep_status = ep.records.data_ptr(), ep.n_records.data_ptr(), ep.status.data_ptr()
    if sets is not None:
        blobs = _stream_beam_sets(x.boost, who, sets, blobs, boost_set, dev, lm)
    x._keep = (tab, blob, out, blobs, boost_set, ep)
    return x


def stream_beam_ep(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, ep, sets=None,
                   boost_set=None, lm=None, alpha=0.0, beta=0.0, out=None, stream=None, blobs=None):
    """qasr_stream_beam_ep: one step of a beam session that is cut into utterances, AFTER stream_emit and stream_endpoint of the
    same rows gave `ep` (a qasr.stream_ep.EpStepBatch of cuda tensors).  The arguments of stream_beam / stream_beam_boost
    (sets=None: bstate is stream_beam_state's, else stream_beam_boost_state's and boost_set cuda int32 [B]).  Returns a
    qasr.stream_beam.BeamEpStepBatch of cuda tensors.  k_stream_beam_ep, one launch, nothing read back; equal to
    qasr.stream_beam.step_batch_ep_host byte for byte, the beam state included.  The table, the model and the sets are
    uploaded by the first call: make that one outside a capture."""
    x = stream_beam_ep_args(state, bstate, S, plan, bplan, slots, flags, cand_id, cand_q, enc_lens, first_frame, blank, ep, sets,
                            boost_set, lm, alpha, beta, out, blobs)
    with torch.cuda.device(state.device):
        _check(load_library().qasr_stream_beam_ep(_stream_ptr(stream), C.byref(x)), 'qasr_stream_beam_ep')
    return x._keep[2]


class StreamEndpointArgs(C.Structure):
    """qasr_stream_endpoint_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('S', 'B', 'Wl', 'C', 'Rr', 'samples_per_frame', 'Tw', 'P', 'E', 'blank', 'Fsil', 'Fstart',
                                          'Fmax', 'Fhard')] +
                [('min_logp', C.c_float), ('state', C.c_void_p), ('state_bytes', C.c_size_t), ('ep_state', C.c_void_p),
                 ('ep_state_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('slots', 'flags', 'tokens', 'frame_score', 'enc_lens', 'first_frame', 'emit_start',
                                           'emit_nframes', 'emit_n_new_labels', 'emit_status', 'records', 'n_records', 'status')])


def stream_ep_state(S, device):
    """Zeroed endpoint state of S fresh streams: an int32 tensor of qasr_stream_ep_state_bytes(S) / 4 words, [S, 80] as
    qasr.stream_ep.EpState.block."""
    from . import stream_ep as qe
    n = int(load_library().qasr_stream_ep_state_bytes(int(S)))
    if n == 0:
        raise ValueError(f'stream_ep_state: S {S} out of range')
    return torch.zeros(n // 4, device=device, dtype=torch.int32).view(int(S), qe.STATE_WORDS)


def stream_endpoint_buffers(B, eplan, device, E=None):
    """k_stream_endpoint's outputs as a qasr.stream_ep.EpStepBatch of cuda tensors"""
    from . import stream_ep as qe
    E = eplan.max_records if E is None else int(E)
    i = lambda *s: torch.empty(*s, device=device, dtype=torch.int32)
    return qe.EpStepBatch(i(B, E, qe.REC_WORDS), i(B), i(B))


def stream_endpoint(state, ep_state, S, plan, eplan, slots, flags, tokens, frame_score, enc_lens, first_frame, emit, blank, out=None,
                    stream=None):
    """qasr_stream_endpoint: the endpoint rule over one step's final frames, AFTER stream_emit of the same rows gave `emit`
    (its StepBatch of cuda tensors); tokens int32 [B, Tw], frame_score float32 [B, Tw], enc_lens / first_frame / slots /
    flags cuda int32 [B]; state: the stream state (read-only), ep_state: stream_ep_state -> a qasr.stream_ep.EpStepBatch of
    cuda tensors.  k_stream_endpoint, one launch, nothing read back; equal to qasr.stream_ep.endpoint_batch_host byte for
    byte, the endpoint state included."""
    from . import stream_ep as qe
    lib = load_library()
    dev = state.device
    if tokens.dim() != 2 or tokens.dtype != torch.int32 or not tokens.is_contiguous() or not tokens.is_cuda:
        raise ValueError(f'stream_endpoint: tokens must be a contiguous cuda int32 tensor [B, Tw], got {tokens.dtype} {tuple(tokens.shape)}')
    B, Tw = tokens.shape
    if frame_score.dtype != torch.float32 or not frame_score.is_contiguous() or frame_score.shape != tokens.shape:
        raise ValueError('stream_endpoint: frame_score must be a contiguous float32 tensor of the shape of tokens')
    for t, w in ((slots, 'slots'), (flags, 'flags'), (enc_lens, 'enc_lens'), (first_frame, 'first_frame'),
                 (emit.n_new_labels, 'emit.n_new_labels'), (emit.status, 'emit.status')):
        _i32dev(t, B, 'stream_endpoint: ' + w)
    P = emit.start.shape[1]
    for t in (emit.start, emit.nframes):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (B, P), 'stream_endpoint: emit'
    assert ep_state.is_cuda and ep_state.dtype == torch.int32 and ep_state.is_contiguous(), 'stream_endpoint: ep_state'
    if out is None:
        out = stream_endpoint_buffers(B, eplan, dev)
    E = out.records.shape[1]
    assert out.records.is_cuda and out.records.dtype == torch.int32 and out.records.is_contiguous() and \
        tuple(out.records.shape) == (B, E, qe.REC_WORDS), 'stream_endpoint: out'
    _i32dev(out.n_records, B, 'stream_endpoint: out')
    _i32dev(out.status, B, 'stream_endpoint: out')
    a = StreamEndpointArgs()
    a.struct_size = C.sizeof(StreamEndpointArgs)
    a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame = int(S), B, plan.Wl, plan.C, plan.Rr, plan.samples_per_frame
    a.Tw, a.P, a.E, a.blank = Tw, P, E, int(blank)
    a.Fsil, a.Fstart, a.Fmax, a.Fhard, a.min_logp = eplan.Fsil, eplan.Fstart, eplan.Fmax, eplan.Fhard, float(eplan.min_logp)
    a.state, a.state_bytes = state.data_ptr(), state.numel() * state.element_size()
    a.ep_state, a.ep_state_bytes = ep_state.data_ptr(), ep_state.numel() * ep_state.element_size()
    a.slots, a.flags, a.tokens, a.frame_score = slots.data_ptr(), flags.data_ptr(), tokens.data_ptr(), frame_score.data_ptr()
    a.enc_lens, a.first_frame = enc_lens.data_ptr(), first_frame.data_ptr()
    a.emit_start, a.emit_nframes = emit.start.data_ptr(), emit.nframes.data_ptr()
    a.emit_n_new_labels, a.emit_status = emit.n_new_labels.data_ptr(), emit.status.data_ptr()
    a.records, a.n_records, a.status = out.records.data_ptr(), out.n_records.data_ptr(), out.status.data_ptr()
    with torch.cuda.device(dev):
        _check(lib.qasr_stream_endpoint(_stream_ptr(stream), C.byref(a)), 'qasr_stream_endpoint')
    return out


class StreamSpotArgs(C.Structure):
    """qasr_stream_spot_args (include/qasr.h)"""
    _fields_ = ([('struct_size', C.c_uint32)] +
                [(n, C.c_int32) for n in ('S', 'B', 'Wl', 'C', 'Rr', 'samples_per_frame', 'Tw', 'n_classes', 'K', 'max_labels', 'blank',
                                          'threshold_q', 'max_span', 'PH', 'max_final_frames')] +
                [('pitch_utt', C.c_int64), ('pitch_frame', C.c_int64), ('log_probs', C.c_void_p), ('star_logp', C.c_void_p),
                 ('star_pitch', C.c_int64), ('state', C.c_void_p), ('state_bytes', C.c_size_t), ('spot_state', C.c_void_p),
                 ('spot_state_bytes', C.c_size_t)] +
                [(n, C.c_void_p) for n in ('slots', 'flags', 'enc_lens', 'first_frame', 'emit_status', 'targets', 'target_lens',
                                           'hit_start', 'hit_end', 'hit_detect', 'hit_score', 'n_new_hits', 'n_hits_total',
                                           'open_start', 'open_end', 'open_score', 'ok', 'status')])


def stream_spot_state(S, splan, device):
    """Zeroed spot state of S fresh streams: an int32 tensor [S, K, 8 + 3 SP] as qasr.stream_spot.SpotState.block, of
    qasr_stream_spot_state_bytes(S, K, max_labels) bytes."""
    n = int(load_library().qasr_stream_spot_state_bytes(int(S), splan.K, splan.ML))
    if n == 0 or n != int(S) * splan.K * splan.block_words * 4:
        raise ValueError(f'stream_spot_state: S {S}, K {splan.K} or max_labels {splan.ML} out of range')
    return torch.zeros(n // 4, device=device, dtype=torch.int32).view(int(S), splan.K, splan.block_words)


def stream_spot_keywords(splan, device):
    """the keyword arrays of a session on the device, uploaded once: (targets int32 [K, ML], target_lens int32 [K])"""
    return (torch.from_numpy(splan.targets).to(device).contiguous(), torch.from_numpy(splan.target_lens).to(device).contiguous())


def stream_spot_buffers(B, splan, device, PH=None):
    """k_stream_spot's outputs as a qasr.stream_spot.SpotStepBatch of cuda tensors"""
    from . import stream_spot as qs
    PH = splan.hit_pitch if PH is None else int(PH)
    P = int(B) * splan.K
    t = lambda dt, *s: torch.empty(*s, device=device, dtype=dt)
    i32, i64 = torch.int32, torch.int64
    return qs.SpotStepBatch(t(i32, P, PH), t(i32, P, PH), t(i32, P, PH), t(i64, P, PH), t(i32, P), t(i32, P), t(i32, P), t(i32, P),
                            t(i64, P), t(i32, P), t(i32, P))


def stream_spot(state, spot_state, S, plan, splan, slots, flags, log_probs, star, enc_lens, first_frame, emit_status, blank,
                keywords=None, out=None, stream=None):
    """qasr_stream_spot: streaming keyword spotting over one step's final frames, AFTER stream_emit of the same rows gave
    emit_status; log_probs: a cuda float32 tensor [B, Tw, C] (any row / frame pitch, classes contiguous), star: the cuda float32
    plane [B, Tw] of ctc_star(log_probs, enc_lens, 0.0); enc_lens / first_frame / slots / flags / emit_status cuda int32 [B];
    state: the stream state (read-only), spot_state: stream_spot_state; keywords: stream_spot_keywords (uploaded here when
    None) -> a qasr.stream_spot.SpotStepBatch of cuda tensors.  k_stream_spot, one launch, nothing read back; equal to
    qasr.stream_spot.spot_batch_host byte for byte, the spot state included."""
    from . import stream_spot as qs
    who, dev = 'stream_spot', state.device
    a, lp, _, (B, Tw, Cn) = _lattice_logp(who, StreamSpotArgs, log_probs, None, '[B, Tw, C]')
    for t, w in ((slots, 'slots'), (flags, 'flags'), (enc_lens, 'enc_lens'), (first_frame, 'first_frame'), (emit_status, 'emit_status')):
        _i32dev(t, B, 'stream_spot: ' + w)
    assert spot_state.is_cuda and spot_state.dtype == torch.int32 and spot_state.is_contiguous(), 'stream_spot: spot_state'
    tg, tl = stream_spot_keywords(splan, dev) if keywords is None else keywords
    assert tg.is_cuda and tg.dtype == torch.int32 and tg.is_contiguous() and tuple(tg.shape) == (splan.K, splan.ML), 'stream_spot: targets'
    _i32dev(tl, splan.K, 'stream_spot: target_lens')
    if out is None:
        out = stream_spot_buffers(B, splan, dev)
    P, PH = B * splan.K, out.hit_start.shape[1]
    _set_outputs(who, a, out, [(n, torch.int64 if n in qs.FIELD_DTYPES else torch.int32, (P, PH) if n.startswith('hit_') else (P,), False)
                               for n in qs.FIELDS])
    st = _set_star(who, a, star, B, Tw, dev)
    a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame, a.Tw = int(S), B, plan.Wl, plan.C, plan.Rr, plan.samples_per_frame, Tw
    a.n_classes, a.K, a.max_labels, a.blank = Cn, splan.K, splan.ML, int(blank)
    a.threshold_q, a.max_span, a.PH, a.max_final_frames = splan.threshold_q, splan.max_span, PH, splan.max_final_frames
    a.state, a.state_bytes = state.data_ptr(), state.numel() * state.element_size()
    a.spot_state, a.spot_state_bytes = spot_state.data_ptr(), spot_state.numel() * spot_state.element_size()
    a.slots, a.flags, a.enc_lens, a.first_frame = slots.data_ptr(), flags.data_ptr(), enc_lens.data_ptr(), first_frame.data_ptr()
    a.emit_status, a.targets, a.target_lens = emit_status.data_ptr(), tg.data_ptr(), tl.data_ptr()
    return _lattice_launch('qasr_stream_spot', a, dev, stream, out, (lp, st, tg, tl))


class Engine:
    """One packed model on one GPU (qasr_engine_*)."""

    def __init__(self, blob: bytes, device=0, debug=False, timing=False, wide_tiles=False,
                 graph=False, tile=None, sep_gen=None, fuse_dw=None, fuse_stem=None, fuse_decoder=None, res_tile128=None,
                 dense_tile128=None, fuse_norm=None, legacy_create=False, mask_skip=None, pair_split=None):
        """Options = qasr_engine_opts (include/qasr.h).  tile: frames per work-group (32 / 64 / 128; `wide_tiles=True` is the
        older spelling of 128); None leaves a choice at the engine's default."""
        lib = load_library()
        if not torch.cuda.is_available():
            raise QasrError('no GPU: the integer engine needs an MI355X (there is no CPU fallback)')
        self.lib = lib
        self.device = torch.device('cuda', device)
        self._blob = blob
        self._h = C.c_void_p()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        o = EngineOpts()
        lib.qasr_engine_default_opts(C.byref(o))
        assert o.struct_size == C.sizeof(EngineOpts), 'qasr_engine_opts: header and binding disagree'
        o.debug = int(bool(debug)) | (2 if timing else 0)
        o.tile_frames = int(tile) if tile else (128 if wide_tiles else 32)
        o.sep_gen = int(sep_gen or 0)
        for name, v in (('fuse_dw', fuse_dw), ('fuse_stem', fuse_stem), ('fuse_decoder', fuse_decoder),
                        ('res_tile128', res_tile128), ('dense_tile128', dense_tile128), ('fuse_norm', fuse_norm),
                        ('mask_skip', mask_skip), ('pair_split', pair_split)):
            if v is not None:
                setattr(o, name, int(bool(v)))
        o.graph = int(bool(graph))
        self.opts = o
        if legacy_create:       # rounds 1 / 2 entry point: the option bits of its `debug` argument (include/qasr.h), nothing else
            bits = o.debug | (8 if o.tile_frames == 128 else 0) | (16 if graph else 0)
            _check(lib.qasr_engine_create(C.cast(buf, C.c_void_p), len(blob), device, bits, C.byref(self._h)), 'qasr_engine_create')
        else:
            _check(lib.qasr_engine_create_ex(C.cast(buf, C.c_void_p), len(blob), device, C.byref(o), C.byref(self._h)),
                   'qasr_engine_create_ex')
        self.debug = debug
        self.n_ops = lib.qasr_engine_num_ops(self._h)
        hdr = np.frombuffer(blob[:40], dtype=np.uint32)
        self.feat_in, self.n_classes = int(hdr[4]), int(hdr[5])
        self.B = self.T = None
        self._ctc = None                    # (frame_score, CtcResult, use_lens) attached to the engine
        self._ctc_auto = False              # ... by a decode= call (dropped again by the next call without decode=)
        self._ctc_cache = {}                # decode=True: persistent buffers of the current (B, T')
        self.reserved = None                # ReserveOpts after reserve()

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            self.lib.qasr_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_frames(self, T):
        return self.lib.qasr_engine_out_frames(self._h, int(T))

    def num_launches(self):
        """kernel launches of one forward of the current plan (after a forward)"""
        return self.lib.qasr_engine_num_launches(self._h)

    # ---- greedy CTC decoding behind the decoder (qasr_engine_attach_ctc)
    def attach_ctc(self, frame_score=None, out=None, use_lens=True):
        """Sticky: every later forward / forward_audio also writes `frame_score` (f32 [B, T'] cuda: the log-probability of
        each frame's arg-max class, from the decoder kernel itself) and, with `out` (a qasr.ctc.CtcResult of cuda tensors,
        e.g. ctc_buffers), collapses its tokens with k_ctc inside the same stream / captured graph.  The buffers are the
        caller's: keep them (and their pointers) for as long as they are attached."""
        if frame_score is None and out is None:
            return self.detach_ctc()
        if frame_score is not None:
            assert frame_score.is_cuda and frame_score.dtype == torch.float32 and frame_score.is_contiguous()
        o = _ctc_out_struct(out) if out is not None else None
        _check(self.lib.qasr_engine_attach_ctc(self._h, _ptr(frame_score), C.byref(o) if o is not None else None,
                                               int(bool(use_lens))), 'qasr_engine_attach_ctc')
        self._ctc = (frame_score, out, bool(use_lens))
        self._ctc_auto = False

    def detach_ctc(self):
        _check(self.lib.qasr_engine_attach_ctc(self._h, None, None, 0), 'qasr_engine_attach_ctc')
        self._ctc = None
        self._ctc_auto = False

    def _decode_begin(self, decode, B, To, device):
        """decode=None: nothing (an attachment a decode= call made is dropped); True: the engine's persistent buffers for
        this shape; a CtcResult: caller-owned buffers (its frame_score, if any, is attached too).  Returns the result."""
        if decode is None or decode is False:
            if self._ctc_auto:
                self.detach_ctc()
            return None
        if decode is True:
            res = self._ctc_cache.get((B, To))
            if res is None:                                  # one buffer set, for the current shape (like the engine's plan)
                res = ctc_buffers(B, To, device, scores=True, blank=self.n_classes - 1)
                self._ctc_cache = {(B, To): res}
        else:
            res = decode
        if self._ctc is None or self._ctc[1] is not res or self._ctc[0] is not res.frame_score or not self._ctc[2]:
            self.attach_ctc(res.frame_score, res, use_lens=True)
            self._ctc_auto = True
        return res

    def forward(self, feats: torch.Tensor, lens: torch.Tensor, want_logp=True, stream=None, out=None, decode=None):
        """feats f32 [B, feat_in, T] (cuda, contiguous), lens [B] -> (log_probs [B,T',C], tokens [B,T'], enc_len [B]).
        decode=True (or a qasr.ctc.CtcResult of caller-owned, pointer-stable cuda buffers): the greedy CTC collapse runs in
        the same call, stopping at the encoded lengths, and the result is returned as a fourth element."""
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 3 and feats.shape[1] == self.feat_in
        feats = feats.contiguous()
        lens32 = lens.to(device=feats.device, dtype=torch.int32).contiguous()
        B, _, T = feats.shape
        To = self.out_frames(T)
        if out is not None:                                  # caller-owned (logp or None, tokens, enc_len): stable pointers
            logp, tokens, enc_len = out
        else:
            logp = torch.empty(B, To, self.n_classes, device=feats.device, dtype=torch.float32) if want_logp else None
            tokens = torch.empty(B, To, device=feats.device, dtype=torch.int32)
            enc_len = torch.empty(B, device=feats.device, dtype=torch.int32)
        res = self._decode_begin(decode, B, To, feats.device)
        _check(self.lib.qasr_engine_forward(self._h, _stream_ptr(stream), _ptr(feats), _ptr(lens32), B, T,
                                            _ptr(logp), _ptr(tokens), _ptr(enc_len)), 'qasr_engine_forward')
        self.B, self.T = B, T
        self._keep = (feats, lens32)        # keep inputs alive until the stream has consumed them
        return (logp, tokens, enc_len) if res is None else (logp, tokens, enc_len, res)

    def forward_audio(self, audio, audio_lens, fb, window, plan, preemph=0.97, pad_to=16, want_logp=True, stream=None,
                      feats=None, feat_lens=None, out=None, decode=None):
        """qasr_engine_forward_audio: audio f32 [B, S] (cuda) -> (log_probs, tokens, enc_len) with the mel front-end inside the
        engine's call (one hipGraph launch per batch once the buffer set has been seen twice).  `plan` = frontend_plan(fb);
        `feats` / `feat_lens` / `out` = caller-owned buffers (stable pointers keep the captured graph)."""
        assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2 and audio.is_contiguous()
        assert audio_lens.is_cuda and audio_lens.dtype == torch.int32 and fb.is_cuda and window.is_cuda
        B, S = audio.shape
        n_mels = fb.shape[0]
        T = self.lib.qasr_frontend_frames(S, pad_to)
        dev = audio.device
        if feats is None:
            feats = torch.empty(B, n_mels, T, device=dev, dtype=torch.float32)
        if feat_lens is None:
            feat_lens = torch.empty(B, device=dev, dtype=torch.int32)
        To = self.out_frames(T)
        if out is not None:
            logp, tokens, enc_len = out
        else:
            logp = torch.empty(B, To, self.n_classes, device=dev, dtype=torch.float32) if want_logp else None
            tokens = torch.empty(B, To, device=dev, dtype=torch.int32)
            enc_len = torch.empty(B, device=dev, dtype=torch.int32)
        res = self._decode_begin(decode, B, To, dev)            # (see forward: the collapse rides in the same call)
        _check(self.lib.qasr_engine_forward_audio(self._h, _stream_ptr(stream), _ptr(audio), _ptr(audio_lens), B, S, _ptr(fb),
                                                  _ptr(window), n_mels, C.c_float(preemph), pad_to, _ptr(plan), plan.numel(),
                                                  _ptr(feats), _ptr(feat_lens), _ptr(logp), _ptr(tokens), _ptr(enc_len)),
               'qasr_engine_forward_audio')
        self.B, self.T = B, T
        self._keep = (audio, audio_lens, feats, feat_lens, fb, window, plan)
        return (logp, tokens, enc_len) if res is None else (logp, tokens, enc_len, res)

    # ---- reserved engines: ragged batches without allocation, one captured graph per bucket (qasr_engine_reserve)
    def reserve(self, max_batch, max_samples=None, max_frames=None, want_logp=True, decode=False, n_mels=None, pad_to=16,
                max_graphs=None):
        """Allocates once for the envelope max_batch x (max_samples audio samples and / or max_frames feature frames): the
        arena, every workspace, staging for the input and the output buffers.  Afterwards forward_ragged /
        forward_ragged_audio take any shape inside it without allocating, and replay one captured graph per bucket
        (qasr/ragged.py has the bucket policy).  decode: False; True (collapse up to the encoded lengths, as
        forward(decode=True)); 'padded' (walk the padded row of the batch's own T', as the reference does).
        A reserved engine refuses forward / forward_audio."""
        o = ReserveOpts()
        o.struct_size = C.sizeof(ReserveOpts)
        o.max_batch = int(max_batch)
        o.max_samples = int(max_samples or 0)
        o.max_frames = int(max_frames or 0)
        o.n_mels = int(n_mels or 0)
        o.pad_to = int(pad_to)
        o.want_logp = int(bool(want_logp))
        o.decode = 2 if decode == 'padded' else int(bool(decode))
        o.max_graphs = int(max_graphs or 0)
        with torch.cuda.device(self.device):
            _check(self.lib.qasr_engine_reserve(self._h, C.byref(o)), 'qasr_engine_reserve')
        self.reserved = o
        return self

    def _ragged_result(self, ro, B, decode_mode):
        dev, To, P, Bm = self.device, ro.out_frames, ro.row_pitch, self.reserved.max_batch
        f32, i32 = torch.float32, torch.int32
        tokens = _view(ro.tokens, (Bm, P), i32, dev)[:B, :To]
        enc_len = _view(ro.lens_out, (Bm,), i32, dev)[:B]
        logp = _view(ro.logp, (Bm, P, ro.n_classes), f32, dev)
        logp = None if logp is None else logp[:B, :To]
        if not decode_mode:
            return logp, tokens, enc_len
        from .ctc import CtcResult
        c = ro.ctc
        res = CtcResult(labels=_view(c.labels, (Bm, P), i32, dev)[:B, :To], n_labels=_view(c.n_labels, (Bm,), i32, dev)[:B],
                        start=_view(c.start, (Bm, P), i32, dev)[:B, :To], nframes=_view(c.nframes, (Bm, P), i32, dev)[:B, :To],
                        score=_view(c.score, (Bm, P), f32, dev)[:B, :To], utt_score=_view(c.utt_score, (Bm,), f32, dev)[:B],
                        blank=self.n_classes - 1, frame_score=_view(ro.frame_score, (Bm, P), f32, dev)[:B, :To])
        return logp, tokens, enc_len, res

    def forward_ragged(self, feats, lens, stream=None):
        """qasr_engine_forward_ragged: feats f32 [B, feat_in, T] (cuda), lens [B] (each <= T), any B <= max_batch and T <=
        max_frames of reserve() -> (log_probs or None, tokens, enc_len[, CtcResult with decode]).  The results are VIEWS
        [:B, :T'] of the engine's own buffers - no copy - and are valid until the next call on this engine: clone what
        must outlive it.  Bit-identical to forward() of an unreserved engine at the exact shape."""
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 3 and feats.shape[1] == self.feat_in
        feats = feats.contiguous()
        lens32 = lens.to(device=feats.device, dtype=torch.int32).contiguous()
        B, _, T = feats.shape
        ro = RaggedOut()
        ro.struct_size = C.sizeof(RaggedOut)
        _check(self.lib.qasr_engine_forward_ragged(self._h, _stream_ptr(stream), _ptr(feats), _ptr(lens32), B, T, C.byref(ro)),
               'qasr_engine_forward_ragged')
        self._keep = (feats, lens32)
        self.last_ragged = ro
        return self._ragged_result(ro, B, getattr(self, 'reserved', None) is not None and self.reserved.decode)

    def forward_ragged_audio(self, audio, audio_lens, fb, window, plan, preemph=0.97, pad_to=16, stream=None):
        """qasr_engine_forward_ragged_audio: audio f32 [B, S] (cuda), audio_lens int32 [B]; any B <= max_batch, S <=
        max_samples of reserve().  Returns what forward_ragged returns, under the same rule: views of engine-owned buffers,
        valid until the next call on this engine."""
        assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2 and audio.is_contiguous()
        assert audio_lens.is_cuda and audio_lens.dtype == torch.int32 and fb.is_cuda and window.is_cuda
        B, S = audio.shape
        ro = RaggedOut()
        ro.struct_size = C.sizeof(RaggedOut)
        _check(self.lib.qasr_engine_forward_ragged_audio(self._h, _stream_ptr(stream), _ptr(audio), _ptr(audio_lens), B, S,
                                                         _ptr(fb), _ptr(window), fb.shape[0], C.c_float(preemph), pad_to,
                                                         _ptr(plan), plan.numel(), C.byref(ro)),
               'qasr_engine_forward_ragged_audio')
        self._keep = (audio, audio_lens, fb, window, plan)
        self.last_ragged = ro
        return self._ragged_result(ro, B, self.reserved.decode)

    def ragged_stats(self):
        """qasr_engine_ragged_stats as a dict: device allocations / frees of this engine since creation, graphs captured,
        graph replays, eager runs, and {bucket edge: calls}."""
        st = RaggedStats()
        st.struct_size = C.sizeof(RaggedStats)
        _check(self.lib.qasr_engine_ragged_stats(self._h, C.byref(st)), 'qasr_engine_ragged_stats')
        return {'device_allocs': int(st.device_allocs), 'device_frees': int(st.device_frees),
                'graphs_captured': int(st.graphs_captured), 'graph_replays': int(st.graph_replays),
                'eager_runs': int(st.eager_runs),
                'buckets': {int(st.bucket_frames[i]): int(st.bucket_calls[i]) for i in range(st.n_buckets)}}

    # ---- parity hooks (debug engines)
    def read_acc(self, op, pane, cout, T_out):
        Tp = (T_out + 63) // 64 * 64
        out = np.empty((self.B, cout, Tp), dtype=np.int32)
        _check(self.lib.qasr_engine_read_acc(self._h, op, pane, out.ctypes.data_as(C.c_void_p), out.size),
               'qasr_engine_read_acc')
        return out[:, :, :T_out]

    def read_tensor(self, tensor, channels, dtype=np.int8):
        T, Tp = C.c_int(), C.c_int()
        _check(self.lib.qasr_engine_read_tensor(self._h, tensor, None, 0, C.byref(T), C.byref(Tp)), 'read_tensor')
        out = np.empty((self.B, channels, Tp.value), dtype=dtype)
        _check(self.lib.qasr_engine_read_tensor(self._h, tensor, out.ctypes.data_as(C.c_void_p), out.nbytes,
                                                C.byref(T), C.byref(Tp)), 'qasr_engine_read_tensor')
        return out[:, :, :T.value]

    def time_ops(self, reps=20, stream=None):
        """Average duration per launch (ms) of every op, each replayed `reps` times between one HIP event pair."""
        ms = np.zeros(self.n_ops, dtype=np.float32)
        _check(self.lib.qasr_engine_time_ops(self._h, _stream_ptr(stream), reps, ms.ctypes.data_as(C.c_void_p),
                                             self.n_ops), 'qasr_engine_time_ops')
        return ms

    def op_labels(self):
        """kernel instantiation every op is routed to (names as rocprofv3 prints them)"""
        out = []
        buf = C.create_string_buffer(96)
        for op in range(self.n_ops):
            _check(self.lib.qasr_engine_op_label(self._h, op, buf, 96), 'qasr_engine_op_label')
            out.append(buf.value.decode())
        return out

    def op_paired(self):
        """per op: does it run in the paired form (qasr_engine_opts.pair_split; after a forward)"""
        return [self.lib.qasr_engine_op_paired(self._h, op) == 1 for op in range(self.n_ops)]

    def op_halved(self):
        """per op: does it run in the halved form, a 128-frame tile as two 64-frame work-groups (QASR_HALF_TILES; after a forward)"""
        return [self.lib.qasr_engine_op_halved(self._h, op) == 1 for op in range(self.n_ops)]

    def pair_timeouts(self):
        """the time-out word of paired launches (synchronises).  Always 0: the members of a pair exchange nothing any more"""
        n = self.lib.qasr_engine_pair_timeouts(self._h)
        if n < 0:
            raise QasrError('qasr_engine_pair_timeouts failed: ' + self.lib.qasr_last_error().decode())
        return n

    def pair_flag_words(self):
        """the flag words of the plan's paired ops as a numpy uint32 array (synchronises; empty without paired ops).  Read-only:
        behind a forward every word of a pair that ran holds 1, because each forward zeroes them first"""
        n = self.lib.qasr_engine_pair_flag_words(self._h, None, 0)
        if n < 0:
            raise QasrError('qasr_engine_pair_flag_words failed: ' + self.lib.qasr_last_error().decode())
        out = np.zeros(n, dtype=np.uint32)
        if n and self.lib.qasr_engine_pair_flag_words(self._h, out.ctypes.data_as(C.c_void_p), n) != n:
            raise QasrError('qasr_engine_pair_flag_words failed: ' + self.lib.qasr_last_error().decode())
        return out

    def run_op(self, op, stream=None):
        _check(self.lib.qasr_engine_run_op(self._h, _stream_ptr(stream), int(op)), 'qasr_engine_run_op')

    def last_op_ms(self):
        ms = np.zeros(self.n_ops, dtype=np.float32)
        _check(self.lib.qasr_engine_last_op_ms(self._h, ms.ctypes.data_as(C.c_void_p), self.n_ops), 'last_op_ms')
        return ms


# ---- stand-alone operators -------------------------------------------------------------------
def _rup(x, m):
    return (x + m - 1) // m * m


def pw_conv_acc(x: torch.Tensor, w: torch.Tensor, bias=None, x_unsigned=False):
    """int32 accumulator of a 1x1 conv.  x int8/uint8 [B,cin,T] cuda, w int8 [cout,cin] (host or cuda)."""
    lib = load_library()
    B, cin, T = x.shape
    cout = w.shape[0]
    Tp, cinp, coutp = _rup(T, 64), _rup(cin, 128), _rup(cout, 128)
    dev = x.device
    xp = torch.zeros(B, cin, Tp, dtype=torch.int8, device=dev)
    xp[:, :, :T] = x.view(torch.int8) if x.dtype == torch.uint8 else x
    from .pack import fragment_order
    wp = torch.zeros(coutp, cinp, dtype=torch.int8)
    wp[:cout, :cin] = w.cpu()
    wp = torch.from_numpy(fragment_order(wp.numpy())).to(dev)
    bp = torch.zeros(coutp, dtype=torch.int32, device=dev)
    if bias is not None:
        bp[:cout] = bias.to(dev)
    if x_unsigned:                          # kernels feed u8 as (x - 128): fold the correction like pack.py does
        bp[:cout] += 128 * w.to(dev).to(torch.int32).sum(1)
    acc = torch.zeros(B, cout, Tp, dtype=torch.int32, device=dev)
    _check(lib.qasr_pw_conv_acc(_stream_ptr(), _ptr(xp), int(x_unsigned), _ptr(wp), _ptr(bp), B, cin, cinp, cout, T,
                                Tp, _ptr(acc)), 'qasr_pw_conv_acc')
    return acc[:, :, :T]


def dw_conv_acc(x: torch.Tensor, w: torch.Tensor, stride=1, dilation=1, padding=0):
    """int32 accumulator of a depthwise conv.  x int8 [B,C,T] cuda (signed), w int8 [C,K]."""
    lib = load_library()
    B, Cc, T = x.shape
    K = w.shape[1]
    T_out = (T + 2 * padding - dilation * (K - 1) - 1) // stride + 1
    Tp, Tpo, kp = _rup(T, 64), _rup(T_out, 64), _rup(K, 4)
    dev = x.device
    xp = torch.zeros(B, Cc, Tp, dtype=torch.int8, device=dev)
    xp[:, :, :T] = x
    wp = torch.zeros(Cc, kp, dtype=torch.int8, device=dev)
    wp[:, :K] = w.to(dev)
    acc = torch.zeros(B, Cc, Tpo, dtype=torch.int32, device=dev)
    _check(lib.qasr_dw_conv_acc(_stream_ptr(), _ptr(xp), 0, _ptr(wp), None, B, Cc, K, kp, stride, dilation, padding, T, Tp,
                                T_out, Tpo, _ptr(acc)), 'qasr_dw_conv_acc')
    return acc[:, :, :T_out]


def requant(acc: torch.Tensor, M: torch.Tensor, lo, hi, sb=None, exact_z=False, relu=False):
    """clamp(rint(z*M[c]), lo, hi) for int32 acc [B,C,T] (T a multiple of 64 after padding)."""
    lib = load_library()
    B, Cc, T = acc.shape
    Tp = _rup(T, 64)
    a = torch.zeros(B, Cc, Tp, dtype=torch.int32, device=acc.device)
    a[:, :, :T] = acc
    out = torch.zeros(B, Cc, Tp, dtype=torch.int8, device=acc.device)
    Md = M.to(device=acc.device, dtype=torch.float64).contiguous()
    sbd = None if sb is None else sb.to(device=acc.device, dtype=torch.float32).contiguous()
    _check(lib.qasr_requant(_stream_ptr(), _ptr(a), _ptr(Md), _ptr(sbd), int(exact_z), int(relu), B, Cc, Tp, lo, hi,
                            _ptr(out)), 'qasr_requant')
    return out[:, :, :T]


def sep_layer(x, lens, wpw, bias, outs, wdw=None, m_dw=None, dw_range=(-128, 127), x_unsigned=False, dilation=1,
              flags=0, sb=None, res=None, tile=32, gen=2, hooks=True, out_fill=0, pair=False, pair_ws=None, sync=True, row_pad=64):
    """One fused separable layer through qasr_sep_layer (the production kernels with caller-made operands).

    x            int8 / uint8 [B, cin, T] (cuda)      lens  valid frames per utterance
    wdw          int8 [cin, K] depthwise taps (None: the layer is a bare 1x1 conv), m_dw f64 [cin], dw_range (lo, hi)
    wpw, bias    int8 [cout, cin], int32 [cout]       sb f32 [cout] conv output scales (QASR_F_EXACT_Z)
    outs         list of dicts(mode, lo, hi, M=f64 [cout] (mode 1) or m=float (mode 0))
    res          None or dict(x [B, rcin, T] (uint8 / int8), w int8 [cout, rcin], bias int32 [cout], m f64 [cout],
                 sb f32 [cout], m_main f64 [cout], qlo, qhi)   -> QASR_F_RESADD
    Biases are the natural ones: the +128 sum(W) correction of u8 inputs is folded here, as pack.py does.
    out_fill     byte the output buffers hold before the call (tests of what a kernel leaves unwritten)
    pair         the paired form (two work-groups per tile; QasrError for a shape without one, or with hooks); pair_ws: its
                 workspace from sep_pair_workspace (made here when None; one per launch in flight), returned as 'pair_ws'
    sync         False: return without synchronising (the launch is in flight on the current stream)
    row_pad      rows are padded to a multiple of this many frames (64; 128 keeps a 128-frame tile at any T)
    Returns dict(outs=[int8 [B, cout, T]...], outs_padded=[the same with the row padding, [B, cout, Tp]], dw_acc, acc, racc
    (int32, None without hooks), label)."""
    from .pack import F_RESADD, fragment_order
    lib = load_library()
    dev = x.device
    B, cin, T = x.shape
    cout = wpw.shape[0]
    Tp, cinp, coutp = _rup(T, int(row_pad)), _rup(cin, 128), _rup(cout, 128)
    keep = []

    def dv(t, dtype=None):
        t = torch.as_tensor(t)
        t = (t.to(dtype) if dtype is not None else t).to(dev).contiguous()
        keep.append(t)
        return t

    def padded_x(t):
        p = torch.zeros(t.shape[0], t.shape[1], Tp, dtype=torch.int8, device=dev)
        p[:, :, :T] = t.view(torch.int8) if t.dtype == torch.uint8 else t
        keep.append(p)
        return p

    def frag(w, rows, cols):
        wp = torch.zeros(rows, cols, dtype=torch.int8)
        wp[:w.shape[0], :w.shape[1]] = torch.as_tensor(w).cpu()
        return dv(torch.from_numpy(fragment_order(wp.numpy())))

    def padvec(v, n, dtype, fill=0):
        o = torch.full((n,), fill, dtype=dtype)
        o[:len(v)] = torch.as_tensor(v).to(dtype).cpu()
        return dv(o)

    a = SepLayerArgs()
    a.B, a.T, a.Tp, a.cin, a.cout, a.dilation, a.tile, a.gen = B, T, Tp, cin, cout, dilation, tile, gen
    a.flags = flags | (F_RESADD if res is not None else 0)
    a.x = padded_x(x).data_ptr()
    a.x_unsigned = int(x_unsigned)
    a.lens = dv(lens, torch.int32).data_ptr()
    if wdw is not None:
        wdw = torch.as_tensor(wdw).cpu().to(torch.int8)
        K = wdw.shape[1]
        kp = _rup(K, 4)
        w1 = torch.zeros(cin, kp, dtype=torch.int8)
        w1[:, :K] = wdw
        w2 = torch.zeros(cin, kp + 32, dtype=torch.int8)
        w2[:, 8:8 + K] = wdw
        a.K = K
        a.wdw, a.wdw2 = dv(w1).data_ptr(), dv(torch.cat([w2.view(-1), torch.zeros(64, dtype=torch.int8)])).data_ptr()
        bdw = 128 * wdw.to(torch.int32).sum(1) if x_unsigned else torch.zeros(cin, dtype=torch.int32)
        a.bias_dw = padvec(bdw, cinp, torch.int32).data_ptr()
        a.m_dw = padvec(m_dw, cinp, torch.float64).data_ptr()
        a.dw_lo, a.dw_hi = dw_range
        pw_bias = torch.as_tensor(bias).to(torch.int32).cpu()
    else:
        a.K = 0
        pw_bias = torch.as_tensor(bias).to(torch.int32).cpu()
        if x_unsigned:
            pw_bias = pw_bias + 128 * torch.as_tensor(wpw).cpu().to(torch.int32).sum(1)
    a.w = frag(wpw, coutp, cinp).data_ptr()
    a.bias = padvec(pw_bias, coutp, torch.int32).data_ptr()
    if sb is not None:
        a.sb = padvec(sb, coutp, torch.float32, 1.0).data_ptr()
    if res is not None:
        rcin = res['x'].shape[1]
        a.rx = padded_x(res['x']).data_ptr()
        a.r_unsigned = int(res['x'].dtype == torch.uint8)
        a.rcin = rcin
        a.rw = frag(res['w'], coutp, _rup(rcin, 128)).data_ptr()
        rb = torch.as_tensor(res['bias']).to(torch.int32).cpu()
        if a.r_unsigned:
            rb = rb + 128 * torch.as_tensor(res['w']).cpu().to(torch.int32).sum(1)
        a.rbias = padvec(rb, coutp, torch.int32).data_ptr()
        a.rm = padvec(res['m'], coutp, torch.float64).data_ptr()
        if res.get('sb') is not None:
            a.rsb = padvec(res['sb'], coutp, torch.float32, 1.0).data_ptr()
        a.m_main = padvec(res['m_main'], coutp, torch.float64).data_ptr()
        a.qlo, a.qhi = res['qlo'], res['qhi']
    a.n_outs = len(outs)
    out_t = []
    for j, o in enumerate(outs):
        t = torch.full((B, cout, Tp), int(out_fill), dtype=torch.int8, device=dev)
        out_t.append(t)
        a.outs[j].ptr = t.data_ptr()
        a.outs[j].mode, a.outs[j].lo, a.outs[j].hi = o['mode'], o['lo'], o['hi']
        if o['mode'] == 1:
            a.outs[j].mtab = padvec(o['M'], coutp, torch.float64).data_ptr()
        elif o['mode'] == 0:
            a.outs[j].m = float(o['m'])
    hk = {}
    if hooks:
        if wdw is not None:
            hk['dw_acc'] = torch.zeros(B, cin, Tp, dtype=torch.int32, device=dev)
            a.dw_acc = hk['dw_acc'].data_ptr()
        hk['acc'] = torch.zeros(B, cout, Tp, dtype=torch.int32, device=dev)
        a.acc = hk['acc'].data_ptr()
        if res is not None:
            hk['racc'] = torch.zeros(B, cout, Tp, dtype=torch.int32, device=dev)
            a.racc = hk['racc'].data_ptr()
    if pair:
        a.pair = 1
        if pair_ws is None and Tp % 128 == 0:
            pair_ws = sep_pair_workspace(B, Tp, dev)
        if pair_ws is not None:
            a.pair_ws, a.pair_ws_bytes = pair_ws.data_ptr(), pair_ws.numel()
    label = C.create_string_buffer(96)
    _check(lib.qasr_sep_layer(_stream_ptr(), C.byref(a), label, 96), 'qasr_sep_layer')
    if sync:
        torch.cuda.synchronize()
    return dict(outs=[t[:, :, :T] for t in out_t], outs_padded=out_t, label=label.value.decode(), pair_ws=pair_ws, keep=keep,
                **{k: (hk[k][:, :, :T] if k in hk else None) for k in ('dw_acc', 'acc', 'racc')})


def sep_pair_workspace(B, Tp, device):
    """zeroed workspace of a paired sep_layer launch of B utterances x Tp frames (Tp a multiple of 128)"""
    n = load_library().qasr_sep_pair_workspace_bytes(int(B), int(Tp))
    if n == 0:
        raise QasrError(f'sep_pair_workspace: no paired form at Tp = {Tp}')
    return torch.zeros(n, dtype=torch.uint8, device=device)


def sep_pair_timeouts(pair_ws, B, Tp):
    """the time-out word of the paired launches that used `pair_ws` (synchronises; no kernel writes it any more: 0)"""
    torch.cuda.synchronize()
    off = load_library().qasr_sep_pair_timeout_offset(int(B), int(Tp))
    return int(pair_ws[off:off + 4].view(torch.int32).item())


def frontend_plan(fb: torch.Tensor):
    """qasr_frontend_plan: the filterbank-only tables of the front-end (filter runs, packed weights, twiddles) as a
    workspace tensor for frontend_mel(..., plan=...).  Read-only afterwards; one plan serves any number of streams."""
    lib = load_library()
    assert fb.is_cuda and fb.dtype == torch.float32 and fb.is_contiguous() and fb.dim() == 2 and fb.shape[1] == 257
    ws = torch.empty(max(lib.qasr_frontend_workspace_bytes(0, 0, fb.shape[0]), 16), dtype=torch.uint8, device=fb.device)
    _check(lib.qasr_frontend_plan(_stream_ptr(), _ptr(fb), fb.shape[0], _ptr(ws), ws.numel()), 'qasr_frontend_plan')
    ws._qasr_fb = fb                                          # the table is only valid for this filterbank: keep it alive
    return ws


def frontend_mel(audio: torch.Tensor, lens: torch.Tensor, fb: torch.Tensor, window: torch.Tensor, preemph=0.97,
                 pad_to=16, out=None, plan=None):
    """qasr_frontend_mel: audio f32 [B,S] (cuda), lens [B] samples, fb [n_mels,257], window [320]
    -> (features f32 [B,n_mels,T_pad], feature lengths i32 [B]).
    out = caller-owned (features, lengths, workspace); plan = frontend_plan(fb) of the same filterbank: skips the
    per-call table build (qasr_frontend_mel_planned)."""
    lib = load_library()
    assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2
    B, S = audio.shape
    n_mels = fb.shape[0]
    dev = audio.device
    T_pad = lib.qasr_frontend_frames(S, pad_to)
    if out is not None:
        feats, flens, ws_out = out
    else:
        feats = torch.empty(B, n_mels, T_pad, device=dev, dtype=torch.float32)
        flens = torch.empty(B, device=dev, dtype=torch.int32)
        ws_out = None
    a = audio.contiguous()
    l32 = lens.to(device=dev, dtype=torch.int32).contiguous()
    fbd = fb.to(device=dev, dtype=torch.float32).contiguous()
    wd = window.to(device=dev, dtype=torch.float32).contiguous()
    if plan is not None:
        _check(lib.qasr_frontend_mel_planned(_stream_ptr(), _ptr(a), _ptr(l32), B, S, _ptr(fbd), _ptr(wd), n_mels,
                                             C.c_float(preemph), pad_to, _ptr(feats), _ptr(flens), _ptr(plan), plan.numel()),
               'qasr_frontend_mel_planned')
        return feats, flens
    ws_bytes = lib.qasr_frontend_workspace_bytes(B, S, n_mels)
    ws = ws_out if ws_out is not None else torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    _check(lib.qasr_frontend_mel(_stream_ptr(), _ptr(a), _ptr(l32), B, S, _ptr(fbd), _ptr(wd), n_mels,
                                 C.c_float(preemph), pad_to, _ptr(feats), _ptr(flens), _ptr(ws), ws.numel()),
           'qasr_frontend_mel')
    return feats, flens


def quantile2(x: torch.Tensor, q_lo: float, q_hi: float):
    """qasr_quantile2: (torch.quantile(x.flatten(), q_lo), torch.quantile(x.flatten(), q_hi)) of a float32 cuda tensor
    as one radix select on device; returns a 2-element float32 cuda tensor (no host synchronisation)."""
    lib = load_library()
    assert x.is_cuda and x.dtype == torch.float32
    flat = x.detach().contiguous().view(-1)
    out = torch.empty(2, device=x.device, dtype=torch.float32)
    ws = torch.empty(lib.qasr_quantile_workspace_bytes(), dtype=torch.uint8, device=x.device)
    _check(lib.qasr_quantile2(_stream_ptr(), _ptr(flat), flat.numel(), C.c_float(q_lo), C.c_float(q_hi), _ptr(out), _ptr(ws),
                              ws.numel()), 'qasr_quantile2')
    return out
