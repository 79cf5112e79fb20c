"""Banded CTC alignment on an MI355X: k_align_band (csrc/qasr_align_band.hip) against its NumPy statement
qasr.align.align_band_host, every byte of every output (band_base and frame_logp included), no tolerance; refused arguments
launch nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_band_cases as bc  # noqa: E402
from qasr import align  # noqa: E402

FILL32, FILL64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
FIELDS = ('start', 'nframes', 'score', 'path_score', 'frame_logp', 'band_base', 'ok')


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _filled_out(P, ML, T, drop=()):
    """caller-owned outputs pre-filled with 0x5a..., so that an unwritten tail shows; `drop`: the optional ones left out"""
    i32 = dict(dtype=torch.int32, device='cuda')
    out = align.BandResult(None, None, torch.full((P, ML), FILL32, **i32), torch.full((P, ML), FILL32, **i32),
                           torch.full((P, ML), FILL32, **i32).view(torch.float32),
                           torch.full((P,), FILL64, dtype=torch.int64, device='cuda'), None, torch.full((P,), FILL32, **i32),
                           bc.BLANK, 1, torch.full((P, T), FILL32, **i32).view(torch.float32),
                           torch.full((P, (T + 31) // 32), FILL32, **i32))
    for f in drop:
        setattr(out, f, None)
    return out


def _assert_equal(got, want, what, drop=()):
    for f in FIELDS:
        if f in drop:
            continue
        g, w = getattr(got, f).cpu().numpy(), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.int32), w.view(np.int32)
        assert np.array_equal(g, w), (what, f, np.argwhere(g != w)[:4].tolist())


def _cuda(*xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


@pytest.mark.parametrize('name', [d[0] for d in bc.DEVICE])
def test_k_align_band_equals_the_twin_every_byte(eng, name):
    """S = 1201 at 256 states (the circular row wraps four times), S = 2401 at 1024, S = 4601 at 4352 (17 states per thread)"""
    bw, lp, tg, tl = bc.device_case(name)
    T, ML = lp.shape[1], tg.shape[1]
    want = align.align_band_host(lp, None, tg, tl, bc.BLANK, band_states=bw)
    assert want.ok[0] == 1 and want.band_base[0].max() == 2 * ML + 1 - bw and (np.diff(want.band_base[0]) >= 0).all()
    lp_d, tg_d, tl_d = _cuda(lp, tg, tl)
    out = _filled_out(1, ML, T)
    eng.ctc_align_band(lp_d, None, tg_d, tl_d, bc.BLANK, band_states=bw, out=out)
    torch.cuda.synchronize()
    _assert_equal(out, want, name)
    wide = torch.full((1, T + 3, bc.C + 7), 7.0, device='cuda')               # both pitches differ from T * C and C
    wide[:, :T, :bc.C] = lp_d
    cut = np.array([T - 45], dtype=np.int32)                                  # and a length inside the row
    want = align.align_band_host(lp, cut, tg, tl, bc.BLANK, band_states=bw)
    out = _filled_out(1, ML, T)
    eng.ctc_align_band(wide[:, :T, :bc.C], _cuda(cut)[0], tg_d, tl_d, bc.BLANK, band_states=bw, out=out)
    torch.cuda.synchronize()
    _assert_equal(out, want, name + ' lens')
    assert (wide[:, T:, :] == 7.0).all() and (wide[:, :, bc.C:] == 7.0).all()


def _three():
    """three recordings of one pitch: a moving band with lens < T, lens = 0, and an empty target"""
    lp, lens, tg, tl = bc.moving_case('short_lens_L400')
    lp = np.concatenate([lp, lp, lp])
    tg = np.concatenate([tg, tg, tg])
    return lp, np.array([int(lens[0]), 0, lp.shape[1] - 1], dtype=np.int32), tg, np.array([400, 400, 0], dtype=np.int32)


def test_k_align_band_three_recordings_each_optional_output_absent_in_turn(eng):
    lp, lens, tg, tl = _three()
    P, T, ML = 3, lp.shape[1], tg.shape[1]
    want = align.align_band_host(lp, lens, tg, tl, bc.BLANK, band_states=256)
    assert want.ok.tolist() == [1, 0, 1] and want.band_base[0].max() > 0
    lp_d, lens_d, tg_d, tl_d = _cuda(lp, lens, tg, tl)
    ws = torch.empty(eng.ctc_align_band_workspace_bytes(P, T, 256), dtype=torch.uint8, device='cuda')
    for drop in [()] + [(f,) for f in FIELDS[:-1]] + [FIELDS[:-1]]:
        out = _filled_out(P, ML, T, drop)
        eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, bc.BLANK, band_states=256, workspace=ws, out=out)
        torch.cuda.synchronize()
        _assert_equal(out, want, drop, drop)
    got = eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, bc.BLANK, band_states=256)       # buffers of its own
    torch.cuda.synchronize()
    _assert_equal(got, want, 'own buffers')
    got = eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, bc.BLANK, band_states=256, want_band_base=False)
    assert got.band_base is None and got.band_states == 256
    # the band that holds every state: k_align's own outputs, at every width
    full = align.align_host(lp[:, :300], lens.clip(0, 300), tg[:, :100], np.array([100, 100, 0]), bc.BLANK, want_total=False)
    for bw in (None,) + align.BAND_STATES:                                    # 201 states fit all; None picks 256
        got = eng.ctc_align_band(lp_d[:, :300], _cuda(lens.clip(0, 300))[0], tg_d[:, :100], _cuda(np.array([100, 100, 0]))[0],
                                 bc.BLANK, band_states=bw)
        torch.cuda.synchronize()
        for f in ('start', 'nframes', 'score', 'path_score', 'ok'):
            g, w = getattr(got, f).cpu().numpy(), getattr(full, f)
            assert np.array_equal(g.view(np.int32) if f == 'score' else g, w.view(np.int32) if f == 'score' else w), (bw, f)
        assert not got.band_base.any()


def test_k_align_band_rows_that_are_not_alignable_leave_the_others_alone(eng):
    lp1, lens, tg1, _ = bc.moving_case('short_lens_L400')
    lp1 = lp1[0]
    T = lp1.shape[0]
    cut = np.concatenate([lp1[:200], lp1[1200:]])                             # 1000 frames of audio deleted: the band loses
    cut = np.concatenate([cut, np.repeat(cut[-1:], T - len(cut), axis=0)])    # the path (test_align_band_cpu.py)
    lp = np.stack([lp1, lp1, lp1, cut, lp1, lp1, lp1, lp1])
    tg = np.stack([tg1[0]] * 8)
    tl = np.array([400] * 8, dtype=np.int32)
    tg[1, 7] = bc.BLANK                                  # a blank inside the target
    tg[4, 0] = bc.C                                      # past the classes: nothing may be read through it
    tg[5, 399] = -1
    tg[5, 5] = 2 ** 31 - 1
    tl[6] = -1                                           # negative length
    tl[7] = 401                                          # above the row pitch
    ln = np.array([int(lens[0]), T, 399, T, T, T, T, T], dtype=np.int32)      # row 2: fewer frames than labels
    want = align.align_band_host(lp, ln, tg, tl, bc.BLANK, band_states=256)
    assert want.ok.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and want.band_base[3].any()
    out = _filled_out(8, 400, T)
    eng.ctc_align_band(*_cuda(lp, ln, tg, tl), bc.BLANK, band_states=256, out=out)
    torch.cuda.synchronize()
    _assert_equal(out, want, 'bad rows')


def test_k_align_band_refuses_bad_arguments_and_writes_nothing(eng):
    lib = eng.load_library()
    P, T, C_, ML, blank = 2, 40, 29, 6, 28
    lp = torch.zeros(P, T, C_, device='cuda')
    tg = torch.zeros(P, ML, dtype=torch.int32, device='cuda')
    tl = torch.full((P,), 2, dtype=torch.int32, device='cuda')
    out = _filled_out(P, ML, T)
    need = eng.ctc_align_band_workspace_bytes(P, T, 256)
    assert need == P * (10 * 256 + 4 * T)
    for bad in (0, 255, 512, 2048, 4096, 8704):
        assert eng.ctc_align_band_workspace_bytes(P, T, bad) == 0
    assert eng.ctc_align_band_workspace_bytes(0, T, 256) == 0 and eng.ctc_align_band_workspace_bytes(P, (1 << 22) + 1, 256) == 0
    assert eng.ctc_align_band_workspace_bytes(1, 180000, 4352) == 45000 * 4352 + 720000           # an hour: 197 MB
    assert eng.ctc_align_band_workspace_bytes(32, 1 << 22, 4352) == 32 * ((1 << 20) * 4352 + (1 << 24)) > 2 ** 32   # size_t
    ws = torch.full((need + 4,), 0x5a, dtype=torch.uint8, device='cuda')

    def args(**kw):
        a = eng.AlignBandArgs()
        a.struct_size = C.sizeof(eng.AlignBandArgs)
        a.B, a.T, a.C, a.blank, a.max_labels, a.band_states = P, T, C_, blank, ML, 256
        a.pitch_utt, a.pitch_frame = T * C_, C_
        a.log_probs, a.targets, a.target_lens = lp.data_ptr(), tg.data_ptr(), tl.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        for f in FIELDS:
            setattr(a, f, getattr(out, f).data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(B=0), dict(T=0), dict(T=(1 << 22) + 1), dict(C=0), dict(max_labels=0),
           dict(max_labels=(1 << 20) + 1), dict(blank=-1), dict(blank=C_), dict(pitch_frame=C_ - 1), dict(pitch_utt=T * C_ - 1),
           dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=ws.data_ptr() + 1)]
    bad += [dict(band_states=b) for b in (0, 255, 512, 2048, 4096, -256)]
    bad += [{k: None} for k in ('log_probs', 'targets', 'target_lens', 'workspace', 'ok')]
    for kw in bad:
        assert lib.qasr_ctc_align_band(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_align_band(s, None) == 1
    with pytest.raises(ValueError, match='band_states'):             # and the binding refuses a width by name
        eng.ctc_align_band(lp, None, tg, tl, blank, band_states=512)
    torch.cuda.synchronize()
    for f in ('start', 'nframes', 'ok', 'band_base'):
        assert (getattr(out, f) == FILL32).all(), f
    assert (out.score.view(torch.int32) == FILL32).all() and (out.frame_logp.view(torch.int32) == FILL32).all()
    assert (out.path_score == FILL64).all() and (ws == 0x5a).all()
    assert lib.qasr_ctc_align_band(s, C.byref(args())) == 0                # and the same block unchanged is accepted
    torch.cuda.synchronize()
    assert (out.ok.cpu().numpy() == 1).all() and (ws[need:] == 0x5a).all()


def test_k_align_band_is_capturable(eng):
    """nothing is allocated and no length is read on the host: the launch replays from a graph on new inputs"""
    a, b = bc.moving_case('dense_L400'), bc.moving_case('lead300_L400')
    T, ML = max(a[0].shape[1], b[0].shape[1]), 400
    lp_d = torch.zeros(1, T, bc.C, device='cuda')
    lens_d = torch.zeros(1, dtype=torch.int32, device='cuda')
    tg_d = torch.zeros(1, ML, dtype=torch.int32, device='cuda')
    tl_d = torch.zeros(1, dtype=torch.int32, device='cuda')
    out = _filled_out(1, ML, T)
    ws = torch.empty(eng.ctc_align_band_workspace_bytes(1, T, 256), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, bc.BLANK, band_states=256, workspace=ws, out=out)
    for lp, _, tg, tl in (a, b):
        n = lp.shape[1]
        pad = np.zeros((1, T, bc.C), dtype=np.float32)
        pad[:, :n] = lp
        lens = np.array([n], dtype=np.int32)
        lp_d.copy_(torch.from_numpy(pad)), lens_d.copy_(torch.from_numpy(lens))
        tg_d.copy_(torch.from_numpy(tg)), tl_d.copy_(torch.from_numpy(tl))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = align.align_band_host(pad, lens, tg, tl, bc.BLANK, band_states=256)
        assert want.ok[0] == 1 and want.band_base.max() > 0
        _assert_equal(out, want, 'replay')
