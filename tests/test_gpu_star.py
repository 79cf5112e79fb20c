"""The wildcard ("star") on an MI355X: k_star (csrc/qasr_star.hip) against qasr.align.star_host, and k_align<., true> /
k_align_band<., true> against the twins with a plane - every byte of every output, no tolerance; the old struct sizes still
work, refused arguments launch nothing, and the chain k_star -> k_align replays from a graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases  # noqa: E402
import star_cases as sc  # noqa: E402
from qasr import align, beam  # noqa: E402

FILL32, FILL64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _i32(*shape):
    return torch.full(shape, FILL32, dtype=torch.int32, device='cuda')


def _filled_align(P, ML, blank, K, total=True):
    return align.AlignResult(None, None, _i32(P, ML), _i32(P, ML), _i32(P, ML).view(torch.float32),
                             torch.full((P,), FILL64, dtype=torch.int64, device='cuda'),
                             torch.full((P,), FILL64, dtype=torch.int64, device='cuda') if total else None, _i32(P), blank, K)


def _filled_band(P, ML, T, blank):
    return align.BandResult(None, None, _i32(P, ML), _i32(P, ML), _i32(P, ML).view(torch.float32),
                            torch.full((P,), FILL64, dtype=torch.int64, device='cuda'), None, _i32(P), blank, 1,
                            _i32(P, T).view(torch.float32), _i32(P, (T + 31) // 32))


class _Host:
    """a device result's arrays on the host, for star_cases.same_bytes"""

    def __init__(self, res, fields):
        for f in fields:
            t = getattr(res, f)
            setattr(self, f, None if t is None else t.cpu().numpy())


def _cuda(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# --------------------------------------------------------------------------------------------------------------- k_star
@pytest.mark.parametrize('C_', [1, 2, 29, 63, 64, 65, 257, 5207])
def test_k_star_equals_star_host_every_byte(eng, C_):
    B = 2
    for T in (1, 5, 33):
        rng = np.random.Generator(np.random.PCG64(100 * C_ + T))
        lp = np.log(rng.dirichlet(np.ones(C_), size=(B, T))).astype(np.float32) - np.float32(0.01)
        lp[0, 0, :] = lp[0, 0, 0]                                   # a tie row
        lp[1, T - 1, :] = -np.inf                                   # a row of all -inf
        if T > 2 and C_ > 2:
            lp[0, 1, [0, C_ - 1]] = 0.0                             # the maximum at both ends of the row: head and tail lanes
            lp[1, 1, :] = -0.0
            lp[1, 1, C_ // 2] = 0.0
        for pitch in (C_, C_ + 3):                                  # C + 3: rows start at every offset from a 16-byte boundary
            wide = torch.full((B, T, pitch), 3.0e38, device='cuda')  # a pad that would win any maximum it leaked into
            wide[:, :, :C_] = torch.from_numpy(lp).cuda()
            src = wide[:, :, :C_]
            for lens in (None, np.array([0, T - 1], dtype=np.int32)):
                lens_d = None if lens is None else torch.from_numpy(lens).cuda()
                for penalty in (0.0, 1.5):
                    want = align.star_host(lp, lens, penalty)
                    for sp in (T, T + 5):
                        buf = _i32(B, sp).view(torch.float32)
                        got = eng.ctc_star(src, lens_d, penalty, out=buf[:, :T])
                        torch.cuda.synchronize()
                        assert got.cpu().numpy().tobytes() == want.tobytes(), (T, pitch, lens, penalty, sp)
                        assert (buf.view(torch.int32)[:, T:] == FILL32).all()
    fresh = eng.ctc_star(src, None, 1.5)                            # a buffer of its own
    assert fresh.cpu().numpy().tobytes() == align.star_host(lp, None, 1.5).tobytes()


def test_k_star_refuses_bad_arguments_and_writes_nothing(eng):
    lib = eng.load_library()
    B, T, C_ = 2, 8, 29
    lp = torch.zeros(B, T, C_, device='cuda')
    out = _i32(B, T).view(torch.float32)

    def args(**kw):
        a = eng.StarArgs()
        a.struct_size = C.sizeof(eng.StarArgs)
        a.B, a.T, a.C, a.pitch_utt, a.pitch_frame = B, T, C_, T * C_, C_
        a.log_probs, a.star, a.star_pitch, a.penalty = lp.data_ptr(), out.data_ptr(), T, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=C.sizeof(eng.StarArgs) + 8), dict(B=0), dict(T=0), dict(C=0), dict(pitch_frame=C_ - 1),
           dict(pitch_utt=T * C_ - 1), dict(star_pitch=T - 1), dict(penalty=-0.5), dict(penalty=16.5), dict(penalty=float('nan')),
           dict(penalty=float('inf')), dict(log_probs=None), dict(star=None)]
    for kw in bad:
        assert lib.qasr_ctc_star(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_star(s, None) == 1
    for pen in (-1, 17, float('nan'), None):
        with pytest.raises(ValueError, match='penalty'):
            eng.ctc_star(lp, None, pen)
    torch.cuda.synchronize()
    assert (out.view(torch.int32) == FILL32).all()
    assert lib.qasr_ctc_star(s, C.byref(args())) == 0 and lib.qasr_ctc_star(s, C.byref(args(penalty=16.0))) == 0
    torch.cuda.synchronize()
    assert (out == -16.0).all()


# ------------------------------------------------------------------------------------------------------ k_align<., true>
@pytest.mark.parametrize('ML', [1, 127, 128, 600])
def test_k_align_with_a_plane_equals_align_host_every_byte(eng, ML):
    """255 / 257 states straddle the step from one state per thread to two; 1201 states run eight per thread.  B = 3, K = 2:
    the six wildcard positions in one launch, a different one per row"""
    C_, B, K, blank = 29, 3, 2, 28
    T = 700 if ML == 600 else 300
    rng = np.random.Generator(np.random.PCG64(200 + ML))
    lp = sc.logp(rng, B, T, C_, blank)
    lens = np.array([T, T - 37, T + 5], dtype=np.int32)
    if ML == 1:
        rows = [[C_], [3], [C_], [], [C_], [C_]]
    else:
        rows = [sc.with_wildcards(sc.labels_without_blank(rng, ML - 3, C_, blank, repeats=0.05), C_, pos) for pos in sc.POSITIONS]
        assert max(len(r) for r in rows) == ML
    tg, tl = align_cases.pad_targets(rows, blank, ML)
    lp_d, lens_d, tg_d, tl_d = _cuda(lp, lens, tg, tl)
    n_ok = 0
    for use_lens in (True, False):
        star = align.star_host(lp, lens if use_lens else None, 1.0)
        star_d = eng.ctc_star(lp_d, lens_d if use_lens else None, 1.0)
        for total in (True, False):
            want = align.align_host(lp, lens if use_lens else None, tg, tl, blank, problems_per_utt=K, want_total=total, star=star)
            out = _filled_align(B * K, ML, blank, K, total)
            eng.ctc_align(lp_d, lens_d if use_lens else None, tg_d, tl_d, blank, problems_per_utt=K, out=out, star=star_d)
            torch.cuda.synchronize()
            sc.same_bytes(_Host(out, sc.ALIGN_FIELDS), want, sc.ALIGN_FIELDS, (ML, use_lens, total))
            n_ok += int(want.ok.sum())
    assert n_ok >= 4 * (5 if ML > 1 else 6)
    # the wildcard's id with a NULL plane: a label outside [0, C), as before
    out = _filled_align(B * K, ML, blank, K)
    eng.ctc_align(lp_d, lens_d, tg_d, tl_d, blank, problems_per_utt=K, out=out)
    torch.cuda.synchronize()
    want = align.align_host(lp, lens, tg, tl, blank, problems_per_utt=K)
    sc.same_bytes(_Host(out, sc.ALIGN_FIELDS), want, sc.ALIGN_FIELDS, 'NULL plane')
    assert want.ok.tolist() == [int(C_ not in r) for r in rows]


def test_k_align_with_a_plane_of_another_pitch_and_special_values(eng):
    C_, B, T, ML, blank = 6, 2, 40, 9, 5
    rng = np.random.Generator(np.random.PCG64(3))
    lp = np.log(rng.dirichlet(np.ones(C_), size=(B, T))).astype(np.float32)
    lp[0, 3, :] = -np.inf                                           # the plane is -inf there: quantize takes its floor
    lp[1, 5, :] = -0.0
    star = align.star_host(lp, None, 0.0)
    tg, tl = align_cases.pad_targets([[1, C_, 2, 2, C_], [C_, 0, C_, C_, 3]], blank, ML)
    want = align.align_host(lp, None, tg, tl, blank, star=star)
    assert want.ok.all()
    lp_d, tg_d, tl_d = _cuda(lp, tg, tl)
    wide = torch.full((B, T + 5), 7.0, device='cuda')
    wide[:, :T] = torch.from_numpy(star).cuda()
    out = _filled_align(B, ML, blank, 1)
    eng.ctc_align(lp_d, None, tg_d, tl_d, blank, out=out, star=wide[:, :T])
    torch.cuda.synchronize()
    sc.same_bytes(_Host(out, sc.ALIGN_FIELDS), want, sc.ALIGN_FIELDS)


# ------------------------------------------------------------------------------------------------- k_align_band<., true>
def test_k_align_band_with_the_band_fixed_equals_k_align(eng):
    C_, B, T, ML, blank = 29, 3, 300, 127, 28
    rng = np.random.Generator(np.random.PCG64(61))
    lp = sc.logp(rng, B, T, C_, blank)
    lens = np.array([T, T - 37, T + 5], dtype=np.int32)
    star = align.star_host(lp, lens, 1.0)
    lp_d, lens_d = _cuda(lp, lens)
    star_d = eng.ctc_star(lp_d, lens_d, 1.0)
    for r in (0, 3):
        rows = [sc.with_wildcards(sc.labels_without_blank(rng, ML - 3, C_, blank, repeats=0.05), C_, pos) for pos in sc.POSITIONS[r:r + 3]]
        tg, tl = align_cases.pad_targets(rows, blank, ML)
        tg_d, tl_d = _cuda(tg, tl)
        band = _filled_band(B, ML, T, blank)
        eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, blank, band_states=256, out=band, star=star_d)
        full = _filled_align(B, ML, blank, 1, total=False)
        eng.ctc_align(lp_d, lens_d, tg_d, tl_d, blank, out=full, star=star_d)
        torch.cuda.synchronize()
        shared = ('start', 'nframes', 'score', 'path_score', 'ok')
        sc.same_bytes(_Host(band, shared), _Host(full, shared), shared, r)
        want = align.align_band_host(lp, lens, tg, tl, blank, band_states=256, star=star)
        sc.same_bytes(_Host(band, sc.BAND_FIELDS), want, sc.BAND_FIELDS, r)
        assert want.ok.all() and not want.band_base.any()


@pytest.mark.parametrize('L,T,bw', [(200, 1200, 256), (600, 2000, 1024)])
def test_k_align_band_with_the_band_moving_equals_the_twin(eng, L, T, bw):
    lp, tg, tl, blank, _ = sc.moving_band_case(L=L, T=T, seed=51 + L, band_states=bw)
    lens = np.array([T - 7], dtype=np.int32)
    star = align.star_host(lp, lens, 1.0)
    want = align.align_band_host(lp, lens, tg, tl, blank, band_states=bw, star=star)
    assert want.ok[0] == 1 and want.band_base.max() > 100
    lp_d, lens_d, tg_d, tl_d = _cuda(lp, lens, tg, tl)
    out = _filled_band(1, tg.shape[1], T, blank)
    eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, blank, band_states=bw, out=out, star=eng.ctc_star(lp_d, lens_d, 1.0))
    torch.cuda.synchronize()
    sc.same_bytes(_Host(out, sc.BAND_FIELDS), want, sc.BAND_FIELDS, (L, T, bw))


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_old_struct_sizes_are_accepted_and_bad_planes_refused(eng):
    lib = eng.load_library()
    B, T, C_, ML, blank = 2, 50, 29, 12, 28
    rng = np.random.Generator(np.random.PCG64(71))
    lp = sc.logp(rng, B, T, C_, blank)
    tg, tl = align_cases.pad_targets([sc.labels_without_blank(rng, 10, C_, blank), sc.labels_without_blank(rng, 12, C_, blank)], blank, ML)
    lp_d, tg_d, tl_d = _cuda(lp, tg, tl)
    star_d = torch.zeros(B, T, device='cuda')
    tab = eng.lae_table_device('cuda')
    s = eng._stream_ptr()
    old_align, old_band = eng.AlignArgs.star_logp.offset, eng.AlignBandArgs.star_logp.offset
    assert old_align == C.sizeof(eng.AlignArgs) - 16 and old_band == C.sizeof(eng.AlignBandArgs) - 16

    # ---- qasr_ctc_align
    out = _filled_align(B, ML, blank, 1)
    ws = torch.empty(eng.ctc_align_workspace_bytes(B, T, ML), dtype=torch.uint8, device='cuda')

    def a_args(**kw):
        a = eng.AlignArgs()
        a.struct_size = C.sizeof(eng.AlignArgs)
        a.B, a.T, a.C, a.P, a.K, a.blank, a.max_labels = B, T, C_, B, 1, blank, ML
        a.pitch_utt, a.pitch_frame = T * C_, C_
        a.log_probs, a.targets, a.target_lens = lp_d.data_ptr(), tg_d.data_ptr(), tl_d.data_ptr()
        a.lae_entries, a.lae_table, a.workspace, a.workspace_bytes = beam.TAB_ENTRIES, tab.data_ptr(), ws.data_ptr(), ws.numel()
        for f in sc.ALIGN_FIELDS:
            setattr(a, f, getattr(out, f).data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw in (dict(star_logp=star_d.data_ptr(), star_pitch=T - 1), dict(star_logp=star_d.data_ptr(), star_pitch=0),
               dict(struct_size=old_align - 8), dict(struct_size=old_align + 8), dict(struct_size=C.sizeof(eng.AlignArgs) + 8)):
        assert lib.qasr_ctc_align(s, C.byref(a_args(**kw))) == 1, kw
    torch.cuda.synchronize()
    assert (out.ok == FILL32).all() and (out.start == FILL32).all() and (out.total == FILL64).all()
    want = align.align_host(lp, None, tg, tl, blank)
    # the old size: the new fields count as absent, whatever lies behind the shorter struct
    assert lib.qasr_ctc_align(s, C.byref(a_args(struct_size=old_align, star_logp=0xdead0000, star_pitch=-1))) == 0
    torch.cuda.synchronize()
    sc.same_bytes(_Host(out, sc.ALIGN_FIELDS), want, sc.ALIGN_FIELDS, 'old size')
    out2 = _filled_align(B, ML, blank, 1)
    for f in sc.ALIGN_FIELDS:
        getattr(out, f).copy_(getattr(out2, f))
    assert lib.qasr_ctc_align(s, C.byref(a_args())) == 0                   # the new size without a plane: the same call
    torch.cuda.synchronize()
    sc.same_bytes(_Host(out, sc.ALIGN_FIELDS), want, sc.ALIGN_FIELDS, 'new size')

    # ---- qasr_ctc_align_band
    band = _filled_band(B, ML, T, blank)
    wsb = torch.empty(eng.ctc_align_band_workspace_bytes(B, T, 256), dtype=torch.uint8, device='cuda')

    def b_args(**kw):
        a = eng.AlignBandArgs()
        a.struct_size = C.sizeof(eng.AlignBandArgs)
        a.B, a.T, a.C, a.blank, a.max_labels, a.band_states = B, T, C_, blank, ML, 256
        a.pitch_utt, a.pitch_frame = T * C_, C_
        a.log_probs, a.targets, a.target_lens = lp_d.data_ptr(), tg_d.data_ptr(), tl_d.data_ptr()
        a.workspace, a.workspace_bytes = wsb.data_ptr(), wsb.numel()
        for f in sc.BAND_FIELDS:
            setattr(a, f, getattr(band, f).data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw in (dict(star_logp=star_d.data_ptr(), star_pitch=T - 1), dict(struct_size=old_band - 8), dict(struct_size=old_band + 8)):
        assert lib.qasr_ctc_align_band(s, C.byref(b_args(**kw))) == 1, kw
    torch.cuda.synchronize()
    assert (band.ok == FILL32).all() and (band.frame_logp.view(torch.int32) == FILL32).all() and (band.band_base == FILL32).all()
    assert lib.qasr_ctc_align_band(s, C.byref(b_args(struct_size=old_band, star_logp=0xdead0000, star_pitch=-1))) == 0
    torch.cuda.synchronize()
    sc.same_bytes(_Host(band, sc.BAND_FIELDS), align.align_band_host(lp, None, tg, tl, blank, band_states=256), sc.BAND_FIELDS, 'old size')


# ---------------------------------------------------------------------------------------------------------------- graph
def test_k_star_then_k_align_is_capturable(eng):
    """nothing is allocated and no length is read on the host: the chain replays from a graph on new log-probabilities"""
    C_, T, B, ML, blank = 29, 64, 2, 20, 28
    rng = np.random.Generator(np.random.PCG64(13))
    lps = [sc.logp(rng, B, T, C_, blank) for _ in range(2)]
    rows = [sc.with_wildcards(sc.labels_without_blank(rng, 12, C_, blank), C_, pos) for pos in ('two_with_a_label_between', 'first')]
    tg, tl = align_cases.pad_targets(rows, blank, ML)
    lens = np.array([T, T - 9], dtype=np.int32)
    lp_d, lens_d, tg_d, tl_d = _cuda(lps[0], lens, tg, tl)
    out = _filled_align(B, ML, blank, 1)
    plane = _i32(B, T).view(torch.float32)
    ws = torch.empty(eng.ctc_align_workspace_bytes(B, T, ML), dtype=torch.uint8, device='cuda')
    eng.lae_table_device('cuda')                         # uploaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_star(lp_d, lens_d, 1.0, out=plane)
            eng.ctc_align(lp_d, lens_d, tg_d, tl_d, blank, workspace=ws, out=out, star=plane)
    for lp in lps[::-1]:
        lp_d.copy_(torch.from_numpy(lp))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        star = align.star_host(lp, lens, 1.0)
        assert plane.cpu().numpy().tobytes() == star.tobytes()
        want = align.align_host(lp, lens, tg, tl, blank, star=star)
        assert want.ok.all()
        sc.same_bytes(_Host(out, sc.ALIGN_FIELDS), want, sc.ALIGN_FIELDS, 'replay')
