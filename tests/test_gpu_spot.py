"""Keyword spotting on an MI355X: k_spot (csrc/qasr_spot.hip) against qasr.spot.spot_host - every byte of the hits, the counts,
ok and both trace planes, outputs pre-filled with 0x5a, no tolerance; refused arguments launch nothing; the chain
k_star -> k_spot replays from a graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spot_cases as sc  # noqa: E402
from qasr import align, beam, spot  # noqa: E402

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


def _i64(*shape):
    return torch.full(shape, FILL64, dtype=torch.int64, device='cuda')


def _filled(P, MH, T, K, trace=True, trace_pitch=None):
    tp = T if trace_pitch is None else trace_pitch
    return spot.SpotResult(_i32(P, MH), _i32(P, MH), _i64(P, MH), _i32(P), _i32(P), _i64(P, tp)[:, :T] if trace else None,
                           _i32(P, tp)[:, :T] if trace else None, K)


class _Host:
    def __init__(self, res, fields):
        for f in fields:
            t = getattr(res, f)
            setattr(self, f, None if t is None else t.cpu().numpy())


def _cuda(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _greedy(lp_u, blank):
    top = lp_u.argmax(1)
    return [int(c) for i, c in enumerate(top) if c != blank and (i == 0 or c != top[i - 1])]


def _run(eng, lp, lens, tg, tl, blank, threshold, max_span, max_hits, trace, wide=False, what=''):
    """one launch against the twin on every byte; wide: log_probs rows of pitch C + 3, a plane of pitch T + 5 and trace rows of
    pitch T + 3, the pads filled with values that would show"""
    B, T, C_ = lp.shape
    K = tg.shape[0]
    star = align.star_host(lp, lens, 0.0)
    want = spot.spot_host(lp, lens, star, tg, tl, blank, spot.check_threshold(threshold, 'test'), max_span, max_hits, want_trace=trace)
    lens_d, tg_d, tl_d = _cuda(lens, tg, tl)
    if wide:
        big = torch.full((B, T, C_ + 3), 3.0e38, device='cuda')
        big[:, :, :C_] = torch.from_numpy(lp).cuda()
        lp_d = big[:, :, :C_]
        plane = torch.full((B, T + 5), 7.0, device='cuda')[:, :T]
    else:
        lp_d = torch.from_numpy(lp).cuda()
        plane = torch.empty(B, T, device='cuda')
    eng.ctc_star(lp_d, lens_d, 0.0, out=plane)
    out = _filled(B * K, max_hits, T, K, trace, T + 3 if wide else None)
    eng.ctc_spot(lp_d, lens_d, plane, tg_d, tl_d, blank, threshold, max_span, max_hits, out=out)
    torch.cuda.synchronize()
    fields = sc.ALL_FIELDS if trace else sc.HIT_FIELDS
    sc.same_bytes(_Host(out, fields), want, fields, what)
    if wide and trace:
        assert (out.trace_score._base[:, T:] == FILL64).all() and (out.trace_start._base[:, T:] == FILL32).all()
    return want


# ---------------------------------------------------------------------------------------------------------------- k_spot
@pytest.mark.parametrize('ML', [1, 2, 31, 32, 63, 64, 127])
def test_k_spot_equals_spot_host_every_byte(eng, ML):
    """31 / 32 labels straddle the step from one state per lane to two (63 / 65 states), 63 / 64 the step to four; K = 3, 5 with
    B = 3 make P no multiple of 4, so the four waves of a work-group see different lim (full, 0, beyond T, short)"""
    hits = overflow = zero = 0
    for lp, lens, tg, tl, blank, threshold, max_span, max_hits, trace, wide in cases(ML):
        want = _run(eng, lp, lens, tg, tl, blank, threshold, max_span, max_hits, trace, wide,
                    what=(ML, lp.shape, tg.shape[0], threshold, max_span, max_hits))
        hits += int(want.n_hits.sum())
        overflow += int((want.n_hits > max_hits).sum())
        zero += int(((want.hit_score == 0) & (np.arange(max_hits)[None, :] < want.n_hits[:, None])).sum())
    assert hits > 0 and overflow > 0 and zero > 0


def cases(ML):
    """C = 2 (one label: all-equal keywords), 29, 5207; T = 1, 2, 37, 300; (B, K) = (1, 1), (3, 3), (3, 5); lens None / full, 0,
    beyond T / short; thresholds at both bounds and between; max_hits 1, 2, 16; max_span 3 .. 65536; with and without the trace;
    contiguous and padded rows - each value of each list occurs, the lists are cycled against one another, not crossed"""
    n = 0
    for ci, C_ in enumerate((2, 29, 5207)):
        blank = C_ - 1 if C_ != 29 else 11
        for ti, T in enumerate((1, 2, 37, 300)):
            rng = np.random.Generator(np.random.PCG64([31, ML, C_, T]))
            B, K = ((1, 1), (3, 3), (3, 5))[n % 3]
            lp = sc.logp(rng, B, T, C_, blank)
            lens = (None, np.array([T, 0, T + 5][:B], dtype=np.int32), np.array([max(T - 7, 1), T, T // 2][:B], dtype=np.int32))[(n // 3) % 3]
            lengths = [ML] + [max(1, ML // 2), 1, 2, ML][:K - 1]    # (ML = 1: the keyword of 2 labels is above the row pitch)
            rows = [sc.star_cases.labels_without_blank(rng, k, C_, blank, repeats=0.1) for k in lengths]
            g = _greedy(lp[0], blank)
            if K > 1 and len(g) >= 2:
                rows[1] = g[:min(len(g), ML, 4)]                    # a piece of the arg-max path: a hit of score exactly 0
            tg, tl = sc.pad(rows, blank, ML)
            threshold = (-16.0, 0.0, -0.7, -16.0)[(ci + ti) % 4]
            max_hits = (1, 2, 16)[(n + n // 3) % 3] if threshold else 2
            max_span = (65536, 25, 3, 300)[(n // 2) % 4]
            yield lp, lens, tg, tl, blank, threshold, max_span, max_hits, n % 5 != 4, n % 2 == 1
            n += 1


def test_all_equal_labels_take_no_skip(eng):
    """y = a a a ...: every label state is entered through the blank below it; L = 20 needs 39 frames"""
    C_, T, blank = 29, 120, 28
    rng = np.random.Generator(np.random.PCG64(41))
    lp = sc.logp(rng, 2, T, C_, blank)
    rows = [[7] * 20, [7] * 33, [7] * 70, [3]]
    for ML in (31, 40, 127):
        tg, tl = sc.pad([r for r in rows if len(r) <= ML], blank, ML)
        want = _run(eng, lp, None, tg, tl, blank, -16.0, 65536, 4, trace=True, what=ML)
        assert want.ok.all() and (want.trace_score[0] != beam.NEG).any()


def test_nan_and_inf_rows_and_invalid_keywords_between_valid_ones(eng):
    C_, T, blank, ML = 29, 64, 28, 127
    rng = np.random.Generator(np.random.PCG64(43))
    lp = sc.logp(rng, 3, T, C_, blank)
    lp[0, 3, :] = -np.inf
    lp[0, 9, :] = np.nan
    lp[1, 5, 2] = np.nan
    lp[1, 6, 4] = -np.inf
    lp[2, 7, :] = 0.0
    lens = np.array([T, T - 9, 0], dtype=np.int32)
    good = sc.star_cases.labels_without_blank(rng, 4, C_, blank)
    rows = [good, [], [1, blank, 2], good[:2], [1, C_], [-1], [2 ** 31 - 1, 1], good]
    tg, tl = sc.pad(rows, blank, ML)
    tl = np.concatenate([tl, [128, -1, 2 ** 31 - 1]]).astype(np.int32)         # lengths above the pitch, negative, huge
    tg = np.concatenate([tg, np.full((3, ML), 1, np.int32)])
    for threshold, max_hits in ((-16.0, 2), (-1.0, 1)):
        want = _run(eng, lp, lens, tg, tl, blank, threshold, 65536, max_hits, trace=True, what=threshold)
        assert want.ok.reshape(3, -1).tolist() == [[1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]] * 3
        assert threshold > -16.0 or want.n_hits[0] > max_hits       # (at -16 every live frame is a candidate)


def test_one_row_past_max_t(eng):
    """70 000 frames: nothing ties k_spot to MAX_T = 65536 (there is no workspace)"""
    C_, T, blank = 29, 70000, 28
    assert T > beam.MAX_T
    rng = np.random.Generator(np.random.PCG64(47))
    lp = sc.logp(rng, 1, T, C_, blank)
    g = _greedy(lp[0, 66000:66400], blank)
    tg, tl = sc.pad([g[:3]], blank)
    want = _run(eng, lp, np.array([T - 1], dtype=np.int32), tg, tl, blank, -0.5, 40, 16, trace=True)
    assert want.n_hits[0] > 16 and int(want.hit_end[0, 0]) >= 0
    ends = np.flatnonzero((want.trace_score[0] == 0) & (np.arange(T) > beam.MAX_T))
    assert len(ends) > 0                                            # exact matches behind frame 65536 are seen


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_launch_nothing(eng):
    lib = eng.load_library()
    B, T, C_, K, ML, MH, blank = 2, 8, 29, 3, 4, 2, 28
    lp = torch.zeros(B, T, C_, device='cuda')
    plane = torch.zeros(B, T, device='cuda')
    tg = torch.ones(K, ML, dtype=torch.int32, device='cuda')
    tl = torch.full((K,), 2, dtype=torch.int32, device='cuda')
    out = _filled(B * K, MH, T, K)
    ts, tb = out.trace_score._base, out.trace_start._base

    def args(**kw):
        a = eng.SpotArgs()
        a.struct_size = C.sizeof(eng.SpotArgs)
        a.B, a.T, a.C, a.K, a.max_labels, a.blank = B, T, C_, K, ML, blank
        a.threshold_q, a.max_span, a.max_hits = -65536, 10, MH
        a.pitch_utt, a.pitch_frame = T * C_, C_
        a.log_probs, a.star_logp, a.star_pitch = lp.data_ptr(), plane.data_ptr(), T
        a.targets, a.target_lens = tg.data_ptr(), tl.data_ptr()
        for f in sc.HIT_FIELDS:
            setattr(a, f, getattr(out, f).data_ptr())
        a.trace_score, a.trace_start, a.trace_pitch = ts.data_ptr(), tb.data_ptr(), T
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=C.sizeof(eng.SpotArgs) + 8), dict(struct_size=C.sizeof(eng.SpotArgs) - 8)]
    bad += [{f: None} for f in ('log_probs', 'star_logp', 'targets', 'target_lens') + sc.HIT_FIELDS]
    bad += [dict(B=0), dict(T=0), dict(C=0), dict(K=0), dict(T=(1 << 22) + 1, star_pitch=1 << 23, trace_pitch=1 << 23, pitch_utt=1 << 40),
            dict(max_labels=0), dict(max_labels=128), dict(blank=-1), dict(blank=C_), dict(star_pitch=T - 1), dict(pitch_frame=C_ - 1),
            dict(pitch_utt=T * C_ - 1), dict(threshold_q=1), dict(threshold_q=-16 * 65536 - 1), dict(max_span=0), dict(max_span=65537),
            dict(max_hits=0), dict(max_hits=-1), dict(trace_score=None), dict(trace_start=None), dict(trace_pitch=T - 1)]
    for kw in bad:
        assert lib.qasr_ctc_spot(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_spot(s, None) == 1
    for thr in (0.5, -17, float('nan'), None):
        with pytest.raises(ValueError, match='threshold'):
            eng.ctc_spot(lp, None, plane, tg, tl, blank, thr, 10, MH)
    for span in (0, 65537):
        with pytest.raises(ValueError, match='max_span'):
            eng.ctc_spot(lp, None, plane, tg, tl, blank, -1.0, span, MH)
    with pytest.raises(ValueError, match='max_hits'):
        eng.ctc_spot(lp, None, plane, tg, tl, blank, -1.0, 10, 0)
    with pytest.raises(ValueError, match='max_labels'):
        eng.ctc_spot(lp, None, plane, torch.ones(K, 128, dtype=torch.int32, device='cuda'), tl, blank, -1.0, 10, MH)
    torch.cuda.synchronize()
    for f in sc.HIT_FIELDS:
        t = getattr(out, f)
        assert (t == (FILL64 if t.dtype == torch.int64 else FILL32)).all(), f
    assert (ts == FILL64).all() and (tb == FILL32).all()
    # the same arguments, unbroken, and the bounds themselves, are taken
    for kw in (dict(), dict(threshold_q=0, max_span=1), dict(trace_score=None, trace_start=None), dict(threshold_q=-16 * 65536, max_span=65536)):
        assert lib.qasr_ctc_spot(s, C.byref(args(**kw))) == 0, kw
    torch.cuda.synchronize()
    want = spot.spot_host(lp.cpu().numpy(), None, plane.cpu().numpy(), tg.cpu().numpy(), tl.cpu().numpy(), blank, -16 * 65536, 65536, MH,
                          want_trace=True)
    sc.same_bytes(_Host(out, sc.ALL_FIELDS), want, sc.ALL_FIELDS, 'unbroken')


# ---------------------------------------------------------------------------------------------------------------- graph
def test_k_star_then_k_spot_is_capturable(eng):
    """nothing is allocated and no length is read on the host: the chain replays from a graph on new log-probabilities, and
    equals the eager run on every byte"""
    C_, T, B, ML, MH, blank = 29, 64, 2, 8, 4, 28
    rng = np.random.Generator(np.random.PCG64(13))
    lps = [sc.logp(rng, B, T, C_, blank) for _ in range(2)]
    rows = [_greedy(lps[0][0], blank)[:3], _greedy(lps[1][1], blank)[:4], [3], sc.star_cases.labels_without_blank(rng, 8, C_, blank)]
    tg, tl = sc.pad(rows, blank, ML)
    lens = np.array([T, T - 9], dtype=np.int32)
    lp_d, lens_d, tg_d, tl_d = _cuda(lps[0], lens, tg, tl)
    K = len(rows)
    out = _filled(B * K, MH, T, K)
    plane = _i32(B, T).view(torch.float32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_star(lp_d, lens_d, 0.0, out=plane)
            eng.ctc_spot(lp_d, lens_d, plane, tg_d, tl_d, blank, -2.0, 30, MH, out=out)
    for lp in lps[::-1]:
        lp_d.copy_(torch.from_numpy(lp))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        replayed = _Host(out, sc.ALL_FIELDS)
        eager = _filled(B * K, MH, T, K)
        eng.ctc_spot(lp_d, lens_d, eng.ctc_star(lp_d, lens_d, 0.0), tg_d, tl_d, blank, -2.0, 30, MH, out=eager)
        torch.cuda.synchronize()
        sc.same_bytes(replayed, _Host(eager, sc.ALL_FIELDS), sc.ALL_FIELDS, 'replay against eager')
        want = sc.host(lp, lens, tg, tl, blank, -2.0, 30, MH)
        assert want.ok.all() and want.n_hits.sum() > 0
        sc.same_bytes(replayed, want, sc.ALL_FIELDS, 'replay against the twin')
