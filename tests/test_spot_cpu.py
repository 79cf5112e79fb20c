"""qasr.spot on the host: spot_host's trace against a brute-force oracle that tries every start frame on its own, the emission's
sign on every kind of row, planted keywords, the hit rule against a plain restatement, invalid keywords, and
EncDecCTCModel.spot / spot_long on CPU tensors against the composition of the twins."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spot_cases as sc  # noqa: E402
from qasr import align, beam, ctc, spot  # noqa: E402

NEG = beam.NEG


# ------------------------------------------------------------------------------------------------ the trace against the oracle
@pytest.mark.parametrize('C', [2, 29])
@pytest.mark.parametrize('T', [1, 2, 17, 40])
def test_trace_equals_the_brute_force_oracle(C, T):
    blank = C - 1
    rng = np.random.Generator(np.random.PCG64([7, C, T]))
    B = 2
    lp = sc.logp(rng, B, T, C, blank)
    lens = np.array([T, max(T - 3, 1)], dtype=np.int32)
    rows = [sc.star_cases.labels_without_blank(rng, n, C, blank) for n in (1, 2, 5)]
    rows += [[rows[2][0]] * 3, [rows[2][0], rows[2][0], rows[2][1], rows[2][1]]]          # repeated labels: a a a, a a b b
    tg, tl = sc.pad(rows, blank)
    star = align.star_host(lp, lens, 0.0)
    res = spot.spot_host(lp, lens, star, tg, tl, blank, -16 * beam.ONE, 65536, 4, want_trace=True)
    assert res.ok.all() and res.trace_score.shape == (B * len(rows), T) and res.trace_start.dtype == np.int32
    live = 0
    for u in range(B):
        lim = int(lens[u])
        for k, y in enumerate(rows):
            p = u * len(rows) + k
            best, dmax = sc.brute(lp[u], star[u], lim, y, blank)
            assert res.trace_score[p, :lim].tolist() == dmax, (u, k)
            for t in range(lim):
                s0 = int(res.trace_start[p, t])
                if dmax[t] == NEG:
                    assert s0 == -1
                else:
                    assert 0 <= s0 <= t and best[s0][t] == dmax[t], (u, k, t)      # a maximiser; ties are not pinned here
                    live += 1
            assert not res.trace_score[p, lim:].any() and not res.trace_start[p, lim:].any()
    assert live > 0 or T < 2


# ------------------------------------------------------------------------------------------------------------- the emission
def test_the_emission_is_never_positive_nan_and_inf_rows_included():
    C, T, blank = 6, 12, 5
    rng = np.random.Generator(np.random.PCG64(3))
    lp = sc.logp(rng, 1, T, C, blank)
    lp[0, 2, :] = -np.inf
    lp[0, 3, :] = np.nan
    lp[0, 4, 1] = np.nan                                            # a NaN among numbers: it is the row's "maximum"
    lp[0, 5, 2] = -np.inf
    lp[0, 6, :] = 0.0
    star = align.star_host(lp, None, 0.0)
    for y in ([1], [1, 2], [2, 2, 3]):
        e = sc.emissions(lp[0], star[0], y, blank)
        assert all(v <= 0 for row in e for v in row[1:])
        res = spot.spot_host(lp, None, star, *sc.pad([y], blank), blank, -16 * beam.ONE, 65536, 4, want_trace=True)
        d = res.trace_score[0]
        assert ((d <= 0) | (d == NEG)).all()
        _, dmax = sc.brute(lp[0], star[0], T, y, blank)
        assert d.tolist() == dmax


# ----------------------------------------------------------------------------------------------------------- planted keywords
def test_a_planted_keyword_is_one_hit_with_score_zero_over_its_stretch():
    C, T, blank = 29, 60, 28
    y = [3, 7, 7, 11]
    lp, spans = sc.planted(y, [10], T, C, blank)
    other = [5, 9]
    tg, tl = sc.pad([y, other], blank)
    # (blank frames score 0, so a wide max_span lets them dilute a mismatch: the span is held to the keyword's own length)
    res = sc.host(lp, None, tg, tl, blank, -0.5, 12, 4)
    assert res.n_hits.tolist() == [1, 0] and res.ok.tolist() == [1, 1]
    assert (int(res.hit_start[0, 0]), int(res.hit_end[0, 0]), int(res.hit_score[0, 0])) == (spans[0][0], spans[0][1], 0)
    assert not res.hit_start[0, 1:].any() and not res.hit_end[0, 1:].any() and not res.hit_score[0, 1:].any()
    hits = spot.to_hits(res, ['keyword', 'other'], 0.02)
    assert len(hits) == 1 and len(hits[0]) == 1
    h = hits[0][0]
    assert isinstance(h, ctc.KeywordHit) and (h.keyword, h.index, h.score, h.frames) == ('keyword', 0, 0.0, spans[0][1] - spans[0][0] + 1)
    assert h.start_s == spans[0][0] * 0.02 and h.end_s == (spans[0][1] + 1) * 0.02


def test_two_planted_occurrences_are_two_hits_in_time_order_and_a_long_one_is_none():
    C, T, blank = 29, 80, 28
    y = [4, 1, 9]
    lp, spans = sc.planted(y, [5, 50], T, C, blank)
    tg, tl = sc.pad([y], blank)
    res = sc.host(lp, None, tg, tl, blank, -0.5, 7, 4)
    assert res.n_hits.tolist() == [2]
    assert [(int(a), int(b), int(d)) for a, b, d in zip(res.hit_start[0, :2], res.hit_end[0, :2], res.hit_score[0, :2])] == \
        [(spans[0][0], spans[0][1], 0), (spans[1][0], spans[1][1], 0)]
    hits = spot.to_hits(res, [tuple(y)], 0.02)[0]
    assert [h.start_s for h in hits] == sorted(h.start_s for h in hits) and len(hits) == 2
    # an occurrence longer than max_span yields none: the row's winner starts at the stretch's first frame
    n = spans[0][1] - spans[0][0] + 1
    assert n == 7
    assert sc.host(lp, None, tg, tl, blank, -0.5, n - 1, 4).n_hits.tolist() == [0]
    assert sc.host(lp, None, tg, tl, blank, -0.5, n, 4).n_hits.tolist() == [2]
    # a last label of three frames: the later ends tie at mean 0 and are dropped, the hit ends on its first frame
    lp3, spans3 = sc.planted(y, [5], T, C, blank, last_frames=3)
    res = sc.host(lp3, None, tg, tl, blank, -0.5, 9, 4)
    assert res.n_hits.tolist() == [1]
    assert (int(res.hit_start[0, 0]), int(res.hit_end[0, 0]), int(res.hit_score[0, 0])) == (spans3[0][0], spans3[0][1] - 2, 0)


# -------------------------------------------------------------------------------------------------------------- the hit rule
@pytest.mark.parametrize('threshold', [0.0, -0.7, -16.0])
@pytest.mark.parametrize('max_hits', [1, 2, 16])
def test_hits_equal_the_restated_rule_run_on_the_trace(threshold, max_hits):
    C, T, blank, B = 5, 120, 4, 2
    rng = np.random.Generator(np.random.PCG64([11, max_hits]))
    lp = sc.logp(rng, B, T, C, blank)
    if threshold == 0.0:                                            # so that a score of exactly 0 exists
        planted, _ = sc.planted([1, 2], [20, 60], T, C, blank)
        lp[0] = planted[0]
    lens = np.array([T, T - 11], dtype=np.int32)
    tg, tl = sc.keywords(rng, (1, 2, 3, 4), C, blank)
    thr = spot.check_threshold(threshold, 'test')
    overflow = overlap = 0
    for max_span in (3, 25, 65536):
        res = sc.host(lp, lens, tg, tl, blank, threshold, max_span, max_hits)
        for p in range(B * 4):
            lim = int(lens[p // 4])
            want = sc.hits_restated(res.trace_score[p, :lim], res.trace_start[p, :lim], thr, max_span)
            assert int(res.n_hits[p]) == len(want), (p, max_span)
            kept = want[:max_hits]
            got = list(zip(res.hit_start[p].tolist(), res.hit_end[p].tolist(), res.hit_score[p].tolist()))
            assert got == kept + [(0, 0, 0)] * (max_hits - len(kept)), (p, max_span)
            assert all(a[1] < b[0] for a, b in zip(want, want[1:]))                 # emitted hits never overlap
            overflow += len(want) > max_hits
            d, s = res.trace_score[p, :lim], res.trace_start[p, :lim].astype(np.int64)
            n = np.arange(lim) - s + 1
            cand = np.flatnonzero((d != NEG) & (n <= max_span) & (d >= thr * n))
            overlap += int((s[cand][1:] <= cand[:-1]).sum())
    assert overlap > 0 or threshold == 0.0
    if max_hits < 16 and threshold < 0:
        assert overflow > 0


# --------------------------------------------------------------------------------------------------------- invalid keywords
def test_invalid_keywords_and_empty_utterances():
    C, T, blank = 29, 30, 28
    rng = np.random.Generator(np.random.PCG64(5))
    lp = sc.logp(rng, 2, T, C, blank)
    lens = np.array([T, 0], dtype=np.int32)
    good = sc.star_cases.labels_without_blank(rng, 4, C, blank)
    rows = [good, [], [1, blank, 2], [1, C], [-1], good]
    tg, tl = sc.pad(rows, blank, 127)
    tl = np.concatenate([tl, [128]]).astype(np.int32)               # L = 128: above the row pitch and above MAX_LABELS
    tg = np.concatenate([tg, np.full((1, 127), 1, np.int32)])
    res = sc.host(lp, lens, tg, tl, blank, -16.0, 65536, 3)
    K = len(tl)
    assert res.ok.reshape(2, K).tolist() == [[1, 0, 0, 0, 0, 1, 0]] * 2
    bad = res.ok == 0
    assert not res.n_hits[bad].any() and not res.hit_start[bad].any() and not res.hit_score[bad].any()
    assert not res.trace_score[bad].any() and not res.trace_start[bad].any()
    assert not res.n_hits[K:].any() and not res.trace_score[K:].any()            # lens = 0: ok = 1 and no hits
    assert res.n_hits[0] > 0 and res.n_hits[0] == res.n_hits[5]
    one = sc.host(lp[:1], lens[:1], tg[:1], tl[:1], blank, -16.0, 65536, 3)
    sc.same_bytes(one, type(one)(*(getattr(res, f)[:1] for f in sc.ALL_FIELDS)), sc.ALL_FIELDS)      # neighbours do not matter
    for kw, name in ((dict(threshold_q=1), 'threshold_q'), (dict(threshold_q=-16 * beam.ONE - 1), 'threshold_q'),
                     (dict(max_span=0), 'max_span'), (dict(max_span=65537), 'max_span'), (dict(max_hits=0), 'max_hits'),
                     (dict(blank=C), 'blank')):
        args = dict(threshold_q=-beam.ONE, max_span=10, max_hits=2, blank=blank)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            spot.spot_host(lp, lens, align.star_host(lp, lens, 0.0), tg, tl, **args)
    with pytest.raises(ValueError, match='max_labels'):
        spot.spot_host(lp, lens, align.star_host(lp, lens, 0.0), np.zeros((1, 128), np.int32), np.array([1], np.int32), blank, 0, 1, 1)


# ------------------------------------------------------------------------------------------------------------------- façade
torch = pytest.importorskip('torch')
_m = None


def model():
    global _m
    if _m is None:
        from nemo.collections.asr.models import EncDecCTCModel
        torch.set_grad_enabled(False)
        _m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
        _m.eval()
        _m.preprocessor.featurizer.dither = 0.0
        _m.set_quant_mode('none')
    return _m


def test_spot_and_spot_long_on_cpu_tensors_equal_the_twins():
    import spot_facade_cases as fc
    fc.check_spot(model(), 'cpu')
    fc.check_spot_long(model(), 'cpu')


def test_refused_arguments_are_refused_by_name():
    import spot_facade_cases as fc
    fc.check_refusals(model(), 'cpu')
