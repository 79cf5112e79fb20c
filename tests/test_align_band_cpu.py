"""Banded CTC alignment on the host: qasr.align.align_band_host (BAND_RULES) against align_host where the full lattice can be
computed, against an independent float64 Viterbi past k_align's label cap, and segment_scores against a plain loop."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_band_cases as bc  # noqa: E402
import align_cases  # noqa: E402
from qasr import align  # noqa: E402
from qasr.beam import NEG, ONE  # noqa: E402

SHARED = ('start', 'nframes', 'score', 'path_score', 'ok')


def _same(got, want, what):
    for f in SHARED:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f)
        if f == 'score':
            g, w = g.view(np.int32), w.view(np.int32)
        assert np.array_equal(g, w), (what, f, np.argwhere(g != w)[:4].tolist())


def _path_logp(lp, lim, y, start, nframes, blank):
    """float32 [T]: the log-probability of the path that start / nframes describe, frame by frame (0 behind lim)"""
    idx = align_cases.path_frames(start, nframes, len(y), lim)
    cls = np.where(idx >= 0, np.asarray(list(y) + [blank])[idx], blank)
    out = np.zeros(lp.shape[0], dtype=np.float32)
    out[:lim] = lp[np.arange(lim), cls]
    return out


@pytest.mark.parametrize('bw', align.BAND_STATES)
@pytest.mark.parametrize('spec', align_cases.FIXTURE_LISTS, ids=lambda s: s[0])
def test_twin_equals_align_host_when_the_band_holds_every_state(spec, bw):
    lp, lens, tg, tl = align_cases.fixture_inputs(spec)
    K = spec[4]
    lp_p, lens_p = np.repeat(lp, K, axis=0), np.repeat(lens, K)               # one problem per recording
    want = align.align_host(lp, lens, tg, tl, spec[1] - 1, problems_per_utt=K, want_total=False)
    got = align.align_band_host(lp_p, lens_p, tg, tl, spec[1] - 1, band_states=bw)
    assert 2 * tg.shape[1] + 1 <= bw and want.ok.any()
    _same(got, want, spec[0])
    assert got.total is None and got.band_states == bw and not got.band_base.any()
    T = lp.shape[1]
    for p in range(len(tl)):
        lim = min(max(int(lens_p[p]), 0), T)
        want_fl = _path_logp(lp_p[p], lim, tg[p, :tl[p]], got.start[p], got.nframes[p], spec[1] - 1) if got.ok[p] else np.zeros(T)
        assert np.array_equal(got.frame_logp[p].view(np.int32), want_fl.astype(np.float32).view(np.int32)), p


@pytest.mark.parametrize('name', list(bc.MOVING))
def test_twin_equals_align_host_with_a_moving_band(name):
    lp, lens, tg, tl = bc.moving_case(name)
    T = lp.shape[1]
    assert T % 4 and T % 32
    want = align.align_host(lp, lens, tg, tl, bc.BLANK, want_total=False)
    got = align.align_band_host(lp, lens, tg, tl, bc.BLANK, band_states=256)
    assert want.ok[0] == 1
    _same(got, want, name)
    base = got.band_base[0]
    lim = T if lens is None else int(lens[0])
    nblk = (lim + 31) // 32                               # the blocks that have a frame < lim; 0 behind
    assert (np.diff(base[:nblk]) >= 0).all() and len(np.unique(base)) >= 5, base      # monotone, and it moves
    assert base.max() <= 2 * int(tl[0]) + 1 - 256 and not base[nblk:].any()
    fl = _path_logp(lp[0], lim, tg[0], got.start[0], got.nframes[0], bc.BLANK)
    assert np.array_equal(got.frame_logp[0].view(np.int32), fl.view(np.int32))
    if name == 'repeats_L600':                            # adjacent repeats do cross a move of the base
        y = tg[0]
        rep = np.flatnonzero(y[1:] == y[:-1]) + 1
        assert len(rep) > 100
    if name == 'dense_L400':
        assert (got.nframes[0] == 1).all()
    if name == 'lead300_L400':
        assert got.start[0, 0] >= 295 and not base[:9].any()


def test_twin_past_k_aligns_label_cap_finds_the_full_lattices_score():
    """L = 2500 (k_align holds 2048), BW = 1024.  One frame's q is within 1 / 2^17 of its log-probability, so a path's fixed-
    point score is within T / 2^17 of its float64 score, and the two optima are within T / 2^16 of each other."""
    lp, y = bc.synth(seed=31, L=2500, a=4.0, per_label=(1, 2), gap=(0, 1), alphabet=10, repeat_p=0.1, lead=10, tail=2)
    T = lp.shape[0]
    assert len(y) > align.MAX_LABELS
    got = align.align_band_host(lp[None], None, np.array([y], dtype=np.int32), np.array([len(y)]), bc.BLANK, band_states=1024)
    assert got.ok[0] == 1 and got.band_base[0].max() == 2 * len(y) + 1 - 1024
    assert align_cases.path_is_valid(got.start[0], got.nframes[0], y, T)
    best = bc.viterbi_f64(lp, y, bc.BLANK)
    walked = float(got.frame_logp[0].astype(np.float64).sum())
    print('fixed', got.path_score[0] / ONE, 'walked float64', walked, 'full lattice float64', best, 'bound', T / ONE)
    assert abs(walked - got.path_score[0] / ONE) <= T / ONE                    # the path it reports is the path it scored
    assert abs(got.path_score[0] / ONE - best) <= T / ONE


def test_rows_that_are_not_alignable_leave_their_neighbours_alone():
    lp1, lens, tg1, tl1 = bc.moving_case('short_lens_L400')
    lp1, y = lp1[0], [int(c) for c in tg1[0]]
    T = lp1.shape[0]
    cut = np.concatenate([lp1[:200], lp1[1200:]])                             # 1000 frames of audio deleted: the band cannot
    cut = np.concatenate([cut, np.repeat(cut[-1:], T - len(cut), axis=0)])    # reach past the labels that have no frames
    lp = np.stack([lp1, lp1, lp1, cut, lp1])
    tg = np.stack([tg1[0]] * 5)
    tl = np.array([400] * 5, dtype=np.int32)
    tg[1, 7] = bc.BLANK                                                       # a blank inside the target
    tg[4, 0] = bc.C                                                           # past the classes
    ln = np.array([int(lens[0]), T, 399, T, T], dtype=np.int32)               # row 2: fewer frames than labels
    full = align.align_host(lp[3:4], None, tg[3:4], tl[3:4], bc.BLANK, want_total=False)
    assert full.ok[0] == 1                                                    # the full lattice still aligns the cut audio:
    got = align.align_band_host(lp, ln, tg, tl, bc.BLANK, band_states=256)    # only the band loses it
    assert got.ok.tolist() == [1, 0, 0, 0, 0]
    alone = align.align_band_host(lp[:1], ln[:1], tg[:1], tl[:1], bc.BLANK, band_states=256)
    for f in SHARED + ('frame_logp', 'band_base'):
        assert np.array_equal(getattr(got, f)[0], getattr(alone, f)[0]), f
    for p in range(1, 5):
        assert got.path_score[p] == NEG
        assert not got.start[p].any() and not got.nframes[p].any() and not got.score[p].any() and not got.frame_logp[p].any()
    assert got.band_base[3].any() and not got.band_base[1].any() and not got.band_base[4].any()   # kept where the path was lost
    hyp = align.to_hypotheses(got, [chr(97 + i) for i in range(bc.C - 1)], 0.02)
    assert hyp[3].utt_score == float('-inf') and hyp[3].start_s == [] and len(hyp[3].text) == 400
    assert len(y) == 400


def test_empty_targets_and_empty_recordings():
    lp, _ = bc.synth(seed=5, L=10, tail=7)
    lp = np.stack([lp, lp])
    tg = np.zeros((2, 4), dtype=np.int32)
    got = align.align_band_host(lp, np.array([0, lp.shape[1]]), tg, np.array([0, 0]), bc.BLANK, band_states=256)
    want = align.align_host(lp, np.array([0, lp.shape[1]]), tg, np.array([0, 0]), bc.BLANK, want_total=False)
    _same(got, want, 'empty')
    assert got.ok.tolist() == [1, 1] and got.path_score[0] == 0 and not got.frame_logp[0].any()
    assert np.array_equal(got.frame_logp[1], lp[1][:, bc.BLANK])


def test_segment_scores_against_a_plain_loop():
    rng = np.random.Generator(np.random.PCG64(9))
    x = (-rng.gamma(1.0, 1.0, size=500)).astype(np.float32)
    f0 = np.array([0, 0, 10, 40, 100, 100, 200, 470, 300, 7])
    f1 = np.array([1, 30, 41, 70, 131, 400, 200, 500, 299, 38])              # 1, 30, 31, 30, 31, 300, 0, 30, -1, 31 frames
    got = align.segment_scores(x, f0, f1)
    assert got.dtype == np.float64
    for i, (a, b) in enumerate(zip(f0, f1)):
        if b <= a:
            want = -np.inf
        elif b - a <= 30:
            want = sum(float(v) for v in x[a:b]) / (b - a)
        else:
            want = min(sum(float(v) for v in x[t:t + 30]) / 30 for t in range(a, b - 29))
        assert got[i] == want or abs(got[i] - want) <= 1e-12 * abs(want), (i, got[i], want)   # float64 sums of 30 terms
    assert got[5] < got[4] + 10 and got[5] <= x[100:400].astype(np.float64).mean()           # the minimum is below the mean


def test_arguments_are_refused_by_name():
    lp = np.zeros((1, 8, 5), dtype=np.float32)
    tg, tl = np.zeros((1, 3), dtype=np.int32), np.array([2])
    for bad in (0, 255, 512, 2048, 4096, -1):
        with pytest.raises(ValueError, match='band_states'):
            align.align_band_host(lp, None, tg, tl, 4, band_states=bad)
    with pytest.raises(ValueError, match='blank'):
        align.align_band_host(lp, None, tg, tl, 5)
    with pytest.raises(ValueError, match='log_probs'):
        align.align_band_host(lp[0], None, tg, tl, 4)
    with pytest.raises(ValueError, match='targets'):
        align.align_band_host(lp, None, np.zeros((2, 3), dtype=np.int32), tl, 4)
    with pytest.raises(ValueError, match='max_labels'):
        align.align_band_host(lp, None, np.zeros((1, 0), dtype=np.int32), tl, 4)
    assert align.pick_band_states(127) == 256 and align.pick_band_states(128) == 1024 and align.pick_band_states(511) == 1024
    assert align.pick_band_states(512) == 4352 and align.pick_band_states(1 << 20) == 4352
    assert align.BAND_MAX_LABELS == 1 << 20 and align.BAND_MAX_FRAMES == 1 << 22 and 'base' in align.BAND_RULES
