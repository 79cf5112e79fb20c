"""CTC posteriors along an alignment on the host: qasr.align.post_host (the NumPy statement k_post follows) against an
independent float64 forward-backward and a brute-force enumeration, its exact cases, the star identity, invalid rows and the
facade on host modules."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases  # noqa: E402
import post_cases as pc  # noqa: E402
import star_cases as sc  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import align, synth  # noqa: E402
from qasr.beam import NEG, ONE, Q_FLOOR  # noqa: E402


def _one(lp, y, blank):
    tg, tl = align_cases.pad_targets([list(y)], blank)
    return pc.align_and_post(lp[None], None, tg, tl, blank)


# ------------------------------------------------------------------------------------------------------ total equality
@pytest.mark.parametrize('spec', align_cases.FIXTURE_LISTS, ids=[s[0] for s in align_cases.FIXTURE_LISTS])
def test_total_is_align_hosts_total_on_every_byte(spec):
    lp, lens, tg, tl = align_cases.fixture_inputs(spec)
    K, blank = spec[4], spec[1] - 1
    for use_lens in (lens, None):
        res, post = pc.align_and_post(lp, use_lens, tg, tl, blank, K)
        assert post.total.dtype == np.int64 and post.total.tobytes() == res.total.tobytes()
        assert post.ok.dtype == np.int32 and post.ok.tobytes() == res.ok.tobytes() and res.ok.sum() >= len(tl) // 2
        assert post.frame_post.dtype == np.int32 and post.frame_post.shape == (len(tl), lp.shape[1]) and post.frame_post.max() <= 0
        assert post.label_post.dtype == np.int32 and post.label_post.shape == tg.shape
        for p in range(len(tl)):
            lim = lp.shape[1] if use_lens is None else min(int(use_lens[p // K]), lp.shape[1])
            assert not post.frame_post[p, lim:].any() and not post.label_post[p, max(int(tl[p]), 0):].any()
            if post.ok[p]:
                for i in range(int(tl[p])):
                    a, n = int(res.start[p, i]), int(res.nframes[p, i])
                    assert post.label_post[p, i] == post.frame_post[p, a:a + n].min()


# ------------------------------------------------------------------------------------------------------ float64 oracle
def test_the_oracle_passes_its_own_check():
    """per frame the posteriors over all states sum to 1"""
    n = 0
    for lp, blank, y, o in align_cases.oracle_cases()[::5]:
        if o is None:
            continue
        gamma, total = pc.oracle_post(lp, y, blank)
        assert abs(total - o[1]) <= 1e-9 * max(1.0, abs(total))
        assert np.abs(np.exp(gamma).sum(axis=1) - 1.0).max() <= 1e-9
        n += 1
    assert n >= 8


def test_frame_post_against_the_float64_oracle():
    """Along the twin's path |frame_post / 2^16 - oracle| <= 131 lim / 2^16 nat wherever the clamp is inactive.  g = A + Bk - q -
    total.  One frame of either pass rounds q once (0.5 unit) and looks the table up twice (32.5 units each: half a unit of the
    entry's rounding, 32 of its 64-unit step, the slope of log1p(exp(-x)) being at most 1 / 2); lae is 1-Lipschitz, so errors add
    and never grow: e_A(t) <= 0.5 + 65.5 t, e_B(t) <= 0.5 + 65.5 (lim - 1 - t).  q itself is off by half a unit, and total by
    e_A(lim - 1) + 32.5 = 65.5 lim - 32.5.  Together: 0.5 + 0.5 + 65.5 (lim - 1) + 0.5 + 65.5 lim - 32.5 < 131 lim units.
    The cases are finite log-probabilities far above the floor of q, so q's clamp plays no part."""
    n, worst, worst_share = 0, 0.0, 0.0
    for lp, blank, y, o in align_cases.oracle_cases():
        res, post = _one(lp, y, blank)
        if o is None:
            assert post.ok[0] == 0 and post.total[0] == NEG and not post.frame_post.any() and not post.label_post.any()
            continue
        T, L = lp.shape[0], len(y)
        assert post.ok[0] == 1 and post.total[0] == res.total[0]
        gamma, total = pc.oracle_post(lp, y, blank)
        states = pc.path_states(res.start[0], res.nframes[0], L, T)
        want = gamma[np.arange(T), states]
        fp = post.frame_post[0].astype(np.int64)
        free = (fp < 0) & (fp > Q_FLOOR)                            # the clamp is inactive
        assert (want[~free] >= -pc.bound(T)).all()                  # where it clamped to 0 the truth is that close to 0
        diff = float(np.abs(fp[free] / ONE - want[free]).max()) if free.any() else 0.0
        print(f'C {lp.shape[1]} T {T} L {L}: largest |frame_post - oracle| {diff:.6f} nat, bound {pc.bound(T):.4f}, '
              f'{int((~free).sum())} frames at the clamp')
        assert diff <= pc.bound(T), (diff, pc.bound(T))
        worst, worst_share = max(worst, diff), max(worst_share, diff / pc.bound(T))
        n += 1
    print(f'largest difference {worst:.6f} nat; largest share of the bound {100 * worst_share:.2f} %')
    assert n >= 40


# --------------------------------------------------------------------------------------------------------- brute force
def test_small_cases_against_every_alignment_enumerated():
    rng = np.random.Generator(np.random.PCG64(71))
    n = 0
    for T, L, C in [(1, 0, 2), (1, 1, 2), (3, 1, 2), (5, 2, 3), (5, 3, 4), (8, 3, 4), (8, 2, 2), (7, 3, 2), (8, 0, 3), (6, 3, 3)]:
        for rep in range(3):
            blank = C - 1
            lp = np.log(rng.dirichlet(np.ones(C), size=T)).astype(np.float32)
            y = sc.labels_without_blank(rng, L, C, blank, repeats=0.4)
            res, post = _one(lp, y, blank)
            mass, n_paths = pc.brute_post(lp, y, blank)
            if mass is None:
                assert post.ok[0] == 0 and n_paths == 0
                continue
            assert post.ok[0] == 1 and n_paths >= 1
            gamma, _ = pc.oracle_post(lp, y, blank)
            states = pc.path_states(res.start[0], res.nframes[0], L, T)
            exact = mass[np.arange(T), states]
            assert np.abs(np.exp(gamma[np.arange(T), states]) - exact).max() <= 1e-9
            assert np.abs(post.frame_post[0] / ONE - np.log(exact)).max() <= pc.bound(T), (T, L, C, rep)
            n += 1
    assert n >= 20


# --------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize('C,T', [(2, 1), (29, 37), (5, 300)])
def test_an_empty_target_has_one_path(C, T):
    rng = np.random.Generator(np.random.PCG64(T))
    lp = np.log(rng.dirichlet(np.ones(C), size=T)).astype(np.float32)
    res, post = _one(lp, [], C - 1)
    assert post.ok[0] == 1 and post.total[0] == res.total[0] == res.path_score[0]
    assert not post.frame_post.any() and not post.label_post.any()


@pytest.mark.parametrize('L', [1, 2, 40])
def test_equal_labels_on_the_fewest_frames_have_one_path(L):
    T, C, blank = 2 * L - 1, 3, 2
    rng = np.random.Generator(np.random.PCG64(L))
    lp = np.log(rng.dirichlet(np.ones(C), size=T)).astype(np.float32)
    res, post = _one(lp, [1] * L, blank)
    assert post.ok[0] == 1 and res.nframes[0, :L].tolist() == [1] * L
    assert post.total[0] == res.path_score[0]
    assert not post.frame_post.any() and not post.label_post.any()


def test_no_frames_and_no_labels():
    lp = np.zeros((2, 4, 3), dtype=np.float32)
    tg, tl = align_cases.pad_targets([[], [1]], 2)
    res, post = pc.align_and_post(lp, np.array([0, 0]), tg, tl, 2)
    assert post.ok.tolist() == [1, 0] and post.total.tolist() == [0, NEG] and not post.frame_post.any()


# --------------------------------------------------------------------------------------------------- planted ambiguity
def test_six_equally_likely_paths():
    """T = 3, one label, uniform over {label, blank}: the paths are a--, aa-, aaa, -a-, -aa, --a, all equally likely.  Whichever
    of them the tie order picks, every frame's posterior is (paths through its state) / 6"""
    lp = np.full((3, 2), math.log(0.5), dtype=np.float32)
    res, post = _one(lp, [0], 1)
    assert post.ok[0] == 1
    mass, n_paths = pc.brute_post(lp, [0], 1)
    assert n_paths == 6
    states = pc.path_states(res.start[0], res.nframes[0], 1, 3)
    through = np.rint(mass[np.arange(3), states] * 6).astype(int)
    assert through.tolist() == [{0: 3, 1: 3}[states[0]], {0: 1, 1: 4, 2: 1}[states[1]], {1: 3, 2: 3}[states[2]]]
    want = np.log(through / 6.0)
    got = post.frame_post[0] / ONE
    print('states', states.tolist(), 'paths through', through.tolist(), 'frame_post', got.tolist())
    assert np.abs(got - want).max() <= pc.bound(3)
    a, n = int(res.start[0, 0]), int(res.nframes[0, 0])
    assert post.label_post[0, 0] == post.frame_post[0, a:a + n].min()


# ------------------------------------------------------------------------------------------------------- star identity
@pytest.mark.parametrize('K', [1, 2])
def test_post_host_with_a_plane_is_post_host_on_the_augmented_matrix(K):
    C, T, B, blank = 29, 60, 3, 28
    rng = np.random.Generator(np.random.PCG64(31))
    lp = sc.logp(rng, B, T, C, blank)
    lens = np.array([T, 41, 1], dtype=np.int32)
    star = align.star_host(lp, lens, 1.5)
    aug = sc.augmented(lp, star)
    n_ok = 0
    for n in (1, 6, 14):
        tg, tl = sc.position_targets(rng, n, C, blank, pitch=20)
        for r in range(0, len(sc.POSITIONS), 3 * K):
            rows = [(r + i) % len(sc.POSITIONS) for i in range(3 * K)]
            for use_lens in (lens, None):
                res, got = pc.align_and_post(lp, use_lens, tg[rows], tl[rows], blank, K, star=star)
                res2, want = pc.align_and_post(aug, use_lens, tg[rows], tl[rows], blank, K)
                sc.same_bytes(res, res2, sc.ALIGN_FIELDS)
                sc.same_bytes(got, want, pc.POST_FIELDS, (n, rows))
                n_ok += int(got.ok.sum())
                # without the plane the wildcard's id is a label outside [0, C): the row is refused, the path notwithstanding
                bare = align.post_host(lp, use_lens, tg[rows], tl[rows], blank, res.start, res.nframes, res.ok, problems_per_utt=K)
                assert not bare.ok.any() and not bare.frame_post.any() and (bare.total == NEG).all()
    assert n_ok >= 20


# -------------------------------------------------------------------------------------------------------- invalid rows
def test_invalid_rows_are_zero_and_leave_the_others_alone():
    C, T, blank, K = 29, 50, 28, 2
    rng = np.random.Generator(np.random.PCG64(11))
    lp = sc.logp(rng, 2, T, C, blank)
    lens = np.array([T, 44], dtype=np.int32)
    rows = [sc.labels_without_blank(rng, n, C, blank) for n in (12, 9, 20, 5)]
    rows[2][1] = rows[2][2]                                         # a repeat at labels 1, 2 of the row that will be broken
    tg, tl = align_cases.pad_targets(rows, blank)
    res, good = pc.align_and_post(lp, lens, tg, tl, blank, K)
    assert res.ok.all() and good.ok.all() and good.frame_post.min() < 0
    for name, (st, nf, ok) in pc.invalid_paths(res, tg, tl, 2, 44).items():
        assert not align_cases.path_is_valid(st[2, :20], nf[2, :20], rows[2], 44) or name == 'ok_in = 0', name
        got = align.post_host(lp, lens, tg, tl, blank, st, nf, ok, problems_per_utt=K)
        assert got.ok.tolist() == [1, 1, 0, 1], name
        assert got.total[2] == NEG and not got.frame_post[2].any() and not got.label_post[2].any(), name
        for p in (0, 1, 3):
            for f in pc.POST_FIELDS:
                assert getattr(got, f)[p].tobytes() == getattr(good, f)[p].tobytes(), (name, p, f)
    # the targets align_host refuses are refused here, whatever the path says
    for bad_tl in (None, -1, tg.shape[1] + 1):
        tg2, tl2 = tg.copy(), tl.copy()
        if bad_tl is None:
            tg2[2, 3] = blank                                       # a blank inside the target
        else:
            tl2[2] = bad_tl
        got = align.post_host(lp, lens, tg2, tl2, blank, res.start, res.nframes, None, problems_per_utt=K)
        assert got.ok.tolist() == [1, 1, 0, 1] and got.total[2] == NEG and not got.frame_post[2].any()
    with pytest.raises(ValueError, match='start / nframes'):
        align.post_host(lp, lens, tg, tl, blank, res.start[:, :5], res.nframes, res.ok, problems_per_utt=K)


# ---------------------------------------------------------------------------------------------------------- the facade
_m = None


def _model():
    global _m
    if _m is None:
        _m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
        _m.eval()
        _m.preprocessor.featurizer.dither = 0.0
        _m.set_quant_mode('none')                                   # float modules on the CPU: the same forward on every call
    return _m


def _tuples(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words, h.lm_score, h.ctc_score, h.segments, h.seams_s)


def _inputs():
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7))
    return dict(processed_signal=x, processed_signal_length=torch.tensor([96, 70, 41]))


def _check_fields(h, fp_row, start, nframes, lim):
    n = len(h.labels)
    assert h.frame_post.dtype == np.float32 and h.frame_post.tolist() == (fp_row[:lim] / ONE).astype(np.float32).tolist()
    assert len(h.post) == len(h.post_min) == n and len(h.word_post) == len(h.words)
    pr = np.exp(fp_row[:lim].astype(np.float64) / ONE)
    for i in range(n):
        run = pr[start[i]:start[i] + nframes[i]]
        assert h.post[i] == float(run.mean()) and h.post_min[i] == float(run.min())
        assert 0.0 <= h.post_min[i] <= h.post[i] <= 1.0
    assert all(0.0 <= w <= 1.0 for w in h.word_post)


def test_facade_align_with_posteriors_on_host_modules():
    m = _model()
    vocab = list(m.decoder.vocabulary)
    blank = len(vocab)
    inputs = _inputs()
    with torch.no_grad():
        logp, enc_len, _ = m(**inputs)
    texts = ['ab c', 'hello you', 'a']
    hyps = m.align(**inputs, texts=texts, posteriors=True)
    rows = [[vocab.index(ch) for ch in t] for t in texts]
    tg, tl = align_cases.pad_targets(rows, blank)
    res, post = pc.align_and_post(logp.numpy(), enc_len.numpy(), tg, tl, blank)
    assert res.ok.all() and post.ok.all()
    for b, h in enumerate(hyps):
        _check_fields(h, post.frame_post[b], res.start[b], res.nframes[b], int(enc_len[b]))
        assert h.ctc_score == post.total[b] / ONE
    # a word's value is the mean over the frames of its labels: 'ab' of 'ab c' is labels 0 and 1
    pr = np.exp(post.frame_post[0].astype(np.float64) / ONE)
    fr = np.concatenate([pr[res.start[0, i]:res.start[0, i] + res.nframes[0, i]] for i in (0, 1)])
    assert [w[0] for w in hyps[0].words] == ['ab', 'c'] and hyps[0].word_post[0] == float(fr.mean())
    # without the argument, and with it False, the call is the one it was and the new fields are None
    plain = m.align(**inputs, texts=texts)
    assert [_tuples(h) for h in plain] == [_tuples(h) for h in hyps]
    assert [_tuples(h) for h in m.align(**inputs, texts=texts, posteriors=False)] == [_tuples(h) for h in plain]
    assert all(h.post is None and h.post_min is None and h.word_post is None and h.frame_post is None for h in plain)
    # with a wildcard: the token is a word of its own and has a value too
    star = m.align(**inputs, texts=['ab * c', '* hello', 'a'], star='*', star_penalty=1.5, posteriors=True)
    assert [w[0] for w in star[0].words] == ['ab', '*', 'c'] and len(star[0].word_post) == 3
    assert all(0.0 <= v <= 1.0 for h in star for v in h.post + h.word_post)
    # a transcript that cannot be aligned: empty lists
    long_row = [[1, 2] * 40, rows[1], rows[2]]
    bad = m.align(**inputs, labels=long_row, posteriors=True)
    assert bad[0].start_s == [] and bad[0].post == [] and bad[0].post_min == [] and bad[0].word_post == [] and len(bad[0].frame_post) == 0
    assert bad[1].post == hyps[1].post


def test_facade_decode_with_posteriors_on_host_modules():
    m = _model()
    inputs = _inputs()
    hyps = m.decode(**inputs, beam_width=4, n_best=2, timestamps=True, posteriors=True)
    plain = m.decode(**inputs, beam_width=4, n_best=2, timestamps=True)
    assert len(hyps) == 3
    with torch.no_grad():
        _, enc_len, _ = m(**inputs)
    for b, (row, prow) in enumerate(zip(hyps, plain)):
        assert [_tuples(h) for h in row] == [_tuples(h) for h in prow] and len(row) >= 1
        for h, ph in zip(row, prow):
            assert len(h.post) == len(h.labels) and len(h.word_post) == len(h.words) and len(h.frame_post) == int(enc_len[b])
            assert all(0.0 <= v <= 1.0 for v in h.post + h.post_min + h.word_post)
            assert ph.post is None and ph.frame_post is None
    with pytest.raises(ValueError, match='posteriors needs beam_width'):
        m.decode(**inputs, posteriors=True)
    with pytest.raises(ValueError, match='posteriors needs beam_width'):
        m.decode(**inputs, timestamps=True, posteriors=True)
    with pytest.raises(ValueError, match='posteriors needs timestamps'):
        m.decode(**inputs, beam_width=4, posteriors=True)
