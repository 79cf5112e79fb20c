"""CTC forced alignment on the host: qasr.align (the NumPy statement k_align follows) against an independent float64 oracle
and torch's ctc_loss, its link to the greedy collapse, the edge cases of the rules, the facade on host modules and the
fixture that pins it."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases  # noqa: E402
import beam_cases  # noqa: E402
import ctc_cases  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import align, beam, ctc, synth  # noqa: E402
from qasr.beam import NEG, ONE  # noqa: E402


def _one(lp, y, blank, lens=None, want_total=True):
    tg, tl = align_cases.pad_targets([list(y)], blank)
    return align.align_host(lp[None], lens, tg, tl, blank, want_total=want_total)


@pytest.fixture(scope='module')
def solved():
    """every oracle case with the twin's result, computed once"""
    return [(lp, blank, y, o, _one(lp, y, blank)) for lp, blank, y, o in align_cases.oracle_cases()]


def test_total_is_the_ctc_log_likelihood(solved):
    """|total / 2^16 - oracle| and |total / 2^16 + ctc_loss| <= (65.5 T + 33) / 2^16: per frame one rounding of q (0.5 unit)
    and two table look-ups (32.5 units each), lae being 1-Lipschitz, and one more look-up at the end"""
    n = 0
    for lp, blank, y, o, res in solved:
        T = lp.shape[0]
        if o is None:
            assert res.ok[0] == 0 and res.total[0] == NEG
            continue
        assert res.ok[0] == 1
        bound = (65.5 * T + 33) / ONE
        got = res.total[0] / ONE
        loss = torch.nn.functional.ctc_loss(torch.from_numpy(lp.astype(np.float64))[:, None, :], torch.tensor([y], dtype=torch.long),
                                            torch.tensor([T]), torch.tensor([len(y)]), blank=blank, reduction='none')
        print(f'C {lp.shape[1]} T {T} L {len(y)}: total {got:.6f} oracle {o[1]:.6f} ctc_loss {-float(loss[0]):.6f} bound {bound:.4f}')
        assert abs(got - o[1]) <= bound, (got, o[1], bound)
        assert abs(got + float(loss[0])) <= bound, (got, float(loss[0]), bound)
        n += 1
    assert n >= 40


def test_path_score_is_within_rounding_of_the_best_path(solved):
    """the float64 score of the twin's path >= the oracle's best path score - T / 2^16 (rounding moves any path by at most
    half a unit per frame), and the twin's own path_score is the exact integer sum of q along its path"""
    for lp, blank, y, o, res in solved:
        if o is None:
            assert res.ok[0] == 0 and res.path_score[0] == NEG
            continue
        T, L = lp.shape[0], len(y)
        st, nf = res.start[0, :L], res.nframes[0, :L]
        assert align_cases.path_is_valid(st, nf, y, T)
        idx = align_cases.path_frames(st, nf, L, T)
        cls = np.where(idx >= 0, np.asarray(y + [blank], dtype=np.int64)[idx], blank)
        along = lp[np.arange(T), cls]
        f64 = float(along.astype(np.float64).sum())
        print(f'C {lp.shape[1]} T {T} L {L}: path {f64:.6f} oracle best {o[0]:.6f}')
        assert f64 >= o[0] - T / ONE, (f64, o[0])
        assert int(res.path_score[0]) == int(beam.quantize(along).astype(np.int64).sum())
        assert res.total[0] >= res.path_score[0]
        for i in range(L):                                          # the confidence: the label's best frame inside its run
            assert res.score[0, i] == lp[st[i]:st[i] + nf[i], y[i]].max()


@pytest.mark.parametrize('C,T,seed', [(29, 63, 1), (29, 250, 2), (5207, 120, 3), (2, 40, 4)])
def test_aligning_the_greedy_labels_is_the_greedy_collapse(C, T, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    blank = C - 1
    B = 3
    tokens = np.stack([ctc_cases.realistic_row(rng, T, blank) for _ in range(B)]).astype(np.int32)
    lp = np.stack([beam_cases.token_logp(tokens[b], C, seed * 10 + b) for b in range(B)])
    top2 = np.sort(lp, axis=2)[:, :, -2:]
    assert ((top2[:, :, 1] - top2[:, :, 0]) > 2.0 ** -15).all()          # the arg-max path is the unique best path in q too
    assert np.array_equal(lp.argmax(2), tokens)
    lens = np.array([T, T // 2, T + 4], dtype=np.int32)
    fs = np.take_along_axis(lp, tokens[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    want = ctc.collapse_host(tokens, fs, lens, blank=blank)
    ml = max(1, int(want.n_labels.max()))
    res = align.align_host(lp, lens, want.labels[:, :ml], want.n_labels, blank)
    assert res.ok.all()
    assert np.array_equal(res.start, want.start[:, :ml]) and np.array_equal(res.nframes, want.nframes[:, :ml])
    assert np.array_equal(res.score.view(np.int32), want.score[:, :ml].view(np.int32))
    for b in range(B):
        lim = min(int(lens[b]), T)
        assert int(res.path_score[b]) == int(beam.quantize(fs[b, :lim]).astype(np.int64).sum())


def _rows(res, p=0):
    return res.start[p].tolist(), res.nframes[p].tolist(), res.score[p].tolist()


def test_edge_cases_of_the_rules():
    rng = np.random.Generator(np.random.PCG64(7))
    C, T, blank = 5, 9, 4
    lp = np.log(rng.dirichlet(np.ones(C), size=T)).astype(np.float32)
    q = beam.quantize(lp).astype(np.int64)
    # L = 0: every frame is blank
    r = _one(lp, [], blank)
    assert r.ok[0] == 1 and r.path_score[0] == r.total[0] == q[:, blank].sum() and _rows(r) == ([0], [0], [0.0])
    # L = 1 against a brute force over (first frame, frame count)
    r = _one(lp, [2], blank)
    best = max((q[:a, blank].sum() + q[a:a + n, 2].sum() + q[a + n:, blank].sum(), -a, -n) for a in range(T)
               for n in range(1, T - a + 1))
    assert r.ok[0] == 1 and r.path_score[0] == best[0]
    assert q[r.start[0, 0]:r.start[0, 0] + r.nframes[0, 0], 2].sum() + q[:, blank].sum() - \
        q[r.start[0, 0]:r.start[0, 0] + r.nframes[0, 0], blank].sum() == best[0]
    # T = 1
    r = _one(lp[:1], [3], blank)
    assert r.ok[0] == 1 and r.path_score[0] == r.total[0] == q[0, 3] and _rows(r) == ([0], [1], [float(lp[0, 3])])
    r = _one(lp[:1], [], blank)
    assert r.ok[0] == 1 and r.path_score[0] == r.total[0] == q[0, blank]
    assert _one(lp[:1], [1, 2], blank).ok[0] == 0
    # lim = 0
    r = _one(lp, [], blank, lens=np.array([0]))
    assert r.ok[0] == 1 and r.path_score[0] == 0 and r.total[0] == 0
    r = _one(lp, [1], blank, lens=np.array([-3]))
    assert r.ok[0] == 0 and r.path_score[0] == NEG and r.total[0] == NEG and _rows(r) == ([0], [0], [0.0])
    # T exactly L + repeats: one alignment, so path_score == total; one frame short: not alignable
    y = [1, 1, 2, 2, 2, 0]                                          # 6 labels + 3 repeats = 9 frames
    r = _one(lp, y, blank)
    assert r.ok[0] == 1 and r.path_score[0] == r.total[0]
    assert r.start[0].tolist() == [0, 2, 3, 5, 7, 8] and r.nframes[0].tolist() == [1] * 6
    r = _one(lp, y, blank, lens=np.array([8]))
    assert r.ok[0] == 0 and r.path_score[0] == NEG and not r.start.any() and not r.nframes.any() and not r.score.any()
    # lens beyond T clamps
    a, b = _one(lp, [1, 3], blank, lens=np.array([T + 7])), _one(lp, [1, 3], blank)
    assert a.path_score[0] == b.path_score[0] and a.total[0] == b.total[0] and _rows(a) == _rows(b)
    # without total: the same alignment, no forward pass
    c = _one(lp, [1, 3], blank, want_total=False)
    assert c.total is None and c.path_score[0] == b.path_score[0] and _rows(c) == _rows(b)


def test_bad_targets_leave_their_neighbours_alone():
    rng = np.random.Generator(np.random.PCG64(8))
    C, T, blank = 6, 20, 5
    lp = np.log(rng.dirichlet(np.ones(C), size=(2, T))).astype(np.float32)
    good = [[1, 2, 3], [0, 0, 4]]
    tg, tl = align_cases.pad_targets([good[0], [1, blank, 2], [1, C, 2], good[1], [1, -1, 2], [2] * 4], blank)
    tl[5] = 5                                                       # above the row pitch
    res = align.align_host(lp, None, tg, tl, blank, problems_per_utt=3)
    assert res.ok.tolist() == [1, 0, 0, 1, 0, 0]
    for p in (1, 2, 4, 5):
        assert res.path_score[p] == NEG and res.total[p] == NEG and not res.start[p].any() and not res.score[p].any()
    tl2 = tl.copy()
    tl2[4] = -1
    assert align.align_host(lp, None, tg, tl2, blank, problems_per_utt=3).ok.tolist() == [1, 0, 0, 1, 0, 0]
    for p, u in ((0, 0), (3, 1)):
        alone = _one(lp[u], good[p // 3], blank)
        assert res.path_score[p] == alone.path_score[0] and res.total[p] == alone.total[0]
        assert res.start[p, :3].tolist() == alone.start[0].tolist() and res.score[p, :3].tolist() == alone.score[0].tolist()


def test_two_classes_and_values_no_decoder_writes():
    rng = np.random.Generator(np.random.PCG64(9))
    lp = np.log(rng.dirichlet(np.ones(2), size=12)).astype(np.float32)
    r = _one(lp, [0, 0, 0], 1)
    o = align_cases.oracle_align(lp, [0, 0, 0], 1)
    assert r.ok[0] == 1 and abs(r.total[0] / ONE - o[1]) <= (65.5 * 12 + 33) / ONE
    sp = np.log(rng.dirichlet(np.ones(4), size=10)).astype(np.float32)
    sp[2, :] = np.nan
    sp[3, 1] = -np.inf
    sp[4, 3] = np.inf
    sp[5, :] = -np.inf
    r = _one(sp, [1, 0], 3)
    assert r.ok[0] == 1 and NEG < r.path_score[0] <= r.total[0]     # NaN and -inf are the floor -2^30, +inf the ceiling: never NEG
    assert align_cases.path_is_valid(r.start[0], r.nframes[0], [1, 0], 10)
    q = beam.quantize(sp).astype(np.int64)
    idx = align_cases.path_frames(r.start[0], r.nframes[0], 2, 10)
    assert r.path_score[0] == q[np.arange(10), np.where(idx >= 0, np.array([1, 0, 3])[idx], 3)].sum()


def test_host_arguments_are_refused():
    lp = np.zeros((2, 4, 3), dtype=np.float32)
    tg, tl = np.zeros((2, 2), dtype=np.int32), np.ones(2, dtype=np.int32)
    for kw in (dict(blank=3), dict(blank=-1), dict(problems_per_utt=0), dict(problems_per_utt=2)):
        with pytest.raises(ValueError):
            align.align_host(lp, None, tg, tl, **{'blank': 2, **kw})
    with pytest.raises(ValueError):
        align.align_host(lp, None, np.zeros((2, align.MAX_LABELS + 1), dtype=np.int32), tl, 2)


# ------------------------------------------------------------------------------------------------------------ the facade
def _host_model():
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')                                   # float modules on the CPU: the same forward on every call
    return m


def _tuples(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words, h.lm_score, h.ctc_score)


def test_facade_align_on_host_modules():
    m = _host_model()
    vocab = m.decoder.vocabulary
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7))
    lens = torch.tensor([96, 70, 41])
    inputs = dict(processed_signal=x, processed_signal_length=lens)
    with torch.no_grad():
        logp, enc_len, _ = m(**inputs)
    spf = m.seconds_per_frame()
    texts = ['ab c', ' Hello  world', 'a']
    hyps = m.align(**inputs, texts=texts)
    assert [h.text for h in hyps] == ['ab c', 'hello world', 'a']
    ids = [[vocab.index(ch) for ch in h.text] for h in hyps]
    tg, tl = align_cases.pad_targets(ids, len(vocab))
    want = align.align_host(logp.numpy(), enc_len.numpy(), tg, tl, len(vocab))
    for b, h in enumerate(hyps):
        dur = int(enc_len[b]) * spf
        assert h.labels == ids[b] and len(h.start_s) == len(h.end_s) == len(h.score) == len(ids[b])
        assert all(0 <= s < e <= dur + 1e-9 for s, e in zip(h.start_s, h.end_s))
        assert all(h.end_s[i] <= h.start_s[i + 1] for i in range(len(ids[b]) - 1))
        assert h.utt_score == want.path_score[b] / ONE and h.ctc_score == want.total[b] / ONE and h.ctc_score >= h.utt_score
        assert ' '.join(w[0] for w in h.words) == ' '.join(h.text.split())
        for w in h.words:                                           # a word spans its labels
            i = h.text.index(w[0])
            assert w[1] in h.start_s and w[2] in h.end_s and w[1] >= h.start_s[i] - 1e-12
    same = m.align(**inputs, labels=ids)
    assert [_tuples(h) for h in same] == [_tuples(h) for h in hyps]
    # refused before anything runs: a text the parser cannot take, an id outside the vocabulary (each named by its index),
    # both / neither source, a wrong count
    for bad, word in ((dict(texts=['ab', None, 'c']), 'text 1'), (dict(texts=['ab', 'c', 5]), 'text 2'),
                      (dict(labels=[[0], [len(vocab)], [1]]), 'transcript 1'), (dict(labels=[[0], [1], [-1]]), 'transcript 2'),
                      (dict(labels=[[0] * (align.MAX_LABELS + 1), [1], [1]]), 'transcript 0'),
                      (dict(texts=texts, labels=ids), 'exactly one'), (dict(), 'exactly one'), (dict(texts=['a']), '1 transcripts')):
        with pytest.raises(ValueError, match=word):
            m.align(**inputs, **bad)
    # a transcript too long for its utterance is not alignable: no times, scores -inf
    long = m.align(**inputs, texts=['a', 'b', 'abcdefghij' * 6])
    assert long[2].text == 'abcdefghij' * 6 and long[2].start_s == [] and long[2].score is None and long[2].words == []
    assert long[2].utt_score == long[2].ctc_score == float('-inf') and long[0].start_s


def test_facade_beam_timestamps_on_host_modules():
    m = _host_model()
    vocab = m.decoder.vocabulary
    x = torch.from_numpy(synth.make_features(3, 16, 96, 8))
    lens = torch.tensor([96, 64, 30])
    inputs = dict(processed_signal=x, processed_signal_length=lens)
    with torch.no_grad():
        logp, enc_len, _ = m(**inputs)
    plain = m.decode(**inputs, beam_width=4, n_best=2)
    want = beam.to_hypotheses(beam.search_host(logp.numpy(), enc_len.numpy(), len(vocab), 4, 2, 40), vocab)
    assert [[_tuples(h) for h in row] for row in plain] == [[_tuples(h) for h in row] for row in want]      # today's output
    assert [[_tuples(h) for h in row] for row in m.decode(**inputs, beam_width=4, n_best=2, timestamps=False)] == \
        [[_tuples(h) for h in row] for row in plain]
    timed = m.decode(**inputs, beam_width=4, n_best=2, timestamps=True)
    spf = m.seconds_per_frame()
    n_timed = 0
    for b, (row_t, row_p) in enumerate(zip(timed, plain)):
        assert len(row_t) == len(row_p)
        for ht, hp in zip(row_t, row_p):
            assert (ht.text, ht.labels, ht.utt_score, ht.lm_score) == (hp.text, hp.labels, hp.utt_score, hp.lm_score)
            tg, tl = align_cases.pad_targets([hp.labels], len(vocab))
            one = align.to_hypotheses(align.align_host(logp[b:b + 1].numpy(), enc_len[b:b + 1].numpy(), tg, tl, len(vocab),
                                                       want_total=False), vocab, spf)[0]
            assert (ht.start_s, ht.end_s, ht.score, ht.words) == (one.start_s, one.end_s, one.score, one.words)
            assert len(ht.start_s) == len(hp.labels)
            n_timed += len(ht.start_s)
    assert n_timed > 0
    best = m.decode(**inputs, beam_width=4, timestamps=True)
    assert [_tuples(h) for h in best] == [_tuples(row[0]) for row in timed]
    assert [(h.text, h.utt_score) for h in best] == [(row[0].text, row[0].utt_score) for row in plain]
    assert all(len(h.start_s) == len(h.labels) for h in best)


def test_to_hypotheses_of_a_row_that_is_not_alignable():
    res = align.AlignResult(np.array([[0, 1], [7, 7]], dtype=np.int32), np.array([2, 2], dtype=np.int32),
                            np.array([[0, 2], [0, 0]], dtype=np.int32), np.array([[1, 3], [0, 0]], dtype=np.int32),
                            np.array([[-0.5, -0.25], [0, 0]], dtype=np.float32), np.array([-3 * ONE, NEG]), np.array([-2 * ONE, NEG]),
                            np.array([1, 0], dtype=np.int32), 2)
    a, b = align.to_hypotheses(res, ['x', ' '], 0.02)
    assert (a.text, a.start_s, a.end_s, a.score, a.utt_score, a.ctc_score) == ('x ', [0.0, 0.04], [0.02, 0.1], [-0.5, -0.25], -3.0, -2.0)
    assert a.words == [('x', 0.0, 0.02, -0.5)]
    assert (b.labels, b.start_s, b.end_s, b.score, b.words, b.utt_score, b.ctc_score) == ([7, 7], [], [], None, [], -np.inf, -np.inf)


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_pins_the_twin(golden_dir):
    d = np.load(os.path.join(golden_dir, 'align.npz'))
    meta = json.loads(str(d['meta']))
    assert [c['name'] for c in meta['cases']] == [s[0] for s in align_cases.FIXTURE_LISTS]
    for spec in align_cases.FIXTURE_LISTS:
        name, C, T, B, K, seed = spec
        lp, lens, tg, tl = align_cases.fixture_inputs(spec)
        assert np.array_equal(tg, d['targets_' + name]) and np.array_equal(lens, d['lens_' + name])
        assert np.array_equal(np.take_along_axis(lp, d['probe_' + name].astype(np.int64), axis=2).view(np.int32),
                              d['probe_lp_' + name].view(np.int32))                 # the seeded inputs are what they were
        res = align.align_host(lp, lens, tg, tl, C - 1, problems_per_utt=K)
        for f in ('start', 'nframes', 'score', 'path_score', 'total', 'ok'):
            got, want = getattr(res, f), d[f + '_' + name]
            assert got.dtype == want.dtype and np.array_equal(got.view(np.int32) if f == 'score' else got,
                                                              want.view(np.int32) if f == 'score' else want), (name, f)
        assert res.ok.sum() >= B
