"""CTC prefix beam search on the host (qasr/beam.py): answers worked by hand, cutoff_top_n = 1 against the greedy collapse,
the fixed-point twin against an independent float64 search (tests/beam_cases.py), the pinned fixture
tests/golden/beam.npz, and BeamSearchDecoderWithLM / decode(beam_width=) on the host."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_cases  # noqa: E402
import ctc_cases  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from nemo.collections.asr.modules import BeamSearchDecoderWithLM  # noqa: E402
from qasr import beam, ctc  # noqa: E402

torch.set_grad_enabled(False)


def _bound(T):
    """What the fixed-point score of one prefix may be off by, in nats, derived: d >> 6 drops fewer than 64 units and
    |d/dd log1p(e^-d)| <= 1/2, so a look-up is off by at most 32.5 units of 2^-16; a score passes through at most three
    look-ups per frame, and q adds half a unit."""
    return 100.0 * T / 65536.0


def _hyps(res, b=0):
    return [(tuple(res.labels[b, h, :res.n_labels[b, h]].tolist()), int(res.score[b, h])) for h in range(int(res.n_hyps[b]))]


def _logp(rows):
    return np.log(np.asarray(rows, dtype=np.float64)).astype(np.float32)[None]


# -------------------------------------------------------------------------------------------------- the arithmetic
def test_table_and_lae():
    tab = beam.lae_table()
    assert tab.dtype == np.uint16 and tab.shape == (16384,) and tab[0] == 45426 and tab.max() == 45426
    assert (np.diff(tab.astype(np.int64)) <= 0).all() and tab[-1] == 0
    N = beam.NEG
    assert beam.lae(N, N) == N and beam.lae(N, -5) == -5 and beam.lae(-7, N) == -7
    assert beam.lae(0, 0) == 45426 and beam.lae(0, -63) == 45426 and beam.lae(0, -64) == int(tab[1])
    assert beam.lae(-100, -100 - 16 * 65536) == -100 and beam.lae(-100, -100 - 16 * 65536 + 1) == -100 + int(tab[-1])
    rng = np.random.default_rng(0)
    a, b = rng.integers(-(1 << 24), 0, 4000), rng.integers(-(1 << 24), 0, 4000)
    assert np.array_equal(beam.lae(a, b), beam.lae(b, a))
    err = np.abs(beam.lae(a, b) / 65536.0 - np.logaddexp(a / 65536.0, b / 65536.0))
    assert err.max() <= 33.0 / 65536.0


def test_quantize():
    x = np.array([0.0, -0.0, -1.0, -100.0, -1e-6, 2.5 / 65536, 3.5 / 65536, np.nan, -np.inf, np.inf, -20000.0, 20000.0], dtype=np.float32)
    q = beam.quantize(x)
    assert q.dtype == np.int32
    assert q.tolist() == [0, 0, -65536, -6553600, 0, 2, 4, beam.Q_FLOOR, beam.Q_FLOOR, beam.Q_CEIL, beam.Q_FLOOR, beam.Q_CEIL]


def test_topn_host_order_and_fill():
    lp = np.array([[[-1.0, -0.5, -0.5, -3.0, -0.0, 0.0]], [[-1.0, -2.0, -3.0, -4.0, -5.0, -6.0]]], dtype=np.float32)
    cid, cq = beam.topn_host(lp, 4, np.array([1, 0]))
    assert cid[0, 0].tolist() == [5, 4, 1, 2]                   # +0 above -0; equal values: the lower class first
    assert cq[0, 0].tolist() == [0, 0, -32768, -32768]
    assert (cid[1] == -1).all() and (cq[1] == beam.EMPTY_Q).all()
    cid, cq = beam.topn_host(lp, 8)                              # N > C: the rest stays empty
    assert cid[1, 0].tolist() == [0, 1, 2, 3, 4, 5, -1, -1] and cq[1, 0, 6:].tolist() == [beam.EMPTY_Q] * 2
    for bad in (0, 65):
        with pytest.raises(ValueError, match='64'):
            beam.topn_host(lp, bad)


# -------------------------------------------------------------------------------------------------- 1. known answers
def test_two_frames_worked_by_hand():
    """frames {a 0.35, b 0.25, blank 0.4} twice: "a" 0.4025, "b" 0.2625, "" 0.16, "ab" and "ba" 0.0875 (greedy says "")"""
    lp = _logp([[0.35, 0.25, 0.4]] * 2)
    got = _hyps(beam.search_host(lp, None, 2, beam_width=16))
    assert [g[0] for g in got] == [(0,), (1,), (), (0, 1), (1, 0)]
    for (_, s), p in zip(got, [0.4025, 0.2625, 0.16, 0.0875, 0.0875]):
        assert abs(s / 65536.0 - math.log(p)) <= _bound(2)
    assert got[3][1] == got[4][1]                                # an exact tie: the extension of the better entry comes first
    assert beam_cases.greedy(lp[0], 2) == ()


def test_small_known_answers():
    a, blank = [0.9, 0.04, 0.06], [0.05, 0.05, 0.9]
    best = lambda rows, **kw: _hyps(beam.search_host(_logp(rows), None, 2, **kw))[0][0]    # noqa: E731
    assert best([a, a], beam_width=8) == (0,)
    assert best([a, blank, a], beam_width=8) == (0, 0)
    assert best([a], beam_width=8) == (0,)                       # T = 1
    assert best([blank] * 7, beam_width=8) == ()                 # all blank
    assert best([a, blank, a], beam_width=1) == (0, 0)           # W = 1
    res = beam.search_host(_logp([a, a, a]), np.array([0]), 2, beam_width=8)            # length 0
    assert _hyps(res) == [((), 0)] and (res.labels == 2).all() and res.score[0, 1] == beam.NEG
    res = beam.search_host(_logp([blank] * 3), None, 2, beam_width=1)
    assert _hyps(res) == [((), 3 * int(beam.quantize(np.log(np.float32(0.9)))))]


def test_arguments_are_checked():
    cid, cq = beam.topn_host(_logp([[0.5, 0.5]]), 2)
    for kw, word in ((dict(beam_width=0), '128'), (dict(beam_width=129), '128'), (dict(beam_width=4, n_best=5), 'n_best'),
                     (dict(beam_width=4, n_best=0), 'n_best')):
        with pytest.raises(ValueError, match=word):
            beam.beam_search_host(cid, cq, None, 1, **kw)
    with pytest.raises(ValueError, match='blank'):
        beam.beam_search_host(cid, cq)


def test_n_best_is_a_prefix_of_the_beam():
    lp = beam_cases.case_list('en_t63_w16_n40')[0][0][None]
    full = beam.search_host(lp, None, 28, 16)
    for nb in (1, 3, 16):
        part = beam.search_host(lp, None, 28, 16, nb)
        assert np.array_equal(part.labels, full.labels[:, :nb]) and np.array_equal(part.score, full.score[:, :nb])
        assert part.n_hyps[0] == min(nb, full.n_hyps[0])


# -------------------------------------------------------------------------------------------------- 2. N = 1 is greedy
@pytest.mark.parametrize('n_labels', [28, 5206])
def test_cutoff_top_n_1_is_the_greedy_collapse(n_labels):
    C = n_labels + 1
    rows = [r for T in (1, 65) for r in ctc_cases.token_matrix(5, T, n_labels)]
    lps = [beam_cases.token_logp(r, C, 7 + i) for i, r in enumerate(rows)]
    rng = np.random.Generator(np.random.PCG64(11))
    lps += [beam_cases.peaky_logp(rng, 120, C, n_labels) for _ in range(10 if n_labels == 28 else 3)]
    for lp in lps:
        tok = lp.argmax(1).astype(np.int32)
        for W in (1, 8):
            res = beam.search_host(lp[None], None, n_labels, W, None, cutoff_top_n=1)
            want = ctc.collapse_host(tok[None], blank=n_labels)
            assert res.n_hyps[0] == 1 and res.n_labels[0, 0] == want.n_labels[0]
            assert np.array_equal(res.labels[0, 0], want.labels[0])
            assert int(res.score[0, 0]) == int(beam.quantize(lp[np.arange(len(tok)), tok]).astype(np.int64).sum())


# -------------------------------------------------------------------------------------------------- 3. twin vs float64
@pytest.mark.parametrize('name', [s[0] for s in beam_cases.CASE_LISTS])
def test_twin_against_the_float64_search(name):
    """(a) no case left out: the twin's best string is in the oracle's final beam, its float64 score no lower than the oracle's
    best minus 100 T / 2^16, and the twin's own score for it within the same distance.  (b) the best strings are equal, except
    where the oracle's top-1 / top-2 gap is below 0.002; at most 10 % of a list may be waived that way."""
    cases = beam_cases.checked_case_list(name)                   # runs the oracle and asserts the 10 % cap on waivers
    waived = differ = ne_greedy = 0
    worst = 0.0
    for lp, blank, W, N, want, gap in cases:
        T = lp.shape[0]
        got = _hyps(beam.search_host(lp[None], None, blank, W, None, N))
        in_beam = dict(want)
        best, score = got[0]
        assert best in in_beam, name
        assert in_beam[best] >= want[0][1] - _bound(T)
        assert abs(score / 65536.0 - in_beam[best]) <= _bound(T)
        worst = max(worst, abs(score / 65536.0 - in_beam[best]))
        if gap < beam_cases.GAP:
            waived += 1
        else:
            assert best == want[0][0], (name, gap)
        differ += best != want[0][0]
        ne_greedy += want[0][0] != beam_cases.greedy(lp, blank)
    print(f'{name}: {len(cases)} cases, gap < {beam_cases.GAP}: {waived}, best strings differ: {differ}, beam != greedy: {ne_greedy}, '
          f'largest |score - float64| {worst:.5f}')
    assert waived <= beam_cases.MAX_WAIVED * len(cases), 'sharpen the input of this list; the cap and the gap stay'
    if name == 'zh_t250_w16_n20_blend':
        assert 3 * ne_greedy >= len(cases)


# -------------------------------------------------------------------------------------------------- 4. the fixture
def test_fixture_pins_the_twin_and_the_oracle(golden_dir):
    d = np.load(os.path.join(golden_dir, 'beam.npz'))
    cases = json.loads(str(d['meta']))['cases']
    assert {c['classes'] for c in cases} == {29, 5207} and [c['name'] for c in cases] == [s[0] for s in beam_cases.FIXTURE_LISTS]
    for c in cases:
        n = c['name']
        lp = beam_cases.dense(d['top_id_' + n], d['top_lp_' + n], c['classes'])
        assert np.array_equal(beam.topn_host(lp, c['N'])[0], d['top_id_' + n])
        spec = next(s for s in beam_cases.FIXTURE_LISTS if s[0] == n)
        full, lens = beam_cases.fixture_inputs(spec)                 # the fixture is what tests/beam_cases.py generates
        assert np.array_equal(lens, d['lens_' + n]) and np.array_equal(beam.topn_host(full, c['N'])[0], d['top_id_' + n])
        cid, cq = beam.topn_host(lp, c['N'], d['lens_' + n])
        res = beam.beam_search_host(cid, cq, d['lens_' + n], c['classes'] - 1, c['W'])
        for f in ('labels', 'n_labels', 'score', 'n_hyps'):
            assert np.array_equal(getattr(res, f), d[f'{f}_{n}']), (n, f)
            assert getattr(res, f).dtype == d[f'{f}_{n}'].dtype
        want = json.loads(str(d['oracle_' + n]))
        for b, rec in enumerate(want):
            L = int(min(d['lens_' + n][b], lp.shape[1]))
            got = beam_cases.oracle_beam(lp[b, :L], c['W'], c['N'], c['classes'] - 1)
            assert [list(p) for p, _ in got] == [r[0] for r in rec]
            np.testing.assert_allclose([s for _, s in got], [r[1] for r in rec], rtol=1e-9, atol=1e-9)


# -------------------------------------------------------------------------------------------------- 5. the module
VOCAB = list("abcdefghijklmnopqrstuvwxyz '")


def test_module_refusals():
    ok = dict(vocab=VOCAB, beam_width=16, alpha=2.0, beta=1.0, lm_path=None, num_cpus=4)
    BeamSearchDecoderWithLM(**ok)
    with pytest.raises(ModuleNotFoundError, match='ctc_decoders'):
        BeamSearchDecoderWithLM(**dict(ok, lm_path='lm.binary'))
    with pytest.raises(ValueError, match='1.0'):
        BeamSearchDecoderWithLM(**ok, cutoff_prob=0.99)
    with pytest.raises(ValueError, match='128'):
        BeamSearchDecoderWithLM(**dict(ok, beam_width=129))
    with pytest.raises(ValueError, match='64'):
        BeamSearchDecoderWithLM(**ok, cutoff_top_n=65)
    with pytest.raises(ValueError, match='classes'):
        BeamSearchDecoderWithLM(**ok, input_tensor=True)(torch.zeros(1, 4, 5), torch.tensor([4]))


def test_module_on_the_host_both_input_forms():
    rng = np.random.Generator(np.random.PCG64(3))
    lp = np.stack([beam_cases.peaky_logp(rng, 80, 29, 28) for _ in range(3)])
    lens = np.array([80, 41, 0])
    want = beam.to_hypotheses(beam.search_host(lp, lens, 28, 8, None, 20), VOCAB)
    assert [len(w) for w in want][2] == 1 and len(want[0]) == 8
    dec = BeamSearchDecoderWithLM(VOCAB, 8, 0.0, 0.0, None, 1, cutoff_top_n=20, input_tensor=True)
    got = dec(torch.from_numpy(lp), torch.from_numpy(lens))
    assert got == [[(h.utt_score, h.text) for h in w] for w in want]
    assert all(isinstance(s, float) and isinstance(t, str) for s, t in got[0]) and got[2] == [(0.0, '')]
    assert [s for s, _ in got[0]] == sorted((s for s, _ in got[0]), reverse=True)
    # the reference's other form: a list of probability arrays cut at their lengths
    dec = BeamSearchDecoderWithLM(VOCAB, 8, 0.0, 0.0, None, 1, cutoff_top_n=20)
    probs = [np.exp(lp[b, :lens[b]].astype(np.float64)).astype(np.float32) for b in range(2)]
    got2 = dec(probs, None)
    want2 = beam.to_hypotheses(beam.search_host(np.stack([np.log(np.pad(p, ((0, 80 - len(p)), (0, 0)), constant_values=1.0)) for p in probs]),
                                                lens[:2], 28, 8, None, 20), VOCAB)
    assert got2 == [[(h.utt_score, h.text) for h in w] for w in want2]
    assert [t for _, t in got2[0]][0] == got[0][0][1]            # exp and log in float32 move scores, not this best string


def test_facade_decode_with_a_beam_on_the_host_modules():
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')
    from qasr import synth
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7))
    lens = torch.tensor([96, 61, 12])
    logp, enc_len, _ = m(processed_signal=x, processed_signal_length=lens)
    greedy = m.decode(processed_signal=x, processed_signal_length=lens)
    vocab = m.decoder.vocabulary
    want = beam.to_hypotheses(beam.search_host(logp.numpy(), enc_len.numpy(), len(vocab), 8, 3, 40), vocab)
    one = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8)
    many = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, n_best=3)
    assert [h.text for h in one] == [w[0].text for w in want] and [h.utt_score for h in one] == [w[0].utt_score for w in want]
    assert [[(h.text, h.labels, h.utt_score) for h in hs] for hs in many] == [[(h.text, h.labels, h.utt_score) for h in w] for w in want]
    assert all(h.start_s == [] and h.end_s == [] and h.score is None and h.words == [] for h in one)
    # cutoff_top_n = 1 walks the arg-max path: the greedy texts, at any width
    assert [h.text for h in m.decode(processed_signal=x, processed_signal_length=lens, beam_width=4, cutoff_top_n=1)] == \
        [h.text for h in greedy]
    def no_forward(*a, **k):
        raise AssertionError('a refused argument must not cost a forward')
    m._forward = no_forward
    for kw in (dict(beam_width=129), dict(beam_width=0), dict(beam_width=4, n_best=5), dict(beam_width=4, cutoff_top_n=65)):
        with pytest.raises(ValueError):
            m.decode(processed_signal=x, processed_signal_length=lens, **kw)

