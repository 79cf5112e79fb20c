"""Posteriors through the facade on an MI355X: align(posteriors=True) on the static engine, under a reservation and on the
dynamic path equals the host composition (align_host + post_host over the same model's log-probabilities) field by field;
decode(beam_width=, timestamps=True, posteriors=True) fills its n-best rows; posteriors=False returns what it returned."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases  # noqa: E402
import post_cases as pc  # noqa: E402
from qasr import align  # noqa: E402
from test_gpu_align_long_facade import model  # noqa: E402  (the committed mini net, calibrated once per process)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _tuples(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words, h.lm_score, h.ctc_score, h.segments, h.seams_s)


def _post_tuples(h):
    return (h.post, h.post_min, h.word_post, None if h.frame_post is None else h.frame_post.tolist())


def _inputs():
    from qasr import synth
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7)).cuda()
    return dict(processed_signal=x, processed_signal_length=torch.tensor([96, 70, 41]).cuda())


def _check_align(m):
    vocab = list(m.decoder.vocabulary)
    W, blank = len(vocab) + 1, len(vocab)
    inputs = _inputs()
    logp, enc_len, _ = m(**inputs)
    torch.cuda.synchronize()
    lp, ln = logp.float().cpu().numpy(), enc_len.cpu().numpy()
    for texts, star in ((['ab c', 'hello world', 'a'], None), (['ab * c', '* hello world *', 'a'], '*')):
        rows = [[W if ch == '*' else vocab.index(ch) for ch in t] for t in texts]
        tg, tl = align_cases.pad_targets(rows, blank)
        plane = align.star_host(lp, ln, 1.0) if star else None
        res, post = pc.align_and_post(lp, ln, tg, tl, blank, star=plane)
        assert res.ok.all() and post.ok.all() and post.frame_post.min() < 0
        want = align.post_to_hypotheses(res, post, vocab, m.seconds_per_frame(), lens=ln, star_token=star)
        got = m.align(**inputs, texts=texts, star=star, posteriors=True)
        assert [_tuples(h) for h in got] == [_tuples(h) for h in want]
        assert [_post_tuples(h) for h in got] == [_post_tuples(h) for h in want]
        for h, n in zip(got, ln):
            assert len(h.frame_post) == n and len(h.word_post) == len(h.words) and all(0.0 <= v <= 1.0 for v in h.post + h.word_post)
        # posteriors=False: the call it was, the new fields None
        plain = m.align(**inputs, texts=texts, star=star)
        assert [_tuples(h) for h in plain] == [_tuples(h) for h in align.to_hypotheses(res, vocab, m.seconds_per_frame(), star_token=star)]
        assert all(_post_tuples(h) == (None, None, None, None) for h in plain)
    # a transcript that cannot be aligned gets empty lists, its neighbours their values
    bad = m.align(**inputs, labels=[[1, 2] * 40, rows[1], rows[2]], star='*', posteriors=True)
    assert bad[0].post == [] and bad[0].word_post == [] and len(bad[0].frame_post) == 0 and bad[1].post == got[1].post


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_align_with_posteriors_equals_the_host_composition(mode):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(4, 4.0) if mode == 'reserved' else m.reserve(None, None)
    try:
        _check_align(m)
        served = m._ragged_engine if mode == 'reserved' else m._engine
        assert type(served).__name__ == ('DynamicRunner' if mode == 'dynamic' else 'Engine')
    finally:
        m.reserve(None, None)


def test_decode_with_posteriors_fills_the_n_best_rows():
    m = model('static')
    m.reserve(None, None)
    inputs = _inputs()
    _, enc_len, _ = m(**inputs)
    hyps = m.decode(**inputs, beam_width=4, n_best=2, timestamps=True, posteriors=True)
    plain = m.decode(**inputs, beam_width=4, n_best=2, timestamps=True)
    assert len(hyps) == 3 and any(len(row) == 2 for row in hyps)
    for b, (row, prow) in enumerate(zip(hyps, plain)):
        assert [_tuples(h) for h in row] == [_tuples(h) for h in prow]                    # the parent's hypotheses, plus:
        for h, ph in zip(row, prow):
            assert len(h.post) == len(h.post_min) == len(h.labels) and len(h.word_post) == len(h.words)
            assert len(h.frame_post) == int(enc_len[b]) and h.frame_post.dtype == np.float32 and (h.frame_post <= 0).all()
            assert all(0.0 <= lo <= v <= 1.0 for lo, v in zip(h.post_min, h.post))
            assert _post_tuples(ph) == (None, None, None, None)
    for kw, word in ((dict(posteriors=True), 'posteriors needs beam_width'),
                     (dict(posteriors=True, timestamps=True), 'posteriors needs beam_width'),
                     (dict(posteriors=True, beam_width=4), 'posteriors needs timestamps')):
        with pytest.raises(ValueError, match=word):
            m.decode(**inputs, **kw)
