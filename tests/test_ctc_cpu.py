"""Greedy CTC decoding on the host (qasr/ctc.py): pinned to the reference's WER.ctc_decoder_predictions_tensor through
tests/golden/ctc_decode.npz, its stated properties on seeded inputs, and the façade's decode() on the host modules."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctc_cases  # noqa: E402
from nemo.collections.asr.metrics.wer import WER  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import ctc  # noqa: E402

torch.set_grad_enabled(False)


def _fixture(golden_dir):
    d = np.load(os.path.join(golden_dir, 'ctc_decode.npz'))
    return d, json.loads(str(d['meta']))['cases']


def test_fixture_holds_every_case_the_generator_promises(golden_dir):
    d, cases = _fixture(golden_dir)
    assert {(c['n_labels'], c['T']) for c in cases} == {(v, T) for v in ctc_cases.FIXTURE_VOCAB for T in ctc_cases.FIXTURE_T}
    for c in cases:
        tok = d['tokens_' + c['name']]
        blank = c['n_labels']
        assert tok.shape == (c['rows'], c['T']) and tok.min() >= 0 and tok.max() <= blank
        # the fixture is what tests/ctc_cases.py generates (the GPU tests rebuild larger ones from the same code)
        assert np.array_equal(tok, ctc_cases.token_matrix(1000 * ctc_cases.FIXTURE_VOCAB.index(blank) + c['T'], c['T'], blank))
        assert (tok == blank).all(1).any(), 'a row that is all blank'
        assert any((r == r[0]).all() and r[0] != blank for r in tok), 'a row that is one non-blank run'
        assert any((r != blank).all() and (r[1:] != r[:-1]).all() for r in tok), 'a row where every frame emits'
        assert any(r[0] != blank and r[-1] != blank for r in tok), 'first and last frames emit'
        if c['T'] >= 250:
            real = tok[0]
            runs = np.flatnonzero(real[1:] != real[:-1])
            assert (real == blank).sum() > 0 and len(runs) > 8
            emitted = [int(real[0])] + [int(real[i + 1]) for i in runs]
            assert any(a == c2 and b == blank for a, b, c2 in zip(emitted, emitted[1:], emitted[2:]) if a != blank), \
                'a label repeated across one blank'


def test_collapse_host_gives_the_reference_strings(golden_dir):
    """every row of every fixture case: collapse_host(lens=None) + to_hypotheses == the reference's hypothesis"""
    d, cases = _fixture(golden_dir)
    n = 0
    for c in cases:
        tok = d['tokens_' + c['name']]
        want = json.loads(str(d['hyps_' + c['name']]))
        vocab = ctc_cases.vocabulary(c['n_labels'])
        res = ctc.collapse_host(tok, blank=c['n_labels'])
        got = [h.text for h in ctc.to_hypotheses(res, vocab, 0.02)]
        assert got == want, c['name']
        # and the façade's own restatement of the loop agrees with both
        assert WER(vocabulary=vocab).ctc_decoder_predictions_tensor(torch.from_numpy(tok)) == want
        n += len(want)
    assert n == sum(c['rows'] for c in cases)


def _check_properties(tok, fs, lens, blank, res):
    B, T = tok.shape
    for b in range(B):
        lim = T if lens is None else int(min(max(int(lens[b]), 0), T))
        n = int(res.n_labels[b])
        assert (res.labels[b, n:] == blank).all() and (res.start[b, n:] == 0).all() and (res.nframes[b, n:] == 0).all()
        st, nf, lab = res.start[b, :n], res.nframes[b, :n], res.labels[b, :n]
        assert (lab != blank).all() and (nf >= 1).all()
        assert (np.diff(st) > 0).all() and (st + nf <= lim).all()
        covered = np.zeros(T, dtype=bool)
        for i in range(n):                                   # runs tile the non-blank frames exactly
            seg = tok[b, st[i]:st[i] + nf[i]]
            assert (seg == lab[i]).all() and not covered[st[i]:st[i] + nf[i]].any()
            covered[st[i]:st[i] + nf[i]] = True
            assert st[i] == 0 or tok[b, st[i] - 1] != lab[i]                     # maximal on both sides
            assert st[i] + nf[i] == lim or tok[b, st[i] + nf[i]] != lab[i]
            if fs is not None:
                assert res.score[b, i] == fs[b, st[i]:st[i] + nf[i]].max()
        assert np.array_equal(covered[:lim], tok[b, :lim] != blank) and not covered[lim:].any()
        if fs is not None:
            assert (res.score[b, n:].view(np.int32) == 0).all()
            x = fs[b, :lim]
            part = [np.float32(0.0)] * 64                    # the 64-lane order, restated in plain Python
            for t in range(lim):
                part[t % 64] = np.float32(part[t % 64] + x[t])
            acc = np.float32(0.0)
            for l in range(64):
                acc = np.float32(acc + part[l])
            assert np.float32(res.utt_score[b]).view(np.int32) == acc.view(np.int32)
            exact = float(np.sum(x.astype(np.float64)))
            bound = max(lim - 1, 0) * 2.0 ** -24 * float(np.sum(np.abs(x.astype(np.float64))))
            assert abs(float(res.utt_score[b]) - exact) <= bound
            if lim == 0:
                assert np.float32(res.utt_score[b]).view(np.int32) == 0


@pytest.mark.parametrize('T', [1, 63, 64, 65, 250, 1000])
@pytest.mark.parametrize('n_labels', [28, 5206])
def test_collapse_host_properties(T, n_labels):
    tok = ctc_cases.token_matrix(77 + T, T, n_labels, n_realistic=6)
    fs = ctc_cases.frame_scores(78 + T, tok.shape)
    B = tok.shape[0]
    rng = np.random.default_rng(T)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = 0, T
    lens[-1] = T + 5                                         # beyond the row: clamps to T
    full = ctc.collapse_host(tok, fs, None, blank=n_labels)
    _check_properties(tok, fs, None, n_labels, full)
    cut = ctc.collapse_host(tok, fs, lens, blank=n_labels)
    _check_properties(tok, fs, lens, n_labels, cut)
    assert cut.n_labels[0] == 0 and cut.utt_score[0] == 0
    for b in range(B):                                       # with lens == the row truncated to lens[b]
        lim = int(min(lens[b], T))
        if lim == 0:
            assert cut.n_labels[b] == 0
            continue
        one = ctc.collapse_host(tok[b:b + 1, :lim], fs[b:b + 1, :lim], None, blank=n_labels)
        n = int(one.n_labels[0])
        assert cut.n_labels[b] == n
        for name in ('labels', 'start', 'nframes'):
            assert np.array_equal(getattr(cut, name)[b, :n], getattr(one, name)[0, :n]), name
        assert np.array_equal(cut.score[b, :n].view(np.int32), one.score[0, :n].view(np.int32))
        assert cut.utt_score[b].view(np.int32) == one.utt_score[0].view(np.int32)
    no_scores = ctc.collapse_host(tok, None, lens, blank=n_labels)
    assert no_scores.score is None and no_scores.utt_score is None
    assert np.array_equal(no_scores.labels, cut.labels) and np.array_equal(no_scores.nframes, cut.nframes)


def test_words_and_times_on_a_hand_written_row():
    vocab = [' ', 'a', 'b', 'c']                              # blank = 4
    _ = 4
    #      t: 0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17
    row = [_, 1, 1, _, 1, 2, _, 0, 0, 3, _, _, 0, 0, _, 2, 2, 2]
    fs = np.array([-.5, -.3, -.2, -.1, -.4, -.6, -.1, -.7, -.9, -.05, -.1, -.1, -.3, -.2, -.1, -.8, -.25, -.5], np.float32)
    res = ctc.collapse_host(np.array([row]), fs[None], None, blank=4)
    assert res.labels[0, :int(res.n_labels[0])].tolist() == [1, 1, 2, 0, 3, 0, 2]
    h, = ctc.to_hypotheses(res, vocab, 0.02)
    assert h.text == 'aab c b' and h.labels == [1, 1, 2, 0, 3, 0, 2]
    np.testing.assert_allclose(h.start_s, [0.02, 0.08, 0.10, 0.14, 0.18, 0.24, 0.30], rtol=0, atol=1e-12)
    np.testing.assert_allclose(h.end_s, [0.06, 0.10, 0.12, 0.18, 0.20, 0.28, 0.36], rtol=0, atol=1e-12)
    assert h.score == [float(np.float32(v)) for v in (-.2, -.4, -.6, -.7, -.05, -.2, -.25)]
    assert [w[0] for w in h.words] == ['aab', 'c', 'b']
    np.testing.assert_allclose([w[1] for w in h.words], [0.02, 0.18, 0.30], atol=1e-12)
    np.testing.assert_allclose([w[2] for w in h.words], [0.12, 0.20, 0.36], atol=1e-12)
    assert [w[3] for w in h.words] == [float(np.float32(-.6)), float(np.float32(-.05)), float(np.float32(-.25))]
    assert h.utt_score == float(ctc.utt_score_host(fs))
    # a vocabulary without ' ': one word per utterance; an empty utterance: no word
    res2 = ctc.collapse_host(np.array([[3, 0, 0, 1, 3], [3, 3, 3, 3, 3]]), None, None, blank=3)
    h2 = ctc.to_hypotheses(res2, ['x', 'y', 'z'], 0.04)
    assert h2[0].text == 'xy' and [w[0] for w in h2[0].words] == ['xy'] and h2[0].words[0][1:] == (0.04, 0.16, None)
    assert h2[1].text == '' and h2[1].words == [] and h2[0].score is None and h2[0].utt_score is None


def test_seconds_per_frame_comes_from_the_model():
    from qasr import configs, topology
    for name in ('QuartzNet15x5Base-En', 'QuartzNet15x5Base-Zh', 'Jasper10x5Dr-En'):
        if name not in topology.MODELS:
            continue
        assert ctc.seconds_per_frame(topology.MODELS[name](), 160 / 16000) == pytest.approx(0.02, abs=1e-15)
    assert len([n for n in ('QuartzNet15x5Base-En', 'QuartzNet15x5Base-Zh') if n in topology.MODELS]) == 2
    m = EncDecCTCModel(configs.model_config(topology.mini_quartznet()))
    assert m.seconds_per_frame() == pytest.approx(0.02, abs=1e-15)
    m.preprocessor.featurizer.hop_length = 320                # not hard-coded: follows the featurizer
    assert m.seconds_per_frame() == pytest.approx(0.04, abs=1e-15)


def test_facade_decode_on_the_host_modules(tmp_path):
    """decode() texts == the metric's loop on rows cut at encoded_len; scores are log_probs at the tokens; transcribe()
    without the new keyword returns what it returned"""
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
    m.set_quant_mode('none')
    m.eval()
    rng = np.random.default_rng(5)
    x = torch.from_numpy((0.1 * rng.standard_normal((3, 16000))).astype(np.float32))
    lens = torch.tensor([16000, 9000, 12345])
    m.preprocessor.featurizer.dither = 0.0
    logp, enc_len, tokens = m(input_signal=x, input_signal_length=lens)
    hyps = m.decode(input_signal=x, input_signal_length=lens)
    wer = WER(vocabulary=m.decoder.vocabulary)
    assert len(hyps) == 3 and all(isinstance(h, ctc.Hypothesis) for h in hyps)
    for b, h in enumerate(hyps):
        L = int(enc_len[b])
        assert h.text == wer.ctc_decoder_predictions_tensor(tokens[b:b + 1, :L])[0]
        assert all(0 <= s <= e <= L * 0.02 + 1e-9 for s, e in zip(h.start_s, h.end_s))
        assert all(s <= 0 for s in h.score) and h.utt_score <= 0
        fs = logp[b, :L].gather(1, tokens[b, :L, None])[:, 0].numpy()
        assert np.float32(h.utt_score).view(np.int32) == ctc.utt_score_host(fs).view(np.int32)
        assert ' '.join(w[0] for w in h.words) == ' '.join(h.text.split())
    import wave
    paths = []
    for i, n in enumerate((16000, 9000)):
        p = str(tmp_path / f't{i}.wav')
        with wave.open(p, 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes((np.clip(x[i, :n].numpy(), -1, 1) * 32767).astype('<i2').tobytes())
        paths.append(p)
    plain = m.transcribe(paths, batch_size=2)
    assert plain == m.transcribe(paths, batch_size=2, return_hypotheses=False) and all(isinstance(h, str) for h in plain)
    rich = m.transcribe(paths, batch_size=2, return_hypotheses=True)
    assert [type(h) for h in rich] == [ctc.Hypothesis] * 2
    # the longest file of the batch has no pad frames: both decoders saw the same frames up to its encoded length
    assert plain[0].startswith(rich[0].text)
