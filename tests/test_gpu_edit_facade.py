"""EncDecCTCModel.error_rate / error_rate_long, WER(device=True) and inference.py --device_wer on an MI355X: the counts the
device chain reads back equal word_error_rate over decode()'s texts and the twin over their ids - on the static engine, a
reserved engine and the dynamic path, greedy and beam, words and characters."""
import json
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.metrics.wer import WER, _levenshtein, word_error_rate  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import edit, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')
KW = dict(window_s=2.0, overlap_s=0.5, guard_s=0.1)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _model(mode, seed=2):
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=seed).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    if mode == 'static':
        qm.calibrate(m)
        L = torch.tensor([96] * 4).cuda()
        for c in synth.make_calibration(3, 4, 16, 96, seed):
            e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
            m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, mode == 'dynamic')
    return m


_models = {}


def model(mode):
    if mode not in _models:
        _models[mode] = _model(mode)
    return _models[mode]


def _references(m, n, seed, width=40):
    """reference ids [n, width] over the model's vocabulary with whitespace here and there, ragged lengths, and their strings"""
    vocab = m.decoder.vocabulary
    g = np.random.default_rng(seed)
    tg = g.integers(0, len(vocab), (n, width)).astype(np.int32)
    if ' ' in vocab:
        tg[g.random((n, width)) < 0.25] = vocab.index(' ')
    tl = g.integers(1, width + 1, n).astype(np.int32)
    tl[0] = width
    texts = [''.join(vocab[c] for c in row[:k]) for row, k in zip(tg, tl)]
    return torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), texts


def _ids(m, text):
    return [m.decoder.vocabulary.index(ch) for ch in text]


def _check_report(m, rep, hyp_texts, ref_texts, use_cer, nbest_texts=None):
    cut = (lambda t: list(t)) if use_cer else (lambda t: t.split())
    assert rep.invalid == 0 and len(rep.per_utterance) == len(ref_texts)
    assert rep.total.rate == word_error_rate(hyp_texts, ref_texts, use_cer=use_cer)
    vocab = list(m.decoder.vocabulary)
    hyp = [_ids(m, t) for t in hyp_texts]
    ref = [_ids(m, t) for t in ref_texts]
    w = lambda rows: max(1, max(len(r) for r in rows))
    pad = lambda rows: np.array([r + [0] * (w(rows) - len(r)) for r in rows], dtype=np.int32)
    want = edit.edit_host(pad(hyp), np.array([len(r) for r in hyp], dtype=np.int32), pad(ref), np.array([len(r) for r in ref], dtype=np.int32),
                          len(vocab), mode='char' if use_cer else 'word', is_space=None if use_cer else edit.space_mask(vocab))
    got = [[c.errors, c.substitutions, c.deletions, c.insertions, c.ref_units, c.hyp_units] for c in rep.per_utterance]
    assert got == want.rows[:, :6].tolist()
    t = rep.total
    assert [t.errors, t.ref_units, t.substitutions, t.deletions, t.insertions, t.hyp_units] == want.totals[:6].tolist()
    assert t.errors == sum(_levenshtein(cut(h), cut(r)) for h, r in zip(hyp_texts, ref_texts)) and t.errors > 0
    if nbest_texts is None:
        assert rep.oracle_errors == t.errors
    else:
        assert rep.oracle_errors == sum(min(_levenshtein(cut(h), cut(r)) for h in row) for row, r in zip(nbest_texts, ref_texts))
        assert rep.oracle_errors <= t.errors


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_error_rate_equals_word_error_rate_over_decodes_texts(mode):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(5, 2.0) if mode == 'reserved' else m.reserve(None, None)
    try:
        audio = torch.from_numpy(synth.make_audio(5, 24000, seed=3)).cuda()
        alen = torch.tensor([24000, 20000, 16001, 9000, 4000]).cuda()
        m.preprocessor.featurizer.pad_to = 16
        io = dict(input_signal=audio, input_signal_length=alen)
        tg, tl, ref_texts = _references(m, 5, 5)
        greedy = [h.text for h in m.decode(**io)]
        assert sum(len(t) for t in greedy) > 0
        for use_cer in (False, True):
            _check_report(m, m.error_rate(**io, targets=tg, target_lengths=tl, use_cer=use_cer), greedy, ref_texts, use_cer)
        assert type(m._engine if mode == 'dynamic' else (m._ragged_engine if mode == 'reserved' else m._engine)).__name__ == \
            ('DynamicRunner' if mode == 'dynamic' else 'Engine')
        # references as texts, and as padded rows without lengths
        by_text = m.error_rate(**io, texts=ref_texts)
        _check_report(m, by_text, greedy, ref_texts, False)
        padded = [''.join(m.decoder.vocabulary[c] for c in row) for row in tg.cpu().tolist()]
        _check_report(m, m.error_rate(**io, targets=tg), greedy, padded, False)
        # the beam's n-best rows: the best row is the total, the oracle the best of the three
        nbest = m.decode(**io, beam_width=8, n_best=3)
        texts3 = [[h.text for h in row] for row in nbest]
        for use_cer in (False, True):
            rep = m.error_rate(**io, targets=tg, target_lengths=tl, use_cer=use_cer, beam_width=8, n_best=3)
            _check_report(m, rep, [row[0] for row in texts3], ref_texts, use_cer, texts3)
        with pytest.raises(ValueError, match='targets .* or as texts'):
            m.error_rate(**io)
        with pytest.raises(ValueError, match='not in the vocabulary'):
            m.error_rate(**io, texts=['#'] * 5)
    finally:
        m.reserve(None, None)


def test_error_rate_on_cpu_tensors_runs_the_twin():
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7))
    lens = torch.tensor([96, 61, 33])
    tg, tl, ref_texts = _references(m, 3, 6)
    io = dict(processed_signal=x, processed_signal_length=lens)
    greedy = [h.text for h in m.decode(**io)]
    _check_report(m, m.error_rate(**io, targets=tg.cpu(), target_lengths=tl.cpu()), greedy, ref_texts, False)


def test_error_rate_long_equals_word_error_rate_over_decode_longs_texts():
    m = model('static')
    m.reserve(None, None)
    S = 32000 + 2 * 24000 + 10000
    audio = torch.from_numpy(synth.make_audio(2, S, seed=8)).cuda()
    lens = torch.tensor([30000, S]).cuda()
    tg, tl, ref_texts = _references(m, 2, 9, width=90)
    texts = [h.text for h in m.decode_long(audio, lens, batch_size=2, **KW)]
    assert len(texts[1]) > 0
    for use_cer in (False, True):
        rep = m.error_rate_long(audio, lens, targets=tg, target_lengths=tl, use_cer=use_cer, batch_size=2, **KW)
        _check_report(m, rep, texts, ref_texts, use_cer)
    rows = m.decode_long(audio, lens, batch_size=2, beam_width=4, n_best=2, **KW)
    texts2 = [[h.text for h in row] for row in rows]
    rep = m.error_rate_long(audio, lens, targets=tg, target_lengths=tl, batch_size=2, beam_width=4, n_best=2, **KW)
    _check_report(m, rep, [row[0] for row in texts2], ref_texts, False, texts2)


@pytest.mark.parametrize('use_cer', [False, True])
def test_wer_device_equals_the_default_metric_over_two_batches(use_cer):
    vocab = [' '] + list('abcdefghijklmnopqrstuvwxyz') + ["'"]
    blank = len(vocab)
    g = torch.Generator().manual_seed(4)
    plain, dev = WER(vocabulary=vocab, use_cer=use_cer), WER(vocabulary=vocab, use_cer=use_cer, device=True)
    for B, T, L in ((7, 130, 40), (3, 75, 90)):
        pred = torch.randint(0, blank + 1, (B, T), generator=g)
        pred[torch.rand(B, T, generator=g) < 0.3] = 0
        tg = torch.randint(0, blank, (B, L), generator=g)
        tg[torch.rand(B, L, generator=g) < 0.25] = 0
        tl = torch.randint(0, L + 1, (B,), generator=g)
        plain.update(pred, tg, tl)
        dev.update(pred.cuda(), tg.cuda(), tl.cuda())
    a, b = plain.compute(), dev.compute()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[1]) > 0
    c = dev.counts()
    assert (c.errors, c.ref_units) == (int(a[1]), int(a[2])) and c.substitutions + c.deletions + c.insertions == c.errors


# ------------------------------------------------------------------------------------------------------------------ CLI
def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def _cli(tmp_path, man, extra):
    out = subprocess.run([sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man),
                          '--weight_bit', '8', '--act_bit', '8', '--dither', '0', '--batch_size', '3', '--synthetic_calib', '2',
                          '--percentile', '99.996'] + extra, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def _printed(stdout, key):
    return re.search(rf'^{re.escape(key)} (.*)$', stdout, re.M).group(1)


def test_cli_device_wer_prints_the_same_wer(tmp_path):
    n_utt, samples = 6, 24000
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            _write_wav(p, audio[i, :samples - 1000 * i])
            f.write(json.dumps(dict(audio_filepath=p, duration=(samples - 1000 * i) / 16000, text='hello wide world'[:16 - i])) + '\n')
    plain = _cli(tmp_path, man, [])
    dev = _cli(tmp_path, man, ['--device_wer'])
    assert _printed(dev, 'WER:') == _printed(plain, 'WER:') and float(_printed(plain, 'WER:')) > 0
    s, d, i = (int(x) for x in _printed(dev, 'S / D / I:').split(' / '))
    assert s + d + i > 0 and 'S / D / I:' not in plain and 'oracle WER:' not in dev
    # the beam with two rows per utterance, characters: the strings of the dump give the printed number on the host
    dump = tmp_path / 'beam.json'
    beam = _cli(tmp_path, man, ['--device_wer', '--cer', '--beam_width', '4', '--n_best', '2', '--dump_hyps', str(dump)])
    rec = json.load(open(dump))
    assert float(_printed(beam, 'WER:')) == rec['wer'] == word_error_rate(rec['hypotheses'], rec['references'], use_cer=True)
    assert float(_printed(beam, 'oracle WER:')) <= rec['wer']
