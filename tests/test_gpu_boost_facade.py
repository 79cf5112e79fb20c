"""decode(beam_width=, boost=), BeamSearchDecoderWithLM(boost=) and inference.py --boost_file on an MI355X: behind the
static engine, a reserved engine and the dynamic device path the hypotheses equal the host path's (the NumPy twin of
qasr.beam on the same log-probabilities copied to the host): text, utt_score, boost_score."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from nemo.collections.asr.modules import BeamSearchDecoderWithLM  # noqa: E402
from qasr import beam, boost, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _model(mode):
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    if mode == 'static':
        qm.calibrate(m)
        L = torch.tensor([96] * 4).cuda()
        for c in synth.make_calibration(2, 4, 16, 96, 2):
            e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
            m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, mode == 'dynamic')
    return m


def _key(h):
    return (h.text, h.labels, h.utt_score, h.boost_score, h.lm_score)


def _phrases(m, **inputs):
    """words of the plain beam's runners-up (so that boosting has something to decide), some with a weight of their own"""
    plain = m.decode(**inputs, beam_width=8, n_best=4)
    words = []
    for hs in plain:
        for h in hs:
            words += [w for w in h.text.split(' ') if w and w not in words]
    assert all(h.boost_score is None for hs in plain for h in hs)
    words = words[:12] or ['a']
    return [words[0]] + [(w, 0.5 + 0.5 * (i % 5)) for i, w in enumerate(words[1:])]


def _check_against_host(m, W, nb, N, **inputs):
    vocab = m.decoder.vocabulary
    phrases = _phrases(m, **inputs)
    ps = boost.PhraseSet(phrases, vocab, weight=1.5)
    logp, enc_len, _ = m(**inputs)
    torch.cuda.synchronize()
    want = beam.to_hypotheses(beam.search_host(logp.cpu().numpy(), enc_len.cpu().numpy(), len(vocab), W, nb, N, boost=ps), vocab)
    many = m.decode(**inputs, beam_width=W, n_best=nb, cutoff_top_n=N, boost=phrases, boost_weight=1.5)
    assert [[_key(h) for h in hs] for hs in many] == [[_key(h) for h in w] for w in want]
    one = m.decode(**inputs, beam_width=W, cutoff_top_n=N, boost=ps)
    assert [_key(h) for h in one] == [_key(w[0]) for w in want]
    assert all(isinstance(h.boost_score, float) for h in one) and any(h.boost_score > 0 for hs in many for h in hs)
    timed = m.decode(**inputs, beam_width=W, cutoff_top_n=N, boost=ps, timestamps=True)
    assert [_key(h) for h in timed] == [_key(h) for h in one]
    assert all(len(h.start_s) == len(h.end_s) == len(h.labels) for h in timed) and any(h.start_s for h in timed)
    return ps, logp, enc_len


def test_static_engine_and_the_module():
    m = _model('static')
    x = torch.from_numpy(synth.make_features(4, 16, 96, 7)).cuda()
    lens = torch.tensor([96, 90, 61, 12]).cuda()
    ps, logp, enc_len = _check_against_host(m, 16, 3, 40, processed_signal=x, processed_signal_length=lens)
    assert type(m._engine).__name__ == 'Engine'
    vocab = m.decoder.vocabulary
    dec = BeamSearchDecoderWithLM(vocab, 16, 0.0, 0.0, None, 1, cutoff_top_n=40, input_tensor=True, boost=ps)
    on_device = dec(logp, enc_len)
    assert on_device == dec(logp.cpu(), enc_len.cpu())
    res = dec.search(logp, enc_len, n_best=2)
    want = beam.search_host(logp.cpu().numpy(), enc_len.cpu().numpy(), len(vocab), 16, 2, 40, boost=ps)
    for f in ('labels', 'n_labels', 'score', 'boost_score', 'n_hyps'):
        assert np.array_equal(getattr(res, f).cpu().numpy(), getattr(want, f)), f


def test_dynamic_path():
    m = _model('dynamic')
    x = torch.from_numpy(synth.make_features(5, 16, 96, 7)).cuda()
    lens = torch.tensor([96, 90, 61, 33, 12]).cuda()
    _check_against_host(m, 16, 3, 40, processed_signal=x, processed_signal_length=lens)
    assert type(m._engine).__name__ == 'DynamicRunner'


def test_reserved_engine_ragged_batches():
    m = _model('static')
    m.preprocessor.featurizer.pad_to = 16
    m.reserve(4, 2.0)
    rng = np.random.default_rng(12)
    for k in range(2):
        B = int(rng.integers(2, 5)) if k else 4
        S = int(rng.integers(8000, 32001)) if k else 32000
        audio = torch.from_numpy(synth.make_audio(B, S, seed=21 + k)).cuda()
        alen = torch.tensor([S] + [int(v) for v in rng.integers(500, S + 1, B - 1)]).cuda()
        _check_against_host(m, 16, 2, 29, input_signal=audio, input_signal_length=alen)
    assert m._ragged_engine is not None


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_cli_with_a_boost_file(tmp_path):
    base = [sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--dataset', 'none.json']
    for extra, why in ((['--boost_file', 'p.txt'], '--beam_width'), (['--beam_width', '4', '--boost_weight', '2'], '--boost_file'),
                       (['--beam_width', '4', '--boost_file', 'p.txt', '--boost_weight', '17'], '0 .. 16')):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)      # refused before a model is built
        assert out.returncode == 2 and why in out.stderr, out.stderr[-500:]
    n_utt, samples = 3, 16000
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            _write_wav(p, audio[i, :samples - 1000 * i])
            f.write(json.dumps(dict(audio_filepath=p, duration=(samples - 1000 * i) / 16000, text='hello world')) + '\n')
    run = [sys.executable, CLI, '--asr_model', 'MiniQuartzNet', '--synthetic_model', '--dataset', str(man), '--dynamic', '--dither', '0',
           '--batch_size', '3', '--beam_width', '8']
    dump = tmp_path / 'plain.json'
    out = subprocess.run(run + ['--dump_hyps', str(dump)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        plain = json.load(f)
    assert 'boost_score' not in plain
    words = [w for h in plain['hypotheses'] for w in h.split(' ') if w][:4] or ['a']
    pf = tmp_path / 'phrases.txt'
    pf.write_text('# hot words\n\n' + words[0] + '\n' + ''.join(f'{w}\t2.5\n' for w in words[1:]), encoding='utf-8')
    dump = tmp_path / 'boost.json'
    out = subprocess.run(run + ['--dump_hyps', str(dump), '--boost_file', str(pf), '--boost_weight', '1.5'], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        rec = json.load(f)
    assert rec['boost_file'] == str(pf) and rec['boost_weight'] == 1.5 and len(rec['boost_score']) == n_utt
    assert all(isinstance(v, float) and v >= 0 for v in rec['boost_score']) and any(v > 0 for v in rec['boost_score'])
    assert rec['beam_width'] == 8 and len(rec['hypotheses']) == n_utt
