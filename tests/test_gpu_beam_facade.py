"""decode(beam_width=), BeamSearchDecoderWithLM and inference.py --beam_width on an MI355X: on the static engine (synthetic
QuartzNet15x5 En and Zh), a reserved engine with ragged batches and the dynamic device path, the hypotheses equal the NumPy
twin (qasr.beam) run on the same log-probabilities copied to the host, and greedy decode() is what it was."""
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
from nemo.collections.asr.metrics.wer import WER, word_error_rate  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from nemo.collections.asr.modules import BeamSearchDecoderWithLM  # noqa: E402
from qasr import beam, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _model(name, mode, feat_in, batch, frames, ncal=2, percentile=None, seed=2):
    m = EncDecCTCModel.from_synthetic(name, seed=seed).cuda() if name == 'MiniQuartzNet' else EncDecCTCModel.from_synthetic(name).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    if percentile is not None:
        qm.set_percentile(m, percentile)
    m.encoder.bn_folding()
    if mode == 'static':
        qm.calibrate(m)
        L = torch.tensor([frames] * batch).cuda()
        cal = synth.make_calibration(ncal, batch, feat_in, frames, seed) if name == 'MiniQuartzNet' else \
            synth.make_calibration(ncal, batch, feat_in, frames)
        for c in cal:
            e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
            m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, mode == 'dynamic')
    return m


def _tuples(hyps):
    return [(h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words) for h in hyps]


def _check_against_twin(m, W, nb, N, **inputs):
    """decode(beam_width=W) and the module on the model's own log-probabilities == the twin on their host copy"""
    vocab = m.decoder.vocabulary
    greedy_before = _tuples(m.decode(**inputs))
    logp, enc_len, tokens = m(**inputs)
    torch.cuda.synchronize()
    want = beam.to_hypotheses(beam.search_host(logp.cpu().numpy(), enc_len.cpu().numpy(), len(vocab), W, nb, N), vocab)
    many = m.decode(**inputs, beam_width=W, n_best=nb, cutoff_top_n=N)
    assert [_tuples(h) for h in many] == [_tuples(w) for w in want]
    one = m.decode(**inputs, beam_width=W, cutoff_top_n=N)
    assert _tuples(one) == [_tuples(w)[0] for w in want]
    dec = BeamSearchDecoderWithLM(vocab, W, 0.0, 0.0, None, 1, cutoff_top_n=N, input_tensor=True)
    full = beam.to_hypotheses(beam.search_host(logp.cpu().numpy(), enc_len.cpu().numpy(), len(vocab), W, None, N), vocab)
    assert dec(logp, enc_len) == [[(h.utt_score, h.text) for h in w] for w in full]
    assert all(len(w) <= W and w[0].utt_score <= 0 for w in full) and sum(len(w[0].text) for w in want) > 0
    # greedy decoding is untouched: the same hypotheses as before the beam ran, and the metric's strings
    assert _tuples(m.decode(**inputs)) == greedy_before
    wer = WER(vocabulary=vocab)
    for b, g in enumerate(greedy_before):
        assert g[0] == wer.ctc_decoder_predictions_tensor(tokens[b:b + 1, :int(enc_len[b])])[0]
    # one candidate per frame walks the arg-max path
    assert [h.text for h in m.decode(**inputs, beam_width=W, cutoff_top_n=1)] == [g[0] for g in greedy_before]
    return want


@pytest.mark.parametrize('name', ['QuartzNet15x5Base-En', 'QuartzNet15x5Base-Zh'])
def test_static_engine_full_size(name):
    m = _model(name, 'static', 64, 3, 200)
    x = torch.from_numpy(synth.make_features(3, 64, 200, 9)).cuda()
    lens = torch.tensor([200, 131, 58]).cuda()
    _check_against_twin(m, 16, 4, 40, processed_signal=x, processed_signal_length=lens)
    assert type(m._engine).__name__ == 'Engine'
    if name.endswith('En'):
        _check_against_twin(m, 128, 128, 29, processed_signal=x, processed_signal_length=lens)
        audio = torch.from_numpy(synth.make_audio(3, 16000, seed=3)).cuda()
        alen = torch.tensor([16000, 12000, 7001]).cuda()
        m.preprocessor.featurizer.pad_to = 16
        _check_against_twin(m, 8, 2, 20, input_signal=audio, input_signal_length=alen)


def test_dynamic_path_mini():
    m = _model('MiniQuartzNet', 'dynamic', 16, 4, 96)
    x = torch.from_numpy(synth.make_features(5, 16, 96, 7)).cuda()
    lens = torch.tensor([96, 90, 61, 33, 12]).cuda()
    _check_against_twin(m, 16, 3, 40, processed_signal=x, processed_signal_length=lens)
    assert type(m._engine).__name__ == 'DynamicRunner'


def test_reserved_engine_ragged_batches():
    m = _model('MiniQuartzNet', 'static', 16, 4, 96)
    m.preprocessor.featurizer.pad_to = 16
    m.reserve(4, 2.0)
    rng = np.random.default_rng(11)
    for k in range(6):
        B = int(rng.integers(1, 5)) if k else 4
        S = int(rng.integers(4000, 32001)) if k else 32000
        audio = torch.from_numpy(synth.make_audio(B, S, seed=11 + k)).cuda()
        alen = torch.tensor([S] + [int(v) for v in rng.integers(500, S + 1, B - 1)]).cuda()
        _check_against_twin(m, 16, 2, 29, input_signal=audio, input_signal_length=alen)
    assert m._ragged_engine is not None


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_cli_beam_width_equals_the_model_in_process(tmp_path):
    n_utt, samples, text = 6, 24000, 'hello world'
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            n = samples - 1000 * i
            _write_wav(p, audio[i, :n])
            f.write(json.dumps(dict(audio_filepath=p, duration=n / 16000, text=text)) + '\n')
    base = [sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
            '--act_bit', '8', '--dither', '0', '--batch_size', '3', '--synthetic_calib', '2', '--percentile', '99.996']
    recs = {}
    for tag, extra in (('greedy', []), ('beam', ['--beam_width', '16'])):
        dump = tmp_path / f'{tag}.json'
        out = subprocess.run(base + ['--dump_hyps', str(dump)] + extra, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        assert 'path: static integer engine (HIP)' in out.stdout
        with open(dump, encoding='utf-8') as f:
            recs[tag] = json.load(f)
    assert 'beam_score' not in recs['greedy'] and recs['beam']['beam_width'] == 16
    m = _model('QuartzNet15x5Base-En', 'static', 64, 3, 500, percentile=99.996)
    m.setup_test_data(test_data_config={'sample_rate': 16000, 'manifest_filepath': str(man), 'labels': m.decoder.vocabulary,
                                        'batch_size': 3, 'normalize_transcripts': True, 'shuffle': False})
    hyps, scores, refs = [], [], []
    labels_map = dict(enumerate(m.decoder.vocabulary))
    for batch in m.test_dataloader():
        for h in m.decode(input_signal=batch[0].cuda().float(), input_signal_length=batch[1].cuda(), beam_width=16):
            hyps.append(h.text)
            scores.append(h.utt_score)
        refs += [''.join(labels_map[c] for c in row) for row in batch[2].cpu().numpy()]
    rec = recs['beam']
    assert rec['hypotheses'] == hyps and rec['beam_score'] == scores and rec['references'] == refs == recs['greedy']['references']
    assert rec['wer'] == word_error_rate(hypotheses=hyps, references=refs)
    assert len(hyps) == n_utt and all(s <= 0 for s in scores) and sum(len(h) for h in hyps) > 0


def test_cli_refuses_a_width_outside_the_limit():
    for w in ('0', '129'):                               # refused at the command line, before a model is built
        out = subprocess.run([sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--dataset', 'none.json', '--beam_width', w],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and '1 .. 128' in out.stderr, out.stderr[-500:]
