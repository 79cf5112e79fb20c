"""EncDecCTCModel.decode and inference.py --timestamps on an MI355X: the static engine (k_ctc inside the engine's call),
the dynamic device path and the host modules all give the metric's strings on rows cut at the encoded length."""
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
from nemo.collections.asr.metrics.wer import WER  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import ctc, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')


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
    if mode == 'host':
        m.set_quant_mode('none')
        return m
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


def _check_hyps(m, hyps, logp, enc_len, tokens):
    wer = WER(vocabulary=m.decoder.vocabulary)
    assert len(hyps) == tokens.shape[0] and sum(len(h.text) for h in hyps) > 0
    for b, h in enumerate(hyps):
        L = int(enc_len[b])
        assert h.text == wer.ctc_decoder_predictions_tensor(tokens[b:b + 1, :L])[0], b
        assert all(0 <= s < e <= L * 0.02 + 1e-9 for s, e in zip(h.start_s, h.end_s))
        assert all(a <= b2 for a, b2 in zip(h.start_s, h.start_s[1:]))
        assert all(s <= 0 for s in h.score) and h.utt_score <= 0
        fs = logp[b, :L].gather(1, tokens[b, :L, None].long())[:, 0].cpu().numpy()
        # two forwards of one path: per-entry log-prob tolerance of this suite (rtol 1e-4, atol 2e-5), summed over L frames
        assert h.utt_score == pytest.approx(float(ctc.utt_score_host(fs)), rel=1e-4, abs=2e-5 * max(L, 1))
        assert ' '.join(w[0] for w in h.words) == ' '.join(h.text.split())


@pytest.mark.parametrize('mode', ['static', 'dynamic', 'host'])
def test_decode_equals_the_metric_on_rows_cut_at_encoded_len(mode):
    m = _model(mode)
    served = {'static': 'Engine', 'dynamic': 'DynamicRunner', 'host': 'NoneType'}[mode]
    x = torch.from_numpy(synth.make_features(5, 16, 96, 7)).cuda()
    lens = torch.tensor([96, 90, 61, 33, 12]).cuda()
    logp, enc_len, tokens = m(processed_signal=x, processed_signal_length=lens)
    hyps = m.decode(processed_signal=x, processed_signal_length=lens)
    assert type(m._engine).__name__ == served
    _check_hyps(m, hyps, logp, enc_len, tokens)
    again = m.decode(processed_signal=x, processed_signal_length=lens)       # static: the attachment is kept, buffers persistent
    assert [h.text for h in again] == [h.text for h in hyps] and [h.score for h in again] == [h.score for h in hyps]
    lp2, el2, tk2 = m(processed_signal=x, processed_signal_length=lens)      # forward is what it was
    assert torch.equal(tk2, tokens) and torch.equal(el2, enc_len) and torch.equal(lp2, logp)
    if mode == 'static':                                                     # from audio: one engine call, front-end included
        audio = torch.from_numpy(synth.make_audio(3, 16000, seed=3)).cuda()
        alen = torch.tensor([16000, 12000, 7001]).cuda()
        m.preprocessor.featurizer.pad_to = 16
        logp, enc_len, tokens = m(input_signal=audio, input_signal_length=alen)
        _check_hyps(m, m.decode(input_signal=audio, input_signal_length=alen), logp, enc_len, tokens)


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def _run_cli(tmp_path, tag, model_args, man, extra):
    dump = tmp_path / f'hyps_{tag}.json'
    out = subprocess.run([sys.executable, CLI] + model_args + ['--dataset', str(man), '--weight_bit', '8', '--act_bit', '8',
                          '--dither', '0', '--batch_size', '3', '--synthetic_calib', '2', '--percentile', '99.996',
                          '--dump_hyps', str(dump)] + extra, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        return out.stdout, json.load(f)


def _check_cli(tmp_path, model_args, text, normalize):
    n_utt, samples = 6, 24000
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    durations = []
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            n = samples - 1000 * i
            _write_wav(p, audio[i, :n])
            durations.append(n / 16000)
            f.write(json.dumps(dict(audio_filepath=p, duration=n / 16000, text=text), ensure_ascii=False) + '\n')
    norm = [] if normalize else ['--normalize_text', '']
    _, plain = _run_cli(tmp_path, 'plain', model_args, man, norm)
    stdout, rec = _run_cli(tmp_path, 'ts', model_args, man, norm + ['--timestamps'])
    assert 'words' not in plain and 'utt_score' not in plain
    assert rec['hypotheses'] == plain['hypotheses'] and rec['wer'] == plain['wer'] and rec['references'] == plain['references']
    assert rec['path'] == 'Engine' and len(rec['words']) == len(rec['utt_score']) == n_utt
    assert sum(len(w) for w in rec['words']) > 0
    for words, utt, dur, hyp in zip(rec['words'], rec['utt_score'], durations, rec['hypotheses']):
        assert utt <= 0
        t = 0.0
        for word, s, e, score in words:
            assert isinstance(word, str) and word and ' ' not in word
            assert t <= s < e <= dur + 0.04 and score <= 0   # (the last encoder frame may reach past the last sample: one frame pair)
            t = s
        # decode() stops at the encoded length, the hypothesis walks the padded row: the words are a prefix of its words
        assert hyp.split()[:max(len(words) - 1, 0)] == [w[0] for w in words][:max(len(words) - 1, 0)]
    return rec


def test_cli_timestamps_en(tmp_path):
    _check_cli(tmp_path, ['--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model'], 'hello world', True)


def test_cli_timestamps_zh_cjk(tmp_path):
    path = str(tmp_path / 'QuartzNet15x5Base-Zh.nemo')
    EncDecCTCModel.from_synthetic('QuartzNet15x5Base-Zh').save_to(path)
    rec = _check_cli(tmp_path, ['--asr_model', path], '一丁 丂七', False)
    assert any(ord(ch) >= 0x4E00 for words in rec['words'] for w in words for ch in w[0])
