"""EncDecCTCModel.forward / decode with sample_rate= on an MI355X: int16 PCM at 8 kHz and interleaved stereo at 44.1 kHz, resampled
on the device in front of the mel front-end, give the tensors and hypotheses of the same model fed with the NumPy twin's float
output (qasr.resample.resample_host) and converted lengths - on the static engine, a reserved engine (without a new device
allocation) and the dynamic device path - and inference.py --input_rate prints the hypotheses of the 16 kHz path on that output."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
import resample_cases as rc  # noqa: E402
from nemo.collections.asr.metrics.wer import WER  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import resample as rs, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')
CASES = ((8000, 1, 'best'), (44100, 2, 'best'), (8000, 1, 'fast'))


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _model(name, mode, feat_in, batch, frames, ncal=2, seed=2, percentile=None):
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


def _hyp_tuple(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words)


def _batch(sr, ch, seconds, seed, B=3):
    """int16 PCM [B][S * ch] with ragged lengths, full-scale fill behind them"""
    S = int(seconds * sr)
    lens = [S] + [int(S * f) for f in (0.71, 0.33, 0.5)[:B - 1]]
    return rc.fill_behind(rc.pcm(B, S, ch, seed=seed), lens, ch), lens


def _check(m, sr, ch, quality, seconds=1.5, seed=0):
    m.resample_quality = quality
    x, lens = _batch(sr, ch, seconds, seed)
    y, ln = rs.resample_host(x, lens, rs.ResamplePlan(sr, 16000, quality), channels=ch)
    want = m(input_signal=torch.from_numpy(y).cuda(), input_signal_length=torch.tensor(ln.astype(np.int64)).cuda())
    got = m(input_signal=torch.from_numpy(x).cuda(), input_signal_length=torch.tensor(lens).cuda(), sample_rate=sr, channels=ch)
    torch.cuda.synchronize()
    for g, w, what in zip(got, want, ('log_probs', 'encoded lengths', 'tokens')):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (sr, ch, quality, what)
    hw = m.decode(input_signal=torch.from_numpy(y).cuda(), input_signal_length=torch.tensor(ln.astype(np.int64)).cuda())
    hg = m.decode(input_signal=torch.from_numpy(x).cuda(), input_signal_length=torch.tensor(lens).cuda(), sample_rate=sr, channels=ch)
    assert [_hyp_tuple(h) for h in hg] == [_hyp_tuple(h) for h in hw] and len(hg) == len(lens)
    assert max((h.end_s[-1] for h in hg if h.end_s), default=0.0) <= seconds + 0.1          # times are seconds of audio, whatever the rate
    m.resample_quality = 'best'


def test_static_engine():
    m = _model('MiniQuartzNet', 'static', 16, 4, 96)
    m.preprocessor.featurizer.pad_to = 16
    for sr, ch, quality in CASES:
        _check(m, sr, ch, quality)
    assert type(m._engine).__name__ == 'Engine' and m._ragged_engine is None
    # float PCM at another rate; the model's own rate in int16 (the bypass) against read_wav's values
    x, lens = _batch(8000, 1, 1.0, 5)
    yf, ln = rs.resample_host(rc.to_float(x), lens, rs.ResamplePlan(8000), channels=1)
    want = m(input_signal=torch.from_numpy(yf).cuda(), input_signal_length=torch.tensor(ln.astype(np.int64)).cuda())
    got = m(input_signal=torch.from_numpy(rc.to_float(x)).cuda(), input_signal_length=torch.tensor(lens).cuda(), sample_rate=8000)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    x16, l16 = _batch(16000, 1, 1.0, 6)
    y16 = rc.to_float(x16)
    for b, n in enumerate(l16):
        y16[b, n:] = 0
    want = m(input_signal=torch.from_numpy(y16).cuda(), input_signal_length=torch.tensor(l16).cuda())
    got = m(input_signal=torch.from_numpy(x16).cuda(), input_signal_length=torch.tensor(l16).cuda(), sample_rate=16000)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # align() takes the keywords too
    al = m.align(input_signal=torch.from_numpy(x).cuda(), input_signal_length=torch.tensor(lens).cuda(), labels=[[1, 2], [3], [4, 4]],
                 sample_rate=8000)
    y, ln = rs.resample_host(x, lens, rs.ResamplePlan(8000))
    al_want = m.align(input_signal=torch.from_numpy(y).cuda(), input_signal_length=torch.tensor(ln.astype(np.int64)).cuda(),
                      labels=[[1, 2], [3], [4, 4]])
    assert [_hyp_tuple(h) + (h.ctc_score,) for h in al] == [_hyp_tuple(h) + (h.ctc_score,) for h in al_want]


def test_reserved_engine_replays_without_allocating():
    m = _model('MiniQuartzNet', 'static', 16, 4, 96)
    m.preprocessor.featurizer.pad_to = 16
    m.reserve(4, 4.0)
    _check(m, 8000, 1, 'best', seconds=2.0, seed=1)                  # builds the reserved engine and the first bucket
    eng = m._ragged_engine
    allocs = eng.ragged_stats()['device_allocs']
    for k, (sr, ch, quality) in enumerate(CASES):
        _check(m, sr, ch, quality, seconds=(1.5, 3.9, 2.0)[k], seed=2 + k)
    st = eng.ragged_stats()
    assert st['device_allocs'] == allocs and m._engine is None and m._ragged_engine is eng      # every call inside the envelope
    assert sum(st['buckets'].values()) == 16 and st['graph_replays'] >= 1


def test_dynamic_path():
    m = _model('MiniQuartzNet', 'dynamic', 16, 4, 96)
    for sr, ch, quality in CASES[:2]:
        _check(m, sr, ch, quality)
    assert type(m._engine).__name__ == 'DynamicRunner'


def test_cli_input_rate_equals_the_16k_path_on_the_twins_output(tmp_path):
    man = tmp_path / 'manifest.json'
    texts = ['hello world', 'a b', 'telephone speech']
    x, lens = _batch(8000, 1, 2.0, 8)
    with open(man, 'w') as f:
        for i, n in enumerate(lens):
            p = str(tmp_path / f'u{i}.wav')
            with wave.open(p, 'wb') as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(8000)
                w.writeframes(x[i, :n].astype('<i2').tobytes())
            f.write(json.dumps(dict(audio_filepath=p, duration=n / 8000, text=texts[i])) + '\n')
    dump = tmp_path / 'hyps.json'
    cmd = [sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
           '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--synthetic_calib', '2', '--percentile', '99.996',
           '--input_rate', '8000', '--resample_quality', 'fast', '--dump_hyps', str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'path: static integer engine (HIP)' in out.stdout
    with open(dump, encoding='utf-8') as f:
        rec = json.load(f)
    m = _model('QuartzNet15x5Base-En', 'static', 64, 2, 500, percentile=99.996)
    wer = WER(vocabulary=m.decoder.vocabulary)
    plan = rs.ResamplePlan(8000, 16000, 'fast')
    want = []
    for b0 in (0, 2):                                                # the loader's batches: rows padded to the batch's longest
        rows, ln = x[b0:b0 + 2, :max(lens[b0:b0 + 2])], lens[b0:b0 + 2]
        y, yl = rs.resample_host(rows, ln, plan)
        _, _, greedy = m(input_signal=torch.from_numpy(y).cuda(), input_signal_length=torch.tensor(yl.astype(np.int64)).cuda())
        want += wer.ctc_decoder_predictions_tensor(greedy)
    assert rec['hypotheses'] == want and len(want) == 3 and sum(len(h) for h in want) > 0
