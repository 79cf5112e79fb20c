"""EncDecCTCModel.stream(input_rate=) on an MI355X: on the calibrated model a session fed int16 PCM at 8 kHz gives the
hypotheses and updates of a session at the model's rate fed k_resample's output of the same audio, however the pushes are
sliced; full-window steps replay one graph without allocating; inference.py --stream_chunk_s --input_rate prints what
decode_stream(..., input_rate=) gives."""
import dataclasses
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

import stream_cases as sc  # noqa: E402
import test_gpu_stream_facade as plain  # noqa: E402
import test_stream_rs_cpu as cpu  # noqa: E402
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import synth  # noqa: E402

KW = sc.FACADE_KW
RATE = 8000


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def test_the_session_equals_the_models_rate_session_on_k_resamples_output():
    from qasr import engine, resample as rs
    m = plain.model('static')
    m.reserve(None, None)
    x, lens = cpu.facade_pcm(RATE, 1, lens_s=(1.9, 5.6))
    plan = rs.ResamplePlan(RATE, 16000, m.resample_quality)
    y, yl = engine.resample(torch.from_numpy(x).cuda(), torch.tensor(lens).cuda(), plan)
    want = cpu.play(m, y.cpu().numpy(), yl.tolist(), 11000, device='cuda')
    assert sum(len(h[0]) for h in want[0]) > 0
    for piece in (int(0.7 * RATE), 333):
        got = cpu.play(m, x, lens, piece, device='cuda', input_rate=RATE)
        assert got == want, piece
    assert m._reserve is None


def test_full_window_steps_replay_without_allocating():
    m = plain.model('static')
    m.reserve(None, None)
    x, lens = cpu.facade_pcm(RATE, 1, lens_s=(1.9, 5.6))
    pcm = torch.from_numpy(x).cuda()
    with m.stream(max_streams=2, input_rate=RATE, **KW) as sess:
        A, Wl = sess.rs_plan.Ain, sess.plan.Wl
        assert A == sess.plan.C // 2
        slot = sess.open()
        stats, done = [], 0
        for k in range(lens[1] // A):
            done += len(sess.push([slot], pcm[1:2, k * A:(k + 1) * A]))
            assert done in (k, k + 1)                                            # a chunk per push, the filter's reach late
            if done * sess.plan.C >= Wl:                                         # the window is full from here on
                stats.append(m._ragged_engine.ragged_stats())
        hyp = sess.close(slot)
    assert len(stats) >= 6 and len(hyp.text) > 0
    assert stats[-1]['device_allocs'] == stats[0]['device_allocs'] and stats[-1]['device_frees'] == stats[0]['device_frees']
    assert stats[-1]['graph_replays'] - stats[0]['graph_replays'] >= len(stats) - 2


def _write_wav(path, x, rate):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(x.astype('<i2').tobytes())


def test_cli_stream_chunk_s_with_input_rate(tmp_path):
    x, lens = cpu.facade_pcm(RATE, 1, lens_s=(2.5, 2.0), seed=4)
    man = tmp_path / 'manifest.json'
    with open(man, 'w') as f:
        for i, n in enumerate(lens):
            path = str(tmp_path / f'u{i}.wav')
            _write_wav(path, x[i, :n], RATE)
            f.write(json.dumps(dict(audio_filepath=path, duration=n / RATE, text='hello world')) + '\n')
    dump = tmp_path / 'hyps.json'
    args = [sys.executable, plain.CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
            '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--synthetic_calib', '2', '--percentile', '99.996',
            '--dump_hyps', str(dump), '--stream_chunk_s', '0.5', '--stream_left_s', '1.0', '--stream_right_s', '0.24',
            '--input_rate', str(RATE)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        rec = json.load(f)
    assert rec['path'] == 'Engine' and len(rec['hypotheses']) == 2 and sum(len(h) for h in rec['hypotheses']) > 0
    # the same model, built as the tool builds it, through decode_stream
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En').cuda()
    m.preprocessor.featurizer.dither = 0.0
    m.eval()
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    qm.set_percentile(m, 99.996)
    m.encoder.bn_folding()
    qm.calibrate(m)
    for c in synth.make_calibration(2, 2, 64, 500):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=torch.tensor([500] * 2).cuda())
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    m.setup_test_data(test_data_config={'sample_rate': 16000, 'manifest_filepath': str(man), 'labels': m.decoder.vocabulary,
                                        'batch_size': 2, 'normalize_transcripts': False, 'shuffle': False, 'input_rate': RATE})
    batch = [t.cuda() for t in next(iter(m.test_dataloader()))]
    assert batch[0].dtype == torch.int16
    hyps = m.decode_stream(batch[0], batch[1], input_rate=RATE, **KW)
    assert [h.text for h in hyps] == rec['hypotheses']
