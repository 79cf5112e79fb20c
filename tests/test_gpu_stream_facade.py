"""EncDecCTCModel.stream on an MI355X: on the static engine, with a caller's reservation and on the dynamic path the updates and
the final hypotheses equal the host composition (qasr.stream twins) over the same model's per-window forwards; on the static
engine a stream's result does not depend on its neighbours; full-window steps replay one graph without allocating; the
caller's reservation comes back; inference.py --stream_chunk_s prints the session's hypotheses."""
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
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')
KW = sc.FACADE_KW


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


def _tuples(xs):
    return [dataclasses.astuple(x) for x in xs]


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_stream_equals_the_host_composition(mode):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(2, 3.0) if mode == 'reserved' else m.reserve(None, None)
    before = m._reserve
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    try:
        slots, ups, hyps, steps = sc.play_session(m, audio, lens, 11000, device='cuda', **KW)      # pieces that split unequally
        assert m._reserve == before                                              # the session's own reservation is gone
        # the composition runs the same model's forwards of the same window batches - on the static engine without the
        # session's reservation, which gives the same bits
        plan, want = sc.compose_on_host(m, audio, lens, device='cuda', **KW)
        assert (plan.C, plan.L, plan.Rr) == (8000, 16000, 3840) and steps == 11 + 2      # chunks 1 - 3 shared, 4 - 11 alone, two END steps
        sc.check_against_composition(m, slots, ups, hyps, want, lens)
        assert sum(len(h.text) for h in hyps) > 0
        again = sc.play_session(m, audio, lens, 8000, device='cuda', **KW)
        assert _tuples(again[2]) == _tuples(hyps) and [_tuples(again[1][s]) for s in slots] == [_tuples(ups[s]) for s in slots]
        if mode == 'static':                                                     # a row does not depend on its neighbours
            alone = sc.play_session(m, audio, lens, 11000, device='cuda', streams=(1,), **KW)
            assert _tuples(alone[2]) == _tuples(hyps[1:]) and _tuples(alone[1][alone[0][0]]) == \
                [dataclasses.astuple(dataclasses.replace(u, slot=alone[0][0])) for u in ups[slots[1]]]
    finally:
        m.reserve(None, None)


def test_full_window_steps_replay_without_allocating():
    m = model('static')
    m.reserve(None, None)
    audio = torch.from_numpy(sc.facade_audio()).cuda()
    with m.stream(max_streams=2, **KW) as sess:
        C, Wl = sess.plan.C, sess.plan.Wl
        slot = sess.open()
        stats, n_steps = [], 0
        for k in range(90000 // C):
            ups = sess.push([slot], audio[1:2, k * C:(k + 1) * C])
            assert len(ups) == 1
            if (k + 1) * C >= Wl:                                                # the window is full from here on
                stats.append(m._ragged_engine.ragged_stats())
        hyp = sess.close(slot)
        n_steps = len(stats)
        assert m._reserve == (2, Wl / 16000.0)
    assert m._reserve is None and n_steps >= 6 and len(hyp.text) > 0
    assert stats[-1]['device_allocs'] == stats[0]['device_allocs'] and stats[-1]['device_frees'] == stats[0]['device_frees']
    assert stats[-1]['graph_replays'] - stats[0]['graph_replays'] >= n_steps - 2


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_cli_stream_chunk_s_prints_the_sessions_hypotheses(tmp_path):
    lens = [40000, 33000, 25520]
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(3, max(lens), seed=4)
    paths = []
    with open(man, 'w') as f:
        for i, n in enumerate(lens):
            paths.append(str(tmp_path / f'u{i}.wav'))
            _write_wav(paths[-1], audio[i, :n])
            f.write(json.dumps(dict(audio_filepath=paths[-1], duration=n / 16000, text='hello world')) + '\n')
    dump = tmp_path / 'hyps.json'
    args = [sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
            '--act_bit', '8', '--dither', '0', '--batch_size', '3', '--synthetic_calib', '2', '--percentile', '99.996']
    out = subprocess.run(args + ['--stream_left_s', '1'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and '--stream_chunk_s' in out.stderr
    out = subprocess.run(args + ['--dump_hyps', str(dump), '--stream_chunk_s', '0.5', '--stream_left_s', '1.0', '--stream_right_s', '0.24'],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        rec = json.load(f)
    assert rec['path'] == 'Engine' and len(rec['hypotheses']) == 3 and sum(len(h) for h in rec['hypotheses']) > 0
    # the same model, built as the tool builds it, through the session API
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En').cuda()
    m.preprocessor.featurizer.dither = 0.0
    m.eval()
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    qm.set_percentile(m, 99.996)
    m.encoder.bn_folding()
    qm.calibrate(m)
    for c in synth.make_calibration(2, 3, 64, 500):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=torch.tensor([500] * 3).cuda())
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    m.setup_test_data(test_data_config={'sample_rate': 16000, 'manifest_filepath': str(man), 'labels': m.decoder.vocabulary,
                                        'batch_size': 3, 'normalize_transcripts': False, 'shuffle': False, 'input_rate': None})
    batch = [x.cuda() for x in next(iter(m.test_dataloader()))]
    lens = batch[1].tolist()
    with m.stream(max_streams=3, **KW) as sess:
        slots = [sess.open() for _ in range(3)]
        for off in range(0, max(lens), 7000):                                    # other pieces than the tool's
            live = [b for b in range(3) if off < lens[b]]
            sess.push([slots[b] for b in live], batch[0][live, off:off + 7000].float(), [min(7000, lens[b] - off) for b in live])
        texts = [sess.close(s).text for s in slots]
    assert texts == rec['hypotheses']
