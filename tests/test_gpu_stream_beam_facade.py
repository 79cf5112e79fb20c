"""EncDecCTCModel.stream(beam=) on an MI355X: on the static engine, with a caller's reservation and on the dynamic path the
updates and the final hypotheses equal the host composition (qasr.stream_beam twins over the same model's per-window
log-probabilities), however the pushes are sliced; decode_stream(beam=) gives the session's hypotheses; full-window steps
replay one graph without allocating; inference.py --stream_chunk_s --beam_width prints the session's hypotheses."""
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

import beam_lm_cases  # noqa: E402
import stream_beam_cases as cases  # noqa: E402
import stream_cases as sc  # noqa: E402
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import ngram, synth  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')
KW = sc.FACADE_KW
LM_PATH = beam_lm_cases.model_path(cases.GOLDEN, 'en3')


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


@pytest.mark.parametrize('mode,with_lm,n_best,lag_s', [('static', True, 3, 0.3), ('reserved', False, 1, 0.3), ('dynamic', False, 2, 100.0)])
def test_stream_beam_equals_the_host_composition(mode, with_lm, n_best, lag_s):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(2, 3.0) if mode == 'reserved' else m.reserve(None, None)
    before = m._reserve
    lm = ngram.NgramLM.from_arpa(LM_PATH, m.decoder.vocabulary) if with_lm else None
    beam = sb.StreamBeam(width=8, n_best=n_best, cutoff_top_n=20, lm=lm, alpha=0.5, beta=0.5, lag_s=lag_s)
    audio, lens = sc.facade_audio()[:, :50000], [20000, 50000]
    try:
        slots, ups, hyps, steps, sess = cases.play_session(m, audio, lens, 11000, beam, device='cuda', **KW)
        assert m._reserve == before and (mode == 'dynamic' or sess.served == 'Engine')
        plan, bplan, want = cases.compose_on_host(m, audio, lens, beam, device='cuda', **KW)
        assert (plan.C, bplan.Lg) == (8000, 15 if lag_s < 1 else 5000) and steps == 6 + 2
        cases.check_against_composition(m, slots, ups, hyps, want, beam)
        if lag_s < 1:
            assert any(int(w['n_new_labels']) > 0 for w in want[1][:-1])         # text was committed before END
        again = cases.play_session(m, audio, lens, 8000, beam, device='cuda', **KW)
        assert repr(again[2]) == repr(hyps) and repr([again[1][s] for s in slots]) == repr([ups[s] for s in slots])
        x = torch.from_numpy(audio).cuda()
        assert repr(m.decode_stream(x, torch.tensor(lens), beam=beam, **KW)) == repr(hyps)
    finally:
        m.reserve(None, None)


def test_full_window_steps_replay_without_allocating():
    m = model('static')
    m.reserve(None, None)
    audio = torch.from_numpy(sc.facade_audio()).cuda()
    with m.stream(max_streams=2, beam=sb.StreamBeam(width=16, lag_s=0.5), **KW) as sess:
        C, Wl = sess.plan.C, sess.plan.Wl
        slot = sess.open()
        stats, text = [], ''
        for k in range(90000 // C):
            ups = sess.push([slot], audio[1:2, k * C:(k + 1) * C])
            assert len(ups) == 1
            text += ups[0].text
            if (k + 1) * C >= Wl:                                                # the window is full from here on
                stats.append(m._ragged_engine.ragged_stats())
        hyp = sess.close(slot)
        assert m._reserve == (2, Wl / 16000.0)
    assert m._reserve is None and len(stats) >= 6 and len(text) > 0 and hyp.text.startswith(text) and hyp.score is None
    assert stats[-1]['device_allocs'] == stats[0]['device_allocs'] and stats[-1]['device_frees'] == stats[0]['device_frees']
    assert len(stats) - 2 <= stats[-1]['graph_replays'] - stats[0]['graph_replays'] <= len(stats) - 1      # one replay per step


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_cli_stream_beam_prints_the_sessions_hypotheses(tmp_path):
    lens = [40000, 25520]
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(2, max(lens), seed=4)
    with open(man, 'w') as f:
        for i, n in enumerate(lens):
            path = str(tmp_path / f'u{i}.wav')
            _write_wav(path, audio[i, :n])
            f.write(json.dumps(dict(audio_filepath=path, duration=n / 16000, text='hello world')) + '\n')
    dump = tmp_path / 'hyps.json'
    args = [sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
            '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--synthetic_calib', '2', '--percentile', '99.996']
    stream = ['--stream_chunk_s', '0.5', '--stream_left_s', '1.0', '--stream_right_s', '0.24']
    for bad, word in ((['--stream_beam_lag_s', '1'], '--stream_beam_lag_s'), (stream + ['--beam_width', '4', '--boost_file', 'x'], '--boost_file')):
        out = subprocess.run(args + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and word in out.stderr
    out = subprocess.run(args + stream + ['--dump_hyps', str(dump), '--beam_width', '8', '--lm_path', LM_PATH, '--alpha', '0.5', '--beta', '0.5',
                                          '--stream_beam_lag_s', '0.3'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        rec = json.load(f)
    assert rec['path'] == 'Engine' and len(rec['hypotheses']) == 2 and sum(len(h) for h in rec['hypotheses']) > 0
    # the same model, built as the tool builds it, through the session API
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
                                        'batch_size': 2, 'normalize_transcripts': False, 'shuffle': False, 'input_rate': None})
    batch = [x.cuda() for x in next(iter(m.test_dataloader()))]
    blens = batch[1].tolist()
    beam = sb.StreamBeam(width=8, lm=LM_PATH, alpha=0.5, beta=0.5, lag_s=0.3)
    with m.stream(max_streams=2, beam=beam, **KW) as sess:
        slots = [sess.open() for _ in range(2)]
        for off in range(0, max(blens), 7000):                                   # other pieces than the tool's
            live = [b for b in range(2) if off < blens[b]]
            sess.push([slots[b] for b in live], batch[0][live, off:off + 7000].float(), [min(7000, blens[b] - off) for b in live])
        hyps = [sess.close(s) for s in slots]
    assert [h.text for h in hyps] == rec['hypotheses'] and [h.utt_score for h in hyps] == rec['beam_score']
    assert [h.lm_score for h in hyps] == rec['lm_score']
