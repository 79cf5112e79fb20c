"""EncDecCTCModel.decode_long on an MI355X: on the static engine, a reserved engine and the dynamic path it equals the host
composition (qasr.longform twins) over the same model's per-window forward outputs; the reserved engine replays graphs
without allocating; the beam path equals beam_search_host on the twin-stitched candidates; PCM at another rate, transcribe
and inference.py --window_s."""
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

import longform_cases as lc  # noqa: E402
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import beam, ctc, longform as lf, resample as rs, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')
KW = dict(window_s=2.0, overlap_s=0.5, guard_s=0.1)
S_LONG = 32000 + 2 * 24000 + 10000                       # four windows of 2 s that overlap by 0.5 s; the last is ragged


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


_models = {}


def model(mode):
    if mode not in _models:
        _models[mode] = _model(mode)
    return _models[mode]


def _recordings():
    audio = torch.from_numpy(synth.make_audio(2, S_LONG, seed=8)).cuda()
    return audio, torch.tensor([30000, S_LONG]).cuda()


def _tuples(hyps):
    return [dataclasses.astuple(h) for h in hyps]


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_decode_long_equals_the_host_composition(mode):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(2, 2.0) if mode == 'reserved' else m.reserve(None, None)
    audio, lens = _recordings()
    try:
        plan, want, parts = lc.compose_on_host(m, audio, lens, batch_size=2, **KW)
        assert plan.count.tolist() == [1, 4]
        got = m.decode_long(audio, lens, batch_size=2, **KW)
        assert type(m._engine if mode == 'dynamic' else m._ragged_engine).__name__ == ('DynamicRunner' if mode == 'dynamic' else 'Engine')
        assert _tuples(got) == _tuples(want)
        assert got[0].seams_s is None and len(got[1].seams_s) == 3 and sum(len(h.text) for h in got) > 0
        assert all(1.5 * k < s < 1.5 * k + 0.5 for k, s in enumerate(got[1].seams_s, 1))
        assert got[1].end_s[-1] > 2.0 and got[1].end_s[-1] <= S_LONG / 16000 + 0.04
        # the frames the composition stitched are the model's forward tokens, its scores the log-probabilities at them
        win, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
        logp, enc_len, tokens = m(input_signal=torch.from_numpy(win[:2]).cuda(), input_signal_length=torch.from_numpy(wl[:2]).cuda().long())
        assert np.array_equal(tokens.cpu().numpy(), parts['tokens'][:2]) and np.array_equal(enc_len.cpu().numpy(), parts['enc'][:2])
        fs = logp.gather(2, tokens.long().unsqueeze(-1)).squeeze(-1).cpu().numpy()
        for b in range(2):                               # (this suite's log-probability tolerance)
            np.testing.assert_allclose(parts['frame_score'][b, :parts['enc'][b]], fs[b, :parts['enc'][b]], rtol=1e-4, atol=2e-5)
        if mode == 'static':                             # the call's own reservation is gone; decode() is what it was
            assert m._reserve is None
            short = audio[:1, :30000].contiguous()       # no recording longer than a window: decode()'s own hypotheses
            assert _tuples(m.decode_long(short, lens[:1], **KW)) == _tuples(m.decode(input_signal=short, input_signal_length=lens[:1]))
            assert _tuples(m.decode_long(audio, lens, batch_size=2, seam='middle', **KW)) == \
                _tuples(lc.compose_on_host(m, audio, lens, batch_size=2, seam='middle', **KW)[1])
    finally:
        m.reserve(None, None)


def test_reserved_engine_replays_without_allocating():
    m = model('static')
    m.reserve(2, 2.0)
    audio, lens = _recordings()
    try:
        head = audio[:1, :32000].clone()
        head[:, 30000:] = 0                                                      # (a window holds zeros behind its length)
        first = m.decode_long(head, lens[:1], batch_size=2, **KW)                # one window: the first batch
        s0 = m._ragged_engine.ragged_stats()
        got = m.decode_long(audio, lens, batch_size=2, **KW)                     # five windows: three batches
        s1 = m._ragged_engine.ragged_stats()
        assert s1['device_allocs'] == s0['device_allocs'] and s1['device_frees'] == s0['device_frees']
        assert s1['graph_replays'] >= 1 and s1['graph_replays'] + s1['graphs_captured'] + s1['eager_runs'] >= 4
        assert _tuples(first) == _tuples(got[:1])
    finally:
        m.reserve(None, None)


def test_beam_equals_the_twin_on_stitched_candidates():
    m = model('static')
    audio, lens = _recordings()
    N, W = 8, 4
    plan = m._long_plan(lens.cpu().numpy(), **KW)
    win, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
    toks, fss, encs, cids, cqs = [], [], [], [], []
    for i in range(0, plan.Wn, 3):
        logp, e, t = m(input_signal=torch.from_numpy(win[i:i + 3]).cuda(), input_signal_length=torch.from_numpy(wl[i:i + 3]).cuda().long())
        lp = logp.float().cpu().numpy()
        cid, cq = beam.topn_host(lp, N, e.cpu().numpy())
        toks.append(t.cpu().numpy().astype(np.int32)), encs.append(e.cpu().numpy().astype(np.int32))
        fss.append(logp.float().gather(2, t.long().unsqueeze(-1)).squeeze(-1).cpu().numpy())
        cids.append(cid), cqs.append(cq)
    blank = len(m.decoder.vocabulary)
    out, total, seams = lf.stitch_host(plan, np.concatenate(encs), np.concatenate(toks), np.concatenate(fss),
                                       [np.concatenate(cids), np.concatenate(cqs)], blank)
    T = int(total.max())
    res = beam.beam_search_host(out[2][:, :T], out[3][:, :T], total, blank, W, 2)
    want = beam.to_hypotheses(res, m.decoder.vocabulary)
    got = m.decode_long(audio, lens, batch_size=3, beam_width=W, n_best=2, cutoff_top_n=N, **KW)
    assert len(got) == 2 and sum(len(h[0].text) for h in got) > 0
    for g_row, w_row in zip(got, want):
        assert [(h.text, h.labels, h.utt_score) for h in g_row] == [(h.text, h.labels, h.utt_score) for h in w_row]
    assert got[1][0].seams_s == [float(s) * m.seconds_per_frame() for s in seams[2:]] and got[1][0].start_s == []
    best = m.decode_long(audio, lens, batch_size=3, beam_width=W, cutoff_top_n=N, **KW)
    assert [h.text for h in best] == [row[0].text for row in want]
    with pytest.raises(ValueError, match='beam_width'):
        m.decode_long(audio, lens, beam_width=200, **KW)


def test_pcm_at_another_rate_equals_the_twin_resampled_call():
    m = model('static')
    n = S_LONG // 2
    pcm = (np.clip(synth.make_audio(2, n, seed=9), -1, 1) * 32767).astype(np.int16)
    lens = np.array([15000, n])
    plan8 = rs.ResamplePlan(8000, 16000, m.resample_quality)
    x16, l16 = rs.resample_host(pcm, lens, plan8, 1)
    want = m.decode_long(torch.from_numpy(x16).cuda(), torch.from_numpy(l16).cuda().long(), batch_size=4, **KW)
    got = m.decode_long(torch.from_numpy(pcm).cuda(), torch.from_numpy(lens).cuda(), batch_size=4, sample_rate=8000, **KW)
    assert _tuples(got) == _tuples(want) and len(got[1].seams_s) == 3


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_transcribe_with_windows_gives_the_plain_strings(tmp_path):
    m = model('static')
    audio = synth.make_audio(3, 25520, seed=4)
    paths = []
    for i in range(3):
        paths.append(str(tmp_path / f'u{i}.wav'))
        _write_wav(paths[-1], audio[i, :25520 - 1600 * i])
    plain = m.transcribe(paths, batch_size=3, return_hypotheses=True)
    got = m.transcribe(paths, batch_size=3, return_hypotheses=True, window_s=2.0, overlap_s=0.5)
    assert [h.text for h in got] == [h.text for h in plain] and sum(len(h.text) for h in got) > 0
    assert [h.labels for h in got] == [h.labels for h in plain] and all(h.seams_s is None for h in got)
    assert m.transcribe(paths, batch_size=3, window_s=2.0, overlap_s=0.5) == [h.text for h in plain]


def _run_cli(tmp_path, tag, man, extra):
    dump = tmp_path / f'hyps_{tag}.json'
    out = subprocess.run([sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man),
                          '--weight_bit', '8', '--act_bit', '8', '--dither', '0', '--batch_size', '3', '--synthetic_calib', '2',
                          '--percentile', '99.996', '--dump_hyps', str(dump)] + extra, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        return json.load(f)


def test_cli_window_s_gives_the_plain_strings(tmp_path):
    """files of one length whose padded row ends at the encoded length (1 + S // 160 = 160 frames, a multiple of pad_to): the
    plain path's strings, which walk the padded row, are then the strings of rows cut at the encoded length"""
    S = 160 * 159 + 80
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(3, S, seed=4)
    with open(man, 'w') as f:
        for i in range(3):
            p = str(tmp_path / f'u{i}.wav')
            _write_wav(p, audio[i])
            f.write(json.dumps(dict(audio_filepath=p, duration=S / 16000, text='hello world')) + '\n')
    plain = _run_cli(tmp_path, 'plain', man, [])
    rec = _run_cli(tmp_path, 'win', man, ['--window_s', '2.0', '--overlap_s', '0.5', '--timestamps'])
    assert rec['hypotheses'] == plain['hypotheses'] and rec['wer'] == plain['wer'] and sum(len(h) for h in rec['hypotheses']) > 0
    assert rec['path'] == 'Engine' and len(rec['words']) == 3
    out = subprocess.run([sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--dataset', str(man), '--overlap_s', '1'],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and '--overlap_s needs --window_s' in out.stderr
