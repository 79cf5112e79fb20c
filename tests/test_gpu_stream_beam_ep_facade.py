"""EncDecCTCModel.stream(beam=StreamBeam(endpoint=)) on an MI355X: on the static engine, with a caller's reservation and on the
dynamic path a session equals the host composition (the emit, endpoint and beam twins over the same model's per-window
log-probabilities), however the pushes are sliced - utterances with their n-best lists, updates and tails; full-window steps
replay one graph without the engine allocating."""
import dataclasses
import os
import sys

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_lm_cases  # noqa: E402
import stream_beam_cases as sbc  # noqa: E402
import stream_beam_ep_cases as cases  # noqa: E402
import stream_cases as sc  # noqa: E402
import stream_ep_cases as ec  # noqa: E402
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import ngram, synth  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402

KW = sc.FACADE_KW
LM_PATH = beam_lm_cases.model_path(sbc.GOLDEN, 'en3')


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


def _words(m, audio, lens):
    x = torch.from_numpy(audio).cuda()
    hyps = m.decode_stream(x, torch.tensor(lens), **KW)
    out = sorted({w[:64] for h in hyps for w in h.text.split(' ')[:6] if len(w) >= 2})
    return out or ['ab']


@pytest.mark.parametrize('mode,with_lm,n_best,lag_s,boosted', [('static', True, 3, 0.1, True), ('reserved', False, 1, 0.1, False),
                                                               ('dynamic', False, 2, 100.0, True)])
def test_stream_beam_endpointing_equals_the_host_composition(mode, with_lm, n_best, lag_s, boosted):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(2, 3.0) if mode == 'reserved' else m.reserve(None, None)
    before = m._reserve
    lm = ngram.NgramLM.from_arpa(LM_PATH, m.decoder.vocabulary) if with_lm else None
    audio, lens = sc.facade_audio()[:, :50000], [20000, 50000]
    try:
        boost = [(w, 2.5) for w in _words(m, audio, lens)] if boosted else None
        open_boost, set_of = ([None, False], [0, -1]) if boosted else (None, None)           # stream 1 opts out of the set
        beam = sb.StreamBeam(width=8, n_best=n_best, cutoff_top_n=20, lm=lm, alpha=0.5, beta=0.5, lag_s=lag_s, boost=boost,
                             endpoint=ec.facade_endpointing())
        got, hyps, ups, sess = cases.play_beam_ep_session(m, audio, lens, 11000, beam, device='cuda', open_boost=open_boost, **KW)
        assert m._reserve == before and (mode == 'dynamic' or sess.served == 'Engine') and sess.steps == 6 + 2
        cbeam = dataclasses.replace(sess.beam, boost=None if not boosted else sess._sets[0], endpoint=sess.beam.endpoint)
        plan, want, steps = cases.compose_beam_utterances(m, audio, lens, cbeam, device='cuda', set_of_stream=set_of, **KW)
        assert got == want and len(want[0]) >= 2 and len(want[1]) > 3
        for i, h in zip((0, 1), hyps):
            assert want[i][-1][2] == 'end'
            assert (dataclasses.astuple(h) if n_best == 1 else [dataclasses.astuple(x) for x in h]) == want[i][-1][7 if n_best == 1 else 8]
        for i in (0, 1):
            assert len(ups[i]) == len(steps[i]) - 1
            for u, (lab, fr, tail) in zip(ups[i], steps[i]):
                assert u.labels == lab and u.tail_text == ''.join(m.decoder.vocabulary[k] for k in tail)
        if boosted:
            assert any(u[7][9] > 0.0 for u in want[0]) and all(u[7][9] == 0.0 for u in want[1])      # boost_score per utterance
        again = cases.play_beam_ep_session(m, audio, lens, 8000, beam, device='cuda', open_boost=open_boost, **KW)
        assert again[0] == got and repr(again[1]) == repr(hyps) and repr(again[2]) == repr(ups)
    finally:
        m.reserve(None, None)


def test_full_window_steps_replay_without_allocating():
    m = model('static')
    m.reserve(None, None)
    audio = torch.from_numpy(sc.facade_audio()).cuda()
    beam = sb.StreamBeam(width=16, lag_s=0.5, boost={'x': ['ab', ('the', 2.0)], 'y': ['cd']}, endpoint=ec.facade_endpointing())
    with m.stream(max_streams=2, beam=beam, **KW) as sess:
        C, Wl = sess.plan.C, sess.plan.Wl
        slot = sess.open(boost='y')
        stats, after_first, n_utts = [], [], 0
        for k in range(90000 // C):
            ups = sess.push([slot], audio[1:2, k * C:(k + 1) * C])
            assert len(ups) == 1
            n_utts += len(sess.take_utterances())
            after_first.append(m._ragged_engine.ragged_stats())                  # the first step has run: nothing is allocated from here on
            if (k + 1) * C >= Wl:                                                # the window is full from here on: one graph
                stats.append(after_first[-1])
        hyp = sess.close(slot)
        last = sess.take_utterances()
    assert len(stats) >= 6 and n_utts > 5 and last[-1].reason == 'end' and last[-1].hypothesis is hyp and hyp.boost_score is not None
    assert len(after_first) > len(stats) and all(x['device_allocs'] == after_first[0]['device_allocs'] and
                                                 x['device_frees'] == after_first[0]['device_frees'] for x in after_first)
    assert len(stats) - 2 <= stats[-1]['graph_replays'] - stats[0]['graph_replays'] <= len(stats) - 1      # one replay per step


def test_cli_beam_width_with_endpointing_puts_it_into_the_stream_beam(tmp_path):
    """inference.py --stream_chunk_s --beam_width --stream_endpoint_silence_s: the tool's utterances, texts and per-utterance
    beam scores are the session's"""
    import json
    import subprocess

    import test_gpu_stream_beam_facade as sbf
    lens = [40000, 25520]
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(2, max(lens), seed=4)
    with open(man, 'w') as f:
        for i, n in enumerate(lens):
            path = str(tmp_path / f'u{i}.wav')
            sbf._write_wav(path, audio[i, :n])
            f.write(json.dumps(dict(audio_filepath=path, duration=n / 16000, text='hello world')) + '\n')
    dump = tmp_path / 'hyps.json'
    args = [sys.executable, sbf.CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
            '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--synthetic_calib', '2', '--percentile', '99.996',
            '--stream_chunk_s', '0.5', '--stream_left_s', '1.0', '--stream_right_s', '0.24', '--beam_width', '8', '--stream_beam_lag_s', '0.1',
            '--stream_endpoint_silence_s', '0.04', '--stream_endpoint_timeout_s', '0.2', '--stream_max_utt_s', '0.5', '--stream_hard_max_s', '0.6',
            '--dump_hyps', str(dump)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        rec = json.load(f)
    assert rec['path'] == 'Engine' and len(rec['hypotheses']) == 2 and f"utterances: {rec['utterances']}" in out.stdout
    assert rec['utterances'] >= 4 and sum(len(s) for s in rec['beam_score']) == rec['utterances']        # one beam score per utterance
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
    from qasr import stream_ep as qse
    beam = sb.StreamBeam(width=8, lag_s=0.1, endpoint=qse.Endpointing(0.04, 0.2, 0.5, 0.6))
    rows = m.decode_stream(batch[0].float(), batch[1], chunk_s=0.5, left_s=1.0, right_s=0.24, beam=beam)
    assert [' '.join(u.hypothesis.text for u in row if u.hypothesis.text) for row in rows] == rec['hypotheses']
    assert [[u.hypothesis.utt_score for u in row] for row in rows] == rec['beam_score']
