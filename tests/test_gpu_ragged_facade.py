"""EncDecCTCModel.reserve and inference.py --reserve on an MI355X: forward / decode / transcribe through the reserved
engine give what a second model without reserve() gives - the path the other suites pin - bit for bit."""
import json
import os
import subprocess
import sys
import warnings
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _model(seed=2):
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=seed).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([96] * 4).cuda()
    for c in synth.make_calibration(3, 4, 16, 96, seed):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    return m


def _hyp_tuple(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words)


def _batches(seed, n, max_batch, max_samples):
    rng = np.random.default_rng(seed)
    for i in range(n):
        B = int(rng.integers(1, max_batch + 1)) if i else max_batch
        S = int(rng.integers(4000, max_samples + 1)) if i else max_samples
        audio = torch.from_numpy(synth.make_audio(B, S, seed=seed + i)).cuda()
        alen = [S] + [int(v) for v in rng.integers(500, S + 1, B - 1)]
        yield audio, torch.tensor(alen).cuda()


def test_forward_and_decode_equal_the_unreserved_model():
    ref, res = _model(), _model()
    for m in (ref, res):
        m.preprocessor.featurizer.pad_to = 16
    assert res.reserve(4, 2.0) is res
    kept = []
    for k, (audio, alen) in enumerate(_batches(11, 12, 4, 32000)):
        want = ref(input_signal=audio, input_signal_length=alen)
        got = res(input_signal=audio, input_signal_length=alen)
        torch.cuda.synchronize()
        for g, w, what in zip(got, want, ('log_probs', 'encoded lengths', 'tokens')):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (k, what)
        hw = ref.decode(input_signal=audio, input_signal_length=alen)
        hg = res.decode(input_signal=audio, input_signal_length=alen)
        assert [_hyp_tuple(h) for h in hg] == [_hyp_tuple(h) for h in hw], k
        for prev_got, prev_want in kept:                       # results of earlier batches are copies: still intact
            for g, w in zip(prev_got, prev_want):
                assert torch.equal(g, w), k
        kept = (kept + [(got, want)])[-2:]
    eng = res._ragged_engine
    assert type(eng).__name__ == 'Engine' and res._engine is None         # everything ran on the reserved engine
    st = eng.ragged_stats()
    assert sum(st['buckets'].values()) == 24 and st['graph_replays'] == 24 - len(st['buckets']) and st['graphs_captured'] >= 1
    # features in (processed_signal): the feature entry of the same engine
    x = torch.from_numpy(synth.make_features(3, 16, 150, 7)).cuda()
    lens = torch.tensor([150, 129, 4]).cuda()
    for g, w in zip(res(processed_signal=x, processed_signal_length=lens), ref(processed_signal=x, processed_signal_length=lens)):
        assert torch.equal(g, w)
    allocs = eng.ragged_stats()['device_allocs']
    # outside the envelope: today's path, one warning, same results
    audio = torch.from_numpy(synth.make_audio(5, 20000, seed=3)).cuda()
    alen = torch.tensor([20000, 15000, 9000, 700, 20000]).cuda()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        got = res(input_signal=audio, input_signal_length=alen)
        got2 = res(input_signal=audio, input_signal_length=alen)
    assert len([w for w in rec if 'reserved envelope' in str(w.message)]) == 1
    want = ref(input_signal=audio, input_signal_length=alen)
    for g, g2, w in zip(got, got2, want):
        assert torch.equal(g, w) and torch.equal(g2, w)
    assert eng.ragged_stats()['device_allocs'] == allocs and type(res._engine).__name__ == 'Engine'


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def _wavs(tmp_path, n, seed):
    rng = np.random.default_rng(seed)
    audio = synth.make_audio(n, 40000, seed=seed)
    paths, lens = [], []
    for i in range(n):
        k = 40000 if i == 0 else int(rng.integers(6000, 40000))
        p = str(tmp_path / f'r{i}.wav')
        _write_wav(p, audio[i, :k])
        paths.append(p)
        lens.append(k)
    return paths, lens


def test_transcribe_equals_the_unreserved_model(tmp_path):
    ref, res = _model(), _model()
    res.reserve(3, 2.5)
    paths, _ = _wavs(tmp_path, 8, 5)
    assert res.transcribe(paths, batch_size=3) == ref.transcribe(paths, batch_size=3)
    hg = res.transcribe(paths, batch_size=3, return_hypotheses=True)
    hw = ref.transcribe(paths, batch_size=3, return_hypotheses=True)
    assert [_hyp_tuple(h) for h in hg] == [_hyp_tuple(h) for h in hw]
    lg, lw = res.transcribe(paths, batch_size=3, logprobs=True), ref.transcribe(paths, batch_size=3, logprobs=True)
    assert len(lg) == len(lw) == 8 and all(torch.equal(a, b) for a, b in zip(lg, lw))
    assert res._engine is None and sum(res._ragged_engine.ragged_stats()['buckets'].values()) == 9


def test_cli_reserve_prints_the_same_hypotheses_and_wer(tmp_path):
    paths, lens = _wavs(tmp_path, 7, 9)
    man = tmp_path / 'manifest.json'
    with open(man, 'w') as f:
        for p, n in zip(paths, lens):
            f.write(json.dumps(dict(audio_filepath=p, duration=n / 16000, text='hello world')) + '\n')
    recs = []
    for tag, extra in (('plain', []), ('reserve', ['--reserve', '2.5'])):
        dump = tmp_path / f'hyps_{tag}.json'
        out = subprocess.run([sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man),
                              '--weight_bit', '8', '--act_bit', '8', '--dither', '0', '--batch_size', '3', '--synthetic_calib', '2',
                              '--percentile', '99.996', '--dump_hyps', str(dump)] + extra, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        assert 'static integer engine (HIP)' in out.stdout
        with open(dump, encoding='utf-8') as f:
            recs.append((json.load(f), [ln for ln in out.stdout.splitlines() if ln.startswith('WER:')]))
    (plain, wer_plain), (resv, wer_resv) = recs
    assert resv['hypotheses'] == plain['hypotheses'] and resv['wer'] == plain['wer'] and wer_plain == wer_resv and wer_plain
    assert sum(len(h) for h in plain['hypotheses']) > 0
