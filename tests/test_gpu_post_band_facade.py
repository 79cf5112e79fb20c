"""Banded posteriors through the facade on an MI355X: align_long(posteriors=True) on the static engine and under a reservation
equals the host composition (the longform twins, align_band_host and post_band_host over the same model's per-window
log-probabilities) field by field; under a reservation the engine allocates nothing after the first call; inference.py
--align --window_s --posteriors writes the new fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_long_cases as alc  # noqa: E402
import post_band_cases as pbc  # noqa: E402
from test_gpu_align_long_facade import CLI, model  # noqa: E402  (the committed mini net, calibrated once per process)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def test_static_engine():
    m = model('static')
    m.reserve(None, None)
    pbc.check_facade(m, 'cuda')
    assert type(m._engine).__name__ == 'Engine'


def test_under_a_reservation_the_engine_allocates_nothing_after_the_first_call():
    m = model('static')
    m.reserve(alc.BATCH, 4.0)
    try:
        first = pbc.check_facade(m, 'cuda')
        assert type(m._ragged_engine).__name__ == 'Engine'
        s0 = m._ragged_engine.ragged_stats()
        again = pbc.check_facade(m, 'cuda')
        s1 = m._ragged_engine.ragged_stats()
        assert s1['device_allocs'] == s0['device_allocs'] and s1['device_frees'] == s0['device_frees']
        assert [(h.post, h.ctc_score) for h in again] == [(h.post, h.ctc_score) for h in first]
    finally:
        m.reserve(None, None)


def test_cli_align_with_window_s_and_posteriors(tmp_path):
    S = 16000 * 9
    man = tmp_path / 'manifest.json'
    from qasr import synth
    audio = synth.make_audio(2, S, seed=4)
    with open(man, 'w') as f:
        for i in range(2):
            p = str(tmp_path / f'u{i}.wav')
            alc.write_wav(p, audio[i])
            f.write(json.dumps(dict(audio_filepath=p, duration=S / 16000, text='hello world')) + '\n')
    calib = tmp_path / 'calib.npz'                        # the mini net has 16 features: its own calibration batches
    np.savez(str(calib), *synth.make_calibration(2, 2, 16, 200))
    out_path = tmp_path / 'aligned.jsonl'
    out = subprocess.run([sys.executable, CLI, '--asr_model', 'MiniQuartzNet', '--synthetic_model', '--dataset', str(man),
                          '--weight_bit', '8', '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--load', str(calib),
                          '--percentile', '99.996', '--window_s', '4.0', '--overlap_s', '1.0', '--align', str(out_path), '--posteriors'],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    recs = [json.loads(ln) for ln in out_path.read_text(encoding='utf-8').splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert r['text'] == 'hello world' and np.isfinite(r['ctc_score']) and r['utt_score'] <= r['ctc_score'] + 1e-3
        assert [w[0] for w in r['words']] == ['hello', 'world'] and len(r['post']) == 2 and all(0.0 <= v <= 1.0 for v in r['post'])
