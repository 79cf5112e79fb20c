"""EncDecCTCModel.spot / spot_long on an MI355X: on the static engine, a reserved engine and the dynamic path they equal the
host composition star_host + spot_host + to_hits over the device's own log-probabilities (for spot_long: over the rows of the
host chain cut_host, forward per batch, stitch_host); refusals name their argument."""
import os
import sys

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_long_cases as alc  # noqa: E402
import spot_facade_cases as fc  # noqa: E402
from test_gpu_align_long_facade import model  # noqa: E402  (the committed mini net, calibrated once per process)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_spot_and_spot_long_equal_the_host_composition(mode):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(alc.BATCH, 4.0) if mode == 'reserved' else m.reserve(None, None)
    try:
        fc.check_spot(m, 'cuda')
        fc.check_spot_long(m, 'cuda')
        assert type(m._engine if mode == 'dynamic' else m._ragged_engine).__name__ == ('DynamicRunner' if mode == 'dynamic' else 'Engine')
    finally:
        m.reserve(None, None)


def test_refused_arguments_are_refused_by_name():
    m = model('static')
    m.reserve(None, None)
    fc.check_refusals(m, 'cuda')


def test_cli_spot_with_and_without_windows(tmp_path):
    """inference.py --spot_file FILE --spot OUT: one JSON line per manifest entry; with --window_s through spot_long; the
    keywords of a recording shorter than a window are found at the same places either way"""
    import json
    import subprocess

    import numpy as np

    from qasr import synth
    from test_gpu_align_long_facade import CLI
    S = 16000 * 3
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(2, S, seed=4)
    with open(man, 'w') as f:
        for i in range(2):
            p = str(tmp_path / f'u{i}.wav')
            alc.write_wav(p, audio[i])
            f.write(json.dumps(dict(audio_filepath=p, duration=S / 16000, text='hello world')) + '\n')
    calib = tmp_path / 'calib.npz'                        # the mini net has 16 features: its own calibration batches
    np.savez(str(calib), *synth.make_calibration(2, 2, 16, 200))
    words = tmp_path / 'keywords.txt'
    words.write_text('# a comment\nab\n\nc d\ne\n', encoding='utf-8')
    base = [sys.executable, CLI, '--asr_model', 'MiniQuartzNet', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
            '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--load', str(calib), '--percentile', '99.996']
    recs = {}
    for name, extra in (('plain', []), ('long', ['--window_s', '4.0', '--overlap_s', '1.0'])):
        out_path = tmp_path / f'{name}.jsonl'
        out = subprocess.run(base + ['--spot_file', str(words), '--spot', str(out_path), '--spot_threshold', '-6', '--spot_max_span_s', '1.0']
                             + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        recs[name] = [json.loads(ln) for ln in out_path.read_text(encoding='utf-8').splitlines()]
        assert len(recs[name]) == 2 and 'spotted' in out.stdout
        for r in recs[name]:
            assert r['audio_filepath'].endswith('.wav') and len(r['hits']) > 0
            assert all(set(h) == {'keyword', 'start', 'end', 'score'} and h['keyword'] in ('ab', 'c d', 'e') for h in r['hits'])
            assert all(0 <= h['start'] < h['end'] <= 3.1 and -6.0 <= h['score'] <= 0 for h in r['hits'])
            assert [h['start'] for h in r['hits']] == sorted(h['start'] for h in r['hits'])
    assert recs['plain'] == recs['long']
    bad = subprocess.run(base + ['--spot', str(tmp_path / 'x.jsonl')], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and '--spot OUT and --spot_file FILE go together' in bad.stderr
