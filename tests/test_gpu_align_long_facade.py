"""EncDecCTCModel.align_long on an MI355X: on the static engine, a reserved engine and the dynamic path it equals the host
chain (qasr.longform and qasr.align twins) over the same model's per-window log-probabilities; segments, refusals, the
command-line tool and inference.py --align --window_s."""
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
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import synth  # noqa: E402

CLI = os.path.join(alc.ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')


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


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_align_long_equals_the_twin_chain(mode):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(alc.BATCH, 4.0) if mode == 'reserved' else m.reserve(None, None)
    try:
        alc.check_equals_the_twin_chain(m, 'cuda')
        assert type(m._engine if mode == 'dynamic' else m._ragged_engine).__name__ == ('DynamicRunner' if mode == 'dynamic' else 'Engine')
        if mode == 'static':
            assert m._reserve is None                    # the call's own reservation is gone
            alc.check_equals_the_twin_chain(m, 'cuda', 1024)
    finally:
        m.reserve(None, None)


def test_segments_tile_the_labels_and_a_lost_path_keeps_its_text():
    alc.check_segments(model('static'), 'cuda')


def test_refusals_name_their_argument():
    alc.check_refusals(model('static'), 'cuda')


def test_the_tool_writes_the_segments_file(tmp_path):
    alc.check_tool_output(tmp_path, [])


def test_cli_align_with_window_s_goes_through_align_long(tmp_path):
    S = 16000 * 9
    man = tmp_path / 'manifest.json'
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
                          '--percentile', '99.996', '--window_s', '4.0', '--overlap_s', '1.0', '--align', str(out_path)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    recs = [json.loads(ln) for ln in out_path.read_text(encoding='utf-8').splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert r['text'] == 'hello world' and r['ctc_score'] is None and np.isfinite(r['utt_score'])
        assert [w[0] for w in r['words']] == ['hello', 'world'] and 0 <= r['words'][0][1] <= r['words'][1][2] <= 9.1
