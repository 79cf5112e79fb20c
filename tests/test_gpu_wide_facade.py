"""QuartzNet15x5Base-Zh through the public interface on the engine (k_decw): EncDecCTCModel (from_synthetic -> save_to ->
restore_from -> calibrate -> forward) against OracleNet, and examples/asr/quantization/inference.py end to end on a
manifest with CJK transcripts and a .nemo of the model."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.metrics.wer import WER, word_error_rate  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import synth, topology  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZH = 'QuartzNet15x5Base-Zh'


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.set_grad_enabled(False)


@pytest.fixture(scope='module')
def zh_nemo(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('zh') / f'{ZH}.nemo')
    EncDecCTCModel.from_synthetic(ZH).save_to(path)
    return path


def _calibrated(path, batch, frames, percentile=None, ncal=2):
    m = EncDecCTCModel.restore_from(path).cuda()
    m.eval()
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    if percentile is not None:
        qm.set_percentile(m, percentile)
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([frames] * batch).cuda()
    for c in synth.make_calibration(ncal, batch, 64, frames):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    return m


def test_facade_zh_save_restore_forward_against_oracle(zh_nemo):
    from oracle import int_oracle as O
    m = _calibrated(zh_nemo, 3, 200)
    assert m.decoder.vocabulary == topology.quartznet15x5_zh().vocabulary      # the vocabulary travels in the .nemo config
    assert m.engine_ready()
    B, T = 2, 200
    x = synth.make_features(B, 64, T, 9)
    lens = [T, T]                                  # full rows: the CTC decode walks the whole padded row
    lp, el, tok = m(processed_signal=torch.from_numpy(x).cuda(), processed_signal_length=torch.tensor(lens).cuda())
    assert 'k_decw' in m._engine.op_labels() and lp.shape == (B, 100, 5207)
    wer = WER(vocabulary=m.decoder.vocabulary)
    hyps = wer.ctc_decoder_predictions_tensor(tok)
    cfg, sd, amin, amax, wbit, abit = m.export_pack_inputs()
    want = O.OracleNet(topology.conv_plan(cfg), cfg, sd, amin, amax, wbit, abit).forward(x, lens)
    assert np.array_equal(el.cpu().numpy(), want['enc_len'])
    assert np.array_equal(tok.cpu().numpy(), want['tokens'])
    assert hyps == wer.ctc_decoder_predictions_tensor(torch.from_numpy(np.asarray(want['tokens'])))
    assert all(len(h) > 0 for h in hyps)
    np.testing.assert_allclose(lp.cpu().numpy(), want['log_probs'], rtol=1e-4, atol=5e-5)


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_cli_zh_nemo_cjk_manifest(zh_nemo, tmp_path):
    """inference.py --asr_model <Zh .nemo> on CJK transcripts.  --normalize_text is argparse type=bool as in the
    reference (inference.py:53, 'Set to False for non-English'): the empty string is its False; the English
    normaliser would strip every CJK character from the references.  Hypotheses, references and WER equal what the
    calibrated host modules decode from the HIP front-end's features."""
    n_utt, samples, text = 6, 24000, '一丁 丂七'
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            n = samples - 1000 * i
            _write_wav(p, audio[i, :n])
            f.write(json.dumps(dict(audio_filepath=p, duration=n / 16000, text=text), ensure_ascii=False) + '\n')
    cli = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')
    dump = tmp_path / 'hyps.json'
    out = subprocess.run([sys.executable, cli, '--asr_model', zh_nemo, '--dataset', str(man), '--normalize_text', '',
                          '--batch_size', '3', '--synthetic_calib', '2', '--percentile', '99.996', '--weight_bit', '8',
                          '--act_bit', '8', '--dither', '0', '--dump_hyps', str(dump)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump, encoding='utf-8') as f:
        rec = json.load(f)
    assert 'path: static integer engine (HIP)' in out.stdout and rec['path'] == 'Engine'
    m = _calibrated(zh_nemo, 3, 500, percentile=99.996)
    m.preprocessor.featurizer.dither = 0.0
    m.setup_test_data(test_data_config={'sample_rate': 16000, 'manifest_filepath': str(man), 'labels': m.decoder.vocabulary,
                                        'batch_size': 3, 'normalize_transcripts': False, 'shuffle': False})
    wer = WER(vocabulary=m.decoder.vocabulary)
    labels_map = dict(enumerate(m.decoder.vocabulary))
    hyps, refs = [], []
    for batch in m.test_dataloader():
        feats, flen = m._frontend_hip(batch[0].cuda().float(), batch[1].cuda())
        e, _, sf = m.encoder(audio_signal=feats, length=flen)
        hyps += wer.ctc_decoder_predictions_tensor(m.decoder(encoder_output=e, encoder_output_scaling_factor=sf).argmax(-1))
        refs += [''.join(labels_map[c] for c in row) for row in batch[2].cpu().numpy()]
    assert rec['references'] == refs == [text] * n_utt
    assert len(rec['hypotheses']) == n_utt and all(len(h) > 0 for h in hyps)
    assert rec['hypotheses'] == hyps
    wer_value = word_error_rate(hypotheses=hyps, references=refs)
    assert rec['wer'] == wer_value and f'WER: {wer_value}' in out.stdout
