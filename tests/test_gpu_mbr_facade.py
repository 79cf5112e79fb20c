"""EncDecCTCModel.decode(mbr=) and error_rate(mbr=) on an MI355X: the lists in MBR order, posterior / mbr_risk / beam_rank and
the counts of the picks equal the host composition - rerank_texts over decode(n_best=)'s texts and scores, word_error_rate over
the picks' texts - on the static engine, a reserved engine and the dynamic path; without mbr the calls return what they did."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.metrics.wer import _levenshtein  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import mbr, synth  # noqa: E402


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


def _io(seed=3):
    audio = torch.from_numpy(synth.make_audio(5, 24000, seed=seed)).cuda()
    return dict(input_signal=audio, input_signal_length=torch.tensor([24000, 20000, 16001, 9000, 4000]).cuda())


def _check(m, io, mode, scale):
    """decode(mbr=) against rerank_texts over decode(n_best=)'s lists; error_rate(mbr=) against the picks' texts"""
    plain = m.decode(**io, beam_width=8, n_best=4)
    got = m.decode(**io, beam_width=8, n_best=4, mbr=mode, mbr_scale=scale)
    want = mbr.rerank_texts([[h.text for h in row] for row in plain], [[h.utt_score for h in row] for row in plain],
                            use_cer=mode == 'char', scale=scale)
    assert len(got) == len(plain) == 5
    for row, base, w in zip(got, plain, want):
        assert [h.beam_rank for h in row] == w.order and sorted(w.order) == list(range(len(base)))
        for h in row:
            k = h.beam_rank
            assert (h.text, h.labels, h.utt_score) == (base[k].text, base[k].labels, base[k].utt_score)
            assert h.posterior == w.posterior[k] and h.mbr_risk == w.expected_errors[k]
        assert row[0].mbr_risk <= min(h.mbr_risk for h in row if h.beam_rank == 0) and abs(sum(h.posterior for h in row) - 1) < 1e-12
    # the counts of the picks, against references made from the beam's own texts so that the rows differ in errors
    refs = [row[-1].text if row[-1].text else 'a' for row in plain]
    use_cer = mode == 'char'
    rep = m.error_rate(**io, texts=refs, use_cer=use_cer, beam_width=8, n_best=4, mbr=mode, mbr_scale=scale)
    base = m.error_rate(**io, texts=refs, use_cer=use_cer, beam_width=8, n_best=4)
    assert rep.mbr_pick == [w.pick for w in want] and base.mbr_total is None and base.mbr_pick is None
    assert (rep.total, rep.oracle_errors, rep.per_utterance) == (base.total, base.oracle_errors, base.per_utterance)
    cut = (lambda t: list(t)) if use_cer else (lambda t: t.split())
    picks = [row[0].text for row in got]
    errors, units = sum(_levenshtein(cut(h), cut(r)) for h, r in zip(picks, refs)), sum(len(cut(r)) for r in refs)
    assert (rep.mbr_total.errors, rep.mbr_total.ref_units) == (errors, units)        # word_error_rate's numerator and denominator
    assert rep.mbr_total.rate == (errors / units if units else float('inf'))
    assert rep.oracle_errors <= rep.mbr_total.errors
    return got


@pytest.mark.parametrize('path', ['static', 'dynamic'])
def test_decode_and_error_rate_equal_the_host_composition(path):
    m = model(path)
    m.reserve(None, None)
    m.preprocessor.featurizer.pad_to = 16
    io = _io()
    _check(m, io, 'word', 1.0)
    got = _check(m, io, 'char', 0.25)
    assert any(len(row) >= 2 for row in got)
    # timestamps align the rows as they lie; the lists are re-ordered afterwards
    timed = m.decode(**io, beam_width=8, n_best=4, mbr='char', mbr_scale=0.25, timestamps=True)
    plain = m.decode(**io, beam_width=8, n_best=4, timestamps=True)
    for row, base, ref in zip(timed, plain, got):
        assert [h.beam_rank for h in row] == [h.beam_rank for h in ref]
        for h in row:
            assert (h.start_s, h.end_s, h.words) == (base[h.beam_rank].start_s, base[h.beam_rank].end_s, base[h.beam_rank].words)


def test_under_a_reservation_the_engine_allocates_nothing_after_the_first_batch():
    m = model('static')
    m.preprocessor.featurizer.pad_to = 16
    m.reserve(5, 2.0)
    try:
        first = _check(m, _io(), 'word', 1.0)
        s0 = m._ragged_engine.ragged_stats()
        again = _check(m, _io(seed=4), 'word', 1.0)
        s1 = m._ragged_engine.ragged_stats()
        assert s1['device_allocs'] == s0['device_allocs'] and s1['device_frees'] == s0['device_frees']
        assert [[h.text for h in row] for row in first] != [[h.text for h in row] for row in again]      # another batch
    finally:
        m.reserve(None, None)


def test_calls_without_mbr_return_what_they_returned_and_refusals_are_by_name():
    m = model('static')
    m.reserve(None, None)
    m.preprocessor.featurizer.pad_to = 16
    io = _io()
    a = m.decode(**io, beam_width=8, n_best=4)
    b = m.decode(**io, beam_width=8, n_best=4, mbr=None, mbr_scale=3.0)
    assert [[dataclasses.astuple(h) for h in row] for row in a] == [[dataclasses.astuple(h) for h in row] for row in b]
    assert all(h.posterior is None and h.mbr_risk is None and h.beam_rank is None for row in a for h in row)
    best = m.decode(**io, beam_width=8)
    assert [h.text for h in best] == [row[0].text for row in a]
    with pytest.raises(ValueError, match='mbr needs beam_width'):
        m.decode(**io, mbr='word')
    with pytest.raises(ValueError, match='mbr needs n_best >= 2'):
        m.decode(**io, beam_width=8, mbr='word')
    with pytest.raises(ValueError, match="mbr must be None, 'word' or 'char'"):
        m.decode(**io, beam_width=8, n_best=4, mbr='phone')
    with pytest.raises(ValueError, match='mbr_scale must be a number in 0 .. 16'):
        m.decode(**io, beam_width=8, n_best=4, mbr='word', mbr_scale=16.5)
    with pytest.raises(ValueError, match='decode_long: mbr is not built for long recordings'):
        m.decode_long(io['input_signal'], io['input_signal_length'], beam_width=8, n_best=4, mbr='word')
    on_dev = mbr.rerank_texts([['a b', 'a c', 'a c'], ['x']], [[-1.0, -1.5, -1.5], [-2.0]], device='cuda')
    on_host = mbr.rerank_texts([['a b', 'a c', 'a c'], ['x']], [[-1.0, -1.5, -1.5], [-2.0]])
    assert on_dev == on_host and on_dev[0].pick == 1


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_mbr_prints_the_picks_wer_and_refuses_by_name(tmp_path):
    import json
    import os
    import re
    import subprocess
    import sys
    import wave
    from nemo.collections.asr.metrics.wer import word_error_rate
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'q-asr_amd', 'examples', 'asr', 'quantization',
                       'inference.py')
    n_utt, samples = 4, 24000
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            with wave.open(p, 'wb') as w:
                w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
                w.writeframes((np.clip(audio[i, :samples - 1000 * i], -1, 1) * 32767).astype('<i2').tobytes())
            f.write(json.dumps(dict(audio_filepath=p, duration=(samples - 1000 * i) / 16000, text='hello wide world'[:16 - i])) + '\n')
    base = [sys.executable, cli, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
            '--act_bit', '8', '--dither', '0', '--batch_size', '4', '--synthetic_calib', '2', '--percentile', '99.996']
    for extra, msg in ((['--mbr', 'word'], '--mbr needs --beam_width'),
                       (['--mbr', 'word', '--beam_width', '4', '--n_best', '1'], '--mbr needs --n_best K with K >= 2'),
                       (['--mbr_scale', '2'], '--mbr_scale needs --mbr')):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and msg in out.stderr, (extra, out.stderr[-500:])
    dump = tmp_path / 'mbr.json'
    out = subprocess.run(base + ['--device_wer', '--cer', '--beam_width', '4', '--n_best', '3', '--mbr', 'char', '--mbr_scale', '0.5',
                                 '--dump_hyps', str(dump)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split(':')[0] for ln in out.stdout.splitlines() if re.match(r'^(WER|S / D / I|MBR WER|oracle WER):', ln)]
    assert lines == ['WER', 'S / D / I', 'MBR WER', 'oracle WER']
    printed = lambda key: float(re.search(rf'^{re.escape(key)} (.*)$', out.stdout, re.M).group(1))
    rec = json.load(open(dump))
    assert printed('MBR WER:') == rec['mbr_wer'] == word_error_rate(rec['hypotheses'], rec['references'], use_cer=True)
    assert printed('oracle WER:') <= printed('MBR WER:') and printed('oracle WER:') <= printed('WER:') == rec['wer']
    assert len(rec['posterior']) == len(rec['mbr_risk']) == n_utt and all(0 < p <= 1 for p in rec['posterior'])
    assert rec['mbr'] == 'char' and rec['mbr_scale'] == 0.5 and rec['n_best'] == 3
