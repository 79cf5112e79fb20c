"""EncDecCTCModel.align and decode(beam_width=, timestamps=True) on an MI355X: on the static engine (synthetic QuartzNet15x5 En
and Zh), a reserved engine with ragged batches and the dynamic device path, the hypotheses equal the NumPy twin (qasr.align)
run on the same call's log-probabilities copied to the host, and decode(beam_width=) without timestamps is what it was."""
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

import align_cases  # noqa: E402
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import align, beam, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _model(name, mode, feat_in, batch, frames, ncal=2, seed=2, percentile=None):
    m = EncDecCTCModel.from_synthetic(name, seed=seed).cuda() if name == 'MiniQuartzNet' else EncDecCTCModel.from_synthetic(name).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    if percentile is not None:
        qm.set_percentile(m, percentile)
    m.encoder.bn_folding()
    if mode == 'static':
        qm.calibrate(m)
        L = torch.tensor([frames] * batch).cuda()
        cal = synth.make_calibration(ncal, batch, feat_in, frames, seed) if name == 'MiniQuartzNet' else \
            synth.make_calibration(ncal, batch, feat_in, frames)
        for c in cal:
            e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
            m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, mode == 'dynamic')
    return m


def _tuples(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words, h.lm_score, h.ctc_score)


def _check_against_twin(m, W, nb, texts=False, **inputs):
    vocab = m.decoder.vocabulary
    blank, spf = len(vocab), m.seconds_per_frame()
    logp, enc_len, _ = m(**inputs)
    torch.cuda.synchronize()
    lp, ln = logp.cpu().numpy(), enc_len.cpu().numpy()
    B, T = lp.shape[:2]
    greedy = m.decode(**inputs)
    # ---- align(labels=): the greedy labels, the greedy labels with one dropped, a transcript of its own, in turn
    rows = []
    for b, h in enumerate(greedy):
        ids = list(h.labels)
        rows.append(ids if b % 3 == 0 else ids[:len(ids) // 2] + ids[len(ids) // 2 + 1:] if b % 3 == 1 else [1, 2, 2, 0, 3])
    tg, tl = align_cases.pad_targets(rows, blank)
    twin = align.align_host(lp, ln, tg, tl, blank)
    want = align.to_hypotheses(twin, vocab, spf)
    got = m.align(**inputs, labels=rows)
    assert [_tuples(h) for h in got] == [_tuples(h) for h in want]
    assert twin.ok.sum() >= 1 and any(h.start_s for h in got)
    for b, h in enumerate(got):
        if twin.ok[b]:
            assert h.ctc_score >= h.utt_score and all(0 <= s < e <= ln[b] * spf + 1e-9 for s, e in zip(h.start_s, h.end_s))
            if b % 3 == 0:                              # the arg-max path is an alignment of the greedy labels
                assert h.utt_score >= greedy[b].utt_score - T / 65536 - 1e-3 * T
    if texts:
        given = ['hello world', 'a', 'the quick brown fox'][:B] + ['ab'] * max(B - 3, 0)
        tg2, tl2 = align_cases.pad_targets([[vocab.index(ch) for ch in t] for t in given], blank)
        want2 = align.to_hypotheses(align.align_host(lp, ln, tg2, tl2, blank), vocab, spf)
        got2 = m.align(**inputs, texts=[t.upper() + '.' for t in given])
        assert [_tuples(h) for h in got2] == [_tuples(h) for h in want2] and [h.text for h in got2] == given
    # ---- decode(beam_width=, timestamps=True): the beam's rows aligned in one launch
    res = beam.search_host(lp, ln, blank, W, nb, 40)
    plain_want = beam.to_hypotheses(res, vocab)
    plain = m.decode(**inputs, beam_width=W, n_best=nb)
    plain = plain if nb > 1 else [[h] for h in plain]
    assert [[_tuples(h) for h in row] for row in plain] == [[_tuples(h) for h in row[:nb]] for row in plain_want]     # as before
    ml = min(T, align.MAX_LABELS)
    ares = align.align_host(lp, ln, res.labels.reshape(B * nb, T)[:, :ml], res.n_labels.reshape(B * nb), blank,
                            problems_per_utt=nb, want_total=False)
    timed_want = align.to_hypotheses(ares, vocab, spf)
    timed = m.decode(**inputs, beam_width=W, n_best=nb, timestamps=True)
    timed = timed if nb > 1 else [[h] for h in timed]
    n = 0
    for b, row in enumerate(timed):
        assert len(row) == len(plain[b])
        for h, (ht, hp) in enumerate(zip(row, plain[b])):
            tw = timed_want[b * nb + h]
            assert (ht.text, ht.labels, ht.utt_score, ht.lm_score, ht.ctc_score) == (hp.text, hp.labels, hp.utt_score, None, None)
            assert (ht.start_s, ht.end_s, ht.score, ht.words) == (tw.start_s, tw.end_s, tw.score, tw.words)
            assert len(ht.start_s) == len(ht.labels)
            n += len(ht.start_s)
    assert n > 0
    assert [_tuples(h) for h in m.decode(**inputs)] == [_tuples(h) for h in greedy]


@pytest.mark.parametrize('name', ['QuartzNet15x5Base-En', 'QuartzNet15x5Base-Zh'])
def test_static_engine_full_size(name):
    m = _model(name, 'static', 64, 3, 200)
    x = torch.from_numpy(synth.make_features(3, 64, 200, 9)).cuda()
    lens = torch.tensor([200, 131, 58]).cuda()
    _check_against_twin(m, 16, 4, texts=name.endswith('En'), processed_signal=x, processed_signal_length=lens)
    assert type(m._engine).__name__ == 'Engine'
    if name.endswith('En'):
        audio = torch.from_numpy(synth.make_audio(3, 16000, seed=3)).cuda()
        alen = torch.tensor([16000, 12000, 7001]).cuda()
        m.preprocessor.featurizer.pad_to = 16
        _check_against_twin(m, 8, 1, texts=True, input_signal=audio, input_signal_length=alen)


def test_dynamic_path_mini():
    m = _model('MiniQuartzNet', 'dynamic', 16, 4, 96)
    x = torch.from_numpy(synth.make_features(5, 16, 96, 7)).cuda()
    lens = torch.tensor([96, 90, 61, 33, 12]).cuda()
    _check_against_twin(m, 16, 3, texts=True, processed_signal=x, processed_signal_length=lens)
    assert type(m._engine).__name__ == 'DynamicRunner'


def test_reserved_engine_ragged_batches():
    m = _model('MiniQuartzNet', 'static', 16, 4, 96)
    m.preprocessor.featurizer.pad_to = 16
    m.reserve(4, 2.0)
    rng = np.random.default_rng(11)
    for k in range(3):
        B = int(rng.integers(1, 5)) if k else 4
        S = int(rng.integers(4000, 32001)) if k else 32000
        audio = torch.from_numpy(synth.make_audio(B, S, seed=11 + k)).cuda()
        alen = torch.tensor([S] + [int(v) for v in rng.integers(500, S + 1, B - 1)]).cuda()
        _check_against_twin(m, 16, 2, texts=True, input_signal=audio, input_signal_length=alen)
    assert m._ragged_engine is not None


def test_align_refuses_before_any_launch():
    m = _model('MiniQuartzNet', 'dynamic', 16, 4, 96)
    x = torch.from_numpy(synth.make_features(2, 16, 96, 7)).cuda()
    lens = torch.tensor([96, 90]).cuda()
    for bad, word in ((dict(texts=['a', None]), 'text 1'), (dict(labels=[[0], [len(m.decoder.vocabulary)]]), 'transcript 1'),
                      (dict(), 'exactly one'), (dict(texts=['a']), '1 transcripts')):
        with pytest.raises(ValueError, match=word):
            m.align(processed_signal=x, processed_signal_length=lens, **bad)
    assert m._engine is None                            # no runner was even built


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_cli_align_equals_the_model_in_process(tmp_path):
    n_utt, samples = 4, 24000
    texts = ['hello world', 'a b', 'Forced, alignment!', 'x' * 200]          # the last one has more labels than frames
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            n = samples - 1000 * i
            _write_wav(p, audio[i, :n])
            f.write(json.dumps(dict(audio_filepath=p, duration=n / 16000, text=texts[i])) + '\n')
    out_path, dump = tmp_path / 'aligned.jsonl', tmp_path / 'hyps.json'
    cmd = [sys.executable, CLI, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man), '--weight_bit', '8',
           '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--synthetic_calib', '2', '--percentile', '99.996',
           '--align', str(out_path), '--dump_hyps', str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'path: static integer engine (HIP)' in out.stdout and 'aligned 4 transcripts (3 with word times)' in out.stdout
    with open(out_path, encoding='utf-8') as f:
        recs = [json.loads(line) for line in f]
    with open(dump, encoding='utf-8') as f:
        hyp_rec = json.load(f)
    assert set(hyp_rec) == {'hypotheses', 'references', 'wer', 'path'}       # what the other flags write is untouched
    m = _model('QuartzNet15x5Base-En', 'static', 64, 2, 500, percentile=99.996)
    m.setup_test_data(test_data_config={'sample_rate': 16000, 'manifest_filepath': str(man), 'labels': m.decoder.vocabulary,
                                        'batch_size': 2, 'normalize_transcripts': True, 'shuffle': False})
    want = []
    for batch in m.test_dataloader():
        ids = [row[:int(n)].tolist() for row, n in zip(batch[2], batch[3])]
        want += m.align(input_signal=batch[0].cuda().float(), input_signal_length=batch[1].cuda(), labels=ids)
    # (the references of --dump_hyps are the collated rows: padded to the batch's longest with label 0, the space)
    assert [r['text'] for r in recs] == ['hello world', 'a b', 'forced alignment', 'x' * 200] == [r.rstrip() for r in hyp_rec['references']]
    for i, (r, h) in enumerate(zip(recs, want)):
        inf = h.utt_score == float('-inf')
        assert r['audio_filepath'] == str(tmp_path / f'u{i}.wav') and inf == (i == 3)
        assert r['utt_score'] == (None if inf else h.utt_score) and r['ctc_score'] == (None if inf else h.ctc_score)
        assert r['words'] == [list(w) for w in h.words] and [w[0] for w in r['words']] == ([] if inf else r['text'].split())
