"""The wildcard through the facade on an MI355X: align(texts with the token) and align_long(star_between=True) on the device
equal the NumPy twins (star_host, align_host / align_band_host with a plane) over the same model's log-probabilities - on the
static engine and under a caller's reservation, where the engine allocates nothing after the first call - and calls without
the new arguments return what they returned."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases  # noqa: E402
import align_long_cases as alc  # noqa: E402
from qasr import align, longform as lf  # noqa: E402
from test_gpu_align_long_facade import model  # noqa: E402  (the committed mini net, calibrated once per process)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _tuples(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words, h.lm_score, h.ctc_score, h.seams_s,
            None if h.segments is None else [(s.text, s.start_s, s.end_s, s.score) for s in h.segments])


def _short_inputs():
    from qasr import synth
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7)).cuda()
    return dict(processed_signal=x, processed_signal_length=torch.tensor([96, 70, 41]).cuda())


def _check_align(m, penalty=1.0):
    vocab = list(m.decoder.vocabulary)
    W, blank = len(vocab) + 1, len(vocab)
    inputs = _short_inputs()
    logp, enc_len, _ = m(**inputs)
    torch.cuda.synchronize()
    lp, ln = logp.float().cpu().numpy(), enc_len.cpu().numpy()
    texts = ['ab * c', '* hello world *', 'a']
    rows = [[W if ch == '*' else vocab.index(ch) for ch in t] for t in texts]
    tg, tl = align_cases.pad_targets(rows, blank)
    star = align.star_host(lp, ln, penalty)
    twin = align.align_host(lp, ln, tg, tl, blank, star=star)
    assert twin.ok.all()
    want = align.to_hypotheses(twin, vocab, m.seconds_per_frame(), star_token='*')
    got = m.align(**inputs, texts=texts, star='*', star_penalty=penalty)
    assert [_tuples(h) for h in got] == [_tuples(h) for h in want]
    assert [h.text for h in got] == texts and got[0].ctc_score is None and got[2].ctc_score is not None
    assert sum(1 for w in got[1].words if w[0] == '*') == 2
    # without the new arguments: the twin without a plane, as before
    plain_rows = [[c for c in r if c != W] for r in rows]
    tg0, tl0 = align_cases.pad_targets(plain_rows, blank)
    want0 = align.to_hypotheses(align.align_host(lp, ln, tg0, tl0, blank), vocab, m.seconds_per_frame())
    assert [_tuples(h) for h in m.align(**inputs, labels=plain_rows)] == [_tuples(h) for h in want0]
    return got


def _twin_chain_between(m, audio, lens, parts, penalty):
    """alc.twin_chain with the star_between layout and the plane of star_host over the stitched log-probabilities"""
    vocab = list(m.decoder.vocabulary)
    W, blank, sp = len(vocab) + 1, len(vocab), vocab.index(' ')
    plan = m._long_plan(lens.cpu().numpy(), **alc.KW)
    win, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
    toks, fss, encs, lps = [], [], [], []
    for i in range(0, plan.Wn, alc.BATCH):
        logp, e, t = m(input_signal=torch.from_numpy(win[i:i + alc.BATCH]).cuda(), input_signal_length=torch.from_numpy(wl[i:i + alc.BATCH]).cuda().long())
        toks.append(t.cpu().numpy().astype(np.int32)), encs.append(e.cpu().numpy().astype(np.int32))
        fss.append(logp.float().gather(2, t.long().unsqueeze(-1)).squeeze(-1).cpu().numpy())
        lps.append(logp.float().cpu().numpy())
    out, total, seams = lf.stitch_host(plan, np.concatenate(encs), np.concatenate(toks), np.concatenate(fss), [np.concatenate(lps)], blank)
    row = [W]
    for p in parts:
        row += [sp] + list(p) + [sp, W]
    tg, tl = align_cases.pad_targets([row], blank)
    star = align.star_host(out[2], total, penalty)
    res = align.align_band_host(out[2], total, tg, tl, blank, band_states=align.pick_band_states(tg.shape[1]), star=star)
    return row, res


def _check_align_long(m, penalty=1.0):
    vocab = list(m.decoder.vocabulary)
    sp = vocab.index(' ')
    audio, lens = alc.recordings('cuda')
    audio, lens = audio[:1], lens[:1]
    ids = m.decode_long(audio, lens, batch_size=alc.BATCH, **alc.KW)[0].labels
    a, b = len(ids) // 3, 2 * len(ids) // 3
    parts = [[c for c in p if c != sp] or [1] for p in (ids[:a], ids[a:b], ids[b:])]
    row, twin = _twin_chain_between(m, audio, lens, parts, penalty)
    assert twin.ok[0] == 1
    want = align.to_hypotheses(twin, vocab, m.seconds_per_frame(), star_token='*')[0]
    got = m.align_long(audio, lens, labels=[parts], batch_size=alc.BATCH, star_between=True, star_penalty=penalty, **alc.KW)[0]
    assert got.labels == row
    assert (got.text, got.start_s, got.end_s, got.score, got.utt_score, got.words, got.ctc_score) == \
        (want.text, want.start_s, want.end_s, want.score, want.utt_score, want.words, None)
    assert len(got.segments) == 3 and sum(1 for w in got.words if w[0] == '*') == 4
    at = 2
    for seg, part in zip(got.segments, parts):
        assert seg.start_s == got.start_s[at] and seg.end_s == got.end_s[at + len(part) - 1] and np.isfinite(seg.score)
        at += len(part) + 3
    return got


def test_static_engine():
    m = model('static')
    m.reserve(None, None)
    _check_align(m)
    _check_align_long(m)


def test_under_a_reservation_the_engine_allocates_nothing_after_the_first_call():
    m = model('static')
    m.reserve(alc.BATCH, 4.0)
    try:
        first = _check_align(m)
        long_first = _check_align_long(m)
        s0 = m._ragged_engine.ragged_stats()
        again = _check_align(m, penalty=2.0)
        long_again = _check_align_long(m, penalty=2.0)
        s1 = m._ragged_engine.ragged_stats()
        assert s1['device_allocs'] == s0['device_allocs'] and s1['device_frees'] == s0['device_frees']
        assert again[0].utt_score < first[0].utt_score and long_again.utt_score < long_first.utt_score   # a dearer wildcard
    finally:
        m.reserve(None, None)


def test_calls_without_the_new_arguments_return_what_they_returned():
    m = model('static')
    m.reserve(None, None)
    got, rows = alc.check_equals_the_twin_chain(m, 'cuda')           # align_long without a wildcard: the twin chain, as before
    dflt = m.align_long(*alc.recordings('cuda'), labels=rows, batch_size=alc.BATCH, star=None, star_penalty=1.0, star_between=False, **alc.KW)
    assert [_tuples(h) for h in dflt] == [_tuples(h) for h in got]
    with pytest.raises(ValueError, match='holds the wildcard label'):
        m.align_long(*alc.recordings('cuda'), labels=[rows[0], [len(m.decoder.vocabulary) + 1]], **alc.KW)


def test_cli_align_with_a_star_token_and_star_between(tmp_path):
    """inference.py --align --window_s --star_token --star_between: the manifest's texts as written, a wildcard at the token and
    around every text"""
    import json
    import subprocess

    from qasr import synth
    from test_gpu_align_long_facade import CLI
    S = 16000 * 9
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(2, S, seed=4)
    with open(man, 'w') as f:
        for i in range(2):
            p = str(tmp_path / f'u{i}.wav')
            alc.write_wav(p, audio[i])
            f.write(json.dumps(dict(audio_filepath=p, duration=S / 16000, text='Hello * world')) + '\n')
    calib = tmp_path / 'calib.npz'                        # the mini net has 16 features: its own calibration batches
    np.savez(str(calib), *synth.make_calibration(2, 2, 16, 200))
    out_path = tmp_path / 'aligned.jsonl'
    out = subprocess.run([sys.executable, CLI, '--asr_model', 'MiniQuartzNet', '--synthetic_model', '--dataset', str(man),
                          '--weight_bit', '8', '--act_bit', '8', '--dither', '0', '--batch_size', '2', '--load', str(calib),
                          '--percentile', '99.996', '--window_s', '4.0', '--overlap_s', '1.0', '--align', str(out_path),
                          '--star_token', '*', '--star_between', '--star_penalty', '2.0'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    recs = [json.loads(ln) for ln in out_path.read_text(encoding='utf-8').splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert r['text'] == '* hello * world *' and r['ctc_score'] is None and np.isfinite(r['utt_score'])
        assert [w[0] for w in r['words']] == ['*', 'hello', '*', 'world', '*']
        assert all(0 <= a[1] < a[2] <= b[1] + 1e-9 for a, b in zip(r['words'], r['words'][1:])) and r['words'][-1][2] <= 9.1
    bad = subprocess.run([sys.executable, CLI, '--asr_model', 'MiniQuartzNet', '--dataset', str(man), '--star_token', '*'],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and '--star_token needs --align' in bad.stderr
