"""Shared checks of EncDecCTCModel.spot / spot_long for the CPU and the GPU façade tests: the calls equal the host composition
star_host + spot_host + to_hits over the model's own log-probabilities (for spot_long: over the stitched rows of the host chain
cut_host, forward per batch, stitch_host).  Keywords are cut out of the greedy transcript, so that there is something to find."""
import numpy as np
import pytest
import torch

import align_long_cases as alc
import spot_cases as sc
from qasr import align, longform as lf, spot, synth

KW = alc.KW
S_TWO = 16000 * 6 + 321             # two windows of 4 s that overlap by 1 s
S_SHORT = 50000                     # shorter than a window
SPOT = dict(threshold=-3.0, max_span_s=2.0, max_hits=3)


def tuples(hits):
    return [[(h.keyword, h.index, h.start_s, h.end_s, h.score, h.frames) for h in row] for row in hits]


def _keywords_from(greedy_rows, blank, rng):
    """label rows to look for: pieces of the greedy transcripts (they occur, with score 0 where the piece is the arg-max path),
    one keyword that occurs nowhere in particular, and a single label"""
    rows = []
    for ids in greedy_rows:
        ids = [int(c) for c in ids]
        if len(ids) >= 3:
            a = int(rng.integers(0, len(ids) - 2))
            rows.append(ids[a:a + 3])
    rows.append([int(c) for c in rng.integers(0, blank, size=4)])
    rows.append([int(rng.integers(0, blank))])
    return rows


def host_hits(m, lp, ln, rows, given):
    blank = len(m.decoder.vocabulary)
    tg, tl = sc.pad(rows, blank)
    span = int(round(SPOT['max_span_s'] / m.seconds_per_frame()))
    res = spot.spot_host(lp, ln, align.star_host(lp, ln, 0.0), tg, tl, blank, spot.check_threshold(SPOT['threshold'], 'test'), span,
                         SPOT['max_hits'])
    assert res.ok.all()
    return spot.to_hits(res, given, m.seconds_per_frame()), res


def check_spot(m, device):
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7)).to(device)
    inputs = dict(processed_signal=x, processed_signal_length=torch.tensor([96, 70, 41]).to(device))
    logp, enc_len, tokens = m(**inputs)
    lp, ln = logp.float().cpu().numpy(), enc_len.cpu().numpy()
    blank = len(m.decoder.vocabulary)
    rng = np.random.Generator(np.random.PCG64(17))
    greedy = [[int(c) for i, c in enumerate(t[:n]) if c != blank and (i == 0 or c != t[i - 1])] for t, n in zip(tokens.cpu().numpy(), ln)]
    rows = _keywords_from(greedy, blank, rng)
    want, res = host_hits(m, lp, ln, rows, [tuple(r) for r in rows])
    got = m.spot(**inputs, labels=rows, **SPOT)
    assert tuples(got) == tuples(want) and len(got) == 3
    assert int(res.n_hits.sum()) > 0 and any(h.score == 0.0 for row in got for h in row) or not any(len(g) >= 3 for g in greedy)
    for row in got:
        assert [h.start_s for h in row] == sorted(h.start_s for h in row) and all(h.score <= 0.0 and h.frames >= 1 for h in row)
    # strings go through the model's parser, as align()'s texts do
    vocab = list(m.decoder.vocabulary)
    words = ['ab', 'c d', 'Hello']
    ids = [[vocab.index(ch) for ch in w.lower()] for w in words]
    want_s, _ = host_hits(m, lp, ln, ids, words)
    assert tuples(m.spot(**inputs, keywords=words, **SPOT)) == tuples(want_s)
    return got


def twin_rows(m, audio, lens):
    """the stitched log-probability rows and their lengths of the host chain over the model's own per-window forward outputs"""
    plan = m._long_plan(lens.cpu().numpy(), **KW)
    win, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
    toks, fss, encs, lps = [], [], [], []
    for i in range(0, plan.Wn, alc.BATCH):
        logp, e, t = m(input_signal=torch.from_numpy(win[i:i + alc.BATCH]).to(audio.device),
                       input_signal_length=torch.from_numpy(wl[i:i + alc.BATCH]).to(audio.device).long())
        toks.append(t.cpu().numpy().astype(np.int32)), encs.append(e.cpu().numpy().astype(np.int32))
        fss.append(logp.float().gather(2, t.long().unsqueeze(-1)).squeeze(-1).cpu().numpy())
        lps.append(logp.float().cpu().numpy())
    blank = len(m.decoder.vocabulary)
    out, total, _ = lf.stitch_host(plan, np.concatenate(encs), np.concatenate(toks), np.concatenate(fss), [np.concatenate(lps)], blank)
    return plan, out[2], total


def check_spot_long(m, device):
    audio = torch.from_numpy(synth.make_audio(2, S_TWO, seed=8)).to(device)
    lens = torch.tensor([S_TWO, S_SHORT]).to(device)
    plan, lp, total = twin_rows(m, audio, lens)
    assert plan.count.tolist() == [2, 1]
    blank = len(m.decoder.vocabulary)
    rng = np.random.Generator(np.random.PCG64(19))
    greedy = [h.labels for h in m.decode_long(audio, lens, batch_size=alc.BATCH, **KW)]
    rows = _keywords_from(greedy, blank, rng)
    want, res = host_hits(m, lp, total, rows, [tuple(r) for r in rows])
    got = m.spot_long(audio, lens, labels=rows, batch_size=alc.BATCH, **KW, **SPOT)
    assert tuples(got) == tuples(want) and len(got) == 2 and int(res.n_hits.sum()) > 0
    assert all(h.end_s <= S_TWO / 16000 + 2 * m.seconds_per_frame() for h in got[0])
    # a recording shorter than one window: spot()'s hits
    short = audio[1:, :S_SHORT].contiguous()
    one = m.spot_long(short, lens[1:], labels=rows, batch_size=alc.BATCH, **KW, **SPOT)
    assert tuples(one) == tuples(m.spot(input_signal=short, input_signal_length=lens[1:], labels=rows, **SPOT))
    return got


def check_refusals(m, device):
    x = torch.from_numpy(synth.make_features(1, 16, 64, 7)).to(device)
    inputs = dict(processed_signal=x, processed_signal_length=torch.tensor([64]).to(device))
    audio = torch.from_numpy(synth.make_audio(1, 16000, seed=8)).to(device)
    lens = torch.tensor([16000]).to(device)
    blank = len(m.decoder.vocabulary)
    for call in (lambda **kw: m.spot(**inputs, **kw), lambda **kw: m.spot_long(audio, lens, **KW, **kw)):
        with pytest.raises(ValueError, match='exactly one of keywords and labels'):
            call()
        with pytest.raises(ValueError, match='exactly one of keywords and labels'):
            call(keywords=['a'], labels=[[1]])
        with pytest.raises(ValueError, match='keyword list is empty'):
            call(keywords=[])
        with pytest.raises(ValueError, match='keyword 1 is empty'):
            call(labels=[[1], []])
        with pytest.raises(ValueError, match='keyword 1 is empty'):
            call(keywords=['ab', '  '])
        with pytest.raises(ValueError, match='keyword 0 has 128 labels'):
            call(labels=[[1, 2] * 64])
        with pytest.raises(ValueError, match='keyword 1 is rejected by the parser'):
            call(keywords=['ab', 7])
        with pytest.raises(ValueError, match='keyword 0 holds a label outside the vocabulary'):
            call(labels=[[blank]])
        for thr in (0.5, -16.5, float('nan')):
            with pytest.raises(ValueError, match='threshold'):
                call(labels=[[1]], threshold=thr)
        for span_s in (0.0, 0.001, 65537 * m.seconds_per_frame()):
            with pytest.raises(ValueError, match='max_span_s'):
                call(labels=[[1]], max_span_s=span_s)
        with pytest.raises(ValueError, match='max_hits'):
            call(labels=[[1]], max_hits=0)
    with pytest.raises(ValueError, match='twice the overlap'):
        m.spot_long(audio, lens, labels=[[1]], window_s=4.0, overlap_s=3.0)
    with pytest.raises(ValueError, match='seam'):
        m.spot_long(audio, lens, labels=[[1]], seam='none', **KW)
    assert len(m.spot(**inputs, labels=[[1] * 127], threshold=-16.0, max_span_s=65536 * m.seconds_per_frame())) == 1
