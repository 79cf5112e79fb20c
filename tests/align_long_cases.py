"""Shared checks of EncDecCTCModel.align_long for the CPU and the GPU façade tests: about 20 s of seeded audio through the
committed mini net, windows of 4 s that overlap by 1 s, the greedy decode_long text given back as the transcript."""
import os
import wave

import numpy as np
import torch

from qasr import align, ctc, longform as lf, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'q-asr_amd', 'tools', 'ctc_segmentation', 'run_ctc_segmentation.py')
KW = dict(window_s=4.0, overlap_s=1.0, guard_s=0.2)
S_LONG = 16000 * 20 + 1234
BATCH = 3


def recordings(device):
    """two recordings: seven windows, and one shorter than a window"""
    audio = torch.from_numpy(synth.make_audio(2, S_LONG, seed=8)).to(device)
    return audio, torch.tensor([S_LONG, 50000]).to(device)


def twin_chain(m, audio, lens, rows, band_states=None):
    """the host statement of align_long over the model's own per-window forward outputs: cut_host, forward per batch,
    stitch_host with the log-probabilities as a plane, align_band_host"""
    plan = m._long_plan(lens.cpu().numpy(), **KW)
    win, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
    toks, fss, encs, lps = [], [], [], []
    for i in range(0, plan.Wn, BATCH):
        logp, e, t = m(input_signal=torch.from_numpy(win[i:i + BATCH]).to(audio.device),
                       input_signal_length=torch.from_numpy(wl[i:i + BATCH]).to(audio.device).long())
        toks.append(t.cpu().numpy().astype(np.int32)), encs.append(e.cpu().numpy().astype(np.int32))
        fss.append(logp.float().gather(2, t.long().unsqueeze(-1)).squeeze(-1).cpu().numpy())
        lps.append(logp.float().cpu().numpy())
    blank = len(m.decoder.vocabulary)
    out, total, seams = lf.stitch_host(plan, np.concatenate(encs), np.concatenate(toks), np.concatenate(fss),
                                       [np.concatenate(lps)], blank)
    tg = np.full((len(rows), max(1, max(len(r) for r in rows))), blank, dtype=np.int32)
    for i, r in enumerate(rows):
        tg[i, :len(r)] = r
    tl = np.array([len(r) for r in rows], dtype=np.int32)
    res = align.align_band_host(out[2], total, tg, tl, blank, band_states=align.pick_band_states(tg.shape[1], band_states))
    return plan, res, seams


def check_equals_the_twin_chain(m, device, band_states=None):
    audio, lens = recordings(device)
    greedy = m.decode_long(audio, lens, batch_size=BATCH, **KW)
    rows = [h.labels for h in greedy]
    assert len(rows[0]) > 20 and len(rows[1]) > 0
    plan, res, seams = twin_chain(m, audio, lens, rows, band_states)
    assert plan.count.tolist() == [7, 1] and res.ok.tolist() == [1, 1]
    want = align.to_hypotheses(res, m.decoder.vocabulary, m.seconds_per_frame())
    got = m.align_long(audio, lens, labels=rows, batch_size=BATCH, band_states=band_states, **KW)
    for g, w, gr in zip(got, want, greedy):
        assert (g.text, g.labels, g.start_s, g.end_s, g.score, g.utt_score, g.words) == \
            (w.text, w.labels, w.start_s, w.end_s, w.score, w.utt_score, w.words)
        assert g.ctc_score is None and g.segments is None and g.seams_s == gr.seams_s and g.text == gr.text
        assert g.utt_score >= gr.utt_score - 1e-3 * abs(gr.utt_score)      # the best alignment is no worse than the greedy path
    assert got[1].seams_s is None and len(got[0].seams_s) == 6
    return got, rows


def check_segments(m, device):
    audio, lens = recordings(device)
    greedy = m.decode_long(audio, lens, batch_size=BATCH, **KW)
    ids = greedy[0].labels
    a, b = len(ids) // 3, 2 * len(ids) // 3
    parts = [ids[:a], ids[a:b], ids[b:]]
    vocab = list(m.decoder.vocabulary)
    space = vocab.index(' ') if ' ' in vocab else None
    got = m.align_long(audio[:1], lens[:1], labels=[parts], batch_size=BATCH, **KW)[0]
    joined = parts[0] + ([space] if space is not None else []) + parts[1] + ([space] if space is not None else []) + parts[2]
    assert got.labels == joined and len(got.segments) == 3
    spf = m.seconds_per_frame()
    at = 0
    for seg, part in zip(got.segments, parts):
        assert isinstance(seg, ctc.Segment) and seg.text == ''.join(vocab[c] for c in part)
        assert seg.start_s == got.start_s[at] and seg.end_s == got.end_s[at + len(part) - 1]      # they tile the labels in order
        assert seg.start_s <= seg.end_s and np.isfinite(seg.score) and seg.score <= 0.0
        at += len(part) + (1 if space is not None else 0)
    assert got.segments[0].end_s <= got.segments[1].start_s and got.segments[1].end_s <= got.segments[2].start_s
    assert got.segments[2].end_s <= S_LONG / 16000 + 2 * spf
    # a transcript that cannot fit: text kept, times empty, scores -inf
    lost = m.align_long(audio[1:, :8000].contiguous(), torch.tensor([8000]).to(device), labels=[[ids[:20], ids[20:40]]], **KW)[0]          # 0.5 s: 26 frames
    assert len(lost.labels) >= 40 and lost.start_s == [] and lost.utt_score == float('-inf')
    assert [(s.start_s, s.end_s, s.score) for s in lost.segments] == [(None, None, float('-inf'))] * 2
    return got


def check_refusals(m, device):
    import pytest
    audio, lens = recordings(device)
    with pytest.raises(ValueError, match='exactly one of texts and labels'):
        m.align_long(audio, lens, **KW)
    with pytest.raises(ValueError, match='utterance 1 of transcript 0 is empty'):
        m.align_long(audio, lens, labels=[[[1, 2], [], [3]], [1]], **KW)
    with pytest.raises(ValueError, match='utterance 1 of transcript 1 is empty'):
        m.align_long(audio, lens, texts=['ab', ['ab', '  ']], **KW)
    with pytest.raises(ValueError, match='band_states'):
        m.align_long(audio, lens, labels=[[1], [1]], band_states=512, **KW)
    with pytest.raises(ValueError, match='1 transcripts for 2 recordings'):
        m.align_long(audio, lens, labels=[[1]], **KW)
    with pytest.raises(ValueError, match='outside the vocabulary'):
        m.align_long(audio, lens, labels=[[1], [len(m.decoder.vocabulary)]], **KW)
    with pytest.raises(ValueError, match='twice the overlap'):
        m.align_long(audio, lens, labels=[[1], [1]], window_s=4.0, overlap_s=3.0)


def write_wav(path, x, rate=16000):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def check_tool_output(tmp_path, extra):
    """runs the tool on a temporary directory with one wav, its transcript of three lines and a _with_punct twin; returns the
    parsed rows [(start, end, score, text, shown)]"""
    import subprocess
    import sys
    data = tmp_path / 'data'
    data.mkdir()
    x = synth.make_audio(1, 16000 * 6, seed=4)[0]
    write_wav(str(data / 'talk.wav'), x)
    (data / 'talk.txt').write_text('ab\nc d\nef\n', encoding='utf-8')
    (data / 'talk_with_punct.txt').write_text('Ab,\nC d.\nEf!\n', encoding='utf-8')
    out = subprocess.run([sys.executable, TOOL, '--data', str(data), '--output_dir', str(tmp_path / 'out'), '--model', 'MiniQuartzNet',
                          '--synthetic_model', '--window_s', '4', '--window_len', '8000'] + extra,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = (tmp_path / 'out' / 'segments' / '8000_talk_segments.txt').read_text(encoding='utf-8').splitlines()
    assert lines[0] == str(data / 'talk.wav') and len(lines) == 4
    rows = []
    for ln, text, shown in zip(lines[1:], ['ab', 'c d', 'ef'], ['Ab,', 'C d.', 'Ef!']):
        head, t, s = [c.strip() for c in ln.split('|')]
        start, end, score = (float(v) for v in head.split())
        assert (t, s) == (text, shown) and 0 <= start <= end <= 6.1 and np.isfinite(score)
        rows.append((start, end, score, t, s))
    assert rows[0][1] <= rows[1][0] and rows[1][1] <= rows[2][0]
    return rows
