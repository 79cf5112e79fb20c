"""Shared generators of the streaming tests (qasr.stream): plans in frames, token / score rows with long runs, ties and
signed zeros, a push schedule that wraps the ring, the emit cases, and a driver that plays one stream through any
implementation of the three steps."""
import numpy as np

from qasr import ctc, stream as st

SPF = 320
RATE = 16000
BLANK = 5
SCORES = np.array([-0.0, 0.0, -1.5, -1.5, -0.25, -3.0, -0.25], dtype=np.float32)      # ties, +0.0 and -0.0


def plan_frames(cf, lf, rf, frames_of=None):
    return st.StreamPlan(cf * SPF / RATE, lf * SPF / RATE, rf * SPF / RATE, RATE, SPF, frames_of)


def model_frames_of(n, hop=160, pad_to=16, stride=2):
    """frames_of as EncDecCTCModel._long_plan builds it for the registered models"""
    t = 1 + n // hop
    if pad_to and t % pad_to:
        t += pad_to - t % pad_to
    return -(-t // stride)


def token_row(rng, T, p_blank, max_run=1):
    """T tokens of 5 labels + blank in runs of 1 .. max_run frames"""
    out = np.empty(T + max_run, dtype=np.int32)
    i = 0
    while i < T:
        k = BLANK if rng.random() < p_blank else int(rng.integers(0, BLANK))
        n = int(rng.integers(1, max_run + 1))
        out[i:i + n] = k
        i += n
    return out[:T]


def score_row(rng, T):
    return SCORES[rng.integers(0, len(SCORES), size=T)]


def play(plan, n_samples, rows, push, window, emit, pieces=None, blank=BLANK, slot=0):
    """One stream of n_samples samples through (push, window, emit): a step whenever another C samples have arrived, END at
    the end.  rows(k, Tw) -> (tokens, frame scores) of step k's window.  push(flag, chunk[n]); window() -> (len, first);
    emit(tokens, scores, enc_len, first, end) -> qasr.stream.StepRow.  Returns the steps as dicts."""
    rng = np.random.default_rng(n_samples)
    audio = rng.standard_normal(n_samples).astype(np.float32)
    steps, r = [], 0

    def step(end):
        ln, first = window()
        start, want_len, want_first = plan.window_of(r)
        assert (ln, first) == (want_len, want_first) and first * plan.samples_per_frame == start
        e = min(int(plan.frames_of(ln)), plan.Tw)
        t, f = rows(len(steps), plan.Tw)
        s = emit(t, f, e, first, end)
        steps.append(dict(step=s, first=first, enc=e, tokens=t, scores=f, r=r, end=end))

    push(st.BEGIN, audio[:0])
    while r < n_samples:
        n = min(plan.C - r % plan.C, n_samples - r)
        push(0, audio[r:r + n])
        r += n
        if r % plan.C == 0:
            step(False)
    step(True)
    return audio, steps


def host_ops(plan, S=1, slot=0, blank=BLANK):
    state = st.StreamState(S, plan)

    def push(flag, x):
        chunk = np.zeros((1, max(len(x), 1)), dtype=np.float32)
        chunk[0, :len(x)] = x
        st.push_host(state, [slot], [flag], [len(x)], chunk)

    def window():
        _, wl, first = st.window_host(state, [slot])
        return int(wl[0]), int(first[0])

    def emit(t, f, e, first, end):
        return st.emit_host(t, f, e, first, state, slot, end, blank, session=True)

    return state, push, window, emit


def check_invariant(steps, tail_pitch, blank=BLANK):
    """The deltas of the steps, concatenated, are collapse_host of the concatenated final frames on every byte; the END
    utt_score is utt_score_host of that row; every tail is what collapse_host finds beyond the committed labels on final +
    look-ahead frames; the final ranges tile [0, total_frames) and never start before the window."""
    fin_t, fin_f, done, committed = [], [], 0, 0
    lab, start, nfr, sc = [], [], [], []
    for d in steps:
        s, first = d['step'], d['first']
        assert s.status == st.STATUS_OK and s.lo == done and s.lo >= first and s.hi >= s.lo
        fin_t.append(d['tokens'][s.lo - first:s.hi - first])
        fin_f.append(d['scores'][s.lo - first:s.hi - first])
        done = s.hi
        assert s.total_frames == done
        lab.append(s.labels), start.append(s.start), nfr.append(s.nframes), sc.append(s.score)
        committed += s.n_new
        look = d['tokens'][s.hi - first:d['enc']] if not d['end'] else d['tokens'][:0]
        row = np.concatenate(fin_t + [look])
        if len(row):
            ref = ctc.collapse_host(row[None], blank=blank)
            want_tail = ref.labels[0, committed:int(ref.n_labels[0])]
        else:
            want_tail = np.zeros(0, dtype=np.int32)
        assert s.tail.tolist() == want_tail[:tail_pitch].tolist()
    row_t, row_f = np.concatenate(fin_t), np.concatenate(fin_f)
    assert len(row_t) == done
    last = steps[-1]['step']
    if done == 0:
        assert committed == 0 and last.utt_score.tobytes() == np.float32(0).tobytes()
        return row_t, row_f
    ref = ctc.collapse_host(row_t[None], row_f[None], blank=blank)
    n = int(ref.n_labels[0])
    assert committed == n
    assert np.concatenate(lab).astype(np.int32).tobytes() == ref.labels[0, :n].tobytes()
    assert np.concatenate(start).astype(np.int32).tobytes() == ref.start[0, :n].tobytes()
    assert np.concatenate(nfr).astype(np.int32).tobytes() == ref.nframes[0, :n].tobytes()
    assert np.concatenate(sc).astype(np.float32).tobytes() == ref.score[0, :n].tobytes()
    assert np.float32(last.utt_score).tobytes() == np.float32(ref.utt_score[0]).tobytes()
    assert np.float32(last.utt_score).tobytes() == np.float32(ctc.utt_score_host(row_f)).tobytes()
    return row_t, row_f


def push_schedule(C, steps=20, B=3):
    """n_new per (step, row): mostly whole chunks so the ring wraps several times, with 0, 1 and 3 in between; flags with a
    BEGIN on every row at step 0 and on row 1 (a used slot) half-way"""
    n = np.full((steps, B), C, dtype=np.int32)
    n[2, 0], n[3, 1], n[5, 2], n[7, 0], n[8, 1], n[11, 2], n[13, 0] = 0, 1, 3, 3, 0, 1, 1
    flags = np.zeros((steps, B), dtype=np.int32)
    flags[0] = st.BEGIN
    flags[steps // 2, 1] = st.BEGIN
    return n, flags


def emit_cases():
    """(name, n final frames, lo, kind, end, carry) for k_stream_emit: kind 'random' / 'blank' / 'onerun' / 'noblank';
    carry: None (no open run), 'same' (the open run's token is the range's first), 'other'"""
    out = []
    for i, n in enumerate((1, 63, 64, 65, 257, 300)):
        for j, lo in enumerate((0, 1, 63, 64, 100)):
            kind = ('random', 'noblank', 'blank', 'onerun', 'random')[(i + j) % 5]
            carry = None if lo == 0 else (None, 'same', 'other')[(i + 2 * j) % 3]
            out.append((f'n{n}_lo{lo}_{kind}', n, lo, kind, (i + j) % 2 == 1, carry))
    out.append(('empty_end_open', 0, 64, 'random', True, 'same'))
    out.append(('empty_open', 0, 64, 'random', False, 'same'))
    out.append(('onerun_end', 300, 1, 'onerun', True, 'same'))
    out.append(('blank_end', 257, 63, 'blank', True, 'other'))
    return out


def emit_case_inputs(rng, plan, n, lo, kind, end, carry, enc='fit'):
    """A state block and a window row that make [lo, lo + n) final.  enc: 'fit' (END: the range's end; else the row pitch),
    'zero' (enc_len 0: nothing final), 'over' (beyond Tw: clamped)"""
    Tw, spf = plan.Tw, plan.samples_per_frame
    first = max(0, lo - 3)
    assert lo + n - first <= Tw
    if kind == 'random':
        tok = token_row(rng, Tw, 0.5, 3)
    elif kind == 'noblank':
        tok = token_row(rng, Tw, 0.0, 1)
    elif kind == 'blank':
        tok = np.full(Tw, BLANK, dtype=np.int32)
    else:
        tok = np.full(Tw, 2, dtype=np.int32)
    fs = score_row(rng, Tw)
    blk = np.zeros(st.STATE_WORDS, dtype=np.int32)
    blk[0:2].view(np.int64)[0] = (lo + n) * spf + plan.Rr + 7          # floor((r - Rr) / spf) = lo + n
    blk[2] = lo
    if carry is not None and lo > 0:
        t0 = int(tok[lo - first]) if n > 0 else 2
        same = t0 if t0 != BLANK else 1
        blk[3] = (same if carry == 'same' else (same + 1) % BLANK) + 1
        blk[4] = lo - 1
        blk[5] = int(ctc._order_key(np.float32(-0.25)).reshape(-1)[0])
        blk[6] = 11
    blk[16:].view(np.float32)[:] = score_row(rng, 64) * np.float32(3)
    e = {'fit': (lo + n - first) if end else Tw, 'zero': 0, 'over': Tw + 1000}[enc]
    return blk, tok, fs, e, first


# ---------------------------------------------------------------------------------------------------------- the façade
FACADE_KW = dict(chunk_s=0.5, left_s=1.0, right_s=0.24)
FACADE_LENS = [30000, 90000]


def facade_audio():
    from qasr import synth
    return synth.make_audio(2, 90000, seed=8)


def compose_on_host(m, audio, lens, device='cpu', streams=(0, 1), **kw):
    """per step: window_host -> model._forward(..., decode='frames') -> emit_host, over the batches a session makes of
    streams pushed side by side: chunk k of every stream that has one runs as one batch, every END step on its own.
    Returns (plan, {stream: [StepRow, ...]})."""
    import torch
    plan = m._stream_plan(**kw)
    blank = len(m.decoder.vocabulary)
    state = st.StreamState(len(streams), plan)
    out = {i: [] for i in streams}

    def step(rows, end):
        win, wl, first = st.window_host(state, rows)
        t, f, e = m._forward(torch.from_numpy(win).to(device), torch.from_numpy(wl).to(device).long(), decode='frames')
        t, f, e = t.cpu().numpy(), f.float().cpu().numpy(), e.cpu().numpy()
        for b, j in enumerate(rows):
            out[streams[j]].append(st.emit_host(t[b], f[b], int(e[b]), int(first[b]), state, j, end, blank, session=True))

    k = 0
    while any(lens[i] > k * plan.C for i in streams):
        rows = [j for j, i in enumerate(streams) if lens[i] > k * plan.C]
        n = [min(plan.C, lens[streams[j]] - k * plan.C) for j in rows]
        chunk = np.zeros((len(rows), plan.C), dtype=np.float32)
        for b, j in enumerate(rows):
            chunk[b, :n[b]] = audio[streams[j], k * plan.C:k * plan.C + n[b]]
        st.push_host(state, rows, [st.BEGIN if k == 0 else 0] * len(rows), n, chunk)
        full = [j for b, j in enumerate(rows) if n[b] == plan.C]
        if full:
            step(full, False)
        k += 1
    for j in range(len(streams)):
        step([j], True)
    return plan, out


def play_session(m, audio, lens, piece, device='cpu', streams=(0, 1), max_streams=2, **kw):
    """the streams of `audio` pushed side by side in pieces of `piece` samples (the shorter one ends earlier, so the pieces
    are unequal); returns (slots, updates per slot, hypotheses, the session's step count)"""
    import torch
    sess = m.stream(max_streams=max_streams, **kw)
    slots = [sess.open() for _ in streams]
    ups = {s: [] for s in slots}
    x = torch.from_numpy(audio).to(device)
    for off in range(0, max(lens[i] for i in streams), piece):
        live = [j for j, i in enumerate(streams) if off < lens[i]]
        n = [min(piece, lens[streams[j]] - off) for j in live]
        sig = torch.zeros(len(live), max(n), device=device)
        for k, j in enumerate(live):
            sig[k, :n[k]] = x[streams[j], off:off + n[k]]
        for u in sess.push([slots[j] for j in live], sig, torch.tensor(n)):
            ups[u.slot].append(u)
    hyps = [sess.close(s) for s in slots]
    steps = sess.steps
    sess.close_all()
    return slots, ups, hyps, steps


def check_against_composition(m, slots, ups, hyps, want, lens, streams=(0, 1)):
    spf_s, vocab = m.seconds_per_frame(), m.decoder.vocabulary
    for s, h, i in zip(slots, hyps, streams):
        steps = want[i]
        assert len(ups[s]) == len(steps) - 1                                     # every step but END came out of a push
        for u, w in zip(ups[s], steps):
            assert u.labels == w.labels.tolist() and u.score == w.score.astype(np.float64).tolist()
            assert u.start_s == (w.start.astype(np.float64) * spf_s).tolist()
            assert u.end_s == ((w.start + w.nframes).astype(np.float64) * spf_s).tolist()
            assert u.text == ''.join(vocab[k] for k in w.labels) and u.tail_text == ''.join(vocab[k] for k in w.tail)
        assert h.labels == np.concatenate([w.labels for w in steps]).tolist() and h.utt_score == float(steps[-1].utt_score)
        assert h.start_s == (np.concatenate([w.start for w in steps]).astype(np.float64) * spf_s).tolist()
        assert h.score == np.concatenate([w.score for w in steps]).astype(np.float64).tolist()
        assert h.text == ''.join(u.text for u in ups[s]) + ''.join(vocab[k] for k in steps[-1].labels)
        assert h.start_s == sorted(h.start_s) and h.end_s == sorted(h.end_s)     # times ascend
        assert not h.end_s or h.end_s[-1] <= lens[i] / 16000 + 0.04
