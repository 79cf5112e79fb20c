"""Shared generators of the endpointing tests (qasr.stream_ep), built on stream_cases: the plans and rule frames, whole-stream
token / score rows (with a long blank stretch; with no four non-blank frames in a row, so that HARD cannot fire under
NO_HARD_RULES), a driver that plays one stream through emit + endpoint twins, the checks of the two invariants, and the
host composition of a session with endpoint=."""
import dataclasses

import numpy as np

import stream_cases as sc
from qasr import ctc, stream as st, stream_ep as se

BLANK = sc.BLANK
PLANS = [dict(shape=(2, 5, 1)), dict(shape=(8, 10, 2)), dict(shape=(4, 6, 2), frames_of=sc.model_frames_of)]
NO_HARD_RULES = (3, 7, 12, 16)                  # Fsil, Fstart, Fmax, Fhard
DENSE_RULES = (2, 2, 5, 5)                      # a cut at least every 5 frames: several records per step
RULES = [NO_HARD_RULES, DENSE_RULES]


def stream_plan(spec):
    return sc.plan_frames(*spec['shape'], frames_of=spec.get('frames_of'))


def frames_for(plan, n_samples):
    """more frames than a stream of n_samples can make final under either frames_of"""
    return n_samples // plan.samples_per_frame + plan.Tw + 64


def whole_rows(rng, T, p_blank=0.45, max_run=2, no_hard=False):
    """A stream's token and score rows by GLOBAL frame.  A stretch of 30 blank frames sits at frame 40 (TIMEOUT repeats
    through it).  no_hard: a blank is written behind every third non-blank frame in a row, so frames Fmax .. Fhard - 1 =
    12 .. 15 of an utterance always hold a blank and HARD never fires under NO_HARD_RULES."""
    tok = sc.token_row(rng, T, p_blank, max_run)
    tok[40:70] = BLANK
    if no_hard:
        run = 0
        for t in range(T):
            run = run + 1 if tok[t] != BLANK else 0
            if run == 4:
                tok[t], run = BLANK, 0
    return tok, sc.score_row(rng, T)


def play_ep(plan, eplan, n_samples, tok_all, fs_all, S=1, slot=0, perturb=True):
    """One stream through stream_cases.play with the endpoint twin behind every emit.  Window rows are the global rows at the
    window's place; with perturb the look-ahead frames of every other step differ from what they become.  Returns (steps -
    play's dicts with 'ep': the step's EpRow -, the stream state, the endpoint state)."""
    state, push, window, emit = sc.host_ops(plan, S, slot)
    ep = se.EpState(S)
    rng = np.random.default_rng(n_samples + 1)
    eps, now = [], {}

    def rows(k, Tw):
        first = plan.window_of(state.received(slot))[2]
        t, f = tok_all[first:first + Tw].copy(), fs_all[first:first + Tw].copy()
        assert len(t) == Tw
        if perturb and k % 2:
            lim = max((state.received(slot) - plan.Rr) // plan.samples_per_frame - first, 0)
            t[lim + 1:] = sc.token_row(rng, Tw, 0.5, 2)[lim + 1:]
        now['k'] = k
        return t, f

    def emit_ep(t, f, e, first, end):
        s = emit(t, f, e, first, end)
        flags = (st.END if end else 0) | (st.BEGIN if now['k'] == 0 else 0)
        eps.append(se.endpoint_host(ep, state, slot, flags, t, f, e, first, s.start, s.nframes, s.n_new, s.status, BLANK, eplan,
                                    session=True))
        return s

    _, steps = sc.play(plan, n_samples, rows, push, window, emit_ep)
    for d, r in zip(steps, eps):
        d['ep'] = r
    return steps, state, ep


def records_of(steps):
    for d in steps:
        assert d['ep'].status == se.STATUS_OK
    return np.concatenate([d['ep'].records for d in steps])


def check_slicing(steps, plan, eplan):
    """Invariant 1: the records of all steps, concatenated, are endpoints_whole_host of the concatenated final frames on every
    byte.  Returns (records, final tokens, final scores)."""
    row_t, row_f = sc.check_invariant(steps, plan.tail_pitch)
    got = records_of(steps)
    want = se.endpoints_whole_host(row_t, row_f, BLANK, eplan)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (got, want)
    return got, row_t, row_f


def delta_arrays(steps):
    cat = lambda name, dt: np.concatenate([getattr(d['step'], name) for d in steps] + [np.zeros(0, dtype=dt)]).astype(dt)
    return cat('labels', np.int32), cat('start', np.int32), cat('nframes', np.int32), cat('score', np.float32)


def check_content(recs, steps, row_t, row_f, collapse=True):
    """Invariant 2: utterances tile [0, T) and the labels; every score is utt_score_host of the utterance's own frames; with
    `collapse` every utterance's labels, starts, nframes and scores are collapse_host of tokens[first:end], offset by first."""
    lab, start, nfr, score = delta_arrays(steps)
    at, done = 0, 0
    for i, r in enumerate(recs):
        first, end = int(r[se.R_FIRST]), int(r[se.R_END])
        assert int(r[se.R_INDEX]) == i and first == at and end >= first
        at = end
        assert se.record_score(r).tobytes() == np.float32(ctc.utt_score_host(row_f[first:end])).tobytes(), i
        le = int(r[se.R_LABEL_END])
        assert le >= done
        if collapse:
            if end > first:
                ref = ctc.collapse_host(row_t[None, first:end], row_f[None, first:end], blank=BLANK)
                n = int(ref.n_labels[0])
                assert le - done == n, (i, r)
                assert lab[done:le].tobytes() == ref.labels[0, :n].tobytes()
                assert start[done:le].tobytes() == (ref.start[0, :n] + first).astype(np.int32).tobytes()
                assert nfr[done:le].tobytes() == ref.nframes[0, :n].tobytes()
                assert score[done:le].tobytes() == ref.score[0, :n].tobytes()
            else:
                assert le == done
        done = le
    assert at == len(row_t) and done == len(lab) and int(recs[-1][se.R_REASON]) == se.UTT_END


def reasons(recs):
    return [int(r[se.R_REASON]) for r in recs]


# ---------------------------------------------------------------------------------------------------------- the façade
def facade_endpointing(plan_spf_s=0.02):
    """two frames of silence, a time-out of 10 frames, MAX at 25 and HARD at 30 frames: cuts are certain on a random net"""
    return se.Endpointing(silence_s=2 * plan_spf_s, start_timeout_s=10 * plan_spf_s, max_utt_s=25 * plan_spf_s, hard_max_s=30 * plan_spf_s)


def compose_utterances(m, audio, lens, endpoint, device='cpu', streams=(0, 1), **kw):
    """The host composition of a session with endpoint=: per step window_host -> model._forward(decode='frames') -> emit_host
    -> endpoint_host, in the batches stream_cases.compose_on_host makes; every record then takes its labels off the
    concatenated deltas.  Returns {stream: [tuple(StreamUtterance with slot = the stream's number), ...]}."""
    import torch
    plan = m._stream_plan(**kw)
    eplan = se.EndpointPlan.for_stream(plan, endpoint)
    vocab, spf_s = m.decoder.vocabulary, plan.seconds_per_frame()
    blank = len(vocab)
    state, ep = st.StreamState(len(streams), plan), se.EpState(len(streams))
    deltas, recs, stepped = {j: [] for j in range(len(streams))}, {j: [] for j in range(len(streams))}, set()

    def step(rows, end):
        win, wl, first = st.window_host(state, rows)
        t, f, e = m._forward(torch.from_numpy(win).to(device), torch.from_numpy(wl).to(device).long(), decode='frames')
        t, f, e = t.cpu().numpy(), f.float().cpu().numpy(), e.cpu().numpy()
        for b, j in enumerate(rows):
            s = st.emit_host(t[b], f[b], int(e[b]), int(first[b]), state, j, end, blank, session=True)
            fl = (st.END if end else 0) | (0 if j in stepped else st.BEGIN)
            stepped.add(j)
            r = se.endpoint_host(ep, state, j, fl, t[b], f[b], int(e[b]), int(first[b]), s.start, s.nframes, s.n_new, s.status, blank,
                                 eplan, session=True)
            assert r.status == 0
            deltas[j].append(s)
            recs[j] += list(r.records)

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
    out = {}
    for j, i in enumerate(streams):
        cat = lambda name, dt: np.concatenate([getattr(s, name) for s in deltas[j]]).astype(dt)
        lab, start, nfr, score = cat('labels', np.int32), cat('start', np.int32), cat('nframes', np.int32), cat('score', np.float32)
        done, utts = 0, []
        for r in recs[j]:
            le = int(r[se.R_LABEL_END])
            res = ctc.CtcResult(lab[None, done:le], np.array([le - done], np.int32), start[None, done:le], nfr[None, done:le],
                                score[None, done:le], se.record_score(r).reshape(1), blank)
            done = le
            sp = int(r[se.R_SP_FIRST]) >= 0
            utts.append(dataclasses.astuple(ctc.StreamUtterance(
                i, int(r[se.R_INDEX]), se.REASONS[int(r[se.R_REASON])], int(r[se.R_FIRST]) * spf_s, int(r[se.R_END]) * spf_s,
                int(r[se.R_SP_FIRST]) * spf_s if sp else None, (int(r[se.R_SP_LAST]) + 1) * spf_s if sp else None,
                ctc.to_hypotheses(res, vocab, spf_s)[0])))
        assert done == len(lab)
        out[i] = utts
    return plan, out


def play_ep_session(m, audio, lens, piece, endpoint, device='cpu', streams=(0, 1), max_streams=2, after_push=None, wrap=None, **kw):
    """stream_cases.play_session with endpoint=: returns ({stream: [tuple(StreamUtterance, slot = the stream's number)]}, the
    hypotheses close() returned, the session's step count); after_push(sess, new utterances) runs behind every push, wrap(sess) once on the new session"""
    import torch
    sess = m.stream(max_streams=max_streams, endpoint=endpoint, **kw)
    if wrap is not None:
        wrap(sess)
    slots = [sess.open() for _ in streams]
    utts = []
    x = torch.from_numpy(audio).to(device)
    for off in range(0, max(lens[i] for i in streams), piece):
        live = [j for j, i in enumerate(streams) if off < lens[i]]
        n = [min(piece, lens[streams[j]] - off) for j in live]
        sig = torch.zeros(len(live), max(n), device=device, dtype=x.dtype)          # float32, or int16 with input_rate= in kw
        for k, j in enumerate(live):
            sig[k, :n[k]] = x[streams[j], off:off + n[k]]
        sess.push([slots[j] for j in live], sig, torch.tensor(n))
        new = sess.take_utterances()
        if after_push is not None:
            after_push(sess, new)
        utts += new
    hyps = [sess.close(s) for s in slots]
    utts += sess.take_utterances()
    steps = sess.steps
    sess.close_all()
    out = {i: [dataclasses.astuple(dataclasses.replace(u, slot=i)) for u in utts if u.slot == s] for s, i in zip(slots, streams)}
    return out, hyps, steps
