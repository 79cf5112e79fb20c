"""Shared generators of the streaming keyword-spotting tests (qasr.stream_spot), built on stream_cases, spot_cases and
beam_cases: keyword sets over the three register layouts with invalid keywords between valid ones, whole-stream log-probability
rows by GLOBAL frame (the blank is the last class), a driver that plays several streams side by side through the push / window /
emit twins with any implementation of the spot step behind every emit, the check of the slicing invariant against spot_host,
and the host composition of a session with spot=.  NumPy only."""
import dataclasses

import numpy as np

import beam_cases
import spot_cases
import star_cases
import stream_cases as sc
from qasr import align, spot, stream as st, stream_spot as ss

PLANS = {'small': (4, 8, 2), 'wide': (70, 10, 2)}              # 'wide': steps make more than 64 frames final
LENGTHS = (1, 2, 31, 32, 63, 64, 127)                           # the three register layouts and their boundaries
# (name, classes, ML, K, plan, threshold, max_span): ML 31 / 32 / 63 / 64 / 127 is NS 1 / 2 / 2 / 4 / 4
KERNEL_CASES = [('c29_ml31_k5', 29, 31, 5, 'small', -16.0, 3), ('c29_ml32_k9', 29, 32, 9, 'small', -6.0, 40),
                ('c2_ml63_k5', 2, 63, 5, 'small', -16.0, 1000), ('c29_ml64_k9', 29, 64, 9, 'wide', -16.0, 1),
                ('c5207_ml127_k5', 5207, 127, 5, 'small', -8.0, 12), ('c29_ml127_k9', 29, 127, 9, 'wide', -16.0, 300)]


def plan_of(name):
    return sc.plan_frames(*PLANS[name])


def keyword_set(rng, C, blank, ML, K):
    """K keywords, row pitch ML: one of every length of LENGTHS that fits (the shortest first, ML itself among them), then
    random lengths; keywords 1 and 3 are invalid (they sit between valid ones), in turn: length 0, a length above ML, a label
    equal to the blank, a label >= C.  Returns (targets int32 [K, ML], target_lens int32 [K], the indices of the invalid)."""
    fit = [n for n in LENGTHS if n <= ML]
    want = [1, ML] + [n for n in fit if n not in (1, ML)]
    lens = (want + [int(rng.integers(1, min(ML, 6) + 1)) for _ in range(K)])[:K]
    rows = [star_cases.labels_without_blank(rng, n, C, blank, 0.2) for n in lens]
    tg, tl = spot_cases.pad(rows, blank, ML)
    kinds = [int(rng.integers(0, 4)), int(rng.integers(0, 4))]
    bad = [1, 3][:max(0, min(2, K - 2))]
    for k, kind in zip(bad, kinds):
        if kind == 0:
            tl[k] = 0
        elif kind == 1:
            tl[k] = ML + 1
        elif kind == 2:
            tg[k, int(tl[k]) // 2] = blank
        else:
            tg[k, 0] = C
    return tg, tl, bad


def frames_for(plan, n_samples):
    """more frames than a stream of n_samples can make final or see"""
    return n_samples // plan.samples_per_frame + plan.Tw + 64


def whole_logp(rng, T, C, blank, odd=False):
    """A stream's log-probabilities by GLOBAL frame, float32 [T, C]; odd: with a NaN row, a -inf row, a row of +inf and NaN
    entries and a single NaN entry among the first frames"""
    lp = beam_cases.peaky_logp(rng, T, C, blank, blend=bool(rng.integers(0, 2)))
    if odd:
        lp[3], lp[5] = np.nan, -np.inf
        lp[7, ::2], lp[7, 1::2] = np.inf, np.nan
        lp[9, 0] = np.nan
    return lp


def plant(lp, y, at, blank, frames_per_label=2):
    """spells y over lp's frames from `at` on as spot_cases.planted does (peaked rows); returns (first, last)"""
    T, C = lp.shape
    one, spans = spot_cases.planted(y, [at], T, C, blank, seed=at, frames_per_label=frames_per_label)
    a, b = spans[0]
    lp[max(a - 2, 0):b + 3] = one[0, max(a - 2, 0):b + 3]
    return a, b


@dataclasses.dataclass
class Step:
    """one spot step of the driver, per row: the inputs the step saw and what it gave"""
    rows: list                # the streams (indices) of the step's rows
    slots: list
    flags: list
    end: bool
    lp: np.ndarray            # [B, Tw, C]
    star: np.ndarray          # [B, Tw]
    enc: np.ndarray
    first: np.ndarray
    emit_status: np.ndarray
    lo: list                  # per row and keyword block: frames_done before (0 when fresh)
    hi: list                  # per row
    out: ss.SpotStepBatch = None


def play(plan, splan, S, slots, n_samples, lp_all, blank, spot_step, state=None, spstate=None, perturb=True, enc_clamp=None):
    """Streams i = 0 .. len(slots) - 1 side by side in slots[i]: chunk k of every stream that has one is pushed as one batch,
    the rows that filled a chunk step together, every END step on its own (what a session does).  The window rows are the
    global rows lp_all[i] at the window's place; with perturb the look-ahead frames of every other step differ from what they
    become.  spot_step(Step, stream state, spot state) -> SpotStepBatch runs behind every emit.  enc_clamp(step number, e) may
    change a step's encoded lengths.  Returns (steps, stream state, spot state)."""
    state = st.StreamState(S, plan) if state is None else state
    spstate = ss.SpotState(S, splan) if spstate is None else spstate
    rng = np.random.default_rng(sum(n_samples) + 1)
    C_cls = lp_all[0].shape[1]
    steps, stepped = [], set()

    def step(rows, end):
        sl = [slots[i] for i in rows]
        _, wl, first = st.window_host(state, sl)
        enc = np.array([min(int(plan.frames_of(int(n))), plan.Tw) for n in wl], dtype=np.int32)
        if enc_clamp is not None:
            enc = enc_clamp(len(steps), enc)
        lp = np.stack([lp_all[i][int(f):int(f) + plan.Tw] for i, f in zip(rows, first)]).astype(np.float32)
        assert lp.shape == (len(rows), plan.Tw, C_cls)
        if perturb and len(steps) % 2:
            for b, s in enumerate(sl):
                lim = max((state.received(s) - plan.Rr) // plan.samples_per_frame - int(first[b]), 0)
                if not end:
                    lp[b, lim + 1:] = beam_cases.peaky_logp(rng, plan.Tw, C_cls, blank)[lim + 1:]
        with np.errstate(invalid='ignore'):
            tok = np.where(np.isnan(lp), -np.inf, lp).argmax(-1).astype(np.int32)
        fs = np.take_along_axis(lp, tok[..., None].astype(np.int64), -1)[..., 0]
        flags = [(st.END if end else 0) | (0 if i in stepped else st.BEGIN) for i in rows]
        stepped.update(rows)
        lo = [[0 if (flags[b] & st.BEGIN or spstate.block[s, k, 1] == 0) else int(spstate.block[s, k, 0]) for k in range(splan.K)]
              for b, s in enumerate(sl)]
        emit = st.emit_batch_host(state, sl, flags, tok, fs, enc, first, blank)
        star = align.star_host(lp, enc, 0.0)
        d = Step(rows, sl, flags, end, lp, star, enc, np.asarray(first, np.int32), emit.status.copy(), lo,
                 [state.frames_done(s) for s in sl])
        d.out = spot_step(d, state, spstate)
        steps.append(d)

    k, Cs = 0, plan.C
    while any(n > k * Cs for n in n_samples):
        rows = [i for i, n in enumerate(n_samples) if n > k * Cs]
        n = [min(Cs, n_samples[i] - k * Cs) for i in rows]
        chunk = np.zeros((len(rows), Cs), dtype=np.float32)
        st.push_host(state, [slots[i] for i in rows], [st.BEGIN if k == 0 else 0] * len(rows), n, chunk)
        full = [i for b, i in enumerate(rows) if n[b] == Cs]
        if full:
            step(full, False)
        k += 1
    for i in range(len(slots)):
        step([i], True)
    return steps, state, spstate


def host_step(d, state, spstate, blank, PH=None):
    return ss.spot_batch_host(spstate, state, d.slots, d.flags, d.lp, d.star, d.enc, d.first, d.emit_status, blank, PH)


def final_rows(steps, i):
    """stream i's final frames as the steps that made them final saw them: (log_probs [T, C], star [T]); the final ranges of
    keyword block 0 tile [0, T)"""
    lp, star, done = [], [], 0
    for d in steps:
        if i not in d.rows:
            continue
        b = d.rows.index(i)
        lo, hi, first = d.lo[b][0], d.hi[b], int(d.first[b])
        assert lo == done and first <= lo <= hi
        lp.append(d.lp[b, lo - first:hi - first]), star.append(d.star[b, lo - first:hi - first])
        done = hi
    return np.concatenate(lp), np.concatenate(star)


def step_hits(steps, i, k, K):
    """the hits (start, end, score, detect) of stream i and keyword k over all steps, concatenated; asserts that no step lost a
    hit to the pitch"""
    out = []
    for d in steps:
        if i not in d.rows:
            continue
        p = d.rows.index(i) * K + k
        n = int(d.out.n_new_hits[p])
        assert n <= d.out.hit_start.shape[1], (n, d.out.hit_start.shape)
        out += [(int(d.out.hit_start[p, j]), int(d.out.hit_end[p, j]), int(d.out.hit_score[p, j]), int(d.out.hit_detect[p, j]))
                for j in range(n)]
    return out


def check_slicing(steps, splan, n_streams, blank, bad=()):
    """The invariant: per stream and keyword the step hits, concatenated, are spot_host's hits over the concatenated final
    frames on every byte of start / end / score and in count; an invalid keyword has ok = 0 and no hit anywhere.  Returns
    {(stream, keyword): [(start, end, score, detect)]}."""
    got = {}
    for i in range(n_streams):
        lp, star = final_rows(steps, i)
        T = lp.shape[0]
        want = None
        if T:
            want = spot.spot_host(lp[None], None, star[None], splan.targets, splan.target_lens, blank, splan.threshold_q,
                                  splan.max_span, max(T, 1))
        for k in range(splan.K):
            hits = step_hits(steps, i, k, splan.K)
            got[i, k] = hits
            oks = {int(d.out.ok[d.rows.index(i) * splan.K + k]) for d in steps if i in d.rows}
            assert oks == ({0} if k in bad else {1}), (i, k, oks)
            if want is None or k in bad:
                assert not hits
                continue
            n = int(want.n_hits[k])
            assert len(hits) == n, (i, k, len(hits), n)
            assert np.array([h[0] for h in hits], np.int32).tobytes() == want.hit_start[k, :n].tobytes(), (i, k)
            assert np.array([h[1] for h in hits], np.int32).tobytes() == want.hit_end[k, :n].tobytes(), (i, k)
            assert np.array([h[2] for h in hits], np.int64).tobytes() == want.hit_score[k, :n].tobytes(), (i, k)
            last = [d for d in steps if i in d.rows][-1]
            assert int(last.out.n_hits_total[last.rows.index(i) * splan.K + k]) == n
    return got


def same_batch(got, want, what=''):
    star_cases.same_bytes(got, want, ss.FIELDS, what)


# ---------------------------------------------------------------------------------------------------------- the façade
FACADE_LABELS = [[3], [5, 9], [1, 1], [20, 4, 7]]


def facade_spot(threshold=-6.0, max_span_s=0.4):
    return ss.StreamSpot(labels=FACADE_LABELS, threshold=threshold, max_span_s=max_span_s)


def compose_hits(m, audio, lens, sspot, device='cpu', streams=(0, 1), **kw):
    """The host composition of a session with spot=: per step window_host -> model._forward (log-probabilities) -> emit_host
    -> star_host -> spot_batch_host, in the batches stream_cases.compose_on_host makes.  Returns (plan, {stream: [StepRow]},
    {stream: [tuple(StreamHit with slot = the stream's number)] in the order of take_hits})."""
    import torch
    from qasr import ctc
    plan = m._stream_plan(**kw)
    given, tg, tl, thr, span, _ = m._spot_args('stream', sspot.keywords, sspot.labels, sspot.threshold, sspot.max_span_s, 1)
    splan = ss.StreamSpotPlan(plan, tg, tl, spot.check_threshold(thr, 'stream'), span)
    blank = len(m.decoder.vocabulary)
    state, spstate = st.StreamState(len(streams), plan), ss.SpotState(len(streams), splan)
    out, hits, stepped = {i: [] for i in streams}, [], set()

    def step(rows, end):
        win, wl, first = st.window_host(state, rows)
        logp, e, t = m._forward(torch.from_numpy(win).to(device), torch.from_numpy(wl).to(device).long())
        logp = logp.float()
        f = m._frame_scores(logp, t).cpu().numpy()
        logp, t, e = logp.cpu().numpy(), t.cpu().numpy(), e.cpu().numpy()
        status = []
        for b, j in enumerate(rows):
            s = st.emit_host(t[b], f[b], int(e[b]), int(first[b]), state, j, end, blank, session=True)
            out[streams[j]].append(s)
            status.append(s.status)
        flags = [(st.END if end else 0) | (0 if j in stepped else st.BEGIN) for j in rows]
        stepped.update(rows)
        o = ss.spot_batch_host(spstate, state, rows, flags, logp, align.star_host(logp, e, 0.0), e, first, status, blank)
        assert int(o.status.max()) == 0 and int(o.n_new_hits.max()) <= splan.hit_pitch
        hits.extend(ss.to_stream_hits(o, [streams[j] for j in rows], given, plan.seconds_per_frame())[0])

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
    by_stream = {i: [dataclasses.astuple(h) for h in ss.sort_hits(hits) if h.slot == i] for i in streams}
    return plan, out, by_stream


def play_spot_session(m, audio, lens, piece, sspot, device='cpu', streams=(0, 1), max_streams=2, wrap=None, **kw):
    """stream_cases.play_session with spot=: returns (slots, updates per slot, hypotheses, {stream: [tuple(StreamHit, slot = the
    stream's number)]}, the pending hits seen behind every push, the session)"""
    import torch
    sess = m.stream(max_streams=max_streams, spot=sspot, **kw)
    if wrap is not None:
        wrap(sess)
    slots = [sess.open() for _ in streams]
    ups, hits, pend = {s: [] for s in slots}, [], []
    x = torch.from_numpy(audio).to(device)
    for off in range(0, max(lens[i] for i in streams), piece):
        live = [j for j, i in enumerate(streams) if off < lens[i]]
        n = [min(piece, lens[streams[j]] - off) for j in live]
        sig = torch.zeros(len(live), max(n), device=device, dtype=x.dtype)
        for k, j in enumerate(live):
            sig[k, :n[k]] = x[streams[j], off:off + n[k]]
        for u in sess.push([slots[j] for j in live], sig, torch.tensor(n)):
            ups[u.slot].append(u)
        hits += sess.take_hits()
        pend.append({s: sess.pending_hits(s) for s in slots})
    hyps = [sess.close(s) for s in slots]
    hits += sess.take_hits()
    sess.close_all()
    by_stream = {i: [dataclasses.astuple(dataclasses.replace(h, slot=i)) for h in hits if h.slot == s] for s, i in zip(slots, streams)}
    return slots, ups, hyps, by_stream, pend, sess
