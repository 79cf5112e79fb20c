"""Inputs of the streaming beam-search tests, the step schedules they share and an independent float64 lagged search to
hold qasr.stream_beam against.  NumPy only.

The oracle follows beam_cases.oracle_beam's style: dicts keyed by prefix tuples, numpy.logaddexp, no table, no fixed
point, no hashes, no ring, no nodes.  Every prefix carries the creation frames of its labels; a prefix that enters the
beam anew takes its parent's frames plus the current frame.  It shares nothing with qasr/stream_beam.py but the rules."""
import math
import os

import numpy as np

import beam_cases
import beam_lm_cases
from beam_cases import GAP, MAX_WAIVED, oracle_topn

K = 32


def oracle_lagged(logp, W, N, blank, lag, K=K):
    """float64 lagged search over logp [T, C]; returns (best prefix tuple, the smallest float64 gap a decision turned on:
    at a round between the best entry and the best entry that the round dropped, at END between the two best entries)"""
    NEGF = -math.inf
    lae = lambda a, b: float(np.logaddexp(a, b))       # noqa: E731
    T, C = logp.shape
    beam = [((), 0.0, NEGF, ())]                        # (prefix, pb, pnb, creation frames)
    gap = math.inf
    for t in range(T):
        cands = [(int(c), float(logp[t, c])) for c in oracle_topn(logp[t], min(N, C))]
        acc = {}
        for i, (pre, pb, pnb, fr) in enumerate(beam):
            acc[pre] = [NEGF, NEGF, (i, -1), fr]
        for i, (pre, pb, pnb, fr) in enumerate(beam):
            sc = lae(pb, pnb)
            last = pre[-1] if pre else -1
            for n, (c, lp) in enumerate(cands):
                if c == blank:
                    acc[pre][0] = lae(acc[pre][0], lp + sc)
                    continue
                if c == last:
                    if pnb != NEGF:
                        acc[pre][1] = lae(acc[pre][1], lp + pnb)
                    if pb == NEGF:
                        continue
                    v = lp + pb
                else:
                    v = lp + sc
                ext = pre + (c,)
                if ext not in acc:
                    acc[ext] = [NEGF, NEGF, (i, n), fr + (t,)]
                acc[ext][1] = lae(acc[ext][1], v)
        ents = [(lae(a[0], a[1]), a[2], pre, a[0], a[1], a[3]) for pre, a in acc.items()]
        ents = [e for e in ents if e[0] != NEGF]
        ents.sort(key=lambda e: (-e[0], e[1]))
        beam = [(e[2], e[3], e[4], e[5]) for e in ents[:W]]
        if (t + 1) % K == 0 and t - lag >= 0 and beam:
            h = t - lag
            old = lambda e: e[0][:sum(f <= h for f in e[3])]      # noqa: E731
            keep = old(beam[0])
            dropped = [lae(e[1], e[2]) for e in beam if old(e) != keep]
            if dropped:
                gap = min(gap, lae(beam[0][1], beam[0][2]) - max(dropped))
            beam = [e for e in beam if old(e) == keep]
    if len(beam) > 1:
        gap = min(gap, lae(beam[0][1], beam[0][2]) - lae(beam[1][1], beam[1][2]))
    return (beam[0][0] if beam else ()), gap


# (name, classes, T, W, N, utterances, seed, blend, sharp, lags): the committed lists of the twin-against-oracle test.  The
# gap of an utterance is the smallest over every round and END, so it shrinks with the number of rounds: the lists are drawn
# sharper (sharp 2.5) than beam_cases' T = 250 lists.
ORACLE_LISTS = (
    ('en_t200_w16_n20', 29, 200, 16, 20, 5, 501, False, 2.5, (7, 40)),
    ('en_t200_w3_n20', 29, 200, 3, 20, 10, 502, False, 2.5, (0, 40)),
)


def oracle_list(name):
    _, C, T, W, N, n, seed, blend, sharp, lags = next(s for s in ORACLE_LISTS if s[0] == name)
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(beam_cases.peaky_logp(rng, T, C, C - 1, sharp=sharp, blend=blend), C - 1, W, N) for _ in range(n)], lags


_checked = {}


def checked_oracle_list(name):
    """[(logp, blank, W, N, lag, oracle's best prefix, gap)]; asserts the cap on waivers here, in the generator: a list that
    trips it is drawn sharper, the cap and the gap stay"""
    if name not in _checked:
        cases, lags = oracle_list(name)
        out = []
        for lp, blank, W, N in cases:
            for lag in lags:
                best, gap = oracle_lagged(lp, W, N, blank, lag)
                out.append((lp, blank, W, N, lag, best, gap))
        waived = sum(c[6] < GAP for c in out)
        assert waived <= MAX_WAIVED * len(out), f'{name}: {waived} of {len(out)} cases have a float64 gap below {GAP}'
        _checked[name] = out
    return _checked[name]


# ------------------------------------------------------------------------------------------------------- streams and steps
def stream_logp(seed, T, C=29, sharp=1.5, blend=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    return beam_cases.peaky_logp(rng, T, C, C - 1, sharp=sharp, blend=blend)


def lm_stream_logp(model, seed, T, sharp=1.5):
    """log-probabilities around sentences of a committed model (beam_lm_cases.MODELS): [T, C], blank = C - 1"""
    spec = next(s for s in beam_lm_cases.MODELS if s[0] == model)
    rng = np.random.Generator(np.random.PCG64(seed))
    return beam_lm_cases.lm_logp(rng, spec, T, sharp)


def load_lm(golden_dir, model):
    from qasr import ngram
    return ngram.NgramLM.from_arpa(beam_lm_cases.model_path(golden_dir, model), beam_lm_cases.vocab_of(model))


# steps of 1, 31, 32, 33, 64 and 95 final frames that start on both sides of multiples of 32 (and on them)
STEP_LENS_A = (31, 1, 32, 33, 95, 64, 1, 31, 33, 95, 32, 64)      # starts 0, 31, 32, 64, 97, 192, 256, 257, 288, 321, 416, 448
STEP_LENS_B = (33, 95, 64, 32, 1, 31, 64, 33, 1, 95, 31, 32)      # starts 0, 33, 128, 192, 224, 225, 256, 320, 353, 354, 449, 480


def cuts_of(step_lens, T):
    """frame indices at which a stream of T frames is cut, cycling through step_lens"""
    out, t, i = [], 0, 0
    while True:
        t += step_lens[i % len(step_lens)]
        if t >= T:
            return out
        out.append(t)
        i += 1


def edges_of(cuts, T):
    return [0] + list(cuts) + [T]


def greedy_final(cid, blank):
    """the greedy collapse of a stream's frames from its top-1 candidates: [(label, first frame)]"""
    out, prev = [], blank
    for t, c in enumerate(np.asarray(cid)[:, 0].tolist()):
        if c != blank and c != prev:
            out.append((c, t))
        prev = c
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---------------------------------------------------------------------------------------------------------- the façade
def compose_on_host(m, audio, lens, beam, device='cpu', streams=(0, 1), **kw):
    """per step: window_host -> model._forward -> topn_host -> step_batch_host -> emit_batch_host, over the batches a
    session makes of streams pushed side by side (stream_cases.compose_on_host's: chunk k of every stream that has one
    runs as one batch, every END step on its own).  Returns (plan, beam plan, {stream: [BeamStepBatch of one row, ...]})."""
    import torch
    from qasr import beam as qb, stream as st, stream_beam as sb
    plan = m._stream_plan(**kw)
    bplan = sb.StreamBeamPlan.for_stream(plan, beam)
    blank = len(m.decoder.vocabulary)
    state, bstate = st.StreamState(len(streams), plan), sb.StreamBeamState(len(streams), bplan)
    out = {i: [] for i in streams}
    begun = set()

    def step(rows, end):
        win, wl, first = st.window_host(state, rows)
        logp, e, t = m._forward(torch.from_numpy(win).to(device), torch.from_numpy(wl).to(device).long())
        logp, e, t = logp.float().cpu(), e.cpu().numpy(), t.cpu()
        f = logp.gather(2, t.long().unsqueeze(-1)).squeeze(-1).numpy()
        cid, cq = qb.topn_host(logp.numpy(), bplan.N, e)
        flags = [(st.END if end else 0) | (0 if j in begun else st.BEGIN) for j in rows]
        begun.update(rows)
        o = sb.step_batch_host(bstate, state, rows, flags, cid, cq, e, first, blank, beam.lm, beam.alpha, beam.beta)
        es = st.emit_batch_host(state, rows, flags, t.numpy(), f, e, first, blank)
        assert o.status.tolist() == [0] * len(rows) and es.status.tolist() == [0] * len(rows)
        for b, j in enumerate(rows):
            out[streams[j]].append({k: (None if v is None else v[b]) for k, v in vars(o).items()})

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
    return plan, bplan, out


def check_against_composition(m, slots, ups, hyps, want, beam, streams=(0, 1)):
    """the session's updates and hypotheses against the composition's rows"""
    from qasr import beam as qb
    spf_s, vocab = m.seconds_per_frame(), m.decoder.vocabulary
    text = lambda ids: ''.join(vocab[k] for k in ids)        # noqa: E731
    for s, h, i in zip(slots, hyps, streams):
        steps = want[i]
        assert len(ups[s]) == len(steps) - 1                                     # every step but END came out of a push
        labels, frames = [], []
        for u, w in zip(ups[s] + [None], steps):
            n = int(w['n_new_labels'])
            lab, fr = w['labels'][:n].tolist(), w['frames'][:n]
            labels += lab
            frames += fr.tolist()
            if u is not None:
                assert u.labels == lab and u.text == text(lab) and u.score == []
                assert u.start_s == (fr.astype(np.float64) * spf_s).tolist() and u.end_s == ((fr + 1).astype(np.float64) * spf_s).tolist()
                assert u.tail_text == text(w['tail_labels'][:int(w['tail_n'])].tolist())
        end = steps[-1]
        rows = h if beam.n_best > 1 else [h]
        assert len(rows) == int(end['n_hyps']) >= 1
        head = labels[:len(labels) - int(end['end_n_labels'][0])]
        for k, hyp in enumerate(rows):
            suffix = end['end_labels'][k, :int(end['end_n_labels'][k])].tolist()
            assert hyp.labels == head + suffix and hyp.text == text(head + suffix)
            assert hyp.utt_score == float(end['end_score'][k]) / qb.ONE
            assert hyp.lm_score == (None if beam.lm is None else float(end['end_lm_score'][k]) / qb.ONE)
        assert rows[0].labels == labels and rows[0].start_s == (np.array(frames, dtype=np.float64) * spf_s).tolist()
        assert frames == sorted(set(frames)) and int(end['commit_len']) == len(labels)


def play_session(m, audio, lens, piece, beam, device='cpu', streams=(0, 1), max_streams=2, **kw):
    """stream_cases.play_session with beam=: (slots, updates per slot, hypotheses, steps, the closed session)"""
    import torch
    sess = m.stream(max_streams=max_streams, beam=beam, **kw)
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
    return slots, ups, hyps, steps, sess
