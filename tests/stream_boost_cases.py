"""Inputs and helpers of the streaming phrase-boosting tests (qasr.stream_beam with boost=, k_stream_beam_boost): phrase sets
per mode, a stepwise runner that keeps the state block after every step, and the host composition of a boosted session.
NumPy only (the composition imports torch when it is called)."""
import numpy as np

import beam_cases
import boost_cases
import stream_beam_cases as sbc
from boost_cases import EN_SPACE, NESTED, Brute
from stream_beam_cases import STEP_LENS_A, STEP_LENS_B, cuts_of  # noqa: F401

# the kinds of sets of the slicing sweep: random_set's phrases (plus pieces of the stream's greedy text, so that matches
# happen), and NESTED with whole words on and off.  A vocabulary without a space (zh) has no whole words: PhraseSet refuses.
SET_KINDS = ('random', 'nested_whole', 'nested_plain')


def phrases_of(kind, seed, lp, blank, space):
    """([(labels, weight)], whole) of one kind for a stream lp [T, C]; None when the kind needs a space and there is none"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == 'nested_whole':
        return (None, True) if space < 0 else ([(p, 1.0 + 0.5 * k) for k, p in enumerate(NESTED)], True)
    if kind == 'nested_plain':
        return [(p, 1.0 + 0.5 * k) for k, p in enumerate(NESTED)], False
    whole = space >= 0 and bool(rng.integers(0, 2))
    ph = boost_cases.random_set(rng, n_labels=4, whole=whole, space=space if whole else 3)
    g = beam_cases.greedy(lp, blank)
    for a in range(0, max(len(g) - 4, 1), 9):                       # pieces of what the frames say
        piece = tuple(c for c in g[a:a + int(rng.integers(2, 5))] if not (whole and c == space))
        if piece:
            ph.append((piece, float(rng.integers(2, 13)) / 4.0))
    return ph, whole


def make_set(phrases, whole, blank, space, **kw):
    from qasr import boost as qboost
    return qboost.PhraseSet([(list(p), w) for p, w in phrases], n_labels=blank, space=space, whole_words=whole, **kw)


def brute_of(phrases, whole, space):
    return Brute(phrases, whole, space)


def run_steps(cid, cq, T, edges, blank, W, n_best, lag, lm=None, alpha=0.0, beta=0.0, boost=None, check=True):
    """one stream through advance_host in the steps `edges` (0 .. T), the last one END; returns (labels, frames, end rows of
    the END step, {edge: the state block after the step that ended there (a copy)}, commit_len after every step)"""
    from qasr import stream_beam as sb
    plan = sb.StreamBeamPlan(W, n_best, cid.shape[1], lag, max(T, 1), boost=boost is not None)
    st = sb.StreamBeamState(1, plan, check)
    aq, bq = sb._weights(lm, alpha, beta, blank)
    labels, frames, blocks, commits, row = [], [], {}, [], None
    for i in range(len(edges) - 1):
        row = sb.advance_host(st, 0, cid, cq, 0, edges[i], edges[i + 1], i == 0, i == len(edges) - 2, blank, lm, aq, bq, boost,
                              0 if boost is not None else -1)
        labels += row.labels
        frames += row.frames
        blocks[edges[i + 1]] = st.block.copy()
        commits.append(row.commit_len)
    return labels, frames, row.end, blocks, commits


# ---------------------------------------------------------------------------------------------------------- the façade
def compose_on_host(m, audio, lens, beam, sets, set_of_stream, device='cpu', streams=(0, 1), **kw):
    """stream_beam_cases.compose_on_host with phrase sets: `sets` a list of PhraseSet, set_of_stream[j] the index of the set
    that stream j uses (-1: none).  Returns (plan, beam plan, {stream: [rows of one step, ...]})."""
    import torch
    from qasr import beam as qb, stream as st, stream_beam as sb
    plan = m._stream_plan(**kw)
    bplan = sb.StreamBeamPlan.for_stream(plan, beam)
    assert bplan.boost
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
        o = sb.step_batch_host(bstate, state, rows, flags, cid, cq, e, first, blank, beam.lm, beam.alpha, beam.beta, boost=sets,
                               boost_set=[set_of_stream[j] for j in rows])
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


def play_session(m, audio, lens, piece, beam, open_boost, device='cpu', streams=(0, 1), max_streams=2, **kw):
    """stream_beam_cases.play_session with open(boost=open_boost[j]) per stream"""
    import torch
    sess = m.stream(max_streams=max_streams, beam=beam, **kw)
    slots = [sess.open(boost=open_boost[j]) for j in range(len(streams))]
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


def check_boost_scores(hyps, want, beam, streams=(0, 1)):
    """boost_score of the session's hypotheses against the composition's END rows (the rest: check_against_composition)"""
    from qasr import beam as qb
    for h, i in zip(hyps, streams):
        end = want[i][-1]
        for k, hyp in enumerate(h if beam.n_best > 1 else [h]):
            assert hyp.boost_score == float(end['end_boost_score'][k]) / qb.ONE


def facade_phrases(m, audio, lens, **kw):
    """phrases that occur in what the model says for the audio: words (or pieces) of the unboosted greedy text"""
    import torch
    hyps = m.decode_stream(torch.from_numpy(audio), torch.tensor(lens), **kw)
    out = []
    for h in hyps:
        words = [w for w in h.text.split(' ') if len(w) >= 2]
        out += [w[:6] for w in words[:4]]
    return sorted(set(out)) or ['ab']


check_against_composition = sbc.check_against_composition
