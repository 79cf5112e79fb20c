"""Inputs and helpers of the streaming beam endpointing tests (qasr.stream_beam's STREAM_BEAM_EP_RULES, k_stream_beam_ep): the
records of a stream - from the endpoint rule over the stream's own greedy frames, or hand-made -, their distribution over
steps, a stepwise runner of the twin that keeps every step's outputs and state block, the conditions that keep the case
lists honest, and the host composition of a session with StreamBeam(endpoint=).  NumPy only (the composition imports torch
when it is called)."""
import dataclasses

import numpy as np

import boost_cases
import stream_beam_cases as sbc
import stream_boost_cases as sboc
import stream_cases as sc
from qasr import beam as qb, ctc, stream as st, stream_beam as sb, stream_ep as se
from stream_beam_cases import STEP_LENS_A, STEP_LENS_B, cuts_of, edges_of  # noqa: F401
from stream_ep_cases import DENSE_RULES  # noqa: F401

LONG_RULES = (9, 40, 70, 80)                    # Fsil, Fstart, Fmax, Fhard: utterances long enough for commit rounds inside them
K = sb.K_ROUND
PARAMS = [(1, 20, 7), (3, 64, 0), (16, 20, 40), (16, 1, 7), (128, 20, 40)]        # (W, N, lag)
# (name, model, alpha, beta, boosted): the four <LM, BOOST> instantiations
MODES = (('none', None, 0.0, 0.0, False), ('lm', 'en3', 0.7, 1.0, False), ('boost', None, 0.0, 0.0, True),
         ('lm_boost', 'en3', 0.7, 1.0, True))
_lms = {}


def lm_of(name):
    if name is not None and name not in _lms:
        _lms[name] = sbc.load_lm(sbc.GOLDEN, name)
    return _lms.get(name)


def stream_of(mode, seed, T):
    """log-probabilities [T, 29] of one stream: around sentences of the model with one, peaky noise without; a stretch of
    blank frames is written into both so that SILENCE and TIMEOUT fire as well"""
    lp = sbc.stream_logp(seed, T) if mode[1] is None else sbc.lm_stream_logp(mode[1], seed, T)
    lp = lp.copy()
    blank = lp.shape[1] - 1
    a = T // 3
    quiet = np.full(lp.shape[1], -9.0, np.float32)
    quiet[blank] = np.float32(np.log1p(-(lp.shape[1] - 1) * np.exp(-9.0)))
    lp[a:a + 24] = quiet
    return lp


def cands_of(lp, N):
    cid, cq = qb.topn_host(lp[None], N)
    return cid[0], cq[0]


def sets_of(lps, blank):
    """two phrase sets over the streams' own text, as test_gpu_stream_boost's: set 0 plain, set 1 whole words"""
    space = boost_cases.EN_SPACE if blank == 28 else -1
    p0 = sboc.phrases_of('nested_plain', 1, lps[0], blank, space)[0] + sboc.phrases_of('random', 2, lps[0], blank, -1)[0]
    rng = np.random.Generator(np.random.PCG64(3))
    p1 = boost_cases.gpu_phrases(rng, np.stack(lps), None, blank, space >= 0, space)
    return [sboc.make_set(p0, False, blank, space), sboc.make_set(p1, space >= 0, blank, space)], [(p0, False, space), (p1, space >= 0, space)]


def rule_records(lp, blank, rules):
    """the records of the whole stream under the endpoint rule over its greedy frames (endpoints_whole_host, which every
    slicing of endpoint_host equals): int32 [n][10], the END record last"""
    eplan = se.EndpointPlan(sc.plan_frames(95, 5, 1), *rules)
    return se.endpoints_whole_host(lp.argmax(1).astype(np.int32), lp.max(1).astype(np.float32), blank, eplan)


def hand_records(ends, T):
    """records with the given ends (rising, repeats allowed) and the END record at T; only index, first, end and reason
    matter to the beam"""
    out, first = [], 0
    for k, e in enumerate(list(ends) + [T]):
        out.append(se._record(k, first, e, 0, 0, 0, se.UTT_END if k == len(ends) else se.HARD, np.float32(0), 0))
        first = e
    return np.stack(out)


def step_records(recs, lo, hi, last, E):
    """the records a step over the frames [lo, hi) writes (end in (lo, hi]; the END record with the last step) as
    (int32 [E][10], n)"""
    mine = [r for r in recs if lo < int(r[se.R_END]) <= hi or (lo == hi == int(r[se.R_END]))]
    if not last:
        mine = [r for r in mine if int(r[se.R_REASON]) != se.UTT_END]
    assert len(mine) <= E, (len(mine), E)
    out = np.zeros((E, se.REC_WORDS), np.int32)
    if mine:
        out[:len(mine)] = np.stack(mine)
    return out, len(mine)


def max_step_records(recs, edges):
    return max(step_records(recs, edges[i], edges[i + 1], i == len(edges) - 2, 1 << 20)[1] for i in range(len(edges) - 1))


@dataclasses.dataclass
class EpRun:
    labels: list
    frames: list
    cut_delta_end: list         # cumulative over the stream
    cuts: list                  # per cut [(suffix, score, lm_tot[, boost_tot])]
    blocks: dict                # {edge: the state block after the step that ended there}
    commits_inside: int = 0     # labels committed by rounds (not by cuts)
    outs: list = None


def run_steps_ep(cid, cq, T, edges, recs, blank, W, n_best, lag, lm=None, alpha=0.0, beta=0.0, boost=None, check=True):
    """one stream through advance_ep_host in the steps `edges` (0 .. T)"""
    plan = sb.StreamBeamPlan(W, n_best, cid.shape[1], lag, max(T, 1), boost=boost is not None)
    state = sb.StreamBeamState(1, plan, check)
    aq, bq = sb._weights(lm, alpha, beta, blank)
    run = EpRun([], [], [], [], {}, 0, [])
    for i in range(len(edges) - 1):
        lo, hi = edges[i], edges[i + 1]
        rec, n = step_records(recs, lo, hi, i == len(edges) - 2, 1 << 12)
        row = sb.advance_ep_host(state, 0, cid, cq, 0, lo, hi, i == 0, rec[:n, se.R_END], blank, lm, aq, bq, boost,
                                 0 if boost is not None else -1)
        run.cut_delta_end += [len(run.labels) + x for x in row.cut_delta_end]
        suffixes = sum(len(c[0][0]) for c in row.cuts if c)
        run.commits_inside += len(row.labels) - suffixes
        run.cuts += row.cuts
        run.labels += row.labels
        run.frames += row.frames
        run.blocks[hi] = state.block.copy()
        run.outs.append(row)
    return run


def honest(recs, edges, K=K):
    """the conditions on a case list: (a step with two or more records, a cut strictly inside a step, a cut on a K boundary)"""
    ends = [int(r[se.R_END]) for r in recs]
    two = any(step_records(recs, edges[i], edges[i + 1], i == len(edges) - 2, 1 << 20)[1] >= 2 for i in range(len(edges) - 1))
    inside = any(edges[i] < e < edges[i + 1] for e in ends for i in range(len(edges) - 1))
    on_k = any(e > 0 and e % K == 0 for e in ends)
    return two, inside, on_k


def distinct_strings(cuts):
    """the most distinct suffix strings any one cut reports"""
    return max([len({tuple(h[0]) for h in c}) for c in cuts] + [0])


# ---------------------------------------------------------------------------------------------------------- the façade
def compose_beam_utterances(m, audio, lens, beam, device='cpu', streams=(0, 1), set_of_stream=None, **kw):
    """The host composition of a session with StreamBeam(endpoint=): per step window_host -> model._forward -> topn_host ->
    emit_batch_host -> endpoint_batch_host -> step_batch_ep_host, in the batches a session makes.  Returns (plan, {stream:
    [tuple(StreamUtterance with slot = the stream's number), ...]}, {stream: [(labels, frames, tail labels) of every step]})."""
    import torch
    plan = m._stream_plan(**kw)
    bplan = sb.StreamBeamPlan.for_stream(plan, beam)
    eplan = se.EndpointPlan.for_stream(plan, beam.endpoint)
    vocab, spf_s = m.decoder.vocabulary, plan.seconds_per_frame()
    blank = len(vocab)
    sets = None if beam.boost is None else list(beam.boost.values()) if isinstance(beam.boost, dict) else [beam.boost]
    state, ep, bstate = st.StreamState(len(streams), plan), se.EpState(len(streams)), sb.StreamBeamState(len(streams), bplan)
    utts, steps, open_delta, begun = {i: [] for i in streams}, {i: [] for i in streams}, {j: ([], []) for j in range(len(streams))}, set()
    text = lambda ids: ''.join(vocab[k] for k in ids)        # noqa: E731

    def step(rows, end):
        win, wl, first = st.window_host(state, rows)
        logp, e, t = m._forward(torch.from_numpy(win).to(device), torch.from_numpy(wl).to(device).long())
        logp, e, t = logp.float().cpu(), e.cpu().numpy(), t.cpu()
        f = logp.gather(2, t.long().unsqueeze(-1)).squeeze(-1).numpy()
        cid, cq = qb.topn_host(logp.numpy(), bplan.N, e)
        flags = [(st.END if end else 0) | (0 if j in begun else st.BEGIN) for j in rows]
        begun.update(rows)
        es = st.emit_batch_host(state, rows, flags, t.numpy(), f, e, first, blank)
        r = se.endpoint_batch_host(ep, state, rows, flags, t.numpy(), f, e, first, es, blank, eplan)
        o = sb.step_batch_ep_host(bstate, state, rows, flags, cid, cq, e, first, r.records, r.n_records, r.status, blank, beam.lm,
                                  beam.alpha, beam.beta, boost=sets,
                                  boost_set=None if sets is None else [set_of_stream[j] if set_of_stream else 0 for j in rows])
        assert o.status.tolist() == [0] * len(rows) and es.status.tolist() == [0] * len(rows) and r.status.tolist() == [0] * len(rows)
        for b, j in enumerate(rows):
            n = int(o.n_new_labels[b])
            lab, fr = o.labels[b, :n].tolist(), o.frames[b, :n].tolist()
            steps[streams[j]].append((lab, fr, o.tail_labels[b, :int(o.tail_n[b])].tolist()))
            at = 0
            for k in range(int(o.n_cuts[b])):
                de = int(o.cut_delta_end[b, k])
                ul, uf = open_delta[j][0] + lab[at:de], open_delta[j][1] + fr[at:de]
                open_delta[j], at = ([], []), de
                rec = r.records[b, k]
                hyps = []
                for h in range(int(o.cut_n_hyps[b, k])):
                    suffix = o.cut_labels[b, k, h, :int(o.cut_n_labels[b, k, h])].tolist()
                    head = ul[:len(ul) - int(o.cut_n_labels[b, k, 0])]
                    labs = head + suffix
                    hyp = ctc.Hypothesis(text(labs), labs, [x * spf_s for x in uf] if h == 0 else [],
                                         [(x + 1) * spf_s for x in uf] if h == 0 else [], None, None, [])
                    hyp.utt_score = float(o.cut_score[b, k, h]) / qb.ONE
                    if o.cut_lm_score is not None:
                        hyp.lm_score = float(o.cut_lm_score[b, k, h]) / qb.ONE
                    if o.cut_boost_score is not None:
                        hyp.boost_score = float(o.cut_boost_score[b, k, h]) / qb.ONE
                    hyps.append(hyp)
                if not hyps:
                    hyps = [ctc.Hypothesis(text(ul), ul, [x * spf_s for x in uf], [(x + 1) * spf_s for x in uf], None, None, [])]
                sp = int(rec[se.R_SP_FIRST]) >= 0
                u = ctc.StreamUtterance(streams[j], int(rec[se.R_INDEX]), se.REASONS[int(rec[se.R_REASON])], int(rec[se.R_FIRST]) * spf_s,
                                        int(rec[se.R_END]) * spf_s, int(rec[se.R_SP_FIRST]) * spf_s if sp else None,
                                        (int(rec[se.R_SP_LAST]) + 1) * spf_s if sp else None, hyps[0])
                if beam.n_best > 1:
                    u.n_best = hyps
                utts[streams[j]].append(dataclasses.astuple(u))
            open_delta[j] = (open_delta[j][0] + lab[at:], open_delta[j][1] + fr[at:])

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
    return plan, utts, steps


def play_beam_ep_session(m, audio, lens, piece, beam, device='cpu', streams=(0, 1), max_streams=2, open_boost=None, wrap=None, **kw):
    """a session with StreamBeam(endpoint=) fed in pieces: ({stream: [tuple(StreamUtterance, slot = the stream's number)]},
    the values close() returned, {stream: [StreamUpdate]}, the closed session)"""
    import torch
    sess = m.stream(max_streams=max_streams, beam=beam, **kw)
    if wrap is not None:
        wrap(sess)
    slots = [sess.open() if open_boost is None else sess.open(boost=open_boost[j]) for j in range(len(streams))]
    utts, ups = [], {s: [] for s in slots}
    x = torch.from_numpy(audio).to(device)
    for off in range(0, max(lens[i] for i in streams), piece):
        live = [j for j, i in enumerate(streams) if off < lens[i]]
        n = [min(piece, lens[streams[j]] - off) for j in live]
        sig = torch.zeros(len(live), max(n), device=device, dtype=x.dtype)
        for k, j in enumerate(live):
            sig[k, :n[k]] = x[streams[j], off:off + n[k]]
        for u in sess.push([slots[j] for j in live], sig, torch.tensor(n)):
            ups[u.slot].append(u)
        utts += sess.take_utterances()
    hyps = [sess.close(s) for s in slots]
    utts += sess.take_utterances()
    sess.close_all()
    out = {i: [dataclasses.astuple(dataclasses.replace(u, slot=i)) for u in utts if u.slot == s] for s, i in zip(slots, streams)}
    return out, hyps, {i: ups[s] for s, i in zip(slots, streams)}, sess
