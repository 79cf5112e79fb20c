"""Streaming beam endpointing on the host (qasr.stream_beam's STREAM_BEAM_EP_RULES): any slicing of a stream with cuts equals the
whole-stream statement on every byte, the state block and the ring after every step included; with a lag at or beyond the
longest utterance every utterance's n-best is qasr.beam's offline search over the utterance's own frames; a stream without a
record is step_batch_host; boost_tot of every utterance hypothesis is the brute-force sum over that utterance's text alone;
committed text never changes; every status leaves the state alone; the plan's sizes hold over a protocol with cuts; and the
façade on CPU tensors is the host composition however the pushes are sliced."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boost_cases  # noqa: E402
import stream_beam_ep_cases as cases  # noqa: E402
import stream_cases as sc  # noqa: E402
import stream_ep_cases as ec  # noqa: E402
from qasr import beam as qb  # noqa: E402
from qasr import stream as st  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402
from qasr import stream_ep as se  # noqa: E402

ZH = ('zh', 'zh2', 1.5, 0.5, False)                        # a character-mode model next to the four modes
ALL_MODES = cases.MODES + (ZH,)


def _setup(mode, seed, T, N):
    lp = cases.stream_of(mode, seed, T)
    blank = lp.shape[1] - 1
    sets, spec = cases.sets_of([lp], blank) if mode[4] else (None, None)
    return lp, blank, cases.cands_of(lp, N), cases.lm_of(mode[1]), mode[2], mode[3], sets, spec


@pytest.mark.parametrize('mode', ALL_MODES, ids=[m[0] for m in ALL_MODES])
@pytest.mark.parametrize('W,N,lag', cases.PARAMS)
def test_any_slicing_equals_the_whole_stream(mode, W, N, lag):
    """Every parameter runs two record lists of its stream, one under DENSE_RULES and one under LONG_RULES.  STEP_LENS_A,
    STEP_LENS_B, one frame per step and one step against lagged_search_ep_host: the delta, cut_delta_end, every cut's rows,
    the state block and the ring; and after EVERY step of both schedules the block against the whole-stream statement of
    the frames so far.  The dense list holds a step with two or more records, a cut strictly inside a step and a cut with
    end % K == 0; under the long list a round commits inside an utterance that is cut later."""
    T = 200 if W == 128 else 320
    lp, blank, (cid, cq), lm, alpha, beta, sets, _ = _setup(mode, 7 + W + lag, T, N)
    nb = min(W, 3)
    bs = None if sets is None else sets[(W + lag) % 2]
    kw = dict(blank=blank, beam_width=W, n_best=nb, lm=lm, alpha=alpha, beta=beta, lag=lag, boost=bs)
    schedules = [cases.edges_of(cases.cuts_of(sl, T), T) for sl in (cases.STEP_LENS_A, cases.STEP_LENS_B)]
    for rules in (cases.DENSE_RULES, cases.LONG_RULES):
        recs = cases.rule_records(lp, blank, rules)
        ends = [int(r[se.R_END]) for r in recs]
        whole = sb.lagged_search_ep_host(cid, cq, T, ends, **kw)
        if W <= 16:
            assert whole == sb.lagged_search_ep_host(cid, cq, T, ends, steps=list(range(1, T)), check=False, **kw)
        assert len(whole.cuts) == len(recs) == len(whole.cut_delta_end) and whole.cut_delta_end[-1] == len(whole.labels)
        assert whole.frames == sorted(set(whole.frames))                        # creation frames rise, across utterances too
        for r, (ul, uf), cut in zip(recs, whole.utts, whole.cuts):              # an utterance's text lies inside its span
            assert all(int(r[se.R_FIRST]) <= f < int(r[se.R_END]) for f in uf)
            assert not cut or ul[len(ul) - len(cut[0][0]):] == cut[0][0]
        assert int(np.frombuffer(whole.block.tobytes(), np.int32)[5]) == len(recs)
        refs = {}
        for edges in schedules:
            assert whole == sb.lagged_search_ep_host(cid, cq, T, ends, steps=edges[1:-1], **kw)
            run = cases.run_steps_ep(cid, cq, T, edges, recs, blank, W, nb, lag, lm, alpha, beta, boost=bs)
            assert run.labels == whole.labels and run.cuts == whole.cuts and run.cut_delta_end == whole.cut_delta_end
            for hi in edges[1:-1]:                                              # the state after EVERY step: the statement of the frames so far
                if hi not in refs:
                    part = [r for r in recs if int(r[se.R_END]) <= hi and int(r[se.R_REASON]) != se.UTT_END]
                    refs[hi] = cases.run_steps_ep(cid, cq, hi, [0, hi], part, blank, W, nb, lag, lm, alpha, beta, boost=bs, check=False).blocks[hi]
                assert run.blocks[hi].tobytes() == refs[hi].tobytes(), (rules, hi)
            assert run.blocks[T].tobytes() == whole.block.tobytes()
        conds = [cases.honest(recs, edges) for edges in schedules]
        if rules == cases.DENSE_RULES:
            assert conds[0] == (True, True, True) and conds[1] == (True, True, True), conds
        else:
            assert conds[0][1] and run.commits_inside > 0                       # a round committed inside an utterance that a cut ended
        if W > 1 and N > 1:
            assert cases.distinct_strings(whole.cuts) >= 2


@pytest.mark.parametrize('mode', ALL_MODES, ids=[m[0] for m in ALL_MODES])
@pytest.mark.parametrize('W,N', [(1, 20), (3, 20), (16, 64)])
def test_a_lag_beyond_every_utterance_is_the_offline_search_per_utterance(mode, W, N):
    """beam_search_host over cand[first:end] alone is pinned against a float64 search: the independent yardstick"""
    T = 320
    lp, blank, (cid, cq), lm, alpha, beta, sets, spec = _setup(mode, 31 + W, T, N)
    recs = cases.rule_records(lp, blank, cases.LONG_RULES)
    ends = [int(r[se.R_END]) for r in recs]
    assert len(recs) >= 3 and max(int(r[se.R_END]) - int(r[se.R_FIRST]) for r in recs) <= 80
    for g, bs in enumerate([None] if sets is None else sets):
        for lag in (80, 400):
            got = sb.lagged_search_ep_host(cid, cq, T, ends, blank, W, W, lm, alpha, beta, lag=lag, boost=bs,
                                           steps=cases.cuts_of(cases.STEP_LENS_A, T))
            for r, cut, (ul, uf) in zip(recs, got.cuts, got.utts):
                first, end = int(r[se.R_FIRST]), int(r[se.R_END])
                if end == first:
                    assert [x[0] for x in cut] == [[]] and cut[0][1] == 0
                    continue
                off = qb.beam_search_host(cid[None, first:end], cq[None, first:end], None, blank, W, W, lm, alpha, beta, boost=bs)
                assert len(cut) == int(off.n_hyps[0]) >= 1 and ul == cut[0][0]    # nothing was committed before the cut
                for h, ent in enumerate(cut):
                    assert ent[0] == off.labels[0, h, :off.n_labels[0, h]].tolist() and ent[1] == int(off.score[0, h]), (first, end, h)
                    assert lm is None or ent[2] == int(off.lm_score[0, h])
                    if bs is not None:
                        assert ent[3] == int(off.boost_score[0, h]) == boost_cases.Brute(*spec[g]).final(ent[0])


@pytest.mark.parametrize('mode', cases.MODES[2:], ids=[m[0] for m in cases.MODES[2:]])
def test_boost_score_is_the_brute_force_sum_over_the_utterance_alone(mode):
    """a short lag: most of every utterance is committed before its cut, and phrase matches of one utterance do not leak
    into the next"""
    W, N, T, lag = 16, 20, 400, 3
    lp, blank, (cid, cq), lm, alpha, beta, sets, spec = _setup(mode, 77, T, N)
    recs = cases.rule_records(lp, blank, cases.LONG_RULES)
    ends = [int(r[se.R_END]) for r in recs]
    hits = 0
    for g, bs in enumerate(sets):
        got = sb.lagged_search_ep_host(cid, cq, T, ends, blank, W, 3, lm, alpha, beta, lag=lag, boost=bs, steps=cases.cuts_of(cases.STEP_LENS_B, T))
        brute = boost_cases.Brute(*spec[g])
        for cut, (ul, uf) in zip(got.cuts, got.utts):
            head = ul[:len(ul) - len(cut[0][0])] if cut else ul
            for ent in cut:
                assert ent[3] == brute.final(head + ent[0]) == bs.score(head + ent[0])
                hits += ent[3] > 0
        assert any(len(ul) > len(cut[0][0]) for cut, (ul, uf) in zip(got.cuts, got.utts) if cut)      # text was committed before a cut
    assert hits > 0


class _Pair:
    """step_batch_host and step_batch_ep_host side by side on streams without a record"""

    def __init__(self, bplan, S, splan):
        self.s1, self.s2 = st.StreamState(S, splan), st.StreamState(S, splan)
        self.b1, self.b2 = sb.StreamBeamState(S, bplan), sb.StreamBeamState(S, bplan)
        for s in (self.s1, self.s2):
            for slot in range(S):
                s.block[slot, 0:2].view(np.int64)[0] = 10 ** 9


@pytest.mark.parametrize('mode', cases.MODES, ids=[m[0] for m in cases.MODES])
def test_without_a_record_every_shared_byte_is_step_batch_host(mode):
    W, N, T, lag = 16, 20, 300, 7
    splan = sc.plan_frames(95, 5, 1)
    lp, blank, (cid, cq), lm, alpha, beta, sets, _ = _setup(mode, 9, T, N)
    bplan = sb.StreamBeamPlan(W, 3, N, lag, splan.max_final_frames, boost=sets is not None)
    p = _Pair(bplan, 1, splan)
    edges = cases.edges_of(cases.cuts_of(cases.STEP_LENS_A, T), T)
    none = np.zeros((1, 2, se.REC_WORDS), np.int32)
    for k in range(len(edges) - 1):
        lo, hi = edges[k], edges[k + 1]
        wid = np.full((1, splan.Tw, N), -1, np.int32)
        wq = np.full((1, splan.Tw, N), qb.EMPTY_Q, np.int32)
        wid[0, :hi - lo], wq[0, :hi - lo] = cid[lo:hi], cq[lo:hi]
        fl = [st.BEGIN if k == 0 else 0]
        kw = dict(boost=sets, boost_set=None if sets is None else [1])
        p.s1.block[0, 2] = lo                                                   # before emit
        a = sb.step_batch_host(p.b1, p.s1, [0], fl, wid, wq, [hi - lo], [lo], blank, lm, alpha, beta, **kw)
        p.s2.block[0, 2] = hi                                                   # as emit left it
        b = sb.step_batch_ep_host(p.b2, p.s2, [0], fl, wid, wq, [hi - lo], [lo], none, [0], [0], blank, lm, alpha, beta, **kw)
        assert a.status.tolist() == b.status.tolist() == [0] and p.b1.header(0)[2] == hi
        for name in ('labels', 'frames', 'n_new_labels', 'commit_len', 'n_live', 'tail_labels', 'tail_n'):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (k, name)
        assert p.b1.block.tobytes() == p.b2.block.tobytes() and not b.n_cuts.any() and (b.cut_score == qb.NEG).all()
    assert p.b1.header(0)[1] > 0


def test_committed_text_never_changes_and_the_plan_holds_over_cuts():
    """stepped frame by frame with the twin's own assertions on: every entry of every beam starts with the committed text of
    its utterance, no live ring row is overwritten although the ring wraps many times, and walk_ep's sizes hold"""
    W, N, lag, T = 16, 20, 7, 400
    mode = cases.MODES[0]
    lp = cases.stream_of(mode, 5, T)
    blank = lp.shape[1] - 1
    cid, cq = cases.cands_of(lp, N)
    recs = cases.rule_records(lp, blank, cases.LONG_RULES)
    ends = [int(r[se.R_END]) for r in recs]
    plan = sb.StreamBeamPlan(W, 4, N, lag, 1)
    assert T >= 8 * plan.F
    assert sb.walk_ep(plan, cid, cq, list(range(1, T + 1)), ends, blank) == len(ends) >= 5
    plan = sb.StreamBeamPlan(W, 4, N, lag, 95)
    steps = cases.edges_of(cases.cuts_of(cases.STEP_LENS_B, T), T)[1:]
    assert sb.walk_ep(plan, cid, cq, steps, ends, blank) == len(ends)
    dense = [int(r[se.R_END]) for r in cases.rule_records(lp, blank, cases.DENSE_RULES)]
    assert sb.walk_ep(plan, cid, cq, steps, dense, blank) == len(dense) > 50
    # committed text: the utterance's delta before the cut is a prefix of what the cut reports
    state = sb.StreamBeamState(1, plan)
    held, rk = [], 0
    for t in range(T):
        mine = [e for e in ends[rk:] if e == t + 1] if t < T - 1 else ends[rk:]
        row = sb.advance_ep_host(state, 0, cid, cq, 0, t, t + 1, t == 0, mine, blank)
        at = 0
        for de, cut in zip(row.cut_delta_end, row.cuts):
            utt = held + row.labels[at:de]
            assert cut and utt[len(utt) - len(cut[0][0]):] == cut[0][0] and utt[:len(held)] == held
            held, at = [], de
        held += row.labels[at:]
        rk += len(mine)
        e, commit, done = state.load(0, None)
        assert commit == len(held) == row.commit_len and done == t + 1
        for i in range(len(e)):
            assert sb._full_labels(state.trail[0], int(e.node[i]))[:commit] == held
    assert rk == len(ends) and held == []


def test_statuses_leave_the_state_alone():
    splan = sc.plan_frames(95, 5, 1)
    W, N, E = 3, 20, 3
    bp = sb.StreamBeamPlan(W, 2, N, 7, splan.max_final_frames)
    S = 8
    ss, bs = st.StreamState(S, splan), sb.StreamBeamState(S, bp)
    lp = cases.stream_of(cases.MODES[0], 3, splan.Tw)
    cid, cq = cases.cands_of(lp, N)
    blank = lp.shape[1] - 1

    def rec(ends, first_index=0, n=None):
        r = np.zeros((E, se.REC_WORDS), np.int32)
        for k, e in enumerate(ends):
            r[k] = se._record(first_index + k, 0, e, 0, 0, 0, se.HARD, np.float32(0), 0)
        return r, len(ends) if n is None else n

    def step(rows, ep_status=None):
        for slot, fl, enc, first, hi, r in rows:
            if 0 <= slot < S:
                ss.block[slot, 2] = hi
        return sb.step_batch_ep_host(bs, ss, [r[0] for r in rows], [r[1] for r in rows], np.stack([cid] * len(rows)), np.stack([cq] * len(rows)),
                                     [r[2] for r in rows], [r[3] for r in rows], np.stack([r[5][0] for r in rows]), [r[5][1] for r in rows],
                                     [0] * len(rows) if ep_status is None else ep_status, blank)

    o = step([(s, st.BEGIN, 40, 0, 40, rec([20])) for s in range(7)])
    assert o.status.tolist() == [0] * 7 and bs.block[0, 5] == 1 and o.n_cuts.tolist() == [1] * 7
    before = bs.block.copy()
    o = step([(9, 0, 40, 0, 60, rec([50], 1)), (0, 0, 60, 41, 60, rec([50], 1)), (1, 0, 60, 0, 39, rec([], 1)), (2, 0, 50, 0, 60, rec([55], 1)),
              (3, 0, 60, 0, 60, rec([50, 55, 58], 1, 4)), (4, 0, 60, 0, 60, rec([55, 50], 1)), (5, 0, 60, 0, 60, rec([40], 1)),
              (6, 0, 60, 0, 60, rec([61], 1))])
    assert o.status.tolist() == [sb.STATUS_SLOT, sb.STATUS_GAP] + [sb.STATUS_SYNC] * 6 and bs.block.tobytes() == before.tobytes()
    o = step([(0, 0, 60, 0, 60, rec([50], 0)), (1, 0, 60, 0, 60, rec([50], 1)), (2, st.BEGIN, 60, 0, 60, rec([50], 1)),
              (4, 0, 60, 0, 60, rec([50], 1, -1))], ep_status=[0, 1, 0, 0])
    assert o.status.tolist() == [sb.STATUS_SYNC] * 4 and bs.block.tobytes() == before.tobytes()
    assert o.n_new_labels.tolist() == [0] * 4 and (o.labels == blank).all() and (o.cut_score == qb.NEG).all() and not o.n_cuts.any()
    big = sb.StreamBeamPlan(128, 1, N, 7, splan.max_final_frames)
    bs2 = sb.StreamBeamState(1, big)
    ss.block[0, 2] = 2 ** 24 + 40
    bs2.block[0, 2], bs2.block[0, 3] = 2 ** 24, 1
    before = bs2.block.copy()
    o = sb.step_batch_ep_host(bs2, ss, [0], [0], cid[None], cq[None], [40], [2 ** 24], rec([])[0][None], [0], [0], blank)
    assert o.status.tolist() == [sb.STATUS_NODES] and bs2.block.tobytes() == before.tobytes()
    # a valid step with two records on the same frame and one at hi still goes through
    o = step([(0, 0, 60, 40, 60, rec([50, 50, 60], 1))])
    assert o.status.tolist() == [0] and o.n_cuts.tolist() == [3] and bs.block[0, 5] == 4 and o.cut_n_hyps[0, 1] == 1


def test_a_dead_beam_lives_again_behind_the_next_cut():
    W, N, T = 3, 20, 190
    lp = cases.stream_of(cases.MODES[0], 4, T)
    blank = lp.shape[1] - 1
    cid, cq = (x.copy() for x in cases.cands_of(lp, N))
    cid[50:60], cq[50:60] = -1, qb.EMPTY_Q
    r = sb.lagged_search_ep_host(cid, cq, T, [40, 80, 120, T], blank, W, W, lag=7, steps=[45, 52, 70, 95])
    assert len(r.cuts[0]) >= 1 and r.cuts[1] == [] and len(r.cuts[2]) >= 1 and len(r.cuts[3]) >= 1
    assert r.cut_delta_end[2] > r.cut_delta_end[1] and all(80 <= f < 120 for f in r.utts[2][1])
    assert all(40 <= f < 50 for f in r.utts[1][1])                              # what was committed before the beam died stays the utterance's


# ---------------------------------------------------------------------------------------------------------- the façade
torch = pytest.importorskip('torch')
KW = sc.FACADE_KW


def _model():
    from nemo.collections.asr.models import EncDecCTCModel
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')
    return m


def _facade_lm(m):
    from qasr import ngram
    import beam_lm_cases
    import stream_beam_cases as sbc
    return ngram.NgramLM.from_arpa(beam_lm_cases.model_path(sbc.GOLDEN, 'en3'), m.decoder.vocabulary)


@pytest.mark.parametrize('with_lm,boosted,n_best,lag_s', [(False, False, 1, 0.1), (True, True, 3, 0.1), (False, True, 2, 100.0)])
def test_session_on_cpu_tensors_is_the_composition(with_lm, boosted, n_best, lag_s):
    import stream_boost_cases as sboc
    torch.set_grad_enabled(False)
    m = _model()
    audio, lens = sc.facade_audio()[:, :50000], [20000, 50000]
    lm = _facade_lm(m) if with_lm else None
    boost = sboc.facade_phrases(m, audio, lens, **KW) if boosted else None
    beam = sb.StreamBeam(width=8, n_best=n_best, cutoff_top_n=20, lm=lm, alpha=0.5, beta=0.5, lag_s=lag_s, boost=boost,
                         endpoint=ec.facade_endpointing())
    sess = m.stream(max_streams=2, beam=beam, **KW)                              # the compiled sets, as the session holds them
    assert sess.endpoint is beam.endpoint and sess.eplan is not None and sess.bplan.boost == boosted
    cbeam = dataclasses.replace(beam, boost=None if not boosted else sess._sets[0], lm=sess.beam.lm, endpoint=beam.endpoint)
    sess.close_all()
    plan, want, steps = cases.compose_beam_utterances(m, audio, lens, cbeam, **KW)
    assert len(want[0]) >= 3 and len(want[1]) > 3 and any(u[2] in ('hard', 'silence', 'max') for u in want[1])
    results = []
    for piece in (1000, 15360, 50000):
        got, hyps, ups, _ = cases.play_beam_ep_session(m, audio, lens, piece, beam, **KW)
        assert got == want
        for i, h in zip((0, 1), hyps):                                           # close() returns the END utterance's hypothesis (list)
            assert want[i][-1][2] == 'end'
            assert (dataclasses.astuple(h) if n_best == 1 else [dataclasses.astuple(x) for x in h]) == want[i][-1][7 if n_best == 1 else 8]
        for i in (0, 1):                                                         # every step but END came out of a push
            assert len(ups[i]) == len(steps[i]) - 1
            for u, (lab, fr, tail) in zip(ups[i], steps[i]):
                assert u.labels == lab and u.tail_text == ''.join(m.decoder.vocabulary[k] for k in tail) and u.score == []
        results.append((got, repr(hyps)))
    assert results[0] == results[1] == results[2]
    if n_best > 1:
        assert any(u[8] is not None and len({x[0] for x in u[8]}) >= 2 for u in want[1])            # an utterance with two distinct strings
    if lag_s < 1:
        assert any(len(lab) > 0 for lab, fr, tail in steps[1][:-1])              # text was committed inside utterances
    rows = m.decode_stream(torch.from_numpy(audio), torch.tensor(lens), beam=beam, **KW)
    assert [[dataclasses.astuple(dataclasses.replace(u, slot=i)) for u in row] for i, row in enumerate(rows)] == [want[0], want[1]]


def test_session_with_input_rate_and_refusals():
    from qasr import resample as qr
    torch.set_grad_enabled(False)
    m = _model()
    ep = ec.facade_endpointing()
    with pytest.raises(ValueError, match='beam= together with endpoint='):
        m.stream(beam=sb.StreamBeam(width=4), endpoint=ep)
    with pytest.raises(ValueError, match='beam= together with endpoint=.*StreamBeam\\(endpoint='):
        m.stream(beam=sb.StreamBeam(width=4), endpoint=ep)
    with pytest.raises(ValueError, match='beam= together with endpoint='):
        m.stream(beam=sb.StreamBeam(width=4, endpoint=ep), endpoint=ep)
    with pytest.raises(ValueError, match='endpoint: .*silence_s'):
        m.stream(beam=sb.StreamBeam(endpoint=se.Endpointing(silence_s=0.0)))
    with pytest.raises(ValueError, match='Endpointing'):
        m.stream(beam=sb.StreamBeam(endpoint=0.8))
    beam = sb.StreamBeam(width=4, n_best=2, cutoff_top_n=20, lag_s=0.1, endpoint=ep)
    sess = m.stream(max_streams=1, beam=beam, **KW)                              # a stream without a sample: the empty END utterance
    s = sess.open()
    h = sess.close(s)
    utts = sess.take_utterances()
    assert sess.steps == 0 and [x.text for x in h] == [''] and h[0].utt_score == 0.0
    assert len(utts) == 1 and utts[0].reason == 'end' and utts[0].index == 0 and utts[0].n_best == h and utts[0].hypothesis is h[0]
    sess.close_all()
    # input_rate=: PCM at 8 kHz through the per-stream resampler in front of the ring; the session equals the session at the
    # model's rate fed the offline resampler's output
    audio, lens = sc.facade_audio()[:, :40000], [16000, 40000]
    rate = 8000
    plan8 = qr.ResamplePlan(rate, 16000, m.resample_quality)
    x8 = np.stack([a[::2] for a in audio]).astype(np.float32)
    lens8 = [n // 2 for n in lens]
    y, yl = qr.resample_host(x8, lens8, plan8, 1)
    want, _, _, _ = cases.play_beam_ep_session(m, np.asarray(y, np.float32), [int(v) for v in yl], 15360, beam, **KW)
    got, _, _, _ = cases.play_beam_ep_session(m, x8, lens8, 3001, beam, input_rate=rate, **KW)
    assert got == want and len(got[0]) >= 2 and len(got[1]) > 2


def test_stream_beam_endpoint_is_an_argument_that_repr_and_eq_see():
    ep = se.Endpointing(silence_s=0.5)
    a = sb.StreamBeam(4, 1, 20, None, 0.0, 0.0, 1.0, None, 1.0, ep)              # the last positional argument
    assert a.endpoint is ep and a == sb.StreamBeam(width=4, cutoff_top_n=20, lag_s=1.0, endpoint=se.Endpointing(silence_s=0.5))
    assert a != sb.StreamBeam(width=4, cutoff_top_n=20, lag_s=1.0) and a != sb.StreamBeam(width=4, cutoff_top_n=20, lag_s=1.0, endpoint=se.Endpointing())
    assert 'endpoint=Endpointing(silence_s=0.5' in repr(a) and repr(sb.StreamBeam()).endswith('endpoint=None)')
    assert sb.StreamBeam().endpoint is None and sb.StreamBeam() == sb.StreamBeam()
    # dataclasses.replace rebuilds from the fields: the endpointing has to be passed along (the class docstring says so)
    assert dataclasses.replace(a, lag_s=2.0).endpoint is None and dataclasses.replace(a, lag_s=2.0, endpoint=a.endpoint).endpoint is ep
    with pytest.raises(TypeError):
        sb.StreamBeam(4, 1, 20, None, 0.0, 0.0, 1.0, None, 1.0, ep, 7)
    with pytest.raises(TypeError):
        sb.StreamBeam(4, 1, 20, None, 0.0, 0.0, 1.0, None, 1.0, ep, endpoint=ep)
