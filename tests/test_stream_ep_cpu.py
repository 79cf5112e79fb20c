"""qasr.stream_ep, the host statement of streaming endpointing (no GPU): the slicing invariant - the records of any sequence of
steps equal the whole-stream pass on every byte -, the content invariant - every utterance's score and labels are those of its
own frames -, HARD's attribution rule, the edge cases (each asserted to be hit), the plan's refusals and its derived record
bound, and the session on CPU tensors against the host composition."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_cases as sc  # noqa: E402
import stream_ep_cases as ec  # noqa: E402
from qasr import ctc, stream as st, stream_ep as se  # noqa: E402

BLANK = sc.BLANK


def _plays(rules, **kw):
    """every plan x four stream lengths (the END step falls at other places of the chunk) under one set of rule frames"""
    for pi, spec in enumerate(ec.PLANS):
        plan = ec.stream_plan(spec)
        eplan = se.EndpointPlan(plan, *rules)
        for n in (5 * plan.C + 7, 9 * plan.C + plan.C // 2 + 33, 14 * plan.C - 1, 3 * plan.Wl + 2 * plan.C + 321):
            rng = np.random.default_rng(1000 * pi + n)
            tok, fs = ec.whole_rows(rng, ec.frames_for(plan, n), **kw)
            yield plan, eplan, ec.play_ep(plan, eplan, n, tok, fs, perturb=not kw.get('no_hard'))[0]


@pytest.mark.parametrize('rules', ec.RULES)
def test_any_slicing_equals_the_whole_stream_pass(rules):
    """invariant 1, and the edges every play is expected to meet between them"""
    seen, on_last, on_first, per_step = set(), 0, 0, set()
    for plan, eplan, steps in _plays(rules, max_run=3):
        recs, row_t, row_f = ec.check_slicing(steps, plan, eplan)
        ec.check_content(recs, steps, row_t, row_f, collapse=False)
        seen |= set(ec.reasons(recs))
        for d in steps:
            ends = [int(r[se.R_END]) for r in d['ep'].records if int(r[se.R_REASON]) != se.UTT_END]
            on_last += d['step'].hi in ends and d['step'].hi > d['step'].lo      # an endpoint on the last final frame of a step
            on_first += d['step'].lo + 1 in ends                                 # ... and on the first of the next
            per_step.add(len(d['ep'].records))
            assert len(d['ep'].records) <= eplan.max_records
    assert on_last > 0 and on_first > 0
    assert {se.SILENCE, se.TIMEOUT, se.UTT_END} <= seen
    if rules == ec.DENSE_RULES:
        assert {2, 3} <= per_step and se.HARD in seen and se.MAX in seen         # two and three records in one step
    else:
        assert se.MAX in seen


def test_utterances_are_the_collapse_of_their_own_frames():
    """invariant 2 on streams where no HARD record fires: labels, starts, nframes and scores of every utterance are
    collapse_host of tokens[first:end] offset by first; every score is utt_score_host of frame_score[first:end]"""
    count = {r: 0 for r in se.REASONS}
    for plan, eplan, steps in _plays(ec.NO_HARD_RULES, no_hard=True, p_blank=0.5, max_run=1):
        recs, row_t, row_f = ec.check_slicing(steps, plan, eplan)
        ec.check_content(recs, steps, row_t, row_f, collapse=True)
        for r in ec.reasons(recs):
            count[r] += 1
    assert count[se.HARD] == 0
    assert count[se.SILENCE] > 20 and count[se.TIMEOUT] > 12 and count[se.MAX] > 0 and count[se.UTT_END] == 12


def test_timeout_repeats_through_a_long_blank_stretch():
    plan = ec.stream_plan(ec.PLANS[1])
    eplan = se.EndpointPlan(plan, *ec.NO_HARD_RULES)
    n = 16 * plan.C
    tok, fs = ec.whole_rows(np.random.default_rng(5), ec.frames_for(plan, n), no_hard=True)
    tok[30:40] = 1                                                               # speech right up to the stretch of 30 blanks
    steps, _, _ = ec.play_ep(plan, eplan, n, tok, fs, perturb=False)
    recs, _, _ = ec.check_slicing(steps, plan, eplan)
    inside = [r for r in recs if 40 < int(r[se.R_END]) <= 70]
    # SILENCE three blanks in (end 43), then a TIMEOUT every 7 frames: ends 50, 57, 64
    assert [(int(r[se.R_REASON]), int(r[se.R_END])) for r in inside] == [(se.SILENCE, 43), (se.TIMEOUT, 50), (se.TIMEOUT, 57), (se.TIMEOUT, 64)]
    for r in inside[1:]:
        assert (int(r[se.R_SP_FIRST]), int(r[se.R_SP_LAST]), int(r[se.R_SP_FRAMES])) == (-1, -1, 0)
        assert int(r[se.R_LABEL_END]) == int(inside[0][se.R_LABEL_END])           # no text


def test_hard_gives_a_spanning_run_to_the_next_utterance():
    """runs of up to 9 frames under Fmax = Fhard = 5: HARD cuts inside runs.  A label belongs to the utterance that holds the
    frame BEHIND its run's last frame (the END utterance when that is the stream's end)"""
    spanning = 0
    for spec in ec.PLANS[:2]:
        plan = ec.stream_plan(spec)
        eplan = se.EndpointPlan(plan, *ec.DENSE_RULES)
        n = 12 * plan.C + 17
        tok, fs = ec.whole_rows(np.random.default_rng(n), ec.frames_for(plan, n), p_blank=0.3, max_run=9)
        steps, _, _ = ec.play_ep(plan, eplan, n, tok, fs)
        recs, row_t, row_f = ec.check_slicing(steps, plan, eplan)
        ec.check_content(recs, steps, row_t, row_f, collapse=False)
        ref = ctc.collapse_host(row_t[None], blank=BLANK)
        owner_of = np.zeros(len(row_t) + 1, dtype=np.int64)
        for i, r in enumerate(recs):
            owner_of[int(r[se.R_FIRST]):int(r[se.R_END])] = i
        owner_of[len(row_t)] = len(recs) - 1
        base = 0
        for i, r in enumerate(recs):
            mine = [j for j in range(int(ref.n_labels[0])) if owner_of[int(ref.start[0, j] + ref.nframes[0, j])] == i]
            assert list(range(base, int(r[se.R_LABEL_END]))) == mine, (i, r)
            base = int(r[se.R_LABEL_END])
            spanning += sum(int(ref.start[0, j]) < int(r[se.R_FIRST]) for j in mine)
            if int(r[se.R_REASON]) == se.HARD and int(r[se.R_END]) < len(row_t) and row_t[int(r[se.R_END]) - 1] != BLANK:
                assert int(r[se.R_END]) - int(r[se.R_FIRST]) == 5
    assert spanning > 5


def _fresh(plan, S=2):
    return st.StreamState(S, plan), se.EpState(S)


def _one(plan, eplan, state, ep, slot, flags, tok, fs, enc, first=0):
    """emit + endpoint twins for one row; the stream has received enough for every encoded frame to be final on END"""
    s = st.emit_host(tok, fs, enc, first, state, slot, bool(flags & st.END), BLANK)
    return se.endpoint_host(ep, state, slot, flags, tok, fs, enc, first, s.start, s.nframes, s.n_new, s.status, BLANK, eplan)


def test_end_without_new_frames_and_on_a_stream_that_never_received_a_sample():
    plan = ec.stream_plan(ec.PLANS[0])
    eplan = se.EndpointPlan(plan, *ec.NO_HARD_RULES)
    state, ep = _fresh(plan)
    tok, fs = np.full(plan.Tw, BLANK, np.int32), np.zeros(plan.Tw, np.float32)
    r = _one(plan, eplan, state, ep, 1, st.BEGIN | st.END, tok, fs, 0)            # never a sample: nothing is final
    assert r.status == 0 and r.records.tobytes() == se._record(0, 0, 0, 0, 0, 0, se.UTT_END, np.float32(0), 0)[None].tobytes()
    tok[:5] = [1, 1, BLANK, 2, 2]
    fs[:5] = sc.SCORES[2:7]
    st.push_host(state, [0], [st.BEGIN], [4 * plan.C], np.zeros((1, 4 * plan.C), np.float32)[:, :plan.C])
    state.block[0, 0:2].view(np.int64)[0] = 5 * plan.samples_per_frame + plan.Rr  # five frames are final
    r = _one(plan, eplan, state, ep, 0, st.BEGIN, tok, fs, plan.Tw)
    assert r.status == 0 and len(r.records) == 0 and state.frames_done(0) == 5 and int(ep.block[0, 4]) == 5
    r = _one(plan, eplan, state, ep, 0, st.END, tok, fs, 0)                      # END with zero new frames
    assert r.status == 0 and len(r.records) == 1 and state.frames_done(0) == 5
    rec = r.records[0]
    assert rec[:7].tolist() == [0, 0, 5, 0, 4, 4, se.UTT_END] and int(rec[se.R_LABEL_END]) == 2 == state.n_labels(0)
    assert se.record_score(rec).tobytes() == np.float32(ctc.utt_score_host(fs[:5])).tobytes()
    assert ep.block[0, :7].tolist() == [5, 1, 5, 0, 0, 0, 2] and not ep.block[0, 7:].any()


def test_min_logp_compares_in_float32():
    plan = ec.stream_plan(ec.PLANS[1])
    tiny = np.float32(-1e-45)                                                    # the largest negative float32
    assert tiny < 0
    fs = np.array([0.0, -0.0, tiny, np.nan, -1.5, -1.5, -3.0, -0.25], dtype=np.float32)
    tok = np.array([1, 2, 1, 2, 1, BLANK, 2, 3], dtype=np.int32)
    for thr, want in ((-0.0, [1, 1, 0, 0, 0, 0, 0, 0]), (0.0, [1, 1, 0, 0, 0, 0, 0, 0]),       # -0.0 >= +0.0: the signs of zero compare equal
                      (-1.5, [1, 1, 1, 0, 1, 0, 0, 1]), (None, [1, 1, 1, 0, 1, 0, 1, 1]), (-np.inf, [1, 1, 1, 0, 1, 0, 1, 1])):
        eplan = se.EndpointPlan(plan, 100, 100, 100, 100, thr)
        state, ep = _fresh(plan)
        st.push_host(state, [0], [st.BEGIN], [plan.C], np.zeros((1, plan.C), np.float32))
        row_t, row_f = np.full(plan.Tw, BLANK, np.int32), np.zeros(plan.Tw, np.float32)
        row_t[:8], row_f[:8] = tok, fs
        r = _one(plan, eplan, state, ep, 0, st.BEGIN | st.END, row_t, row_f, 8)
        rec = r.records[0]
        idx = np.flatnonzero(want)
        assert (int(rec[se.R_SP_FIRST]), int(rec[se.R_SP_LAST]), int(rec[se.R_SP_FRAMES])) == (idx[0], idx[-1], len(idx)), thr
        whole = se.endpoints_whole_host(tok, fs, BLANK, eplan)
        assert whole.tobytes() == r.records.tobytes()
    # a NaN score is not speech even without a threshold, so SILENCE can fire on a non-blank frame
    eplan = se.EndpointPlan(plan, 1, 100, 100, 100)
    state, ep = _fresh(plan)
    st.push_host(state, [0], [st.BEGIN], [plan.C], np.zeros((1, plan.C), np.float32))
    row_t[:8], row_f[:8] = 1, [-1.0, -1.0, np.nan, -1.0, -1.0, -1.0, -1.0, -1.0]
    r = _one(plan, eplan, state, ep, 0, st.BEGIN | st.END, row_t, row_f, 8)
    assert [int(x[se.R_REASON]) for x in r.records] == [se.SILENCE, se.UTT_END] and int(r.records[0][se.R_END]) == 3
    assert [int(x[se.R_LABEL_END]) for x in r.records] == [0, 1]                 # the run spans the cut: it goes to the next utterance


def test_begin_on_a_used_slot_and_the_statuses_leave_the_state_alone():
    plan = ec.stream_plan(ec.PLANS[1])
    eplan = se.EndpointPlan(plan, *ec.NO_HARD_RULES)
    rng = np.random.default_rng(9)
    tok, fs = sc.token_row(rng, plan.Tw, 0.4, 2), sc.score_row(rng, plan.Tw)
    results = []
    for used in (False, True):
        state, ep = _fresh(plan)
        if used:
            ep.block[0] = rng.integers(1, 50, size=se.STATE_WORDS)
        st.push_host(state, [0], [st.BEGIN], [plan.C], np.zeros((1, plan.C), np.float32))
        state.block[0, 0:2].view(np.int64)[0] = 12 * plan.samples_per_frame + plan.Rr
        r = _one(plan, eplan, state, ep, 0, st.BEGIN, tok, fs, plan.Tw)
        results.append((r.status, r.records.tobytes(), ep.block[0].tobytes()))
    assert results[0] == results[1] and results[0][0] == 0
    # statuses: the state bytes do not change, no record is written - BEGIN rows included
    ep.block[1] = rng.integers(1, 50, size=se.STATE_WORDS)
    ep.block[1, 0] = 12
    before = ep.block.copy()
    emit = st.StepBatch(*[np.zeros((1, plan.emit_pitch), dt) for dt in (np.int32, np.int32, np.int32, np.float32)],
                        *[np.zeros(1, dt) for dt in (np.int32, np.int32, np.int32, np.float32)], None, None)
    call = lambda slot, flags, first, enc, status=0: se.endpoint_batch_host(
        ep, state, [slot], [flags], tok[None], fs[None], [enc], [first], dataclasses.replace(emit, status=np.array([status], np.int32)),
        BLANK, eplan)
    for flags in (0, st.BEGIN, st.END):
        o = call(0, flags, 0, plan.Tw, status=1)                                 # emit reported lost frames
        assert o.status.tolist() == [se.STATUS_GAP] and o.n_records.tolist() == [0] and not o.records.any()
        o = call(2, flags, 0, plan.Tw)                                           # no such slot
        assert o.status.tolist() == [se.STATUS_SLOT] and o.n_records.tolist() == [0]
        o = call(-1, flags, 0, plan.Tw)
        assert o.status.tolist() == [se.STATUS_SLOT]
    state.block[1, 2] = 11
    assert call(1, 0, 0, plan.Tw).status.tolist() == [se.STATUS_RANGE]           # lo = 12 > hi = 11
    state.block[1, 2] = 20
    assert call(1, st.END, 13, plan.Tw).status.tolist() == [se.STATUS_RANGE]     # lo = 12 < first_frame = 13
    assert call(1, st.BEGIN, 1, plan.Tw).status.tolist() == [se.STATUS_RANGE]    # BEGIN: lo = 0 < first_frame = 1
    assert call(1, 0, 12, 7).status.tolist() == [se.STATUS_RANGE]                # hi = 20 beyond first_frame + enc_len = 19
    assert call(1, 0, 12, 8).status.tolist() == [0]
    after = ep.block.copy()
    after[1] = before[1]
    assert after.tobytes() == before.tobytes() and ep.block[1, 0] == 20


def test_plan_refusals_and_the_walked_record_bound():
    plan = ec.stream_plan(ec.PLANS[1])
    E = se.Endpointing
    ok = se.EndpointPlan.for_stream(plan, E())
    assert (ok.Fsil, ok.Fstart, ok.Fmax, ok.Fhard) == (40, 250, 1500, 2000) and ok.min_logp == np.float32(-np.inf)
    assert ok.min_logp.dtype == np.float32
    for kw, name in ((dict(silence_s=float('nan')), 'silence_s'), (dict(start_timeout_s=float('inf')), 'start_timeout_s'),
                     (dict(max_utt_s=float('-inf')), 'max_utt_s'), (dict(hard_max_s=float('nan')), 'hard_max_s'),
                     (dict(silence_s=0.009), 'silence_s 0.009'), (dict(start_timeout_s=0.0), 'start_timeout_s 0.0'),
                     (dict(max_utt_s=-1.0), 'max_utt_s -1.0'), (dict(hard_max_s=29.0), 'hard_max_s 29.0'),
                     (dict(max_utt_s=400000.0, hard_max_s=400000.0), 'max_utt_s 400000.0'), (dict(hard_max_s=400000.0), 'hard_max_s 400000.0'),
                     (dict(silence_s=400000.0), 'silence_s 400000.0'), (dict(min_logp=float('nan')), 'min_logp')):
        with pytest.raises(ValueError, match=name):
            se.EndpointPlan.for_stream(plan, E(**kw))
    for frames, name in (((0, 1, 1, 1), 'Fsil 0'), ((1, 0, 1, 1), 'Fstart 0'), ((1, 1, 0, 1), 'Fmax 0'), ((1, 1, 5, 4), 'Fhard 4'),
                         ((1, 1, 1, 2 ** 24 + 1), 'Fhard')):
        with pytest.raises(ValueError, match=name):
            se.EndpointPlan(plan, *frames)
    assert se.EndpointPlan(plan, 2 ** 24, 2 ** 24, 2 ** 24, 2 ** 24).max_records == 2
    # E over the walked protocol: the walk's largest step (max_final_frames) with fires min_gap apart, and END
    for spec in ec.PLANS + [dict(shape=(70, 10, 2))]:
        p = ec.stream_plan(spec)
        for rules in ec.RULES + [(1, 1, 1, 1), (3, 7, 2, 16)]:
            ep = se.EndpointPlan(p, *rules)
            gap = min(rules[:3])
            assert ep.min_gap == gap and ep.max_records <= 1 + (p.max_final_frames - 1) // gap + 1
            assert ep.max_records <= p.max_final_frames // min(rules) + 2 and ep.max_records >= 1 + (p.chunk_frames - 1) // gap
    # all-blank frames under (1, 1, 1, 1): a record on every frame, the bound is met with equality
    p = ec.stream_plan(ec.PLANS[1])
    ep1 = se.EndpointPlan(p, 1, 1, 1, 1)
    n = 7 * p.C - 1                                                              # the END step that makes the most frames final
    steps, _, _ = ec.play_ep(p, ep1, n, np.full(ec.frames_for(p, n), BLANK, np.int32), np.zeros(ec.frames_for(p, n), np.float32), perturb=False)
    assert max(len(d['ep'].records) for d in steps) == ep1.max_records


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


def test_session_on_cpu_tensors_is_the_composition():
    torch.set_grad_enabled(False)
    m = _model()
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    ep = ec.facade_endpointing()
    plan, want = ec.compose_utterances(m, audio, lens, ep, **KW)
    assert all(len(want[i]) > 3 for i in want) and any(u[2] in ('hard', 'silence') for u in want[1])

    def after_push(sess, new):
        for s, stt in sess._open.items():
            held = sum(len(d[0]) for d in stt['deltas'])
            assert held <= sess.eplan.Fhard + sess.plan.max_final_frames         # bounded by one utterance (and one step)

    def wrap(sess):
        cut = sess._cut

        def checked(slot, records=None):
            n = len(sess._utts)
            hyp = cut(slot, records)
            if len(sess._utts) > n and sess._utts[-1].reason != 'hard':          # deltas are empty after each cut that is not HARD
                assert sess._open[slot]['deltas'] == []
                cuts.append(slot)
            return hyp
        sess._cut = checked

    cuts = []
    results = []
    for piece in (1000, 15360, 50000):
        got, hyps, _ = ec.play_ep_session(m, audio, lens, piece, ep, after_push=after_push, wrap=wrap, **KW)
        assert got == want
        for i, h in zip((0, 1), hyps):                                           # close() returns the END utterance's Hypothesis
            assert want[i][-1][2] == 'end' and dataclasses.astuple(h) == want[i][-1][7]
        results.append(got)
    assert results[0] == results[1] == results[2] and len(cuts) > 9
    # the whole stream's text is the utterances' texts in order: nothing is lost or doubled at a cut
    plain = sc.play_session(m, audio, lens, 15360, **KW)[2]
    for i in (0, 1):
        assert ''.join(u[7][0] for u in want[i]) == plain[i].text
        assert [x for u in want[i] for x in u[7][1]] == plain[i].labels
    rows = m.decode_stream(torch.from_numpy(audio), torch.tensor(lens), endpoint=ep, **KW)
    assert [[dataclasses.astuple(dataclasses.replace(u, slot=i)) for u in row] for i, row in enumerate(rows)] == [want[0], want[1]]


def test_session_refusals_and_a_stream_without_a_sample():
    from qasr.stream_beam import StreamBeam
    m = _model()
    with pytest.raises(ValueError, match='beam= together with endpoint='):
        m.stream(beam=StreamBeam(width=4), endpoint=se.Endpointing())
    with pytest.raises(ValueError, match='endpoint: .*silence_s'):
        m.stream(endpoint=se.Endpointing(silence_s=0.0))
    with pytest.raises(ValueError, match='Endpointing'):
        m.stream(endpoint=0.8)
    with pytest.raises(ValueError, match='endpoint='):
        m.stream(max_streams=1, **KW).take_utterances()
    sess = m.stream(max_streams=1, endpoint=se.Endpointing(), **KW)
    s = sess.open()
    h = sess.close(s)
    utts = sess.take_utterances()
    assert len(utts) == 1 and sess.take_utterances() == []
    u = utts[0]
    assert (u.slot, u.index, u.reason, u.start_s, u.end_s, u.speech_start_s, u.speech_end_s) == (s, 0, 'end', 0.0, 0.0, None, None)
    assert u.hypothesis is h and h.text == '' and h.utt_score == 0.0
    sess.close_all()
