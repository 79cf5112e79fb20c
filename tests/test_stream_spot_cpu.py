"""qasr.stream_spot, the host statement of streaming keyword spotting (no GPU): the slicing invariant - the hits of any sequence
of steps equal spot_host over the concatenated final frames on every byte -, that the early close never changes the list, the
detection delay, the pending hits, the derived hit pitch, planted keywords across a step boundary, the statuses, the façade's
refusals and the session on CPU tensors against the host composition."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spot_cases  # noqa: E402
import stream_cases as sc  # noqa: E402
import stream_spot_cases as pc  # noqa: E402
from qasr import align, beam, spot, stream as st, stream_spot as ss  # noqa: E402


def _case(name, C, ML, K, plan_name, threshold, max_span, seed=0):
    rng = np.random.default_rng([seed, C, ML, K])
    plan = pc.plan_of(plan_name)
    blank = C - 1
    tg, tl, bad = pc.keyword_set(rng, C, blank, ML, K)
    splan = ss.StreamSpotPlan(plan, tg, tl, spot.check_threshold(threshold, name), max_span)
    return rng, plan, blank, splan, bad


def _lens(plan):
    """three streams: END at three places of a chunk (its first sample, its middle, its last sample)"""
    return [2 * plan.C + 1, 3 * plan.C + plan.C // 2, 4 * plan.C]


CPU_CASES = [c for c in pc.KERNEL_CASES if c[1] != 5207] + [('c5207_ml31_k5', 5207, 31, 5, 'small', -8.0, 12)]


@pytest.mark.parametrize('case', CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_any_slicing_equals_spot_host_over_the_final_frames(case):
    rng, plan, blank, splan, bad = _case(*case)
    C = case[1]
    n = _lens(plan)
    lp_all = [pc.whole_logp(rng, pc.frames_for(plan, x), C, blank, odd=(i == 1)) for i, x in enumerate(n)]
    rows_seen = []

    def step(d, state, spstate):
        o = ss.spot_batch_host(spstate, state, d.slots, d.flags, d.lp, d.star, d.enc, d.first, d.emit_status, blank, rows_out=rows_seen)
        assert int(o.status.max()) == 0
        return o

    steps, state, spstate = pc.play(plan, splan, 5, [3, 0, 4], n, lp_all, blank, step)
    hits = pc.check_slicing(steps, splan, 3, blank, bad)
    assert sum(len(h) for h in hits.values()) > 0
    for r in rows_seen:                                              # the derived pitch holds every hit of a step
        assert len(r.hits) <= 2 * (r.hi - r.lo) + 1 <= splan.hit_pitch
    # a second stream on a used slot (BEGIN): the same list as on a fresh state
    lp2 = [pc.whole_logp(rng, pc.frames_for(plan, n[0]), C, blank)]
    again, _, _ = pc.play(plan, splan, 5, [0], [n[0]], lp2, blank, step, state=state, spstate=spstate)
    fresh, _, _ = pc.play(plan, splan, 5, [0], [n[0]], lp2, blank, step)
    assert pc.check_slicing(again, splan, 1, blank, bad) == pc.check_slicing(fresh, splan, 1, blank, bad)
    for a, b in zip(again, fresh):
        pc.same_batch(a.out, b.out)


def test_the_early_close_never_changes_the_list_and_bounds_the_delay():
    """the sweep of the rule's argument: 60 random rows, 2 / 5 / 29 classes, 20 .. 400 frames, spans 3 .. 1000, thresholds -0.5 ..
    -16: spot_whole_host (one pass with the early close) against spot_host (which closes only at a candidate or the end)"""
    total, delays = 0, []
    for i in range(60):
        rng = np.random.default_rng([7, i])
        C = (2, 5, 29)[i % 3]
        T = int(rng.integers(20, 401))
        span = int((3, 10, 50, 1000)[int(rng.integers(0, 4))])
        thr = spot.check_threshold(float((-0.5, -2.0, -6.0, -16.0)[int(rng.integers(0, 4))]), 'sweep')
        blank = C - 1
        lp = spot_cases.logp(rng, 1, T, C, blank)
        star = align.star_host(lp, None, 0.0)
        tg, tl = spot_cases.keywords(rng, [1, 2, int(rng.integers(1, 6))], C, blank)
        want = spot.spot_host(lp, None, star, tg, tl, blank, thr, span, T)
        for k in range(3):
            got = ss.spot_whole_host(lp[0], star[0], tg[k, :tl[k]], blank, thr, span)
            n = int(want.n_hits[k])
            assert got.shape == (n, 4)
            assert got[:, 0].astype(np.int32).tobytes() == want.hit_start[k, :n].tobytes()
            assert got[:, 1].astype(np.int32).tobytes() == want.hit_end[k, :n].tobytes()
            assert got[:, 2].tobytes() == want.hit_score[k, :n].tobytes()
            total += n
            for s, e, _, det in got:
                assert det >= e
                if det < T - 1:                                      # closed by a frame, not by END
                    assert det - e < span
                    delays.append(int(det - e))
    assert total > 2000 and len(delays) > 1500


def test_pending_hits_overlap_the_next_final_hit_and_a_hit_stays_open_across_steps():
    rng, plan, blank, splan, bad = _case('pending', 29, 31, 5, 'small', -6.0, 40)
    n = [6 * plan.C + 3]
    lp_all = [pc.whole_logp(rng, pc.frames_for(plan, n[0]), 29, blank)]
    steps, _, _ = pc.play(plan, splan, 1, [0], n, lp_all, blank, lambda d, s, sp: pc.host_step(d, s, sp, blank))
    pc.check_slicing(steps, splan, 1, blank, bad)
    carried = 0
    for k in range(splan.K):
        pend = None
        for d in steps:
            fin = [(int(d.out.hit_start[k, j]), int(d.out.hit_end[k, j])) for j in range(int(d.out.n_new_hits[k]))]
            if pend is not None and fin:                             # the hit emitted next overlaps what was pending
                assert fin[0][0] <= pend[1] and pend[0] <= fin[0][1], (k, pend, fin)
                carried += 1
            pend = (int(d.out.open_start[k]), int(d.out.open_end[k])) if int(d.out.open_start[k]) >= 0 else (pend if not fin else None)
        assert int(steps[-1].out.open_start[k]) == -1               # END leaves nothing open
    assert carried > 0


@pytest.mark.parametrize('span', [1, 2, 3])
def test_the_hit_pitch_holds_the_densest_steps(span):
    rng, plan, blank, splan, bad = _case('dense', 5, 31, 5, 'wide', -16.0, span)
    assert splan.hit_pitch == 2 * plan.max_final_frames + 1 and plan.max_final_frames > 64
    n = [2 * plan.C + 5]
    lp_all = [pc.whole_logp(rng, pc.frames_for(plan, n[0]), 5, blank)]
    rows = []
    steps, _, _ = pc.play(plan, splan, 1, [0], n, lp_all, blank,
                          lambda d, s, sp: ss.spot_batch_host(sp, s, d.slots, d.flags, d.lp, d.star, d.enc, d.first, d.emit_status, blank,
                                                              rows_out=rows))
    pc.check_slicing(steps, splan, 1, blank, bad)                   # (asserts that no step lost a hit to the pitch)
    most = max(len(r.hits) / max(r.hi - r.lo, 1) for r in rows)
    assert all(len(r.hits) <= 2 * (r.hi - r.lo) + 1 for r in rows) and most >= (1.0 if span == 1 else 0.3)


def test_planted_keywords_across_a_step_boundary_are_found_with_their_spans():
    C, blank = 29, 28
    plan = pc.plan_of('small')
    y = [3, 7, 7, 11]
    tg, tl = spot_cases.pad([y], blank, 31)
    splan = ss.StreamSpotPlan(plan, tg, tl, spot.check_threshold(-0.5, 'planted'), 50)
    n = [8 * plan.C]
    T = pc.frames_for(plan, n[0])
    boundary = 3 * plan.chunk_frames                                 # a multiple of the chunk: steps end their final range here
    lp, spans = spot_cases.planted(y, [boundary - 4, boundary + 9], T, C, blank, frames_per_label=3)
    steps, _, _ = pc.play(plan, splan, 1, [0], n, [lp[0]], blank, lambda d, s, sp: pc.host_step(d, s, sp, blank), perturb=False)
    hits = pc.check_slicing(steps, splan, 1, blank)[0, 0]
    assert [(h[0], h[1]) for h in hits] == spans and all(h[2] == 0 for h in hits)
    cut = [d.hi[0] for d in steps]
    assert any(spans[0][0] < c <= spans[0][1] for c in cut)         # the first occurrence does span a step boundary


def test_statuses_and_invalid_keywords_leave_the_state_untouched():
    rng, plan, blank, splan, bad = _case('status', 29, 31, 5, 'small', -6.0, 40)
    n = [3 * plan.C]
    lp_all = [pc.whole_logp(rng, pc.frames_for(plan, n[0]), 29, blank)]
    seen = {}

    def step(d, state, spstate):
        if len(seen) == 0 and not d.end and spstate.block[2, 0, 1] and 0 < spstate.block[2, 0, 0] < d.hi[0]:
            before = spstate.block.copy()
            args = (d.lp, d.star, d.enc, d.first)
            o = ss.spot_batch_host(spstate, state, [7], d.flags, *args, d.emit_status, blank)                  # no such slot
            assert o.status.tolist() == [2] * splan.K and o.ok.tolist() == [0 if k in bad else 1 for k in range(splan.K)]
            o1 = ss.spot_batch_host(spstate, state, d.slots, d.flags, *args, [1], blank)                       # emit lost frames
            assert o1.status.tolist() == [1] * splan.K
            o3 = ss.spot_batch_host(spstate, state, d.slots, d.flags, *args, d.emit_status, blank, PH=3)
            # (that was a real step: undo it, then the three range refusals)
            spstate.block[:] = before
            want3 = [0 if k in bad else 3 for k in range(splan.K)]
            lo = int(before[2, 0, 0])
            o = ss.spot_batch_host(spstate, state, d.slots, d.flags, d.lp, d.star, d.enc, d.first + lo + 1, d.emit_status, blank)
            assert o.status.tolist() == want3                                                                 # lo < first_frame
            o = ss.spot_batch_host(spstate, state, d.slots, d.flags, d.lp, d.star, np.zeros_like(d.enc), d.first, d.emit_status, blank)
            assert o.status.tolist() == want3                                                                 # hi beyond first + enc_len
            state.block[2, st._W_DONE] -= d.hi[0] - lo + 1
            o = ss.spot_batch_host(spstate, state, d.slots, d.flags, *args, d.emit_status, blank)
            assert o.status.tolist() == want3                                                                 # lo > hi
            state.block[2, st._W_DONE] += d.hi[0] - lo + 1
            keep, splan.max_final_frames = splan.max_final_frames, d.hi[0] - lo - 1
            o = ss.spot_batch_host(spstate, state, d.slots, d.flags, *args, d.emit_status, blank)
            assert o.status.tolist() == want3                                                                 # more than a step walks
            splan.max_final_frames = keep
            for x in (o, o1):
                assert not x.n_new_hits.any() and not x.hit_start.any() and (x.open_start == -1).all() and not x.n_hits_total.any()
            assert spstate.block.tobytes() == before.tobytes()
            assert (o3.status == 0).all()
            seen['done'] = True
        o = pc.host_step(d, state, spstate, blank)
        for k in bad:                                                # an invalid keyword never writes its block
            assert not spstate.block[d.slots[0], k].any()
        return o

    steps, _, spstate = pc.play(plan, splan, 3, [2], n, lp_all, blank, step)
    assert seen and len(bad) == 2
    pc.check_slicing(steps, splan, 1, blank, bad)


def test_plan_and_state_layout():
    plan = pc.plan_of('small')
    for ML, NS in ((1, 1), (31, 1), (32, 2), (63, 2), (64, 4), (127, 4)):
        sp = ss.StreamSpotPlan(plan, np.zeros((3, ML), np.int32), np.ones(3, np.int32), -65536, 10)
        assert (sp.NS, sp.SP, sp.block_words) == (NS, 64 * NS, 8 + 192 * NS)
        assert ss.spot_state_bytes(5, 3, ML) == 5 * 3 * 4 * sp.block_words == ss.SpotState(5, sp).block.nbytes
    assert ss.spot_state_bytes(0, 3, 5) == ss.spot_state_bytes(1, 0, 5) == ss.spot_state_bytes(1, 1, 128) == ss.spot_state_bytes(1, 1, 0) == 0
    for bad_kw, name in ((dict(targets=np.zeros((1, 128), np.int32)), 'max_labels'), (dict(threshold_q=1), 'threshold_q'),
                         (dict(max_span=0), 'max_span'), (dict(targets=np.zeros((0, 4), np.int32), target_lens=np.zeros(0, np.int32)), 'targets')):
        kw = dict(targets=np.zeros((1, 4), np.int32), target_lens=np.ones(1, np.int32), threshold_q=-65536, max_span=10)
        kw.update(bad_kw)
        if 'target_lens' not in bad_kw:
            kw['target_lens'] = np.ones(kw['targets'].shape[0], np.int32)
        with pytest.raises(ValueError, match=name):
            ss.StreamSpotPlan(plan, **kw)


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
    sspot = pc.facade_spot()
    plan, steps, want = pc.compose_hits(m, audio, lens, sspot, **KW)
    assert all(len(want[i]) > 3 for i in want) and len({h[1][1] for i in want for h in want[i]}) > 1     # several keywords hit
    results = []
    for piece in (1000, 15360, 50000):
        slots, ups, hyps, got, pend, sess = pc.play_spot_session(m, audio, lens, piece, sspot, **KW)
        assert got == want
        sc.check_against_composition(m, slots, ups, hyps, steps, lens)                                 # updates and hypotheses unchanged
        results.append(got)
    assert results[0] == results[1] == results[2]
    assert any(p[s] for p in pend for s in p)                        # the provisional hits showed up
    plain = sc.play_session(m, audio, lens, 15360, **KW)[2]
    assert [dataclasses.astuple(h) for h in plain] == [dataclasses.astuple(h) for h in hyps]
    # offline, over the same final frames the hits are spot_host's: every streamed hit's (start, end, score) is in seconds here
    for i in want:
        for h in want[i]:
            assert h[2] >= h[1][3] - 1e-9 and h[1][2] < h[1][3]
    rows = m.decode_stream(torch.from_numpy(audio), torch.tensor(lens), spot=sspot, **KW)
    assert [dataclasses.astuple(h) for h in rows[0]] == [dataclasses.astuple(h) for h in plain]
    assert [[dataclasses.astuple(k) for k in row] for row in rows[1]] == [[h[1] for h in want[i]] for i in (0, 1)]
    assert m.decode_stream(torch.from_numpy(audio), torch.tensor(lens), **KW)[0].text == plain[0].text  # without spot: today's value


def test_session_refusals():
    from qasr.stream_beam import StreamBeam
    m = _model()
    with pytest.raises(ValueError, match='spot= together with beam='):
        m.stream(beam=StreamBeam(width=4), spot=pc.facade_spot())
    with pytest.raises(ValueError, match='StreamSpot'):
        m.stream(spot=['a'])
    with pytest.raises(ValueError, match='exactly one of keywords and labels'):
        m.stream(spot=ss.StreamSpot())
    with pytest.raises(ValueError, match='keyword list is empty'):
        m.stream(spot=ss.StreamSpot(labels=[]))
    with pytest.raises(ValueError, match='keyword 1 is empty'):
        m.stream(spot=ss.StreamSpot(labels=[[1], []]))
    with pytest.raises(ValueError, match='outside the vocabulary'):
        m.stream(spot=ss.StreamSpot(labels=[[10 ** 6]]))
    with pytest.raises(ValueError, match='at most 127'):
        m.stream(spot=ss.StreamSpot(labels=[[1] * 128]))
    with pytest.raises(ValueError, match='threshold'):
        m.stream(spot=ss.StreamSpot(labels=[[1]], threshold=0.5))
    with pytest.raises(ValueError, match='max_span_s'):
        m.stream(spot=ss.StreamSpot(labels=[[1]], max_span_s=0.0))
    sess = m.stream(max_streams=1, **KW)
    with pytest.raises(ValueError, match='spot='):
        sess.take_hits()
    with pytest.raises(ValueError, match='spot='):
        sess.pending_hits(0)
    sess.close_all()
    sess = m.stream(max_streams=1, spot=pc.facade_spot(), **KW)      # a stream that never received a sample: no hits
    s = sess.open()
    assert sess.pending_hits(s) == []
    h = sess.close(s)
    assert h.text == '' and sess.take_hits() == []
    sess.close_all()
