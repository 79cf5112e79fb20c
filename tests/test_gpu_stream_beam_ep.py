"""k_stream_beam_ep<LM, BOOST> on an MI355X against its NumPy twin (qasr.stream_beam.step_batch_ep_host), every byte after every
step, the beam block and its ring included: the four instantiations over streams of 500 frames in two slots whose records
come from the endpoint rule (dense and long rules) and from hand-made lists; with a lag beyond every utterance against
qasr_ctc_beam[_lm|_boost] per utterance; a beam that dies and lives again behind the next cut; every status; one captured
chain of top-N, emit, endpoint and this kernel replayed on new data; and the refusals of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_beam_ep_cases as cases  # noqa: E402
import stream_beam_refusal_cases as refusals  # noqa: E402
import stream_cases as sc  # noqa: E402
from qasr import beam as qb  # noqa: E402
from qasr import stream as st  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402
from qasr import stream_ep as se  # noqa: E402

FIELDS = ('labels', 'frames', 'n_new_labels', 'commit_len', 'n_live', 'status', 'tail_labels', 'tail_n', 'n_cuts', 'cut_n_hyps',
          'cut_delta_end', 'cut_labels', 'cut_n_labels', 'cut_score', 'cut_lm_score', 'cut_boost_score')
PLAN = (95, 5, 1)                                                              # Tw = 102: steps of up to 95 final frames


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _i32(x):
    return torch.tensor(np.asarray(x).tolist(), dtype=torch.int32).cuda()


def _same(got, want, what=''):
    for name in FIELDS:
        w = getattr(want, name)
        if w is None:
            assert getattr(got, name) is None, (what, name)
            continue
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g, w)


def _window(cid, cq, first, Tw):
    wid = np.full((Tw, cid.shape[1]), -1, np.int32)
    wq = np.full((Tw, cid.shape[1]), qb.EMPTY_Q, np.int32)
    n = max(0, min(Tw, cid.shape[0] - first))
    wid[:n], wq[:n] = cid[first:first + n], cq[first:first + n]
    return wid, wq


class Rig:
    """the kernel and the twin side by side: the same stream blocks (frames_done as emit left it), the same beam blocks, the
    same records, one launch per step, everything compared"""

    def __init__(self, bplan, S, blank, E, sets=None, lm=None, alpha=0.0, beta=0.0):
        from qasr import engine
        self.splan, self.bplan, self.S, self.blank, self.E = sc.plan_frames(*PLAN), bplan, S, blank, E
        self.sets, self.lm, self.alpha, self.beta = sets, lm, alpha, beta
        self.ts, self.tb = st.StreamState(S, self.splan), sb.StreamBeamState(S, bplan)
        self.ds = engine.stream_state(S, self.splan, 'cuda')
        self.db = (engine.stream_beam_boost_state if bplan.boost else engine.stream_beam_state)(S, bplan, 'cuda')
        assert self.db.numel() * 4 == sb.state_bytes(S, bplan.W, bplan.F, bplan.boost)

    def block(self):
        from qasr import engine
        return engine.stream_beam_block(self.db, self.S, self.bplan).cpu().numpy()

    def step(self, slots, flags, wins, enc, first, hi, recs, bset=None, ep_status=None, what=''):
        """hi: the stream block's frames_done of every row as emit left it; recs: per row (int32 [E][10], n)"""
        from qasr import engine
        B = len(slots)
        for s, h in zip(slots, hi):
            if 0 <= s < self.S:
                self.ts.block[s, 0:2].view(np.int64)[0] = 10 ** 9
                self.ts.block[s, 2] = h
        engine.stream_block(self.ds, self.S).copy_(_cuda(self.ts.block))
        wid, wq = np.stack([w[0] for w in wins]), np.stack([w[1] for w in wins])
        rec, nrec = np.stack([r[0] for r in recs]), np.array([r[1] for r in recs], np.int32)
        eps = np.zeros(B, np.int32) if ep_status is None else np.asarray(ep_status, np.int32)
        bset = ([-1] * B if bset is None else bset) if self.sets is not None else None
        want = sb.step_batch_ep_host(self.tb, self.ts, slots, flags, wid, wq, enc, first, rec, nrec, eps, self.blank, self.lm,
                                     self.alpha, self.beta, boost=self.sets, boost_set=bset)
        out = engine.stream_beam_ep_buffers(B, self.bplan, self.E, 'cuda', self.lm is not None)
        for n in FIELDS:                                                       # every output is written, tails included
            if getattr(out, n) is not None:
                getattr(out, n).fill_(-77)
        ep = se.EpStepBatch(_cuda(rec), _cuda(nrec), _cuda(eps))
        got = engine.stream_beam_ep(self.ds, self.db, self.S, self.splan, self.bplan, _i32(slots), _i32(flags), _cuda(wid), _cuda(wq),
                                    _i32(enc), _i32(first), self.blank, ep, self.sets, None if bset is None else _i32(bset), self.lm,
                                    self.alpha, self.beta, out=out)
        torch.cuda.synchronize()
        _same(got, want, what)
        assert self.block().tobytes() == self.tb.block.tobytes(), what
        assert engine.stream_block(self.ds, self.S).cpu().numpy().tobytes() == self.ts.block.tobytes(), what      # read-only
        return want


def _mode(mode, seeds, T):
    name, model, alpha, beta, boosted = mode
    lps = [cases.stream_of(mode, s, T) for s in seeds]
    blank = lps[0].shape[1] - 1
    sets = cases.sets_of(lps, blank)[0] if boosted else None
    return lps, blank, cases.lm_of(model), alpha, beta, sets


def _play(rig, cands, lens, edges, recs, slots, set_of, per_step=None):
    """rows side by side through their own step schedules; returns per row dict(labels, frames, cuts, cut_delta_end)"""
    nrow = len(slots)
    got = [dict(labels=[], frames=[], cuts=[], cde=[]) for _ in range(nrow)]
    for k in range(max(len(e) for e in edges) - 1):
        rows = [b for b in range(nrow) if k < len(edges[b]) - 1]
        sl, fl, wins, enc, first, hi, rr = [], [], [], [], [], [], []
        for b in rows:
            lo, h = edges[b][k], edges[b][k + 1]
            f = max(0, lo - (k % 6))
            last = k == len(edges[b]) - 2
            sl.append(slots[b]), fl.append((st.BEGIN if k == 0 else 0) | (st.END if last else 0)), first.append(f), enc.append(h - f)
            hi.append(h), wins.append(_window(*cands[b], f, rig.splan.Tw)), rr.append(cases.step_records(recs[b], lo, h, last, rig.E))
        o = rig.step(sl, fl, wins, enc, first, hi, rr, [set_of[b] if k == 0 else 99 - b for b in rows], what=(k, rows))
        for i, b in enumerate(rows):
            n = int(o.n_new_labels[i])
            assert o.status[i] == 0 and rig.tb.header(slots[b])[2] == edges[b][k + 1] and int(o.n_cuts[i]) == rr[i][1]
            g = got[b]
            g['cde'] += [len(g['labels']) + int(x) for x in o.cut_delta_end[i, :rr[i][1]]]
            g['labels'] += o.labels[i, :n].tolist()
            g['frames'] += o.frames[i, :n].tolist()
            for c in range(rr[i][1]):
                g['cuts'].append([(o.cut_labels[i, c, h, :o.cut_n_labels[i, c, h]].tolist(), int(o.cut_score[i, c, h]),
                                   0 if o.cut_lm_score is None else int(o.cut_lm_score[i, c, h])) +
                                  (() if o.cut_boost_score is None else (int(o.cut_boost_score[i, c, h]),))
                                  for h in range(int(o.cut_n_hyps[i, c]))])
            if per_step is not None:
                per_step(k, b, o, i)
    return got


@pytest.mark.parametrize('mode', cases.MODES, ids=[m[0] for m in cases.MODES])
@pytest.mark.parametrize('W,N,lag', cases.PARAMS)
def test_steps_with_rule_records_equal_the_twin(mode, W, N, lag):
    """two slots of S = 3 in permuted order; row 0 is cut under DENSE_RULES (many records in a step), row 1 under
    LONG_RULES (commit rounds inside utterances); the boosted modes mix set 0 / set 1 / no set over the parameters"""
    T = 500
    lps, blank, lm, alpha, beta, sets = _mode(mode, (100 + W + lag, 101 + W + lag), T)
    cands = [cases.cands_of(lp, N) for lp in lps]
    recs = [cases.rule_records(lps[0], blank, cases.DENSE_RULES), cases.rule_records(lps[1], blank, cases.LONG_RULES)]
    edges = [cases.edges_of(cases.cuts_of(s, T), T) for s in (cases.STEP_LENS_A, cases.STEP_LENS_B)]
    E = max(cases.max_step_records(r, e) for r, e in zip(recs, edges))
    nb = min(W, 3)
    bplan = sb.StreamBeamPlan(W, nb, N, lag, sc.plan_frames(*PLAN).max_final_frames, boost=sets is not None)
    assert bplan.slot_words == 16 + (24 if sets is not None else 20) * W + 2 * bplan.F * W
    rig = Rig(bplan, 3, blank, E, sets, lm, alpha, beta)
    set_of = [(0, 1), (1, -1)][(W + lag) % 2] if sets is not None else (-1, -1)
    got = _play(rig, cands, [T, T], edges, recs, [2, 0], set_of)
    conds = [cases.honest(r, e) for r, e in zip(recs, edges)]
    assert all(any(c[i] for c in conds) for i in range(3)), conds                # two records in a step, a cut inside a step, a cut on K
    for b in range(2):
        bs = sets[set_of[b]] if sets is not None and set_of[b] >= 0 else None
        whole = cases.run_steps_ep(*cands[b], T, [0, T], recs[b], blank, W, nb, lag, lm, alpha, beta, boost=bs, check=False)
        pad = (lambda c: [x + (0,) for x in c]) if sets is not None and bs is None else (lambda c: c)
        assert got[b]['labels'] == whole.labels and got[b]['frames'] == whole.frames and got[b]['cde'] == whole.cut_delta_end
        assert got[b]['cuts'] == [pad(c) for c in whole.cuts] and len(got[b]['cuts']) == len(recs[b])
        if b == 1:
            assert whole.commits_inside > 0                                      # a round committed inside an utterance that was cut later
        if W > 1 and N > 1:
            assert cases.distinct_strings(whole.cuts) >= 2
        assert rig.tb.block[[2, 0][b], 5] == len(recs[b])


@pytest.mark.parametrize('mode', cases.MODES, ids=[m[0] for m in cases.MODES])
def test_hand_made_records(mode):
    """a cut after every frame of a stretch, a cut at hi, cuts on K boundaries, two records with the same end, an END record on
    a row without frames, and BEGIN on a used slot"""
    W, N, lag, T = 16, 20, 7, 200
    lps, blank, lm, alpha, beta, sets = _mode(mode, (7, 8), T)
    cands = [cases.cands_of(lp, N) for lp in lps]
    ends = [[31, 32, 32, 64, 65, 66, 67, 68, 69, 70, 96, 150, 150, 150], [33, 128, 160, 160, 192]]
    recs = [cases.hand_records(e, T) for e in ends]
    edges = [[0, 31, 32, 64, 70, 96, 160, T], [0, 33, 128, 192, T, T]]          # row 1 ends with a step without frames: the END record's
    E = max(cases.max_step_records(r, e) for r, e in zip(recs, edges))
    bplan = sb.StreamBeamPlan(W, 3, N, lag, sc.plan_frames(*PLAN).max_final_frames, boost=sets is not None)
    rig = Rig(bplan, 2, blank, E, sets, lm, alpha, beta)
    set_of = (1, 0) if sets is not None else (-1, -1)
    got = _play(rig, cands, [T, T], edges, recs, [1, 0], set_of)
    assert [len(g['cuts']) for g in got] == [len(r) for r in recs]
    assert all(cases.honest(r, e) == (True, True, True) for r, e in zip(recs, edges))
    assert [x[0] for x in got[0]['cuts'][2]] == [[]] and got[0]['cde'][2] == got[0]['cde'][1]     # the second record at 32: a fresh beam
    cde = got[1]['cde']                                                                           # END on a row without frames:
    assert len(got[1]['cuts'][-1]) >= 1 and all(f >= 192 for f in got[1]['frames'][cde[-2]:cde[-1]])      # what the beam held since 192
    # BEGIN on a used slot: the stream starts over, the cut count too
    again = _play(rig, cands[:1], [T], [edges[0]], recs[:1], [1], set_of[:1])
    assert again[0] == got[0]


@pytest.mark.parametrize('mode', cases.MODES, ids=[m[0] for m in cases.MODES])
def test_a_lag_beyond_every_utterance_is_the_offline_search_per_utterance(mode):
    """the rows of every cut against qasr_ctc_beam[_lm|_boost] over the utterance's own candidates"""
    from qasr import engine
    W, N, T, nb = 16, 20, 300, 16
    lps, blank, lm, alpha, beta, sets = _mode(mode, (41, 42), T)
    cands = [cases.cands_of(lp, N) for lp in lps]
    recs = [cases.rule_records(lp, blank, cases.LONG_RULES) for lp in lps]
    edges = [cases.edges_of(cases.cuts_of(cases.STEP_LENS_B, T), T)] * 2
    E = max(cases.max_step_records(r, e) for r, e in zip(recs, edges))
    bplan = sb.StreamBeamPlan(W, nb, N, 100, sc.plan_frames(*PLAN).max_final_frames, boost=sets is not None)
    rig = Rig(bplan, 2, blank, E, sets, lm, alpha, beta)
    got = _play(rig, cands, [T, T], edges, recs, [1, 0], (1, 1))
    checked = 0
    for b in range(2):
        assert len(recs[b]) >= 3 and max(int(r[se.R_END]) - int(r[se.R_FIRST]) for r in recs[b]) <= 100
        for r, cut in zip(recs[b], got[b]['cuts']):
            first, end = int(r[se.R_FIRST]), int(r[se.R_END])
            if end == first:
                assert [x[0] for x in cut] == [[]]
                continue
            off = engine.ctc_beam(_cuda(cands[b][0][None, first:end]), _cuda(cands[b][1][None, first:end]), None, blank, W, nb, lm=lm,
                                  alpha=alpha, beta=beta, boost=sets[1] if sets is not None else None)
            torch.cuda.synchronize()
            n_lab, lab = off.n_labels.cpu().numpy()[0], off.labels.cpu().numpy()[0]
            assert len(cut) == int(off.n_hyps.cpu()[0]) >= 1
            for h, ent in enumerate(cut):
                assert ent[0] == lab[h, :n_lab[h]].tolist() and ent[1] == int(off.score.cpu()[0, h]), (b, first, end, h)
                assert lm is None or ent[2] == int(off.lm_score.cpu()[0, h])
                assert sets is None or ent[3] == int(off.boost_score.cpu()[0, h])
            checked += 1
    assert checked >= 4


def test_a_dead_beam_lives_again_behind_the_next_cut():
    W, N, T = 3, 20, 190
    mode = cases.MODES[0]
    lps, blank, lm, alpha, beta, sets = _mode(mode, (4, 5), T)
    cands = [tuple(x.copy() for x in cases.cands_of(lp, N)) for lp in lps]
    cands[0][0][50:60], cands[0][1][50:60] = -1, qb.EMPTY_Q                        # a stretch without a live candidate
    recs = [cases.hand_records([40, 80, 120], T), cases.hand_records([55, 56], T)]
    edges = [[0, 45, 52, 70, 95, T]] * 2
    bplan = sb.StreamBeamPlan(W, 2, N, 7, sc.plan_frames(*PLAN).max_final_frames)
    rig = Rig(bplan, 2, blank, 2)
    live = {}
    got = _play(rig, cands, [T, T], edges, recs, [0, 1], (-1, -1), per_step=lambda k, b, o, i: live.__setitem__((k, b), int(o.n_live[i])))
    assert [live[(k, 0)] for k in range(5)][1:3] == [0, 0] and live[(0, 0)] > 0 and live[(3, 0)] > 0 and live[(4, 0)] > 0
    assert got[0]['cuts'][1] == [] and len(got[0]['cuts'][0]) >= 1 and len(got[0]['cuts'][2]) >= 1
    cde = got[0]['cde']
    assert cde[2] > cde[1] and all(80 <= f < 120 for f in got[0]['frames'][cde[1]:cde[2]])      # the revived beam's utterance has text


def test_every_status_leaves_the_state_alone():
    W, N = 16, 20
    mode = cases.MODES[2]
    lps, blank, lm, alpha, beta, sets = _mode(mode, (61,), 102)
    c = cases.cands_of(lps[0], N)
    bplan = sb.StreamBeamPlan(W, 2, N, 7, sc.plan_frames(*PLAN).max_final_frames, boost=True)
    E = 3
    rig = Rig(bplan, 8, blank, E, sets)
    win = _window(*c, 0, rig.splan.Tw)
    rec = lambda ends, first_index=0, n=None: (np.stack([se._record(first_index + k, 0, e, 0, 0, 0, se.HARD, np.float32(0), 0) for k, e in enumerate(ends)] +  # noqa: E731
                                                         [np.zeros(10, np.int32)] * (E - len(ends))), len(ends) if n is None else n)
    o = rig.step(list(range(7)), [st.BEGIN] * 7, [win] * 7, [40] * 7, [0] * 7, [40] * 7, [rec([20])] * 7, [0, 1, -1, 0, 0, 0, 0], what='begin')
    assert o.status.tolist() == [0] * 7 and rig.tb.block[0, 5] == 1
    before = rig.tb.block.copy()
    rows = [
        (9, 0, 40, 0, 60, rec([50], 1), 0, 0),                   # no such slot
        (0, 0, 60, 41, 60, rec([50], 1), 0, 0),                  # the gap: lo < first_frame
        (1, 0, 60, 0, 39, rec([], 1), 0, 0),                     # lo > hi
        (2, 0, 50, 0, 60, rec([55], 1), 0, 0),                   # hi beyond first_frame + enc_len
        (3, 0, 60, 0, 60, rec([50, 55, 58], 1, 4), 0, 0),        # more records than E
        (4, 0, 60, 0, 60, rec([55, 50], 1), 0, 0),               # ends that fall
        (5, 0, 60, 0, 60, rec([40], 1), 0, 0),                   # end == lo on a row with frames
        (6, 0, 60, 0, 60, rec([61], 1), 0, 0),                   # an end beyond hi
    ]
    o = rig.step([r[0] for r in rows], [r[1] for r in rows], [win] * 8, [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows],
                 [r[5] for r in rows], [0] * 8, what='statuses 1')
    assert o.status.tolist() == [sb.STATUS_SLOT, sb.STATUS_GAP] + [sb.STATUS_SYNC] * 6 and rig.tb.block.tobytes() == before.tobytes()
    rows = [
        (0, 0, 60, 0, 60, rec([50], 0), 0, 0),                   # the record's index is not the block's cut count
        (1, 0, 60, 0, 60, rec([50], 1), 1, 0),                   # the endpoint step refused the row
        (2, st.BEGIN, 60, 0, 60, rec([50], 1), 0, 0),            # BEGIN counts cuts from 0
        (3, st.BEGIN, 60, 0, 60, rec([50], 0), 0, 2),            # a BEGIN row with a set that is none
        (4, 0, 60, 0, 60, rec([50], 1, -1), 0, 0),               # a negative record count
    ]
    o = rig.step([r[0] for r in rows], [r[1] for r in rows], [win] * 5, [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows],
                 [r[5] for r in rows], [r[7] for r in rows], ep_status=[r[6] for r in rows], what='statuses 2')
    assert o.status.tolist() == [sb.STATUS_SYNC] * 3 + [sb.STATUS_SET, sb.STATUS_SYNC] and rig.tb.block.tobytes() == before.tobytes()
    assert (o.labels == blank).all() and not o.n_cuts.any() and (o.cut_score == qb.NEG).all() and not o.cut_n_hyps.any()
    big = sb.StreamBeamPlan(128, 1, N, 7, sc.plan_frames(*PLAN).max_final_frames, boost=True)
    rig = Rig(big, 1, blank, E, sets)
    rig.tb.block[0, 2], rig.tb.block[0, 3] = 2 ** 24, 1
    from qasr import engine
    engine.stream_beam_block(rig.db, 1, big).copy_(_cuda(rig.tb.block))
    o = rig.step([0], [0], [win], [40], [2 ** 24], [2 ** 24 + 40], [rec([])], [0], what='node ids')
    assert o.status.tolist() == [sb.STATUS_NODES] and rig.tb.header(0)[2] == 2 ** 24


def test_capture_and_replay():
    """qasr_ctc_topn -> qasr_stream_emit -> qasr_stream_endpoint -> qasr_stream_beam_ep captured once as a chain on a side
    stream; three replays with nothing but device memory changing in between; outputs and all three states equal the twins'"""
    from qasr import engine
    splan = sc.plan_frames(32, 5, 1)
    eplan = se.EndpointPlan(splan, *cases.DENSE_RULES)
    W, N, S, B, slots = 16, 20, 3, 2, [2, 0]
    mode = cases.MODES[3]
    lm, alpha, beta = cases.lm_of('en3'), 0.7, 1.0
    Tw, E = splan.Tw, eplan.max_records
    lps = [cases.stream_of(mode, s, 200) for s in (81, 82)]
    Cn = lps[0].shape[1]
    blank = Cn - 1
    sets = cases.sets_of(lps, blank)[0]
    bplan = sb.StreamBeamPlan(W, 2, N, 7, splan.max_final_frames, boost=True)
    ts, tb, te = st.StreamState(S, splan), sb.StreamBeamState(S, bplan), se.EpState(S)
    ds, db, de = engine.stream_state(S, splan, 'cuda'), engine.stream_beam_boost_state(S, bplan, 'cuda'), engine.stream_ep_state(S, 'cuda')
    sl, fl, bset = _i32(slots), _i32([0] * B), _i32([1, 0])
    logp = torch.zeros(B, Tw, Cn, device='cuda')
    tok = torch.zeros(B, Tw, dtype=torch.int32, device='cuda')
    fs = torch.zeros(B, Tw, device='cuda')
    enc, first = _i32([Tw] * B), _i32([0] * B)
    cand = (torch.empty(B, Tw, N, dtype=torch.int32, device='cuda'), torch.empty(B, Tw, N, dtype=torch.int32, device='cuda'))
    bout = engine.stream_beam_ep_buffers(B, bplan, E, 'cuda', True)
    eout = engine.stream_emit_buffers(B, splan, 'cuda')
    pout = engine.stream_endpoint_buffers(B, eplan, 'cuda')
    engine.lae_table_device('cuda'), engine.lm_device(lm, 'cuda')               # uploads happen outside the capture
    blobs = [engine.boost_device(s, 'cuda') for s in sets]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.ctc_topn(logp, None, N, out=cand)
            engine.stream_emit(ds, S, splan, sl, fl, tok, fs, enc, first, blank, out=eout)
            engine.stream_endpoint(ds, de, S, splan, eplan, sl, fl, tok, fs, enc, first, eout, blank, out=pout)
            engine.stream_beam_ep(ds, db, S, splan, bplan, sl, fl, cand[0], cand[1], enc, first, blank, pout, sets, bset, lm, alpha, beta,
                                  out=bout, blobs=blobs)
    torch.cuda.synchronize()
    ds.zero_(), db.zero_(), de.zero_()
    spf = splan.samples_per_frame
    n_cuts = 0
    for k in range(3):
        r = (k + 1) * splan.C + (0 if k < 2 else 777)
        f = splan.window_of(r)[2]
        flags = [st.BEGIN if k == 0 else (st.END if k == 2 else 0)] * B
        x = np.zeros((B, Tw, Cn), np.float32)
        for b in range(B):
            x[b] = lps[b][f:f + Tw]
        for s in slots:
            ts.block[s, 0:2].view(np.int64)[0] = r
        engine.stream_block(ds, S)[:, 0:2].copy_(_cuda(ts.block[:, 0:2]))       # `received`, as k_stream_push leaves it
        t_np, f_np = x.argmax(2).astype(np.int32), x.max(2)
        e = [Tw, Tw - 1] if k < 2 else [min(Tw, r // spf + 1 - f)] * B
        logp.copy_(_cuda(x)), tok.copy_(_cuda(t_np)), fs.copy_(_cuda(f_np)), enc.copy_(_i32(e)), first.copy_(_i32([f] * B)), fl.copy_(_i32(flags))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        cid, cq = qb.topn_host(x, N)
        want_e = st.emit_batch_host(ts, slots, flags, t_np, f_np, e, [f] * B, blank)
        want_p = se.endpoint_batch_host(te, ts, slots, flags, t_np, f_np, e, [f] * B, want_e, blank, eplan)
        want_b = sb.step_batch_ep_host(tb, ts, slots, flags, cid, cq, e, [f] * B, want_p.records, want_p.n_records, want_p.status, blank,
                                       lm, alpha, beta, boost=sets, boost_set=[1, 0])
        _same(bout, want_b, k)
        assert want_b.status.tolist() == [0, 0] and want_e.status.tolist() == [0, 0] and want_p.status.tolist() == [0, 0]
        assert pout.records.cpu().numpy().tobytes() == want_p.records.tobytes()
        assert engine.stream_beam_block(db, S, bplan).cpu().numpy().tobytes() == tb.block.tobytes(), k
        assert engine.stream_block(ds, S).cpu().numpy().tobytes() == ts.block.tobytes(), k
        n_cuts += int(want_b.n_cuts.sum())
    assert n_cuts >= 4 and tb.header(2)[2] == ts.frames_done(2) > 2 * 32 and tb.block[2, 4] == 2 and tb.block[0, 4] == 1


def test_abi_refusals_leave_the_outputs_alone():
    from qasr import engine
    lib = engine.load_library()
    splan = sc.plan_frames(*PLAN)
    W, N, S, B, E = 16, 20, 3, 2, 3
    mode = cases.MODES[3]
    lm = cases.lm_of('en3')
    lp = cases.stream_of(mode, 91, splan.Tw)
    blank = lp.shape[1] - 1
    sets = cases.sets_of([lp], blank)[0]
    cid, cq = (_cuda(np.stack([x] * B)) for x in cases.cands_of(lp, N))
    sl, fl, enc, first, bset = _i32([0, 1]), _i32([0, 0]), _i32([40, 40]), _i32([0, 0]), _i32([0, 1])
    ep = se.EpStepBatch(torch.zeros(B, E, 10, dtype=torch.int32, device='cuda'), _i32([0, 0]), _i32([0, 0]))
    s = engine._stream_ptr()
    for boosted in (True, False):
        bplan = sb.StreamBeamPlan(W, 2, N, 7, splan.max_final_frames, boost=boosted)
        state = engine.stream_state(S, splan, 'cuda')
        bstate = (engine.stream_beam_boost_state if boosted else engine.stream_beam_state)(S, bplan, 'cuda')
        state.fill_(0x5a5a5a5a), bstate.fill_(0x5a5a5a5a)
        poison = (state.clone(), bstate.clone())
        out = engine.stream_beam_ep_buffers(B, bplan, E, 'cuda', True)
        outs = [getattr(out, n) for n in FIELDS if getattr(out, n) is not None]
        for t in outs:
            t.fill_(-9)

        def args(inner=None, mid=None, **kw):
            a = engine.stream_beam_ep_args(state, bstate, S, splan, bplan, sl, fl, cid, cq, enc, first, blank, ep, sets if boosted else None,
                                           bset if boosted else None, lm, 0.5, 0.5, out=out)
            for k, v in (inner or {}).items():
                setattr(a.boost.beam, k, v)
            for k, v in (mid or {}).items():
                if isinstance(v, tuple):
                    getattr(a.boost, k)[v[0]] = v[1]
                else:
                    setattr(a.boost, k, v)
            for k, v in kw.items():
                setattr(a, k, v)
            return a

        inner = refusals.step_mutations(splan, bplan, S, state, bstate, engine.lm_device(lm, 'cuda').data_ptr(), blank, ends=False)
        assert len(inner) == 42 + 17
        mid = [dict(struct_size=8), dict(n_sets=9), dict(n_sets=-1)]
        if boosted:
            blob1 = engine.boost_device(sets[1], 'cuda')
            inner.append(dict(beam_state_bytes=lib.qasr_stream_beam_state_bytes(S, W, bplan.F)))
            mid += [dict(boost_set=None), dict(sets=(1, None)), dict(sets=(0, blob1.data_ptr() + 8)), dict(set_bytes=(1, 64)),
                    dict(set_bytes=(0, 1 << 31))]
        outer = [dict(struct_size=8), dict(E=0), dict(E=-1), dict(E=1 << 30), dict(cut_lm_score=None)] + \
            ([dict(cut_boost_score=None)] if boosted else []) + \
            [{n: None} for n in ('records', 'n_records', 'ep_status', 'n_cuts', 'cut_n_hyps', 'cut_delta_end', 'cut_labels', 'cut_n_labels',
                                 'cut_score')]
        for kw in inner:
            assert lib.qasr_stream_beam_ep(s, C.byref(args(kw))) == 1, kw            # QASR_ERR_ARG
            assert lib.qasr_last_error()
        for kw in mid:
            assert lib.qasr_stream_beam_ep(s, C.byref(args(None, kw))) == 1, kw
        for kw in outer:
            assert lib.qasr_stream_beam_ep(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_stream_beam_ep(s, None) == 1
        torch.cuda.synchronize()
        assert torch.equal(state, poison[0]) and torch.equal(bstate, poison[1])
        for t in outs:
            assert bool((t == -9).all())
        # the END outputs of the embedded struct are ignored: NULL there is no refusal (the slots hold poison: every row gets a status)
        a = args(dict(end_labels=None, end_n_labels=None, end_score=None, n_hyps=None, end_lm_score=None), dict(end_boost_score=None))
        assert lib.qasr_stream_beam_ep(s, C.byref(a)) == 0
        torch.cuda.synchronize()
        assert torch.equal(bstate, poison[1]) and bool((out.status != 0).all())
