"""k_stream_beam_boost<false> and <true> on an MI355X against their NumPy twin (qasr.stream_beam with boost=), every byte after
every step, the boosted beam block (bst, boost_tot, pad) and its ring included: rows that mix set 0, set 1 (whole words) and
no set, odd widths with several slots, permuted slots; with a lag beyond the stream against qasr_ctc_beam_boost on the same
candidates; a weight-0 set against qasr_stream_beam; every status, the new 5 included; one captured chain of top-N, boosted
beam and emit replayed on new data; and the refusals of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boost_cases  # noqa: E402
import stream_beam_cases as sbc  # noqa: E402
import stream_beam_refusal_cases as refusals  # noqa: E402
import stream_boost_cases as cases  # noqa: E402
import stream_cases as sc  # noqa: E402
from qasr import beam as qb  # noqa: E402
from qasr import stream as st  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402

FIELDS = ('labels', 'frames', 'n_new_labels', 'commit_len', 'n_live', 'status', 'tail_labels', 'tail_n', 'end_labels',
          'end_n_labels', 'end_score', 'end_lm_score', 'n_hyps', 'end_boost_score')
PLAN = (95, 5, 1)                                                              # Tw = 102: steps of up to 95 final frames
_lms = {}


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


def _lm(name):
    if name is not None and name not in _lms:
        _lms[name] = sbc.load_lm(sbc.GOLDEN, name)
    return _lms.get(name)


def _same(got, want, what='', fields=FIELDS):
    for name in fields:
        w = getattr(want, name)
        if w is None:
            continue
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g, w)


def _cands(lp, N):
    cid, cq = qb.topn_host(lp[None], N)
    return cid[0], cq[0]


def _window(cid, cq, first, Tw):
    wid = np.full((Tw, cid.shape[1]), -1, np.int32)
    wq = np.full((Tw, cid.shape[1]), qb.EMPTY_Q, np.int32)
    n = max(0, min(Tw, cid.shape[0] - first))
    wid[:n], wq[:n] = cid[first:first + n], cq[first:first + n]
    return wid, wq


def _sets(lps, blank):
    """two sets over the streams' own text: set 0 plain (NESTED and pieces of the greedy text), set 1 whole words where the
    vocabulary has a space (boost_cases.gpu_phrases: words of the greedy text, and a pair of them)"""
    space = boost_cases.EN_SPACE if blank == 28 else -1
    p0 = cases.phrases_of('nested_plain', 1, lps[0], blank, space)[0] + cases.phrases_of('random', 2, lps[0], blank, -1)[0]
    rng = np.random.Generator(np.random.PCG64(3))
    p1 = boost_cases.gpu_phrases(rng, np.stack(lps), None, blank, space >= 0, space)
    return [cases.make_set(p0, False, blank, space), cases.make_set(p1, space >= 0, blank, space)]


class Rig:
    """the kernel and the twin side by side, as test_gpu_stream_beam's: the same stream blocks, the same boosted beam blocks,
    one launch per step, everything compared"""

    def __init__(self, bplan, S, blank, sets, lm=None, alpha=0.0, beta=0.0):
        from qasr import engine
        self.splan, self.bplan, self.S, self.blank, self.lm, self.alpha, self.beta = sc.plan_frames(*PLAN), bplan, S, blank, lm, alpha, beta
        self.sets = sets
        self.ts, self.tb = st.StreamState(S, self.splan), sb.StreamBeamState(S, bplan)
        self.ds, self.db = engine.stream_state(S, self.splan, 'cuda'), engine.stream_beam_boost_state(S, bplan, 'cuda')
        assert self.db.numel() * 4 == sb.state_bytes(S, bplan.W, bplan.F, True)
        for s in range(S):
            self.stream(s, 10 ** 9, 0)

    def stream(self, slot, received, done):
        self.ts.block[slot, 0:2].view(np.int64)[0] = received
        self.ts.block[slot, 2] = done

    def block(self):
        from qasr import engine
        return engine.stream_beam_block(self.db, self.S, self.bplan).cpu().numpy()

    def step(self, slots, flags, wins, enc, first, bset, what='', advance=True):
        from qasr import engine
        engine.stream_block(self.ds, self.S).copy_(_cuda(self.ts.block))
        wid, wq = np.stack([w[0] for w in wins]), np.stack([w[1] for w in wins])
        want = sb.step_batch_host(self.tb, self.ts, slots, flags, wid, wq, enc, first, self.blank, self.lm, self.alpha, self.beta,
                                  boost=self.sets, boost_set=bset)
        out = engine.stream_beam_boost_buffers(len(slots), self.bplan, 'cuda', self.lm is not None)
        for n in FIELDS:                                                       # every output is written, tails included
            if getattr(out, n) is not None:
                getattr(out, n).fill_(-77)
        got = engine.stream_beam_boost(self.ds, self.db, self.S, self.splan, self.bplan, _i32(slots), _i32(flags), _cuda(wid),
                                       _cuda(wq), _i32(enc), _i32(first), self.blank, self.sets, _i32(bset), self.lm, self.alpha,
                                       self.beta, out=out)
        torch.cuda.synchronize()
        _same(got, want, what)
        assert self.block().tobytes() == self.tb.block.tobytes(), what
        assert engine.stream_block(self.ds, self.S).cpu().numpy().tobytes() == self.ts.block.tobytes(), what      # read-only
        if advance:
            for b, s in enumerate(slots):
                if want.status[b] == 0:
                    self.ts.block[s, 2] = self.tb.header(s)[2]
        return want


MODES = (('none', None, 0.0, 0.0), ('en3', 'en3', 0.7, 1.0), ('zh2', 'zh2', 1.5, 0.5))


def _streams(mode, seeds, T):
    what, model, alpha, beta = mode
    if model is None:
        return [sbc.stream_logp(s, T) for s in seeds], None, 0.0, 0.0
    return [sbc.lm_stream_logp(model, s, T) for s in seeds], _lm(model), alpha, beta


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('W,N,lag', [(1, 20, 7), (3, 64, 0), (16, 20, 40), (16, 1, 7), (128, 20, 40), (16, 20, 400)])
def test_steps_and_whole_streams_equal_the_twin(mode, W, N, lag):
    """S = 5 slots, 3 rows in permuted slot order (set 0, set 1 - whole words where the vocabulary has a space -, no set),
    streams of 300 / 260 / 200 frames (W = 128: 200 / 160 / 120) cut by two schedules; W = 3 with S = 5 puts every other
    slot's block at an odd multiple of 4 bytes were it not for the pad"""
    T = 200 if W == 128 else 300
    lens = [T, T - 40, T - 100]
    lps, lm, alpha, beta = _streams(mode, (11 + W, 12 + lag, 13 + N), T)
    blank = lps[0].shape[1] - 1
    cands = [_cands(lp[:n], N) for lp, n in zip(lps, lens)]
    nb = min(W, 3)
    sets = _sets(lps, blank)
    bplan = sb.StreamBeamPlan(W, nb, N, lag, sc.plan_frames(*PLAN).max_final_frames, boost=True)
    assert bplan.slot_words == 16 + 24 * W + 2 * bplan.F * W and (bplan.slot_words * 4) % 8 == 0
    rig = Rig(bplan, 5, blank, sets, lm, alpha, beta)
    slots, set_of = [3, 0, 4], [0, 1, -1]
    edges = [sbc.edges_of(sbc.cuts_of(sl, n), n) for sl, n in zip((sbc.STEP_LENS_A, sbc.STEP_LENS_B, sbc.STEP_LENS_A), lens)]
    got = [dict(labels=[], frames=[], end=None) for _ in slots]
    for k in range(max(len(e) for e in edges) - 1):
        rows = [b for b in range(3) if k < len(edges[b]) - 1]
        sl, fl, wins, enc, first = [], [], [], [], []
        for b in rows:
            lo, hi = edges[b][k], edges[b][k + 1]
            f = max(0, lo - (k % 6))
            last = k == len(edges[b]) - 2
            sl.append(slots[b]), fl.append((st.BEGIN if k == 0 else 0) | (st.END if last else 0)), first.append(f), enc.append(hi - f)
            wins.append(_window(*cands[b], f, rig.splan.Tw))
        # the input is read on BEGIN rows only: later steps pass garbage
        o = rig.step(sl, fl, wins, enc, first, [set_of[b] if k == 0 else 99 - b for b in rows], (k, rows))
        for i, b in enumerate(rows):
            n = int(o.n_new_labels[i])
            assert o.status[i] == 0 and rig.tb.header(slots[b])[2] == edges[b][k + 1] and rig.tb.block[slots[b], 4] == set_of[b] + 1
            got[b]['labels'] += o.labels[i, :n].tolist()
            got[b]['frames'] += o.frames[i, :n].tolist()
            if fl[i] & st.END:
                got[b]['end'] = [(o.end_labels[i, h, :o.end_n_labels[i, h]].tolist(), int(o.end_score[i, h]),
                                  0 if lm is None else int(o.end_lm_score[i, h]), int(o.end_boost_score[i, h]))
                                 for h in range(int(o.n_hyps[i]))]
                got[b]['commit'] = int(o.commit_len[i])
    for b in range(3):
        bs = sets[set_of[b]] if set_of[b] >= 0 else None
        whole = sb.lagged_search_host(*cands[b], lens[b], blank, W, nb, lm, alpha, beta, lag=lag, check=False, boost=bs)
        assert got[b]['labels'] == whole.labels and got[b]['frames'] == whole.frames and got[b]['commit'] == len(whole.labels)
        head = whole.labels[:whole.commit_len_before_end]
        want = [tuple(x) + ((0,) if bs is None else ()) for x in whole.hyps]
        assert [(head + x[0],) + x[1:] for x in got[b]['end']] == want, b
        if bs is not None:
            assert all(x[3] == bs.score(head + x[0]) for x in got[b]['end'])
    assert any(x[3] > 0 for b in (0, 1) for x in got[b]['end']) or N == 1      # the sets do match the streams' text


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
def test_a_lag_beyond_the_stream_is_qasr_ctc_beam_boost(mode):
    """the END rows of streams stepped with Lg >= their length against k_beam_boost over the same candidates"""
    from qasr import engine
    W, N, T, nb = 16, 20, 200, 16
    lps, lm, alpha, beta = _streams(mode, (41, 42), T)
    blank = lps[0].shape[1] - 1
    cands = [_cands(lp, N) for lp in lps]
    sets = _sets(lps, blank)
    bplan = sb.StreamBeamPlan(W, nb, N, T, sc.plan_frames(*PLAN).max_final_frames, boost=True)
    rig = Rig(bplan, 2, blank, sets, lm, alpha, beta)
    edges = sbc.edges_of(sbc.cuts_of(sbc.STEP_LENS_B, T), T)
    for k in range(len(edges) - 1):
        lo, hi = edges[k], edges[k + 1]
        fl = (st.BEGIN if k == 0 else 0) | (st.END if k == len(edges) - 2 else 0)
        o = rig.step([1, 0], [fl, fl], [_window(*c, lo, rig.splan.Tw) for c in cands], [hi - lo] * 2, [lo] * 2, [1, 1], k)
    off = engine.ctc_beam(_cuda(np.stack([c[0] for c in cands])), _cuda(np.stack([c[1] for c in cands])), None, blank, W, nb,
                          lm=lm, alpha=alpha, beta=beta, boost=sets[1])
    torch.cuda.synchronize()
    n_lab, lab = off.n_labels.cpu().numpy(), off.labels.cpu().numpy()
    assert o.n_hyps.tobytes() == off.n_hyps.cpu().numpy().tobytes() and o.end_n_labels.tobytes() == n_lab.tobytes()
    assert o.end_score.tobytes() == off.score.cpu().numpy().tobytes()
    assert o.end_boost_score.tobytes() == off.boost_score.cpu().numpy().tobytes() and o.end_boost_score.any()
    assert lm is None or o.end_lm_score.tobytes() == off.lm_score.cpu().numpy().tobytes()
    for b in range(2):
        for h in range(nb):
            assert o.end_labels[b, h, :n_lab[b, h]].tolist() == lab[b, h, :n_lab[b, h]].tolist()


@pytest.mark.parametrize('mode', [MODES[0], MODES[1]], ids=['none', 'en3'])
def test_a_weight_0_set_is_qasr_stream_beam(mode):
    """every byte that the boosted layout shares with k_stream_beam's: outputs and state, against the other KERNEL"""
    from qasr import engine
    W, N, T, lag, S = 3, 20, 190, 7, 2
    lps, lm, alpha, beta = _streams(mode, (55, 56), T)
    blank = lps[0].shape[1] - 1
    space = boost_cases.EN_SPACE
    cands = [_cands(lp, N) for lp in lps]
    ph, whole = cases.phrases_of('random', 4, lps[0], blank, space)
    zero = cases.make_set([(p, 0.0) for p, _ in ph], whole, blank, space)
    splan = sc.plan_frames(*PLAN)
    bp = sb.StreamBeamPlan(W, 2, N, lag, splan.max_final_frames, boost=True)
    pp = sb.StreamBeamPlan(W, 2, N, lag, splan.max_final_frames)
    rig = Rig(bp, S, blank, [zero], lm, alpha, beta)
    pstate = engine.stream_beam_state(S, pp, 'cuda')
    for k in range(2):
        lo, hi = 95 * k, 95 * (k + 1)
        fl = [(st.BEGIN if k == 0 else 0) | (st.END if k == 1 else 0)] * 2
        wins = [_window(*c, lo, splan.Tw) for c in cands]
        o = rig.step([1, 0], fl, wins, [95] * 2, [lo] * 2, [0, 0], k, advance=False)
        wid, wq = np.stack([w[0] for w in wins]), np.stack([w[1] for w in wins])
        p = engine.stream_beam(rig.ds, pstate, S, splan, pp, _i32([1, 0]), _i32(fl), _cuda(wid), _cuda(wq), _i32([95] * 2), _i32([lo] * 2),
                               blank, lm, alpha, beta)
        torch.cuda.synchronize()
        _same(p, o, k, FIELDS[:-1])
        assert not o.end_boost_score.any()
        b, q = rig.block(), engine.stream_beam_block(pstate, S, pp).cpu().numpy()
        hdr = sb.HDR_WORDS
        for s in range(S):
            ent = b[s, hdr:hdr + 24 * W]
            assert b[s, :4].tolist() == q[s, :4].tolist() and b[s, 4] == 1 and not b[s, 5:hdr].any() and not q[s, 4:hdr].any()
            assert ent[:16 * W].tobytes() == q[s, hdr:hdr + 16 * W].tobytes() and ent[18 * W:22 * W].tobytes() == q[s, hdr + 16 * W:hdr + 20 * W].tobytes()
            assert not ent[16 * W:18 * W].any() and not ent[23 * W:].any()
            assert b[s, hdr + 24 * W:].tobytes() == q[s, hdr + 20 * W:].tobytes()
        for s in range(S):
            rig.ts.block[s, 2] = rig.tb.header(s)[2]


def test_every_status_leaves_the_state_alone():
    W, N = 16, 20
    lp = sbc.stream_logp(61, 102)
    blank = lp.shape[1] - 1
    c = _cands(lp, N)
    sets = _sets([lp], blank)
    bplan = sb.StreamBeamPlan(W, 2, N, 7, sc.plan_frames(*PLAN).max_final_frames, boost=True)
    rig = Rig(bplan, 5, blank, sets)
    win = _window(*c, 0, rig.splan.Tw)
    rig.step([0, 1, 2, 3], [st.BEGIN] * 4, [win] * 4, [40] * 4, [0] * 4, [0, 1, -1, 0], 'begin')
    rig.stream(1, 10 ** 9, 41)                                                  # the stream block ran ahead of the beam block
    rig.stream(3, 10 ** 9, 0)                                                   # a stream that begins again, with a set that is none
    before = rig.tb.block.copy()
    o = rig.step([7, 0, 1, 2, 3], [0, 0, st.END, st.BEGIN, st.BEGIN], [win] * 5, [40, 40, 60, 60, 40], [0, 41, 0, 0, 0], [0, 0, 0, 0, 2],
                 'statuses', advance=False)
    assert o.status.tolist() == [sb.STATUS_SLOT, sb.STATUS_GAP, sb.STATUS_SYNC, sb.STATUS_SYNC, sb.STATUS_SET]
    assert rig.tb.block.tobytes() == before.tobytes()
    o = rig.step([3], [st.BEGIN], [win], [40], [0], [-2], 'below -1', advance=False)
    assert o.status.tolist() == [5] and rig.tb.block.tobytes() == before.tobytes()
    big = sb.StreamBeamPlan(128, 1, N, 7, sc.plan_frames(*PLAN).max_final_frames, boost=True)
    rig = Rig(big, 1, blank, sets)
    rig.stream(0, 10 ** 12, 2 ** 24)
    rig.tb.block[0, 2], rig.tb.block[0, 3] = 2 ** 24, 1
    from qasr import engine
    engine.stream_beam_block(rig.db, 1, big).copy_(_cuda(rig.tb.block))
    o = rig.step([0], [0], [win], [40], [2 ** 24], [0], 'node ids', advance=False)
    assert o.status.tolist() == [sb.STATUS_NODES] and rig.tb.header(0)[2] == 2 ** 24


def test_capture_and_replay():
    """qasr_ctc_topn -> qasr_stream_beam_boost -> qasr_stream_emit captured once as a chain on a side stream; three replays
    with nothing but device memory changing in between; outputs and both states equal the twins' after each"""
    from qasr import engine
    splan = sc.plan_frames(32, 5, 1)
    W, N, S, B, slots = 16, 20, 3, 2, [2, 0]
    lm, alpha, beta = _lm('en3'), 0.7, 1.0
    Tw = splan.Tw
    lps = [sbc.lm_stream_logp('en3', s, 200) for s in (81, 82)]
    Cn = lps[0].shape[1]
    blank = Cn - 1
    sets = _sets(lps, blank)
    bplan = sb.StreamBeamPlan(W, 2, N, 7, splan.max_final_frames, boost=True)
    ts, tb = st.StreamState(S, splan), sb.StreamBeamState(S, bplan)
    ds, db = engine.stream_state(S, splan, 'cuda'), engine.stream_beam_boost_state(S, bplan, 'cuda')
    sl, fl, bset = _i32(slots), _i32([0] * B), _i32([1, 0])
    logp = torch.zeros(B, Tw, Cn, device='cuda')
    tok = torch.zeros(B, Tw, dtype=torch.int32, device='cuda')
    fs = torch.zeros(B, Tw, device='cuda')
    enc, first = _i32([Tw] * B), _i32([0] * B)
    cand = (torch.empty(B, Tw, N, dtype=torch.int32, device='cuda'), torch.empty(B, Tw, N, dtype=torch.int32, device='cuda'))
    bout = engine.stream_beam_boost_buffers(B, bplan, 'cuda', True)
    eout = engine.stream_emit_buffers(B, splan, 'cuda')
    engine.lae_table_device('cuda'), engine.lm_device(lm, 'cuda')               # uploads happen outside the capture
    blobs = [engine.boost_device(s, 'cuda') for s in sets]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.ctc_topn(logp, None, N, out=cand)
            engine.stream_beam_boost(ds, db, S, splan, bplan, sl, fl, cand[0], cand[1], enc, first, blank, sets, bset, lm, alpha, beta,
                                     out=bout, blobs=blobs)
            engine.stream_emit(ds, S, splan, sl, fl, tok, fs, enc, first, blank, out=eout)
    torch.cuda.synchronize()
    ds.zero_(), db.zero_()
    spf = splan.samples_per_frame
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
        want_b = sb.step_batch_host(tb, ts, slots, flags, cid, cq, e, [f] * B, blank, lm, alpha, beta, boost=sets, boost_set=[1, 0])
        want_e = st.emit_batch_host(ts, slots, flags, t_np, f_np, e, [f] * B, blank)
        _same(bout, want_b, k)
        assert want_b.status.tolist() == [0, 0] and want_e.status.tolist() == [0, 0]
        assert eout.labels.cpu().numpy().tobytes() == want_e.labels.tobytes() and eout.total_frames.cpu().numpy().tobytes() == want_e.total_frames.tobytes()
        assert engine.stream_beam_block(db, S, bplan).cpu().numpy().tobytes() == tb.block.tobytes(), k
        assert engine.stream_block(ds, S).cpu().numpy().tobytes() == ts.block.tobytes(), k
    assert want_b.n_hyps.tolist() == [2, 2] and tb.header(2)[2] == ts.frames_done(2) > 2 * 32
    assert tb.block[2, 4] == 2 and tb.block[0, 4] == 1


def test_abi_refusals_leave_the_outputs_alone():
    from qasr import engine
    lib = engine.load_library()
    splan = sc.plan_frames(*PLAN)
    W, N, S, B = 16, 20, 3, 2
    bplan = sb.StreamBeamPlan(W, 2, N, 7, splan.max_final_frames, boost=True)
    lm = _lm('en3')
    state, bstate = engine.stream_state(S, splan, 'cuda'), engine.stream_beam_boost_state(S, bplan, 'cuda')
    state.fill_(0x5a5a5a5a), bstate.fill_(0x5a5a5a5a)
    poison = (state.clone(), bstate.clone())
    lp = sbc.stream_logp(91, splan.Tw)
    blank = lp.shape[1] - 1
    sets = _sets([lp], blank)
    cid, cq = (_cuda(np.stack([x] * B)) for x in _cands(lp, N))
    sl, fl, enc, first, bset = _i32([0, 1]), _i32([0, 0]), _i32([40, 40]), _i32([0, 0]), _i32([0, 1])
    out = engine.stream_beam_boost_buffers(B, bplan, 'cuda', True)
    outs = [getattr(out, n) for n in FIELDS]
    for t in outs:
        t.fill_(-9)

    def args(inner=None, **kw):
        a = engine.stream_beam_boost_args(state, bstate, S, splan, bplan, sl, fl, cid, cq, enc, first, blank, sets, bset, lm, 0.5, 0.5, out=out)
        for k, v in (inner or {}).items():
            setattr(a.beam, k, v)
        for k, v in kw.items():
            if isinstance(v, tuple):                                            # (index, value) of an array field
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a

    nbb = bstate.numel() * 4
    assert nbb == sb.state_bytes(S, W, bplan.F, True) == lib.qasr_stream_beam_boost_state_bytes(S, W, bplan.F)
    assert nbb > lib.qasr_stream_beam_state_bytes(S, W, bplan.F)
    blob1 = engine.boost_device(sets[1], 'cuda')
    inner = refusals.step_mutations(splan, bplan, S, state, bstate, engine.lm_device(lm, 'cuda').data_ptr(), blank, ends=True) + \
        [dict(beam_state_bytes=lib.qasr_stream_beam_state_bytes(S, W, bplan.F)), dict(space=-1, lm=None, end_lm_score=None)]
    assert len(inner) == 43 + 21 + 2
    outer = [dict(struct_size=8), dict(n_sets=0), dict(n_sets=9), dict(n_sets=-1), dict(boost_set=None), dict(end_boost_score=None),
             dict(sets=(1, None)), dict(sets=(0, blob1.data_ptr() + 8)), dict(set_bytes=(1, 64)), dict(set_bytes=(0, 1 << 31))]
    s = engine._stream_ptr()
    for kw in inner:
        assert lib.qasr_stream_beam_boost(s, C.byref(args(kw))) == 1, kw            # QASR_ERR_ARG
        assert lib.qasr_last_error()
    for kw in outer:
        assert lib.qasr_stream_beam_boost(s, C.byref(args(**kw))) == 1, kw
    assert lib.qasr_stream_beam_boost(s, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(state, poison[0]) and torch.equal(bstate, poison[1])
    for t in outs:
        assert bool((t == -9).all())
    assert lib.qasr_stream_beam_boost_state_bytes(0, W, 8) == 0 and lib.qasr_stream_beam_boost_state_bytes(1, 129, 8) == 0
    assert lib.qasr_stream_beam_boost_state_bytes(1, W, 0) == 0 and lib.qasr_stream_beam_boost_state_bytes(1, W, (1 << 20) + 1) == 0
