"""k_stream_beam<false> and <true> on an MI355X against their NumPy twin (qasr.stream_beam), every byte after every step,
the beam block and its ring included: steps of 1 .. 95 final frames on both sides of the rounds, permuted slots, windows that
do not start at frame 0, BEGIN on a used slot, END without new frames, a dead beam, every status with poisoned outputs;
whole streams against lagged_search_host and, with a lag beyond the stream, against qasr_ctc_beam[_lm] on the same
candidates; one captured chain of top-N, beam and emit replayed on new data; and the refusals of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_beam_cases as cases  # noqa: E402
import stream_beam_refusal_cases as refusals  # noqa: E402
import stream_cases as sc  # noqa: E402
from qasr import beam as qb  # noqa: E402
from qasr import stream as st  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402

FIELDS = ('labels', 'frames', 'n_new_labels', 'commit_len', 'n_live', 'status', 'tail_labels', 'tail_n', 'end_labels',
          'end_n_labels', 'end_score', 'end_lm_score', 'n_hyps')
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
        _lms[name] = cases.load_lm(cases.GOLDEN, name)
    return _lms.get(name)


def _same(got, want, what=''):
    for name in FIELDS:
        w = getattr(want, name)
        if w is None:
            continue
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g, w)


def _cands(lp, N):
    cid, cq = qb.topn_host(lp[None], N)
    return cid[0], cq[0]


def _window(cid, cq, first, Tw):
    """rows first .. first + Tw of a stream's candidates (empty slots behind its end)"""
    wid = np.full((Tw, cid.shape[1]), -1, np.int32)
    wq = np.full((Tw, cid.shape[1]), qb.EMPTY_Q, np.int32)
    n = max(0, min(Tw, cid.shape[0] - first))
    wid[:n], wq[:n] = cid[first:first + n], cq[first:first + n]
    return wid, wq


class Rig:
    """the kernel and the twin side by side: the same stream blocks (written here: `received` far ahead, frames_done as
    k_stream_emit would leave it), the same beam blocks, one launch per step, everything compared"""

    def __init__(self, bplan, S, blank, lm=None, alpha=0.0, beta=0.0):
        from qasr import engine
        self.splan, self.bplan, self.S, self.blank, self.lm, self.alpha, self.beta = sc.plan_frames(*PLAN), bplan, S, blank, lm, alpha, beta
        self.ts, self.tb = st.StreamState(S, self.splan), sb.StreamBeamState(S, bplan)
        self.ds, self.db = engine.stream_state(S, self.splan, 'cuda'), engine.stream_beam_state(S, bplan, 'cuda')
        for s in range(S):
            self.stream(s, 10 ** 9, 0)

    def stream(self, slot, received, done):
        self.ts.block[slot, 0:2].view(np.int64)[0] = received
        self.ts.block[slot, 2] = done

    def block(self):
        from qasr import engine
        return engine.stream_beam_block(self.db, self.S, self.bplan).cpu().numpy()

    def step(self, slots, flags, wins, enc, first, what='', advance=True, **pitches):
        from qasr import engine
        engine.stream_block(self.ds, self.S).copy_(_cuda(self.ts.block))
        wid, wq = np.stack([w[0] for w in wins]), np.stack([w[1] for w in wins])
        want = sb.step_batch_host(self.tb, self.ts, slots, flags, wid, wq, enc, first, self.blank, self.lm, self.alpha, self.beta, **pitches)
        out = engine.stream_beam_buffers(len(slots), self.bplan, 'cuda', self.lm is not None, **pitches)
        for n in FIELDS:                                                       # every output is written, tails included
            if getattr(out, n) is not None:
                getattr(out, n).fill_(-77)
        got = engine.stream_beam(self.ds, self.db, self.S, self.splan, self.bplan, _i32(slots), _i32(flags), _cuda(wid), _cuda(wq),
                                 _i32(enc), _i32(first), self.blank, self.lm, self.alpha, self.beta, out=out)
        torch.cuda.synchronize()
        _same(got, want, what)
        assert self.block().tobytes() == self.tb.block.tobytes(), what
        assert engine.stream_block(self.ds, self.S).cpu().numpy().tobytes() == self.ts.block.tobytes(), what      # read-only
        if advance:                                                            # what k_stream_emit does to frames_done
            for b, s in enumerate(slots):
                if want.status[b] == 0:
                    self.ts.block[s, 2] = self.tb.header(s)[2]
        return want


MODES = (('none', None, 0.0, 0.0), ('en3', 'en3', 0.7, 1.0), ('zh2', 'zh2', 1.5, 0.5))


def _streams(mode, seeds, T):
    what, model, alpha, beta = mode
    if model is None:
        return [cases.stream_logp(s, T) for s in seeds], None, 0.0, 0.0
    return [cases.lm_stream_logp(model, s, T) for s in seeds], _lm(model), alpha, beta


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('W,N,lag', [(1, 20, 7), (3, 64, 0), (16, 20, 40), (16, 1, 7), (128, 20, 40), (16, 20, 400)])
def test_steps_and_whole_streams_equal_the_twin(mode, W, N, lag):
    """S = 5 slots, 3 rows in permuted slot order, streams of 300 / 260 / 200 frames (W = 128: 200 / 160 / 120) cut by two
    schedules; windows start up to 5 frames before lo; the shorter rows END earlier and then sit out"""
    T = 200 if W == 128 else 300
    lens = [T, T - 40, T - 100]
    lps, lm, alpha, beta = _streams(mode, (11 + W, 12 + lag, 13 + N), T)
    blank = lps[0].shape[1] - 1
    cands = [_cands(lp[:n], N) for lp, n in zip(lps, lens)]
    nb = min(W, 3)
    bplan = sb.StreamBeamPlan(W, nb, N, lag, sc.plan_frames(*PLAN).max_final_frames)
    if lag < 100:
        assert lens[0] >= 4 * bplan.F or W == 128                              # the ring wraps several times
    rig = Rig(bplan, 5, blank, lm, alpha, beta)
    slots = [3, 0, 4]
    edges = [cases.edges_of(cases.cuts_of(sl, n), n) for sl, n in zip((cases.STEP_LENS_A, cases.STEP_LENS_B, cases.STEP_LENS_A), lens)]
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
        o = rig.step(sl, fl, wins, enc, first, (k, rows))
        for i, b in enumerate(rows):
            n = int(o.n_new_labels[i])
            assert o.status[i] == 0 and rig.tb.header(slots[b])[2] == edges[b][k + 1]
            got[b]['labels'] += o.labels[i, :n].tolist()
            got[b]['frames'] += o.frames[i, :n].tolist()
            if fl[i] & st.END:
                got[b]['end'] = [(o.end_labels[i, h, :o.end_n_labels[i, h]].tolist(), int(o.end_score[i, h]),
                                  0 if lm is None else int(o.end_lm_score[i, h])) for h in range(int(o.n_hyps[i]))]
                got[b]['commit'] = int(o.commit_len[i])
    for b in range(3):
        whole = sb.lagged_search_host(*cands[b], lens[b], blank, W, nb, lm, alpha, beta, lag=lag, check=False)
        assert got[b]['labels'] == whole.labels and got[b]['frames'] == whole.frames and got[b]['commit'] == len(whole.labels)
        head = whole.labels[:whole.commit_len_before_end]
        assert [(head + x[0], x[1], x[2]) for x in got[b]['end']] == whole.hyps, b
        if lag >= T:
            assert head == []


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
def test_a_lag_beyond_the_stream_is_qasr_ctc_beam(mode):
    """the END rows of a stream stepped with Lg >= its length against k_beam / k_beam_lm over the same candidates"""
    from qasr import engine
    W, N, T, nb = 16, 20, 200, 16
    lps, lm, alpha, beta = _streams(mode, (41, 42), T)
    blank = lps[0].shape[1] - 1
    cands = [_cands(lp, N) for lp in lps]
    bplan = sb.StreamBeamPlan(W, nb, N, T, sc.plan_frames(*PLAN).max_final_frames)
    rig = Rig(bplan, 2, blank, lm, alpha, beta)
    edges = cases.edges_of(cases.cuts_of(cases.STEP_LENS_B, T), T)
    for k in range(len(edges) - 1):
        lo, hi = edges[k], edges[k + 1]
        fl = (st.BEGIN if k == 0 else 0) | (st.END if k == len(edges) - 2 else 0)
        o = rig.step([1, 0], [fl, fl], [_window(*c, lo, rig.splan.Tw) for c in cands], [hi - lo] * 2, [lo] * 2, k)
    off = engine.ctc_beam(_cuda(np.stack([c[0] for c in cands])), _cuda(np.stack([c[1] for c in cands])), None, blank, W, nb,
                          lm=lm, alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    n_lab, lab = off.n_labels.cpu().numpy(), off.labels.cpu().numpy()
    assert o.n_hyps.tobytes() == off.n_hyps.cpu().numpy().tobytes() and o.end_n_labels.tobytes() == n_lab.tobytes()
    assert o.end_score.tobytes() == off.score.cpu().numpy().tobytes()
    assert lm is None or o.end_lm_score.tobytes() == off.lm_score.cpu().numpy().tobytes()
    for b in range(2):
        for h in range(nb):
            assert o.end_labels[b, h, :n_lab[b, h]].tolist() == lab[b, h, :n_lab[b, h]].tolist()


@pytest.mark.parametrize('mode', [MODES[0], MODES[1]], ids=['none', 'en3'])
def test_begin_on_a_used_slot_end_without_frames_and_a_dead_beam(mode):
    W, N, T = 16, 20, 140
    lps, lm, alpha, beta = _streams(mode, (51, 52), T)
    blank = lps[0].shape[1] - 1
    a, b = (_cands(lp, N) for lp in lps)
    dead = (a[0].copy(), a[1].copy())
    dead[0][50], dead[1][50] = -1, qb.EMPTY_Q                                   # frame 50 has no candidate: the beam dies there
    bplan = sb.StreamBeamPlan(W, 2, N, 7, sc.plan_frames(*PLAN).max_final_frames)
    rig = Rig(bplan, 2, blank, lm, alpha, beta)
    Tw = rig.splan.Tw
    rig.step([1], [st.BEGIN], [_window(*a, 0, Tw)], [70], [0], 'first')
    o = rig.step([1], [st.END], [_window(*a, 60, Tw)], [10], [60], 'END, nothing new')
    assert o.n_hyps[0] == 2 and o.n_new_labels[0] > 0 and o.tail_n[0] == 0
    rig.stream(1, 10 ** 9, 0)                                                   # k_stream_push with BEGIN zeroes the stream block
    o = rig.step([1], [st.BEGIN], [_window(*b, 0, Tw)], [64], [0], 'BEGIN on a used slot')
    assert rig.tb.header(1)[2] == 64 and o.status[0] == 0
    rig.step([0], [st.BEGIN], [_window(*dead, 0, Tw)], [40], [0], 'alive')
    o = rig.step([0], [0], [_window(*dead, 38, Tw)], [22], [38], 'dies at 50')
    assert o.n_live[0] == 0 and rig.tb.header(0)[:3] == (0, o.commit_len[0], 60)
    o = rig.step([0], [st.END], [_window(*dead, 60, Tw)], [80], [60], 'stays dead')
    assert o.n_hyps[0] == 0 and o.n_new_labels[0] == 0 and rig.tb.header(0)[2] == 140


def test_every_status_leaves_the_state_alone():
    W, N = 16, 20
    lp = cases.stream_logp(61, 102)
    blank = lp.shape[1] - 1
    c = _cands(lp, N)
    bplan = sb.StreamBeamPlan(W, 2, N, 7, sc.plan_frames(*PLAN).max_final_frames)
    rig = Rig(bplan, 4, blank)
    win = _window(*c, 0, rig.splan.Tw)
    rig.step([0, 1, 2], [st.BEGIN] * 3, [win] * 3, [40] * 3, [0] * 3, 'begin')
    rig.stream(1, 10 ** 9, 41)                                                  # the stream block ran ahead of the beam block
    before = rig.tb.block.copy()
    o = rig.step([7, 0, 1, 2], [0, 0, st.END, st.BEGIN], [win] * 4, [40, 40, 60, 60], [0, 41, 0, 0], 'statuses', advance=False)
    assert o.status.tolist() == [sb.STATUS_SLOT, sb.STATUS_GAP, sb.STATUS_SYNC, sb.STATUS_SYNC]      # BEGIN: the stream did not begin
    assert rig.tb.block.tobytes() == before.tobytes()
    big = sb.StreamBeamPlan(128, 1, N, 7, sc.plan_frames(*PLAN).max_final_frames)
    rig = Rig(big, 1, blank)
    rig.stream(0, 10 ** 12, 2 ** 24)
    rig.tb.block[0, 2], rig.tb.block[0, 3] = 2 ** 24, 1
    from qasr import engine
    engine.stream_beam_block(rig.db, 1, big).copy_(_cuda(rig.tb.block))
    o = rig.step([0], [0], [win], [40], [2 ** 24], 'node ids', advance=False)
    assert o.status.tolist() == [sb.STATUS_NODES] and rig.tb.header(0)[2] == 2 ** 24


def test_narrow_tail_pitch_and_wide_pitches():
    """Ptail below the tail: the first Ptail labels, the true count; wider P / Pend: the tails are filled"""
    W, N = 16, 20
    lp = cases.stream_logp(71, 102)
    blank = lp.shape[1] - 1
    c = _cands(lp, N)
    bplan = sb.StreamBeamPlan(W, 2, N, 40, sc.plan_frames(*PLAN).max_final_frames)
    rig = Rig(bplan, 1, blank)
    o = rig.step([0], [st.BEGIN], [_window(*c, 0, rig.splan.Tw)], [95], [0], 'narrow', Ptail=3, P=bplan.delta_pitch + 9, Pend=bplan.end_pitch + 5)
    assert o.tail_n[0] > 3 and (o.tail_labels[0] != blank).all()


def test_capture_and_replay():
    """qasr_ctc_topn -> qasr_stream_beam -> qasr_stream_emit captured once as a chain on a side stream; three replays with
    nothing but device memory changing in between; outputs and both states equal the twins' after each"""
    from qasr import engine
    splan = sc.plan_frames(32, 5, 1)
    W, N, S, B, slots = 16, 20, 3, 2, [2, 0]
    lm, alpha, beta = _lm('en3'), 0.7, 1.0
    Tw = splan.Tw
    lps = [cases.lm_stream_logp('en3', s, 200) for s in (81, 82)]
    Cn = lps[0].shape[1]
    blank = Cn - 1
    bplan = sb.StreamBeamPlan(W, 2, N, 7, splan.max_final_frames)
    ts, tb = st.StreamState(S, splan), sb.StreamBeamState(S, bplan)
    ds, db = engine.stream_state(S, splan, 'cuda'), engine.stream_beam_state(S, bplan, 'cuda')
    sl, fl = _i32(slots), _i32([0] * B)
    logp = torch.zeros(B, Tw, Cn, device='cuda')
    tok = torch.zeros(B, Tw, dtype=torch.int32, device='cuda')
    fs = torch.zeros(B, Tw, device='cuda')
    enc, first = _i32([Tw] * B), _i32([0] * B)
    cand = (torch.empty(B, Tw, N, dtype=torch.int32, device='cuda'), torch.empty(B, Tw, N, dtype=torch.int32, device='cuda'))
    bout = engine.stream_beam_buffers(B, bplan, 'cuda', True)
    eout = engine.stream_emit_buffers(B, splan, 'cuda')
    engine.lae_table_device('cuda'), engine.lm_device(lm, 'cuda')               # uploads happen outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.ctc_topn(logp, None, N, out=cand)
            engine.stream_beam(ds, db, S, splan, bplan, sl, fl, cand[0], cand[1], enc, first, blank, lm, alpha, beta, out=bout)
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
        want_b = sb.step_batch_host(tb, ts, slots, flags, cid, cq, e, [f] * B, blank, lm, alpha, beta)
        want_e = st.emit_batch_host(ts, slots, flags, t_np, f_np, e, [f] * B, blank)
        _same(bout, want_b, k)
        assert want_b.status.tolist() == [0, 0] and want_e.status.tolist() == [0, 0]
        assert eout.labels.cpu().numpy().tobytes() == want_e.labels.tobytes() and eout.total_frames.cpu().numpy().tobytes() == want_e.total_frames.tobytes()
        assert engine.stream_beam_block(db, S, bplan).cpu().numpy().tobytes() == tb.block.tobytes(), k
        assert engine.stream_block(ds, S).cpu().numpy().tobytes() == ts.block.tobytes(), k
    assert want_b.n_hyps.tolist() == [2, 2] and tb.header(2)[2] == ts.frames_done(2) > 2 * 32


def test_abi_refusals_leave_the_outputs_alone():
    from qasr import engine
    lib = engine.load_library()
    splan = sc.plan_frames(*PLAN)
    W, N, S, B = 16, 20, 3, 2
    bplan = sb.StreamBeamPlan(W, 2, N, 7, splan.max_final_frames)
    lm = _lm('en3')
    state, bstate = engine.stream_state(S, splan, 'cuda'), engine.stream_beam_state(S, bplan, 'cuda')
    state.fill_(0x5a5a5a5a), bstate.fill_(0x5a5a5a5a)
    poison = (state.clone(), bstate.clone())
    lp = cases.stream_logp(91, splan.Tw)
    cid, cq = (_cuda(np.stack([x] * B)) for x in _cands(lp, N))
    sl, fl, enc, first = _i32([0, 1]), _i32([0, 0]), _i32([40, 40]), _i32([0, 0])
    out = engine.stream_beam_buffers(B, bplan, 'cuda', True)
    outs = [getattr(out, n) for n in FIELDS]
    for t in outs:
        t.fill_(-9)

    def args(**kw):
        a = engine.stream_beam_args(state, bstate, S, splan, bplan, sl, fl, cid, cq, enc, first, lp.shape[1] - 1, lm, 0.5, 0.5, out=out)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    nbb = bstate.numel() * 4
    assert nbb == sb.state_bytes(S, W, bplan.F) == lib.qasr_stream_beam_state_bytes(S, W, bplan.F)
    bad = refusals.step_mutations(splan, bplan, S, state, bstate, engine.lm_device(lm, 'cuda').data_ptr(), lp.shape[1] - 1, ends=True)
    assert len(bad) == 43 + 21
    s = engine._stream_ptr()
    for kw in bad:
        assert lib.qasr_stream_beam(s, C.byref(args(**kw))) == 1, kw                # QASR_ERR_ARG
        assert lib.qasr_last_error()
    assert lib.qasr_stream_beam(s, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(state, poison[0]) and torch.equal(bstate, poison[1])
    for t in outs:
        assert bool((t == -9).all())
    assert lib.qasr_stream_beam_state_bytes(0, W, 8) == 0 and lib.qasr_stream_beam_state_bytes(1, 129, 8) == 0
    assert lib.qasr_stream_beam_state_bytes(1, W, 0) == 0 and lib.qasr_stream_beam_state_bytes(1, W, (1 << 20) + 1) == 0
