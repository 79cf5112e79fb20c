"""k_stream_endpoint on an MI355X against its NumPy twin (qasr.stream_ep), every byte, records and state blocks, after every step:
three rows in permuted slots through whole streams under both sets of rule frames, END at other places of the chunk, BEGIN on
used slots; a plan whose steps make more than 64 frames final, with endpoints on frames 63, 64 and 65 of a step's range (the
ballot chunk's boundary); statuses; min_logp with signed zeros and NaN; the chain push -> window -> emit -> endpoint captured
once and replayed on new data; and the refusals of the C ABI.  Every device step runs once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_cases as sc  # noqa: E402
import stream_ep_cases as ec  # noqa: E402
from qasr import stream as st, stream_ep as se  # noqa: E402

BLANK = sc.BLANK


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


def _same(got, want, what):
    for name in ('records', 'n_records', 'status'):
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g, w)


class Both:
    """S slots on the device and in the twins; every call runs both and compares everything it wrote"""

    def __init__(self, plan, eplan, S):
        from qasr import engine
        self.plan, self.eplan, self.S = plan, eplan, S
        self.twin, self.ep_twin = st.StreamState(S, plan), se.EpState(S)
        self.state, self.ep = engine.stream_state(S, plan, 'cuda'), engine.stream_ep_state(S, 'cuda')

    def push(self, slots, flags, n, x):
        from qasr import engine
        engine.stream_push(self.state, self.S, self.plan, _i32(slots), _i32(flags), _i32(n), _cuda(x))
        st.push_host(self.twin, slots, flags, n, x)

    def window(self, slots):
        return st.window_host(self.twin, slots)

    def step(self, slots, flags, tok, fs, enc, first, what, E=None):
        """emit + endpoint on both sides with the same flags (emit reads END only)"""
        from qasr import engine
        sl, fl, t, f, e, fi = _i32(slots), _i32(flags), _cuda(tok), _cuda(fs), _i32(enc), _i32(first)
        emit = engine.stream_emit(self.state, self.S, self.plan, sl, fl, t, f, e, fi, BLANK)
        want_emit = st.emit_batch_host(self.twin, slots, flags, tok, fs, enc, first, BLANK)
        out = engine.stream_endpoint_buffers(len(slots), self.eplan, 'cuda', E=E)
        out.records.fill_(-77), out.n_records.fill_(-77), out.status.fill_(-77)  # every output is written, tails included
        got = engine.stream_endpoint(self.state, self.ep, self.S, self.plan, self.eplan, sl, fl, t, f, e, fi, emit, BLANK, out=out)
        want = se.endpoint_batch_host(self.ep_twin, self.twin, slots, flags, tok, fs, enc, first, want_emit, BLANK, self.eplan, E=E)
        torch.cuda.synchronize()
        assert emit.status.cpu().numpy().tobytes() == want_emit.status.tobytes()
        _same(got, want, what)
        assert self.ep.cpu().numpy().tobytes() == self.ep_twin.block.tobytes(), what
        assert engine.stream_block(self.state, self.S).cpu().numpy().tobytes() == self.twin.block.tobytes(), what
        return want, want_emit


def _rows_at(globals_, first, Tw):
    return (np.stack([g[0][f:f + Tw] for g, f in zip(globals_, first)]), np.stack([g[1][f:f + Tw] for g, f in zip(globals_, first)]))


@pytest.mark.parametrize('rules', ec.RULES)
@pytest.mark.parametrize('spec', ec.PLANS + [dict(shape=(70, 10, 2))])
def test_kernel_equals_the_twin_after_every_step(spec, rules):
    """three streams side by side in slots 3, 0, 4 of 5: whole chunks, an END step at three different places of the chunk, then
    a second stream on the used slots (BEGIN).  The concatenated records are the whole-stream pass."""
    plan = ec.stream_plan(spec)
    eplan = se.EndpointPlan(plan, *rules)
    S, slots, B = 5, [3, 0, 4], 3
    both = Both(plan, eplan, S)
    rng = np.random.default_rng(plan.C + rules[0])
    K = 7 if plan.chunk_frames < 64 else 3
    per_step = set()
    for life in range(2):
        T = ec.frames_for(plan, (K + 1) * plan.C)
        rows = [ec.whole_rows(rng, T, max_run=3) for _ in range(B)]
        finals, recs = [([], []) for _ in range(B)], [[] for _ in range(B)]
        tail = [7, plan.C // 2, plan.C - 1]
        for k in range(K + 1):
            end = k == K
            n = tail if end else [plan.C] * B
            both.push(slots, [st.BEGIN if k == 0 else 0] * B, n, rng.standard_normal((B, plan.C)).astype(np.float32))
            _, wl, first = both.window(slots)
            tok, fs = _rows_at(rows, first, plan.Tw)
            enc = [min(int(plan.frames_of(int(x))), plan.Tw) for x in wl]
            lo = [both.twin.frames_done(s) for s in slots]
            flags = [(st.BEGIN if k == 0 else 0) | (st.END if end else 0)] * B
            want, _ = both.step(slots, flags, tok, fs, enc, first, (life, k))
            assert want.status.tolist() == [0] * B
            for b, s in enumerate(slots):
                hi = both.twin.frames_done(s)
                finals[b][0].append(tok[b, lo[b] - first[b]:hi - first[b]]), finals[b][1].append(fs[b, lo[b] - first[b]:hi - first[b]])
                recs[b] += list(want.records[b, :want.n_records[b]])
                per_step.add(int(want.n_records[b]))
        for b in range(B):
            whole = se.endpoints_whole_host(np.concatenate(finals[b][0]), np.concatenate(finals[b][1]), BLANK, eplan)
            assert np.stack(recs[b]).tobytes() == whole.tobytes()
    assert max(per_step) >= 1
    if rules == ec.DENSE_RULES and spec['shape'] == (8, 10, 2):
        assert {2, 3} <= per_step                                                # two and three records in one step
    untouched = [s for s in range(S) if s not in slots]
    assert not both.ep_twin.block[untouched].any()


def test_endpoints_on_frames_63_64_65_of_a_steps_range():
    """chunks of 70 frames: a step's range crosses the 64-frame ballot chunk.  Speech everywhere but on frames 63, 64, 65 of
    the range under (Fsil, Fstart, Fmax, Fhard) = (1, 1, 200, 200): SILENCE on 63, TIMEOUT on 64 and on 65"""
    plan = sc.plan_frames(70, 10, 2)
    eplan = se.EndpointPlan(plan, 1, 1, 200, 200)
    assert plan.max_final_frames > 64
    S, slots, B = 3, [2, 0], 2
    both = Both(plan, eplan, S)
    rng = np.random.default_rng(70)
    seen = []
    for k in range(3):
        both.push(slots, [st.BEGIN if k == 0 else 0] * B, [plan.C] * B, rng.standard_normal((B, plan.C)).astype(np.float32))
        _, wl, first = both.window(slots)
        lo = [both.twin.frames_done(s) for s in slots]
        tok = np.stack([1 + (np.arange(plan.Tw) // 2 + b) % 3 for b in range(B)]).astype(np.int32)
        fs = np.stack([sc.score_row(rng, plan.Tw) for _ in range(B)])
        for b in range(B):
            at = lo[b] - first[b] + (63 if b == 0 else 62)                       # row 1: one frame earlier, 62 .. 64
            tok[b, at:at + 3] = BLANK
        enc = [min(int(plan.frames_of(int(x))), plan.Tw) for x in wl]
        want, _ = both.step(slots, [st.BEGIN if k == 0 else 0] * B, tok, fs, enc, first, k)
        for b, s in enumerate(slots):
            n = both.twin.frames_done(s) - lo[b]
            if n >= 67:
                r = want.records[b, :want.n_records[b]]
                off = 63 if b == 0 else 62
                assert [(int(x[se.R_REASON]), int(x[se.R_END]) - 1 - lo[b]) for x in r] == \
                    [(se.SILENCE, off), (se.TIMEOUT, off + 1), (se.TIMEOUT, off + 2)], (k, b, r)
                assert int(r[0][se.R_SP_FRAMES]) == int(r[0][se.R_END]) - 1 - int(r[0][se.R_FIRST])
                seen.append(b)
    assert 0 in seen and 1 in seen


def test_statuses_truncation_and_min_logp():
    """one launch: min_logp = 0.0 against +0.0, -0.0, the largest negative float32 and NaN (row 0); this block's frames_done
    ahead of the stream's (row 1); behind the window's first frame (row 2); no such slot (row 3); BEGIN | END on a used slot
    with more records than E = 2 (row 4).  Then a row whose frames emit reported lost."""
    from qasr import engine
    plan = ec.stream_plan(ec.PLANS[1])
    S = 6
    eplan = se.EndpointPlan(plan, 1, 2, 6, 6, 0.0)
    both = Both(plan, eplan, S)
    rng = np.random.default_rng(4)
    both.push([0, 1, 2, 3, 4], [st.BEGIN] * 5, [plan.C] * 5, rng.standard_normal((5, plan.C)).astype(np.float32))
    used = [1, 2, 4]
    both.ep_twin.block[used] = rng.integers(1, 9, size=(3, se.STATE_WORDS))
    both.ep_twin.block[used, se._W_PART:] = sc.score_row(rng, 3 * 64).reshape(3, 64).view(np.int32)
    both.ep_twin.block[1, 0], both.ep_twin.block[2, 0] = 9, 0
    both.ep.copy_(_cuda(both.ep_twin.block))
    both.twin.block[2, 2] = 1                                                    # slot 2: one frame is done, so emit takes first_frame = 1
    engine.stream_block(both.state, S).copy_(_cuda(both.twin.block))
    tok = np.stack([sc.token_row(rng, plan.Tw, 0.3, 2) for _ in range(5)])
    fs = np.stack([sc.score_row(rng, plan.Tw) for _ in range(5)])
    fs[0, :6] = [0.0, -0.0, np.float32(-1e-45), np.nan, -1.5, 0.0]
    tok[0, :6] = [1, 2, 1, 2, 1, BLANK]
    before = both.ep_twin.block.copy()
    want, _ = both.step([0, 1, 2, 7, 4], [st.BEGIN, 0, 0, 0, st.BEGIN | st.END], tok, fs, [plan.Tw] * 5, [0, 0, 1, 0, 0], 'statuses', E=2)
    assert want.status.tolist() == [0, se.STATUS_RANGE, se.STATUS_RANGE, se.STATUS_SLOT, 0]
    assert both.ep_twin.block[[1, 2]].tobytes() == before[[1, 2]].tobytes()
    assert want.n_records.tolist() == [2, 0, 0, 0, 2] and int(both.ep_twin.block[4, 1]) > 2      # row 4: dropped past E, counted in the state
    r = want.records[0]                                                          # +0.0 and -0.0 are speech, the other three are not
    assert [(int(x[se.R_REASON]), int(x[se.R_END]), int(x[se.R_SP_FRAMES])) for x in r] == [(se.SILENCE, 3, 2), (se.TIMEOUT, 5, 0)]
    both.push([5], [st.BEGIN], [plan.C], rng.standard_normal((1, plan.C)).astype(np.float32))
    want, want_emit = both.step([5], [st.BEGIN], tok[:1], fs[:1], [plan.Tw], [3], 'gap')
    assert want_emit.status.tolist() == [st.STATUS_GAP] and want.status.tolist() == [se.STATUS_GAP]


def test_capture_and_replay():
    """push -> window -> (synthetic tokens) -> emit -> endpoint captured once as a linear chain on a side stream; four replays
    with nothing but device memory changing in between; outputs and both states equal the twins' after each"""
    from qasr import engine
    plan = ec.stream_plan(ec.PLANS[0])
    eplan = se.EndpointPlan(plan, *ec.DENSE_RULES)
    S, slots, B = 4, [2, 0, 3], 3
    rng = np.random.default_rng(21)
    twin, ep_twin = st.StreamState(S, plan), se.EpState(S)
    state, ep = engine.stream_state(S, plan, 'cuda'), engine.stream_ep_state(S, 'cuda')
    sl, fl, nn = _i32(slots), _i32([st.BEGIN] * B), _i32([plan.C] * B)
    chunk = torch.zeros(B, plan.C, device='cuda')
    tok = torch.full((B, plan.Tw), BLANK, dtype=torch.int32, device='cuda')
    fs = torch.zeros(B, plan.Tw, device='cuda')
    enc = _i32([plan.Tw] * B)
    win = (torch.empty(B, plan.Wl, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'))
    out = engine.stream_emit_buffers(B, plan, 'cuda')
    eout = engine.stream_endpoint_buffers(B, eplan, 'cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.stream_push(state, S, plan, sl, fl, nn, chunk)
            engine.stream_window(state, S, plan, sl, out=win)
            engine.stream_emit(state, S, plan, sl, fl, tok, fs, enc, win[2], BLANK, out=out)
            engine.stream_endpoint(state, ep, S, plan, eplan, sl, fl, tok, fs, enc, win[2], out, BLANK, out=eout)
    torch.cuda.synchronize()
    state.zero_(), ep.zero_()                                                    # whatever the capture left: four fresh replays
    n_rec = 0
    for k in range(4):
        x = rng.standard_normal((B, plan.C)).astype(np.float32)
        t = np.stack([sc.token_row(rng, plan.Tw, 0.5, 2) for _ in range(B)])
        f = np.stack([sc.score_row(rng, plan.Tw) for _ in range(B)])
        n = [plan.C, plan.C if k != 2 else 3, plan.C]
        e = [plan.Tw, plan.Tw - k, 5 + k]
        flags = [st.BEGIN if k == 0 else 0, st.BEGIN if k == 0 else 0, st.END if k == 3 else (st.BEGIN if k == 0 else 0)]
        chunk.copy_(_cuda(x)), tok.copy_(_cuda(t)), fs.copy_(_cuda(f)), nn.copy_(_i32(n)), enc.copy_(_i32(e)), fl.copy_(_i32(flags))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        st.push_host(twin, slots, flags, n, x)
        w = st.window_host(twin, slots)
        want_emit = st.emit_batch_host(twin, slots, flags, t, f, e, w[2], BLANK)
        want = se.endpoint_batch_host(ep_twin, twin, slots, flags, t, f, e, w[2], want_emit, BLANK, eplan)
        _same(eout, want, k)
        assert ep.cpu().numpy().tobytes() == ep_twin.block.tobytes(), k
        assert engine.stream_block(state, S).cpu().numpy().tobytes() == twin.block.tobytes(), k
        n_rec += int(want.n_records.sum())
    assert n_rec > 4


def test_abi_refusals_leave_the_outputs_alone():
    from qasr import engine
    lib = engine.load_library()
    plan = ec.stream_plan(ec.PLANS[0])
    eplan = se.EndpointPlan(plan, *ec.NO_HARD_RULES)
    S, B = 3, 2
    state, ep = engine.stream_state(S, plan, 'cuda'), engine.stream_ep_state(S, 'cuda')
    state.fill_(0x5a5a5a5a), ep.fill_(0x5a5a5a5a)
    poison, ep_poison = state.clone(), ep.clone()
    sl, fl = _i32([0, 1]), _i32([0, 0])
    tok = torch.zeros(B, plan.Tw, dtype=torch.int32, device='cuda')
    fs = torch.zeros(B, plan.Tw, device='cuda')
    enc, first = _i32([plan.Tw] * B), _i32([0] * B)
    emit = engine.stream_emit_buffers(B, plan, 'cuda')
    for t in (emit.start, emit.nframes, emit.n_new_labels, emit.status):
        t.zero_()
    out = engine.stream_endpoint_buffers(B, eplan, 'cuda')
    outs = [out.records, out.n_records, out.status]
    for t in outs:
        t.fill_(-9)
    nbytes, ep_bytes = state.numel() * 4, ep.numel() * 4
    assert ep_bytes == lib.qasr_stream_ep_state_bytes(S) == se.ep_state_bytes(S) and lib.qasr_stream_ep_state_bytes(0) == 0

    def args(**kw):
        a = engine.StreamEndpointArgs()
        a.struct_size = C.sizeof(engine.StreamEndpointArgs)
        a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame = S, B, plan.Wl, plan.C, plan.Rr, plan.samples_per_frame
        a.Tw, a.P, a.E, a.blank = plan.Tw, plan.emit_pitch, eplan.max_records, BLANK
        a.Fsil, a.Fstart, a.Fmax, a.Fhard, a.min_logp = eplan.Fsil, eplan.Fstart, eplan.Fmax, eplan.Fhard, float('-inf')
        a.state, a.state_bytes, a.ep_state, a.ep_state_bytes = state.data_ptr(), nbytes, ep.data_ptr(), ep_bytes
        a.slots, a.flags, a.tokens, a.frame_score = sl.data_ptr(), fl.data_ptr(), tok.data_ptr(), fs.data_ptr()
        a.enc_lens, a.first_frame = enc.data_ptr(), first.data_ptr()
        a.emit_start, a.emit_nframes = emit.start.data_ptr(), emit.nframes.data_ptr()
        a.emit_n_new_labels, a.emit_status = emit.n_new_labels.data_ptr(), emit.status.data_ptr()
        a.records, a.n_records, a.status = out.records.data_ptr(), out.n_records.data_ptr(), out.status.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(struct_size=8), dict(B=0), dict(B=S + 1), dict(Wl=0), dict(C=0), dict(samples_per_frame=0), dict(Wl=plan.Wl + 1),
           dict(C=plan.C - 1), dict(state_bytes=nbytes - 4), dict(Rr=plan.Rr + 1), dict(Rr=-plan.samples_per_frame), dict(Rr=plan.Wl),
           dict(P=0), dict(Tw=0), dict(E=0), dict(E=-1), dict(Fsil=0), dict(Fstart=0), dict(Fmax=0), dict(Fhard=eplan.Fmax - 1),
           dict(Fsil=2 ** 24 + 1), dict(Fstart=2 ** 24 + 1), dict(Fmax=2 ** 24 + 1, Fhard=2 ** 24 + 1), dict(Fhard=2 ** 24 + 1),
           dict(min_logp=float('nan')), dict(ep_state_bytes=ep_bytes - 4), dict(ep_state_bytes=0), dict(ep_state=ep.data_ptr() + 4)] + \
        [{n: None} for n in ('state', 'ep_state', 'slots', 'flags', 'tokens', 'frame_score', 'enc_lens', 'first_frame', 'emit_start',
                             'emit_nframes', 'emit_n_new_labels', 'emit_status', 'records', 'n_records', 'status')]
    s = engine._stream_ptr()
    for kw in bad:
        assert lib.qasr_stream_endpoint(s, C.byref(args(**kw))) == 1, kw             # QASR_ERR_ARG
        assert lib.qasr_last_error()
    assert lib.qasr_stream_endpoint(s, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(state, poison) and torch.equal(ep, ep_poison)
    for t in outs:
        assert bool((t == -9).all())
