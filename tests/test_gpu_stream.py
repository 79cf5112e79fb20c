"""k_stream_push, k_stream_window and k_stream_emit on an MI355X against their NumPy twins (qasr.stream), every byte, the
state block included: a ring that wraps, permuted slots, float32 and int16 chunks on the vector and the scalar path, BEGIN on
a used slot, the production size; final ranges around the 64-frame chunks and the work-group's round, carried runs, ties and
signed zeros, END, gaps, clamped lengths; the collapse invariant over a whole stream; one captured chain of the three
kernels replayed on new data; and the refusals of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_cases as sc  # noqa: E402
from qasr import stream as st  # noqa: E402


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


def _blocks(state, S):
    from qasr import engine
    return engine.stream_block(state, S).cpu().numpy()


def _same_batch(got, want, what=''):
    for name in ('labels', 'start', 'nframes', 'score', 'n_new_labels', 'status', 'total_frames', 'utt_score', 'tail_labels', 'tail_n'):
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g, w)


@pytest.mark.parametrize('dtype', ['float32', 'int16'])
@pytest.mark.parametrize('extra', [0, 1])
@pytest.mark.parametrize('off', [0, 1, 3])
def test_push_and_window_equal_the_twins(dtype, off, extra):
    """C = 640, Wl = 2560: 20 steps wrap the ring of 3200 samples several times; rows in permuted slot order"""
    from qasr import engine
    plan = sc.plan_frames(2, 5, 1)
    assert (plan.C, plan.Wl, plan.cap) == (640, 2560, 3200)
    S, slots, pitch = 5, [3, 0, 4], plan.C + extra
    n_new, flags = sc.push_schedule(plan.C)
    rng = np.random.default_rng(off + 10 * extra)
    twin = st.StreamState(S, plan)
    state = engine.stream_state(S, plan, 'cuda')
    sl = _i32(slots)
    for k in range(len(n_new)):
        if dtype == 'int16':
            x = rng.integers(-32768, 32768, size=(3, pitch)).astype(np.int16)
        else:
            x = rng.standard_normal((3, pitch)).astype(np.float32)
        base = torch.zeros(off + 3 * pitch, dtype=getattr(torch, dtype), device='cuda')
        chunk = base[off:off + 3 * pitch].view(3, pitch)                          # the base offset decides the rows' alignment
        chunk.copy_(_cuda(x))
        engine.stream_push(state, S, plan, sl, _i32(flags[k]), _i32(n_new[k]), chunk)
        st.push_host(twin, slots, flags[k], n_new[k], x)
        win, wl, first = engine.stream_window(state, S, plan, sl)
        want = st.window_host(twin, slots)
        torch.cuda.synchronize()
        for g, w in zip((win, wl, first), want):
            assert g.cpu().numpy().tobytes() == w.tobytes(), (k, dtype, off, extra)
        assert _blocks(state, S).tobytes() == twin.block.tobytes(), k
    assert max(twin.received(s) for s in slots) > 3 * plan.cap
    ring = state[S * st.STATE_WORDS:].view(torch.float32).view(S, plan.cap).cpu().numpy()
    assert ring.tobytes() == twin.ring.tobytes()                                 # untouched slots stayed zero


def test_push_clamps_and_skips():
    from qasr import engine
    plan = sc.plan_frames(2, 5, 1)
    S = 2
    twin, state = st.StreamState(S, plan), engine.stream_state(S, plan, 'cuda')
    x = np.random.default_rng(0).standard_normal((2, plan.C + 40)).astype(np.float32)
    for slots, n in (([1, 0], [plan.C + 40, -5]), ([7, 1], [3, 3]), ([-1, 0], [1, 2 ** 30])):
        engine.stream_push(state, S, plan, _i32(slots), _i32([0, 0]), _i32(n), _cuda(x))
        st.push_host(twin, slots, [0, 0], n, x)
        win, wl, first = engine.stream_window(state, S, plan, _i32(slots))
        want = st.window_host(twin, slots)
        torch.cuda.synchronize()
        for g, w in zip((win, wl, first), want):
            assert g.cpu().numpy().tobytes() == w.tobytes(), slots
    full = state.cpu().numpy()
    assert full[:S * st.STATE_WORDS].tobytes() == twin.block.tobytes() and full[S * st.STATE_WORDS:].tobytes() == twin.ring.tobytes()
    assert [twin.received(0), twin.received(1)] == [plan.C, plan.C + 3]


def test_one_step_at_the_production_size():
    from qasr import engine
    plan = sc.plan_frames(48, 300, 48)
    assert (plan.C, plan.Wl) == (15360, 96000 + 15360 + 15360)
    S, slots = 3, [2, 0]
    twin, state = st.StreamState(S, plan), engine.stream_state(S, plan, 'cuda')
    rng = np.random.default_rng(3)
    sl = _i32(slots)
    for k in range(11):                                                          # the window fills, slides and the ring wraps
        x = rng.standard_normal((2, plan.C)).astype(np.float32)
        n = [plan.C, plan.C if k % 4 else plan.C - 321]
        engine.stream_push(state, S, plan, sl, _i32([st.BEGIN if k == 0 else 0] * 2), _i32(n), _cuda(x))
        st.push_host(twin, slots, [st.BEGIN if k == 0 else 0] * 2, n, x)
    win, wl, first = engine.stream_window(state, S, plan, sl)
    want = st.window_host(twin, slots)
    torch.cuda.synchronize()
    for g, w in zip((win, wl, first), want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    assert want[2].tolist()[0] > 0 and want[1].tolist()[0] == plan.Wl and _blocks(state, S).tobytes() == twin.block.tobytes()


EMIT_PLAN = (4, 330, 2)                                                          # Tw = 337 frames: ranges of 300 frames fit


def _emit_both(plan, S, slots, flags, blks, tok, fs, enc, first, P):
    """the same blocks on both sides, one launch, everything compared"""
    from qasr import engine
    twin = st.StreamState(S, plan)
    for s, b in zip(slots, blks):
        if 0 <= s < S:
            twin.block[s] = b
    state = engine.stream_state(S, plan, 'cuda')
    engine.stream_block(state, S).copy_(_cuda(twin.block))
    want = st.emit_batch_host(twin, slots, flags, tok, fs, enc, first, sc.BLANK, P=P)
    out = engine.stream_emit_buffers(len(slots), plan, 'cuda', P=P)
    for t in (out.labels, out.start, out.nframes, out.n_new_labels, out.status, out.total_frames, out.tail_labels, out.tail_n):
        t.fill_(-77)                                                             # every output is written, tails included
    out.score.fill_(float('nan'))
    out.utt_score.fill_(float('nan'))
    got = engine.stream_emit(state, S, plan, _i32(slots), _i32(flags), _cuda(tok), _cuda(fs), _i32(enc), _i32(first), sc.BLANK, out=out)
    torch.cuda.synchronize()
    _same_batch(got, want, (slots, flags))
    assert _blocks(state, S).tobytes() == twin.block.tobytes(), (slots, flags)
    return want, twin


def test_emit_equals_the_twin_case_by_case():
    plan = sc.plan_frames(*EMIT_PLAN)
    assert plan.Tw == 337
    cases = sc.emit_cases()
    rng = np.random.default_rng(11)
    S = len(cases)
    rows = [sc.emit_case_inputs(rng, plan, n, lo, kind, end, carry) for _, n, lo, kind, end, carry in cases]
    slots = list(rng.permutation(S))                                             # every case its own slot, one launch for all
    flags = [st.END if c[4] else 0 for c in cases]
    blks, tok, fs, enc, first = (np.stack([r[i] for r in rows]) if i < 3 else [r[i] for r in rows] for i in range(5))
    want, _ = _emit_both(plan, S, [int(s) for s in slots], flags, blks, tok, fs, enc, first, P=302)
    for b, (name, n, lo, kind, end, carry) in enumerate(cases):
        assert want.status[b] == 0 and want.total_frames[b] == lo + n, name
    assert want.n_new_labels.max() > 64 and (want.n_new_labels == 0).any() and want.tail_n.max() == plan.tail_pitch


def test_emit_clamps_refuses_and_truncates():
    plan = sc.plan_frames(*EMIT_PLAN)
    rng = np.random.default_rng(12)
    mk = lambda n, lo, kind, end, carry, enc='fit': sc.emit_case_inputs(rng, plan, n, lo, kind, end, carry, enc)
    rows = [mk(65, 64, 'random', False, 'same', 'zero'),                         # enc_len 0: nothing final, the open run stays
            mk(65, 64, 'random', True, 'same', 'zero'),                          # ... END: the carried run closes at lo
            mk(100, 1, 'noblank', True, 'other', 'over'),                        # enc_len beyond Tw: clamped to Tw
            mk(100, 1, 'noblank', False, None, 'over'),
            mk(10, 100, 'random', False, 'same'),                                # the gap: lo < first
            mk(10, 100, 'random', True, None),
            mk(300, 1, 'noblank', True, 'other')]                                # more labels than P: dropped, counted in the state
    rows[4] = (rows[4][0], rows[4][1], rows[4][2], rows[4][3], 101)
    rows[5] = (rows[5][0], rows[5][1], rows[5][2], rows[5][3], 120)
    slots = [0, 1, 2, 3, 4, 9, 5]                                                # row 5: no such slot
    flags = [0, st.END, st.END, 0, 0, st.END, st.END]
    blks, tok, fs = (np.stack([r[i] for r in rows]) for i in range(3))
    want, twin = _emit_both(plan, 7, slots, flags, blks, tok, fs, [r[3] for r in rows], [r[4] for r in rows], P=40)
    assert want.status.tolist() == [0, 0, 0, 0, st.STATUS_GAP, st.STATUS_SLOT, 0]
    assert want.n_new_labels.tolist()[:2] == [0, 1] and want.n_new_labels[6] == 40 and twin.n_labels(5) > 40 + 11
    assert want.total_frames.tolist()[:4] == [64, 64, plan.Tw, 101]


def _gpu_ops(plan, S, slot):
    """the three kernels behind stream_cases.play's interface, next to a twin that must agree after every call"""
    from qasr import engine
    twin, state = st.StreamState(S, plan), engine.stream_state(S, plan, 'cuda')
    sl = _i32([slot])

    def push(flag, x):
        chunk = np.zeros((1, max(len(x), 1)), dtype=np.float32)
        chunk[0, :len(x)] = x
        engine.stream_push(state, S, plan, sl, _i32([flag]), _i32([len(x)]), _cuda(chunk))
        st.push_host(twin, [slot], [flag], [len(x)], chunk)

    def window():
        _, wl, first = engine.stream_window(state, S, plan, sl)
        return int(wl.item()), int(first.item())

    def emit(t, f, e, first, end):
        o = engine.stream_emit(state, S, plan, sl, _i32([st.END if end else 0]), _cuda(t[None]), _cuda(f[None]), _i32([e]), _i32([first]), sc.BLANK)
        w = st.emit_batch_host(twin, [slot], [st.END if end else 0], t[None], f[None], [e], [first], sc.BLANK)
        torch.cuda.synchronize()
        _same_batch(o, w)
        assert _blocks(state, S).tobytes() == twin.block.tobytes()
        n, tn = int(o.n_new_labels.item()), int(o.tail_n.item())
        lo = int(twin_done[0])
        twin_done[0] = int(o.total_frames.item())
        return st.StepRow(o.labels[0, :n].cpu().numpy(), o.start[0, :n].cpu().numpy(), o.nframes[0, :n].cpu().numpy(),
                          o.score[0, :n].cpu().numpy(), n, int(o.status.item()), twin_done[0], o.utt_score[0].cpu().numpy(),
                          o.tail_labels[0, :tn].cpu().numpy(), lo, twin_done[0])

    twin_done = [0]
    return push, window, emit


@pytest.mark.parametrize('shape,max_run,n_chunks', [((2, 5, 1), 9, 9), ((70, 80, 3), 200, 4)])
def test_invariant_over_a_stream(shape, max_run, n_chunks):
    """a whole stream through the kernels: the deltas are collapse_host of the final frames (chunks of 70 frames: every step
    crosses a 64-frame chunk of the collapse, runs of up to 200 frames cross three steps)"""
    plan = sc.plan_frames(*shape, frames_of=sc.model_frames_of)
    rng = np.random.default_rng(max_run)
    rows = lambda k, Tw: (sc.token_row(rng, Tw, 0.4, max_run), sc.score_row(rng, Tw))
    push, window, emit = _gpu_ops(plan, 3, 1)
    _, steps = sc.play(plan, n_chunks * plan.C + 333, rows, push, window, emit)
    row_t, _ = sc.check_invariant(steps, plan.tail_pitch)
    assert len(row_t) >= n_chunks * shape[0]


def test_capture_and_replay():
    """the three kernels captured once as a linear chain on a side stream; four replays with nothing but device memory
    changing in between; outputs and state equal the twins' after each"""
    from qasr import engine
    plan = sc.plan_frames(2, 5, 1)
    S, slots, B = 4, [2, 0, 3], 3
    rng = np.random.default_rng(21)
    twin, state = st.StreamState(S, plan), engine.stream_state(S, plan, 'cuda')
    sl, fl, nn = _i32(slots), _i32([st.BEGIN] * B), _i32([plan.C] * B)
    chunk = torch.zeros(B, plan.C, device='cuda')
    tok = torch.full((B, plan.Tw), sc.BLANK, dtype=torch.int32, device='cuda')
    fs = torch.zeros(B, plan.Tw, device='cuda')
    enc = _i32([plan.Tw] * B)
    win = (torch.empty(B, plan.Wl, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'))
    out = engine.stream_emit_buffers(B, plan, 'cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.stream_push(state, S, plan, sl, fl, nn, chunk)
            engine.stream_window(state, S, plan, sl, out=win)
            engine.stream_emit(state, S, plan, sl, fl, tok, fs, enc, win[2], sc.BLANK, out=out)
    torch.cuda.synchronize()
    state.zero_()                                                                # whatever the capture left: four fresh replays
    for k in range(4):
        x = rng.standard_normal((B, plan.C)).astype(np.float32)
        t = np.stack([sc.token_row(rng, plan.Tw, 0.3, 4) for _ in range(B)])
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
        want = st.emit_batch_host(twin, slots, flags, t, f, e, w[2], sc.BLANK)
        for a, b in zip(win, w):
            assert a.cpu().numpy().tobytes() == b.tobytes(), k
        _same_batch(out, want, k)
        assert _blocks(state, S).tobytes() == twin.block.tobytes(), k


def test_abi_refusals_leave_the_outputs_alone():
    from qasr import engine
    lib = engine.load_library()
    plan = sc.plan_frames(2, 5, 1)
    S, B = 3, 2
    state = engine.stream_state(S, plan, 'cuda')
    state.fill_(0x5a5a5a5a)
    poison = state.clone()
    sl, fl, nn = _i32([0, 1]), _i32([0, 0]), _i32([plan.C, plan.C])
    chunk = torch.ones(B, plan.C, device='cuda')
    win = torch.full((B, plan.Wl), 7.0, device='cuda')
    wl, first = torch.full((B,), -3, dtype=torch.int32, device='cuda'), torch.full((B,), -3, dtype=torch.int32, device='cuda')
    tok = torch.zeros(B, plan.Tw, dtype=torch.int32, device='cuda')
    fs = torch.zeros(B, plan.Tw, device='cuda')
    enc = _i32([plan.Tw] * B)
    out = engine.stream_emit_buffers(B, plan, 'cuda')
    outs = [t for t in (out.labels, out.start, out.nframes, out.score, out.n_new_labels, out.status, out.total_frames, out.utt_score,
                        out.tail_labels, out.tail_n)]
    for t in outs:
        t.fill_(-9)
    nbytes = state.numel() * 4

    def push_args(**kw):
        a = engine.StreamPushArgs()
        a.struct_size = C.sizeof(engine.StreamPushArgs)
        a.S, a.B, a.Wl, a.C, a.samples_per_frame, a.dtype = S, B, plan.Wl, plan.C, plan.samples_per_frame, engine.PCM_F32
        a.state, a.state_bytes, a.slots, a.flags, a.n_new = state.data_ptr(), nbytes, sl.data_ptr(), fl.data_ptr(), nn.data_ptr()
        a.chunk, a.pitch = chunk.data_ptr(), plan.C
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def window_args(**kw):
        a = engine.StreamWindowArgs()
        a.struct_size = C.sizeof(engine.StreamWindowArgs)
        a.S, a.B, a.Wl, a.C, a.samples_per_frame = S, B, plan.Wl, plan.C, plan.samples_per_frame
        a.state, a.state_bytes, a.slots = state.data_ptr(), nbytes, sl.data_ptr()
        a.windows, a.window_lens, a.first_frame = win.data_ptr(), wl.data_ptr(), first.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def emit_args(**kw):
        a = engine.StreamEmitArgs()
        a.struct_size = C.sizeof(engine.StreamEmitArgs)
        a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame = S, B, plan.Wl, plan.C, plan.Rr, plan.samples_per_frame
        a.Tw, a.P, a.Ptail, a.blank = plan.Tw, plan.emit_pitch, plan.tail_pitch, sc.BLANK
        a.state, a.state_bytes, a.slots, a.flags = state.data_ptr(), nbytes, sl.data_ptr(), fl.data_ptr()
        a.tokens, a.frame_score, a.enc_lens, a.first_frame = tok.data_ptr(), fs.data_ptr(), enc.data_ptr(), first.data_ptr()
        for n in ('labels', 'start', 'nframes', 'score', 'n_new_labels', 'status', 'total_frames', 'utt_score', 'tail_labels', 'tail_n'):
            setattr(a, n, getattr(out, n).data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    geometry = [dict(struct_size=8), dict(B=0), dict(B=S + 1), dict(Wl=0), dict(C=0), dict(samples_per_frame=0),
                dict(Wl=plan.Wl + 1), dict(C=plan.C - 1), dict(state=None), dict(slots=None), dict(state_bytes=nbytes - 4)]
    bad_push = geometry + [dict(flags=None), dict(n_new=None), dict(chunk=None), dict(dtype=7), dict(pitch=-1)]
    bad_window = geometry + [dict(windows=None), dict(window_lens=None), dict(first_frame=None)]
    bad_emit = geometry + [dict(Rr=plan.Rr + 1), dict(Rr=-plan.samples_per_frame), dict(Rr=plan.Wl), dict(P=0), dict(Tw=0), dict(Ptail=0),
                           dict(tail_n=None)] + \
        [{n: None} for n in ('flags', 'tokens', 'frame_score', 'enc_lens', 'first_frame', 'labels', 'start', 'nframes', 'score',
                             'n_new_labels', 'status', 'total_frames', 'utt_score')]
    s = engine._stream_ptr()
    for make, fn, cases in ((push_args, lib.qasr_stream_push, bad_push), (window_args, lib.qasr_stream_window, bad_window),
                            (emit_args, lib.qasr_stream_emit, bad_emit)):
        for kw in cases:
            assert fn(s, C.byref(make(**kw))) == 1, (fn.__name__, kw)                # QASR_ERR_ARG
            assert lib.qasr_last_error()
        assert fn(s, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(state, poison) and bool((win == 7.0).all()) and bool((wl == -3).all()) and bool((first == -3).all())
    for t in outs:
        assert bool((t == -9).all())
    assert lib.qasr_stream_state_bytes(0, plan.Wl, plan.C) == 0 and lib.qasr_stream_state_bytes(S, plan.Wl, plan.C) == st.state_bytes(S, plan)
    assert lib.qasr_stream_state_bytes(2, 2 ** 31 - 8, 640) == 0
    assert lib.qasr_stream_emit(s, C.byref(emit_args(tail_labels=None, tail_n=None, Ptail=0))) in (0,)      # the tail is optional
    torch.cuda.synchronize()
    assert bool((out.tail_labels == -9).all()) and not bool((out.status == -9).any())
