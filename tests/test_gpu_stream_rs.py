"""k_stream_rs_append and k_stream_rs_fir on an MI355X against their NumPy twin (qasr.stream_rs.push_rs_host), every byte: after
every call of a seeded schedule - rows joining and leaving, BEGIN on a used slot, an out-of-range slot, the history-full clamp,
FLUSH twice - the stream state (blocks and rings), the resampler state (blocks and histories) and n_taken / n_out / status
equal the twin's; both FIR instantiations; one captured push replayed on new device-resident inputs; the C ABI's refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_rs_cases as cases  # noqa: E402
from qasr import stream as st, stream_rs as srs  # noqa: E402

SP = cases.SP
S, B = 4, 3


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


def _same_state(state, rs_state, call, p, what):
    full = state.cpu().numpy()
    nb = S * st.STATE_WORDS
    assert full[:nb].tobytes() == call['block'].tobytes(), (what, 'stream blocks')
    assert full[nb:].tobytes() == call['ring'].tobytes(), (what, 'rings')
    rfull = rs_state.cpu().numpy()
    nr = S * srs.RS_STATE_WORDS
    assert rfull[:nr].tobytes() == call['rs_block'].tobytes(), (what, 'resampler blocks')
    assert rfull[nr:].tobytes() == call['hist'].tobytes(), (what, 'histories')


def _run_schedule(name, dtype, ch):
    from qasr import engine
    p = cases.splan(name, ch)
    state, rs_state = engine.stream_state(S, SP, 'cuda'), engine.stream_rs_state(S, p, 'cuda')
    assert rs_state.numel() * 4 == srs.rs_state_bytes(S, p)
    work = engine.stream_rs_work(B, 'cuda')
    seen = set()
    for c, call in enumerate(cases.schedule(name, dtype, ch, S=S, B=B)):
        if call.get('done'):
            break
        out = engine.stream_rs_push(state, rs_state, S, p, _i32(call['slots']), _i32(call['flags']), _i32(call['n_in']),
                                    _i32(call['out_limit']), _cuda(call['chunk']), work=work)
        torch.cuda.synchronize()
        for g, w, what in zip(out, (call['n_taken'], call['n_out'], call['status']), ('n_taken', 'n_out', 'status')):
            assert g.cpu().numpy().tobytes() == w.tobytes(), (name, dtype, ch, c, what, g.cpu().numpy(), w)
        _same_state(state, rs_state, call, p, (name, dtype, ch, c))
        seen |= set(call['status'].tolist())
    assert {0, 1, 2} <= seen                                                     # the clamp and the skipped slot were part of it


@pytest.mark.parametrize('name,dtype,ch', cases.combos())
def test_every_call_of_the_schedule_equals_the_twin(name, dtype, ch):
    assert cases.staged(cases.rplan(name))                                       # these plans take the staged instantiation
    _run_schedule(name, dtype, ch)


@pytest.mark.parametrize('dtype,ch', [('int16', 2), ('float32', 1)])
def test_the_direct_instantiation_equals_the_twin(dtype, ch):
    """256000 Hz 'fast' (1 / 16, W 302): 255 * 16 + 1 + 604 = 4685 frames per tile exceed the stage of 4096"""
    assert not cases.staged(cases.rplan(cases.DIRECT[0]))
    _run_schedule(cases.DIRECT[0], dtype, ch)


def test_a_format_change_appends_nothing():
    from qasr import engine
    p = cases.splan('12000_fast', 2)
    state, rs_state = engine.stream_state(S, SP, 'cuda'), engine.stream_rs_state(S, p, 'cuda')
    tw, trs = st.StreamState(S, SP), srs.ResampleState(S, p)
    rng = np.random.default_rng(1)
    for k, dtype in enumerate(('int16', 'float32', 'int16')):
        x = np.stack([cases.signal(rng, dtype, 300, 2) for _ in range(2)])
        args = ([1, 3], [st.BEGIN if k == 0 else 0] * 2, [300, 200], [SP.C, 7])
        want = srs.push_rs_host(tw, trs, *args, x)
        got = engine.stream_rs_push(state, rs_state, S, p, *[_i32(a) for a in args], _cuda(x))
        torch.cuda.synchronize()
        assert [g.cpu().numpy().tolist() for g in got] == [w.tolist() for w in want]
        assert want[2].tolist() == ([srs.STATUS_FORMAT] * 2 if k == 1 else [0, 0])
        _same_state(state, rs_state, dict(block=tw.block, ring=tw.ring, rs_block=trs.block, hist=trs.hist), p, k)


def test_capture_and_replay():
    """one push (both launches) captured on a side stream; replays with nothing but device memory changing in between:
    new n_in / flags / out_limit / chunk contents; states and outputs equal the twin's after each"""
    from qasr import engine
    name, dtype, ch = '44100_fast', 'int16', 2
    p = cases.splan(name, ch)
    slots = [2, 0, 3]
    state, rs_state = engine.stream_state(S, SP, 'cuda'), engine.stream_rs_state(S, p, 'cuda')
    tw, trs = st.StreamState(S, SP), srs.ResampleState(S, p)
    work = engine.stream_rs_work(B, 'cuda')
    sl, fl, nn, lim = _i32(slots), _i32([st.BEGIN] * B), _i32([0] * B), _i32([0] * B)
    chunk = torch.zeros(B, p.Ain * ch, dtype=torch.int16, device='cuda')
    out = tuple(torch.empty(B, dtype=torch.int32, device='cuda') for _ in range(3))
    engine.resample_plan(p.resample_plan, 'cuda')                                # the table's upload stays outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.stream_rs_push(state, rs_state, S, p, sl, fl, nn, lim, chunk, work=work, out=out)
    torch.cuda.synchronize()
    state.zero_(), rs_state.zero_()
    rng = np.random.default_rng(4)
    for k in range(6):
        x = np.stack([cases.signal(rng, dtype, p.Ain, ch) for _ in range(B)])
        n = [p.Ain, [p.Ain, 7, 0, p.W + 1, 1, 0][k], p.Ain if k < 4 else 0]
        flags = [st.BEGIN if k == 0 else 0, st.BEGIN if k == 0 else 0, (st.BEGIN if k == 0 else 0) | (srs.FLUSH if k >= 4 else 0)]
        limit = [SP.C, [SP.C, 0, 5, SP.C, SP.C, 2 ** 30][k], SP.C]
        chunk.copy_(_cuda(x)), nn.copy_(_i32(n)), fl.copy_(_i32(flags)), lim.copy_(_i32(limit))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = srs.push_rs_host(tw, trs, slots, flags, n, limit, x)
        assert [t.cpu().numpy().tolist() for t in out] == [w.tolist() for w in want], k
        _same_state(state, rs_state, dict(block=tw.block, ring=tw.ring, rs_block=trs.block, hist=trs.hist), p, k)
    assert tw.received(2) > 0 and tw.received(3) == p.out_len(trs.in_received(3))


def test_abi_refusals_leave_everything_alone():
    from qasr import engine
    lib = engine.load_library()
    p = cases.splan('8000_best', 2)
    rp = p.resample_plan
    state, rs_state = engine.stream_state(S, SP, 'cuda'), engine.stream_rs_state(S, p, 'cuda')
    work = engine.stream_rs_work(B, 'cuda')
    for t in (state, rs_state, work):
        t.fill_(0x5a5a5a5a)
    poison = [t.clone() for t in (state, rs_state, work)]
    sl, fl, nn, lim = _i32([0, 1, 2]), _i32([0] * B), _i32([100] * B), _i32([SP.C] * B)
    chunk = torch.ones(B, 100 * 2, dtype=torch.int16, device='cuda')
    out = tuple(torch.full((B,), -9, dtype=torch.int32, device='cuda') for _ in range(3))

    def args(**kw):
        a = engine.stream_rs_args(state, rs_state, S, p, sl, fl, nn, lim, chunk, work=work, out=out)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert C.sizeof(engine.StreamRsPushArgs) == 4 * 12 + 8 * 17                  # the struct of include/qasr.h, no padding
    base = args()
    bad = [dict(struct_size=8), dict(B=0), dict(B=S + 1), dict(Wl=0), dict(C=0), dict(samples_per_frame=0), dict(Wl=SP.Wl + 1),
           dict(state_bytes=base.state_bytes - 4), dict(rs_state_bytes=base.rs_state_bytes - 4), dict(work_bytes=base.work_bytes - 4),
           dict(channels=0), dict(channels=9), dict(dtype=7), dict(L=0), dict(M=0), dict(W=0), dict(W=4097), dict(L=4, M=2),
           dict(hcap=0), dict(hcap=p.hcap + 1), dict(hcap=2 * p.W - 4), dict(hcap=(1 << 26) + 4), dict(blob_bytes=base.blob_bytes - 4),
           dict(pitch=-1), dict(state=base.state + 4), dict(rs_state=base.rs_state + 8), dict(work=base.work + 4), dict(blob=base.blob + 4)]
    bad += [{n: None} for n in ('state', 'rs_state', 'work', 'blob', 'slots', 'flags', 'n_in', 'out_limit', 'chunk', 'n_taken', 'n_out',
                                'status')]
    s = engine._stream_ptr()
    for kw in bad:
        assert lib.qasr_stream_rs_push(s, C.byref(args(**kw))) == 1, kw          # QASR_ERR_ARG
        assert lib.qasr_last_error()
    assert lib.qasr_stream_rs_push(s, None) == 1
    torch.cuda.synchronize()
    for t, q in zip((state, rs_state, work), poison):
        assert torch.equal(t, q)
    assert all(bool((t == -9).all()) for t in out)
    assert lib.qasr_stream_rs_state_bytes(S, p.hcap) == srs.rs_state_bytes(S, p) and lib.qasr_stream_rs_work_bytes(B) == 32 * B
    assert lib.qasr_stream_rs_state_bytes(0, 8) == 0 and lib.qasr_stream_rs_state_bytes(1, 6) == 0 and lib.qasr_stream_rs_work_bytes(0) == 0
    assert (rp.L, rp.M) == (2, 1)
