"""k_stream_spot<1 / 2 / 4> on the device against qasr.stream_spot's twin: every byte of every output and of the whole state
block after every step of whole streams, the statuses, the refusals of the C ABI, and the chain k_star -> k_stream_spot captured
once and replayed on new data.  Every device step runs once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_spot_cases as pc  # noqa: E402
from qasr import align, spot, stream as st, stream_spot as ss  # noqa: E402

SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()


def _i32(x):
    return torch.tensor(np.asarray(x).tolist(), dtype=torch.int32).cuda()


class Device:
    """the spot step on the device next to the twin: every call runs both and compares everything either wrote"""

    def __init__(self, plan, splan, S, blank, PH=None):
        from qasr import engine
        self.engine, self.plan, self.splan, self.S, self.blank, self.PH = engine, plan, splan, S, blank, PH
        self.state = engine.stream_state(S, plan, 'cuda')
        self.sp = engine.stream_spot_state(S, splan, 'cuda')
        self.kw = engine.stream_spot_keywords(splan, 'cuda')
        self.rows = []

    def __call__(self, d, state, spstate):
        e = self.engine
        B, Tw, Cn = d.lp.shape
        want = ss.spot_batch_host(spstate, state, d.slots, d.flags, d.lp, d.star, d.enc, d.first, d.emit_status, self.blank, self.PH,
                                  rows_out=self.rows)
        e.stream_block(self.state, self.S).copy_(torch.from_numpy(state.block).cuda())      # the stream block as emit left it
        big = torch.full((B, Tw + 3, Cn + 5), float('nan'), device='cuda')                   # pitches larger than the shapes
        lp = big[:, :Tw, :Cn]
        lp.copy_(torch.from_numpy(d.lp).cuda())
        plane = torch.full((B, Tw + 7), float('nan'), device='cuda')[:, :Tw]
        enc = _i32(d.enc)
        e.ctc_star(lp, enc, 0.0, out=plane)
        assert plane.cpu().numpy().tobytes() == d.star.tobytes()
        out = e.stream_spot_buffers(B, self.splan, 'cuda', self.PH)
        for n in ss.FIELDS:                                          # a sentinel everywhere: every tail is written
            getattr(out, n).view(torch.int32).fill_(SENTINEL)
        got = e.stream_spot(self.state, self.sp, self.S, self.plan, self.splan, _i32(d.slots), _i32(d.flags), lp, plane, enc,
                            _i32(d.first), _i32(d.emit_status), self.blank, keywords=self.kw, out=out)
        torch.cuda.synchronize()
        host = ss.SpotStepBatch(*[getattr(got, n).cpu().numpy() for n in ss.FIELDS])
        pc.same_batch(host, want, what=len(self.rows))
        assert self.sp.cpu().numpy().tobytes() == spstate.block.tobytes(), len(self.rows)
        return want


def _case(name, C, ML, K, plan_name, threshold, max_span):
    rng = np.random.default_rng([1, C, ML, K])
    plan = pc.plan_of(plan_name)
    blank = C - 1
    tg, tl, bad = pc.keyword_set(rng, C, blank, ML, K)
    return rng, plan, blank, ss.StreamSpotPlan(plan, tg, tl, spot.check_threshold(threshold, name), max_span), bad


@pytest.mark.parametrize('case', pc.KERNEL_CASES, ids=[c[0] for c in pc.KERNEL_CASES])
def test_kernel_equals_the_twin_through_whole_streams(case):
    """three rows in the slots 3, 0, 4 of 5; END at three places of a chunk; NaN and infinite rows in stream 1; the encoded
    lengths of step 1 beyond Tw (clamped); then a second stream on a used slot"""
    rng, plan, blank, splan, bad = _case(*case)
    Cn = case[1]
    n = [2 * plan.C + 1, 3 * plan.C + plan.C // 2, 4 * plan.C]
    lp_all = [pc.whole_logp(rng, pc.frames_for(plan, x), Cn, blank, odd=(i == 1)) for i, x in enumerate(n)]
    dev = Device(plan, splan, 5, blank)
    clamp = lambda k, e: e + 1000 if k == 1 else e
    steps, state, spstate = pc.play(plan, splan, 5, [3, 0, 4], n, lp_all, blank, dev, enc_clamp=clamp)
    hits = pc.check_slicing(steps, splan, 3, blank, bad)
    assert sum(len(h) for h in hits.values()) > 0
    if splan.max_span > 1:                                       # (a span of 1 closes every hit in its own frame)
        assert any(int(d.out.open_start.max()) >= 0 for d in steps if not d.end)                 # a hit open across a step boundary
    lp2 = [pc.whole_logp(rng, pc.frames_for(plan, n[0]), Cn, blank)]
    again, _, _ = pc.play(plan, splan, 5, [0], [n[0]], lp2, blank, dev, state=state, spstate=spstate)
    pc.check_slicing(again, splan, 1, blank, bad)
    if case[0] in ('c29_ml31_k5', 'c29_ml64_k9'):               # the dense cases: an early close on a step's first and last frame
        early = [(t - r.lo, r.hi - 1 - t) for r in dev.rows for t in r.early]
        assert any(a == 0 for a, _ in early) and any(b == 0 for _, b in early), early[:8]


def test_hits_overflow_the_pitch_and_a_zero_length_row():
    """PH = 1: the first hit of a step is stored, every hit is counted; a row whose encoded length is 0 makes nothing final, and
    the step after it walks more than max_final_frames frames: status 3, the block untouched, on the device as in the twin"""
    rng, plan, blank, splan, bad = _case('overflow', 29, 31, 5, 'small', -16.0, 1)
    n = [4 * plan.C + 2, 4 * plan.C]
    lp_all = [pc.whole_logp(rng, pc.frames_for(plan, x), 29, blank) for x in n]
    dev = Device(plan, splan, 2, blank, PH=1)

    def clamp(k, e):
        return np.zeros_like(e) if k == 1 else e

    steps, _, _ = pc.play(plan, splan, 2, [1, 0], n, lp_all, blank, dev, enc_clamp=clamp)
    assert max(int(d.out.n_new_hits.max()) for d in steps) > 1
    status = [int(x) for d in steps for x in d.out.status]
    assert 3 in status and 0 in status


def test_statuses():
    from qasr import engine
    rng, plan, blank, splan, bad = _case('status', 29, 32, 5, 'small', -6.0, 40)
    S, Cn = 4, 29
    dev = Device(plan, splan, S, blank)
    state, spstate = st.StreamState(S, plan), ss.SpotState(S, splan)
    lp = np.stack([pc.whole_logp(rng, plan.Tw, Cn, blank) for _ in range(4)])
    enc = np.full(4, plan.Tw, np.int32)
    star = align.star_host(lp, enc, 0.0)
    for s, done in ((0, 3), (1, 2), (2, 5)):
        state.block[s, st._W_DONE] = done
    # rows: ok; no such slot; emit lost frames; a window that begins behind the block's frames_done
    d = pc.Step([0, 1, 2, 3], [0, 9, 1, 2], [st.BEGIN, st.BEGIN, st.BEGIN, st.BEGIN], False, lp, star, enc, np.array([0, 0, 0, 1], np.int32),
                np.array([0, 0, 1, 0], np.int32), None, None)
    want = dev(d, state, spstate)
    K = splan.K
    valid = [k for k in range(K) if k not in bad]
    assert [int(want.status[b * K + valid[0]]) for b in range(4)] == [0, 2, 1, 3]
    assert [int(want.status[b * K + bad[0]]) for b in range(4)] == [0, 2, 1, 0] and not want.ok.reshape(4, K)[:, bad].any()
    assert not spstate.block[1].any() and not spstate.block[2].any() and spstate.block[0, valid[0], 1] == 1


def test_capture_and_replay():
    """k_star -> k_stream_spot captured once as a linear chain on a side stream; four replays with nothing but device memory
    changing in between; outputs and the state equal the twin's after each"""
    from qasr import engine
    rng, plan, blank, splan, bad = _case('graph', 29, 63, 5, 'small', -6.0, 20)
    S, slots, B, Cn, Tw = 4, [2, 0, 3], 3, 29, plan.Tw
    twin, sp_twin = st.StreamState(S, plan), ss.SpotState(S, splan)
    state, sp = engine.stream_state(S, plan, 'cuda'), engine.stream_spot_state(S, splan, 'cuda')
    kw = engine.stream_spot_keywords(splan, 'cuda')
    sl, fl, enc, first, est = _i32(slots), _i32([st.BEGIN] * B), _i32([Tw] * B), _i32([0] * B), _i32([0] * B)
    lp = torch.zeros(B, Tw, Cn, device='cuda')
    plane = torch.zeros(B, Tw, device='cuda')
    out = engine.stream_spot_buffers(B, splan, 'cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.ctc_star(lp, enc, 0.0, out=plane)
            engine.stream_spot(state, sp, S, plan, splan, sl, fl, lp, plane, enc, first, est, blank, keywords=kw, out=out)
    torch.cuda.synchronize()
    state.zero_(), sp.zero_()                                        # whatever the capture left: four fresh replays
    n_hits, done = 0, [0, 0, 0]
    for k in range(4):
        x = np.stack([pc.whole_logp(rng, Tw, Cn, blank) for _ in range(B)])
        flags = [st.BEGIN if k == 0 else 0, st.BEGIN if k == 0 else 0, st.END if k == 3 else (st.BEGIN if k == 0 else 0)]
        f0 = [max(0, x - 2) for x in done]
        done = [min(done[b] + 3 + b, f0[b] + Tw) for b in range(B)]
        e = [Tw, Tw - k, Tw]
        for b, s in enumerate(slots):
            twin.block[s, st._W_DONE] = done[b]
        engine.stream_block(state, S).copy_(torch.from_numpy(twin.block).cuda())
        lp.copy_(torch.from_numpy(x).cuda()), fl.copy_(_i32(flags)), enc.copy_(_i32(e)), first.copy_(_i32(f0))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = ss.spot_batch_host(sp_twin, twin, slots, flags, x, align.star_host(x, np.array(e), 0.0), e, f0, [0] * B, blank)
        pc.same_batch(ss.SpotStepBatch(*[getattr(out, n).cpu().numpy() for n in ss.FIELDS]), want, what=k)
        assert sp.cpu().numpy().tobytes() == sp_twin.block.tobytes(), k
        assert int(want.status.max()) == 0
        n_hits += int(want.n_new_hits.sum())
    assert n_hits > 4


def test_abi_refusals_leave_the_outputs_alone():
    from qasr import engine
    lib = engine.load_library()
    rng, plan, blank, splan, bad = _case('abi', 29, 31, 5, 'small', -6.0, 20)
    S, B, Cn, Tw, K = 3, 2, 29, plan.Tw, splan.K
    state, sp = engine.stream_state(S, plan, 'cuda'), engine.stream_spot_state(S, splan, 'cuda')
    state.fill_(SENTINEL), sp.fill_(SENTINEL)
    poison, sp_poison = state.clone(), sp.clone()
    tg, tl = engine.stream_spot_keywords(splan, 'cuda')
    sl, fl, enc, first, est = _i32([0, 1]), _i32([0, 0]), _i32([Tw] * B), _i32([0] * B), _i32([0] * B)
    lp = torch.zeros(B, Tw, Cn, device='cuda')
    plane = torch.zeros(B, Tw, device='cuda')
    out = engine.stream_spot_buffers(B, splan, 'cuda')
    outs = [getattr(out, n) for n in ss.FIELDS]
    for t in outs:
        t.fill_(-9)
    nbytes, sp_bytes = state.numel() * 4, sp.numel() * 4
    q = lib.qasr_stream_spot_state_bytes
    assert sp_bytes == q(S, K, splan.ML) == ss.spot_state_bytes(S, K, splan.ML)
    assert q(0, K, 31) == q(S, 0, 31) == q(S, K, 0) == q(S, K, 128) == 0 and q(1, 1, 127) == 4 * (8 + 3 * 256)

    def args(**kw):
        a = engine.StreamSpotArgs()
        a.struct_size = C.sizeof(engine.StreamSpotArgs)
        a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame, a.Tw = S, B, plan.Wl, plan.C, plan.Rr, plan.samples_per_frame, Tw
        a.n_classes, a.K, a.max_labels, a.blank = Cn, K, splan.ML, blank
        a.threshold_q, a.max_span, a.PH, a.max_final_frames = splan.threshold_q, splan.max_span, splan.hit_pitch, splan.max_final_frames
        a.pitch_utt, a.pitch_frame, a.star_pitch = Tw * Cn, Cn, Tw
        a.log_probs, a.star_logp = lp.data_ptr(), plane.data_ptr()
        a.state, a.state_bytes, a.spot_state, a.spot_state_bytes = state.data_ptr(), nbytes, sp.data_ptr(), sp_bytes
        a.slots, a.flags, a.enc_lens, a.first_frame = sl.data_ptr(), fl.data_ptr(), enc.data_ptr(), first.data_ptr()
        a.emit_status, a.targets, a.target_lens = est.data_ptr(), tg.data_ptr(), tl.data_ptr()
        for n in ss.FIELDS:
            setattr(a, n, getattr(out, n).data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad_args = [dict(struct_size=8), dict(struct_size=C.sizeof(engine.StreamSpotArgs) + 8), dict(B=0), dict(B=S + 1), dict(Wl=0), dict(C=0),
                dict(samples_per_frame=0), dict(Wl=plan.Wl + 1), dict(C=plan.C - 1), dict(state_bytes=nbytes - 4), dict(Rr=plan.Rr + 1),
                dict(Rr=-plan.samples_per_frame), dict(Rr=plan.Wl), dict(Tw=0), dict(n_classes=0), dict(K=0), dict(max_labels=0),
                dict(max_labels=128), dict(blank=-1), dict(blank=Cn), dict(pitch_frame=Cn - 1), dict(pitch_utt=Tw * Cn - 1),
                dict(star_pitch=Tw - 1), dict(threshold_q=1), dict(threshold_q=-(16 << 16) - 1), dict(max_span=0), dict(max_span=65537),
                dict(PH=0), dict(PH=-1), dict(max_final_frames=0), dict(max_final_frames=Tw + 1), dict(spot_state_bytes=sp_bytes - 4),
                dict(spot_state_bytes=0), dict(spot_state=sp.data_ptr() + 4), dict(K=K + 1), dict(K=2 ** 31 - 1), dict(max_labels=32)] + \
        [{n: None} for n in ('state', 'spot_state', 'slots', 'flags', 'log_probs', 'star_logp', 'enc_lens', 'first_frame', 'emit_status',
                             'targets', 'target_lens') + ss.FIELDS]
    s = engine._stream_ptr()
    for kw in bad_args:
        assert lib.qasr_stream_spot(s, C.byref(args(**kw))) == 1, kw                 # QASR_ERR_ARG
        assert lib.qasr_last_error()
    assert lib.qasr_stream_spot(s, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(state, poison) and torch.equal(sp, sp_poison)
    for t in outs:
        assert bool((t == -9).all())
