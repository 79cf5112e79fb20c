"""qasr.stream on the CPU: the final ranges tile every stream exactly once and stay inside emit_pitch; the per-step deltas are
collapse_host of the concatenated final frames on every byte; windows are the recording's latest samples; gaps are refused;
EncDecCTCModel.stream on CPU tensors is the composition of the twins over the model's own per-window forwards, however the
audio is sliced."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_cases as sc  # noqa: E402
from qasr import ctc, stream as st  # noqa: E402

SHAPES = [(1, 0, 0), (2, 5, 1), (3, 4, 0), (48, 200, 48)]


@pytest.mark.parametrize('shape', SHAPES)
def test_final_ranges_tile_every_stream(shape):
    """pure arithmetic: the rule over the counters alone, with the encoded lengths frames_of gives"""
    plan = sc.plan_frames(*shape, frames_of=sc.model_frames_of)
    C, spf = plan.C, plan.samples_per_frame
    assert plan.Wl == sum(shape) * spf and plan.emit_pitch == plan.max_final_frames + 1
    for n in range(0, 4 * plan.Wl + 700, 137):
        done = 0
        steps = [(r, False) for r in range(C, n + 1, C)] + [(n, True)]          # a step per chunk, then END
        for r, end in steps:
            start, ln, first = plan.window_of(r)
            assert first * spf == start and 0 <= ln <= plan.Wl and (ln == r or ln > plan.Wl - spf)
            lo, hi = plan.final_range(r, done, first, min(plan.frames_of(ln), plan.Tw), end)
            assert lo == done and lo >= first and hi >= lo, (n, r, end)          # consecutive ranges abut: one owner per frame
            assert hi - lo <= plan.max_final_frames < plan.emit_pitch, (n, r, end, hi - lo)
            done = hi
        start, ln, first = plan.window_of(n)
        assert done == first + min(plan.frames_of(ln), plan.Tw)                  # total_frames: the last window's last frame


def test_plan_refuses_by_name():
    for kw, name in ((dict(chunk_s=0.001), 'chunk_s'), (dict(left_s=-1.0), 'left_s'), (dict(right_s=-0.5), 'right_s'),
                     (dict(chunk_s=float('nan')), 'chunk_s'), (dict(left_s=float('inf')), 'left_s'),
                     (dict(samples_per_frame=0), 'samples_per_frame')):
        with pytest.raises(ValueError, match=name):
            st.StreamPlan(**kw)
    p = st.StreamPlan()
    assert (p.C, p.L, p.Rr, p.Wl) == (15360, 64000, 15360, 94720) and p.tail_pitch == 50


@pytest.mark.parametrize('p_blank', [0.0, 0.5, 0.9, 1.0])
@pytest.mark.parametrize('shape,max_run', [((2, 5, 1), 1), ((2, 5, 1), 9), ((3, 4, 0), 4), ((1, 0, 0), 3), ((4, 6, 3), 30)])
def test_deltas_are_the_collapse_of_the_final_frames(shape, max_run, p_blank):
    """random rows per window; runs longer than a chunk (max_run 9 over chunks of 2 frames crosses three steps and more)"""
    plan = sc.plan_frames(*shape, frames_of=sc.model_frames_of)
    rng = np.random.default_rng(hash((shape, max_run, int(10 * p_blank))) % 2 ** 32)
    long_run = sc.token_row(rng, 4096, p_blank, max_run)                         # one global row: runs survive the re-run windows
    fs_all = sc.score_row(rng, 4096)
    for n in (0, 1, plan.C - 1, plan.C, plan.Wl + 3 * plan.C + 77, 3 * plan.Wl + 5):
        state, push, window, emit = sc.host_ops(plan)

        def rows(k, Tw):
            first = plan.window_of(state.received(0))[2]
            t, f = long_run[first:first + Tw].copy(), fs_all[first:first + Tw].copy()
            if k % 2:                                                            # look-ahead frames differ from what they become
                lim = max((state.received(0) - plan.Rr) // plan.samples_per_frame - first, 0)
                t[lim + 1:] = sc.token_row(rng, Tw, p_blank, 2)[lim + 1:]
            return t, f

        _, steps = sc.play(plan, n, rows, push, window, emit)
        row_t, _ = sc.check_invariant(steps, plan.tail_pitch)
        assert state.n_labels(0) == sum(d['step'].n_new for d in steps) and state.block[0, 3] == 0


def test_independent_rows_per_window():
    """every window's row drawn afresh: the final frames are whatever each step's row held"""
    plan = sc.plan_frames(2, 5, 1, frames_of=sc.model_frames_of)
    rng = np.random.default_rng(5)
    for p_blank in (0.0, 0.5, 0.9, 1.0):
        state, push, window, emit = sc.host_ops(plan)
        rows = lambda k, Tw: (sc.token_row(rng, Tw, p_blank, 5), sc.score_row(rng, Tw))
        _, steps = sc.play(plan, 4 * plan.Wl + 123, rows, push, window, emit)
        row_t, _ = sc.check_invariant(steps, plan.tail_pitch)
        assert len(row_t) > 4 * plan.Wl // plan.samples_per_frame


def test_windows_are_the_latest_samples():
    plan = sc.plan_frames(2, 5, 1)
    C, rng = plan.C, np.random.default_rng(1)
    state = st.StreamState(4, plan)
    rec = {s: np.zeros(0, dtype=np.float32) for s in (3, 0, 2)}
    sizes = [0, 1, 3, C, C, 3, C, 1, C, C, 0, C, C, C, C, 3, C, C, 1, C, C, C] + [C] * 10
    for k, n in enumerate(sizes):
        for i, slot in enumerate((3, 0, 2)):
            m = sizes[(k + i) % len(sizes)]
            begin = (k == 0) or (k == len(sizes) // 2 and slot == 0)             # slot 0 re-opened half-way
            if k % 2:
                pcm = rng.integers(-32768, 32768, size=(1, C + 2)).astype(np.int16)
                x = pcm.astype(np.float32) / np.float32(32768.0)
            else:
                pcm = x = rng.standard_normal((1, C + 2)).astype(np.float32)
            st.push_host(state, [slot], [st.BEGIN if begin else 0], [m], pcm)
            rec[slot] = np.concatenate([rec[slot][:0] if begin else rec[slot], x[0, :m]])
        win, wl, first = st.window_host(state, [3, 0, 2])
        for i, slot in enumerate((3, 0, 2)):
            r = len(rec[slot])
            assert state.received(slot) == r
            start = max(0, plan.samples_per_frame * -(-(r - plan.Wl) // plan.samples_per_frame))
            want = np.zeros(plan.Wl, dtype=np.float32)
            want[:r - start] = rec[slot][start:r]
            assert win[i].tobytes() == want.tobytes() and wl[i] == r - start and first[i] * plan.samples_per_frame == start
    assert max(len(v) for v in rec.values()) > 2 * plan.cap                      # the ring wrapped more than once
    st.push_host(state, [1], [0], [C + 50], np.ones((1, C + 50), dtype=np.float32))
    assert state.received(1) == C                                               # n_new is clamped to the chunk
    st.push_host(state, [7, -1], [0, 0], [3, 3], np.ones((2, 3), dtype=np.float32))      # no such slots: skipped


def test_a_gap_is_refused():
    plan = sc.plan_frames(2, 5, 1)
    state = st.StreamState(1, plan)
    for _ in range(3 * (plan.Wl // plan.C) + 2):                                 # far more than L + C samples without a step
        st.push_host(state, [0], [0], [plan.C], np.zeros((1, plan.C), dtype=np.float32))
    _, wl, first = st.window_host(state, [0])
    before = state.block.copy()
    out = st.emit_batch_host(state, [0], [0], np.zeros((1, plan.Tw), np.int32), np.zeros((1, plan.Tw), np.float32), [plan.Tw], first, sc.BLANK)
    assert first[0] > 0 and out.status[0] == st.STATUS_GAP and out.n_new_labels[0] == 0 and out.tail_n[0] == 0
    assert (out.labels == sc.BLANK).all() and not out.start.any() and state.block.tobytes() == before.tobytes()
    out = st.emit_batch_host(state, [3], [0], np.zeros((1, plan.Tw), np.int32), np.zeros((1, plan.Tw), np.float32), [plan.Tw], first, sc.BLANK)
    assert out.status[0] == st.STATUS_SLOT and state.block.tobytes() == before.tobytes()


# ---------------------------------------------------------------------------------------------------------- the façade
torch = pytest.importorskip('torch')
KW = sc.FACADE_KW


def _model(mode):
    import nemo.quantization.utils.quantize_model as qm
    from nemo.collections.asr.models import EncDecCTCModel
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    if mode == 'host':
        m.set_quant_mode('none')
        return m
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.evaluate(m)
    qm.set_dynamic(m, True)
    return m


@pytest.mark.parametrize('mode', ['host', 'dynamic'])
def test_facade_on_cpu_tensors_is_the_composition(mode):
    torch.set_grad_enabled(False)
    m = _model(mode)
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    plan, want = sc.compose_on_host(m, audio, lens, **KW)
    results = []
    for piece in (1000, 15360, 50000):
        slots, ups, hyps, _ = sc.play_session(m, audio, lens, piece, **KW)
        sc.check_against_composition(m, slots, ups, hyps, want, lens)
        results.append(([dataclasses.astuple(h) for h in hyps], [[dataclasses.astuple(u) for u in ups[s]] for s in slots]))
    assert results[0] == results[1] == results[2]                                # however the audio was sliced
    assert sum(len(h[0]) for h in results[0][0]) > 0


def test_facade_refusals():
    m = _model('host')
    with pytest.raises(ValueError, match='sample_rate'):
        m.stream(sample_rate=8000)
    with pytest.raises(ValueError, match='beam_width'):
        m.stream(beam_width=4)
    with pytest.raises(ValueError, match='chunk_s'):
        m.stream(chunk_s=0.0)
    with pytest.raises(ValueError, match='max_streams'):
        m.stream(max_streams=0)
    sess = m.stream(max_streams=1, **KW)
    s = sess.open()
    with pytest.raises(ValueError, match='max_streams'):
        sess.open()
    with pytest.raises(ValueError, match='slot'):
        sess.push([s + 1], torch.zeros(1, 1000), torch.tensor([1000]))
    with pytest.raises(ValueError, match='slot'):
        sess.close(5)
    assert sess.push([s], torch.randn(1, 1000), torch.tensor([1000])) == []          # no chunk completed: no step
    assert isinstance(sess.close(s), ctc.Hypothesis)
    assert sess.open(0) == 0
    with pytest.raises(ValueError, match='slot'):
        sess.open(0)
    sess.close_all()
