"""EncDecCTCModel.stream(endpoint=) on an MI355X: on the static engine, with a caller's reservation and on the dynamic path the
utterances equal the host composition (the qasr.stream and qasr.stream_ep twins over the same model's per-window forwards);
two slicings of the pushes give equal utterance lists; close() returns the END utterance's Hypothesis; full-window steps
replay one graph without engine allocations; an input_rate=8000 int16 session gives the utterances of a session at the
model's rate fed the offline resampler's output."""
import dataclasses
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_cases as sc  # noqa: E402
import stream_ep_cases as ec  # noqa: E402
import test_gpu_stream_facade as plain  # noqa: E402
import test_stream_rs_cpu as rs_cpu  # noqa: E402

KW = sc.FACADE_KW
RATE = 8000


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_utterances_equal_the_host_composition(mode):
    m = plain.model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(2, 3.0) if mode == 'reserved' else m.reserve(None, None)
    before = m._reserve
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    ep = ec.facade_endpointing()
    try:
        got, hyps, steps = ec.play_ep_session(m, audio, lens, 11000, ep, device='cuda', **KW)      # pieces that split unequally
        assert m._reserve == before and steps == 11 + 2
        plan, want = ec.compose_utterances(m, audio, lens, ep, device='cuda', **KW)
        assert got == want
        reasons = [u[2] for i in want for u in want[i]]
        assert 'hard' in reasons or 'silence' in reasons                         # cuts fire on the random-weight net
        assert all(want[i][-1][2] == 'end' and len(want[i]) > 3 for i in want) and sum(len(u[7][0]) for u in want[1]) > 0
        for i, h in zip((0, 1), hyps):                                           # close() returns the END utterance's Hypothesis
            assert dataclasses.astuple(h) == want[i][-1][7]
        again, _, _ = ec.play_ep_session(m, audio, lens, 8000, ep, device='cuda', **KW)            # another slicing of the same streams
        assert again == got
    finally:
        m.reserve(None, None)


def test_full_window_steps_replay_without_allocating():
    m = plain.model('static')
    m.reserve(None, None)
    audio = torch.from_numpy(sc.facade_audio()).cuda()
    n_utts = 0
    with m.stream(max_streams=2, endpoint=ec.facade_endpointing(), **KW) as sess:
        C = sess.plan.C
        slot = sess.open()
        stats = []
        for k in range(90000 // C):
            assert len(sess.push([slot], audio[1:2, k * C:(k + 1) * C])) == 1
            n_utts += len(sess.take_utterances())
            if k >= 1:                                                           # the first step has run: nothing is allocated from here on
                stats.append(m._ragged_engine.ragged_stats())
        sess.close(slot)
        n_utts += len(sess.take_utterances())
    assert len(stats) >= 9 and n_utts > 3
    assert stats[-1]['device_allocs'] == stats[0]['device_allocs'] and stats[-1]['device_frees'] == stats[0]['device_frees']


def test_input_rate_session_equals_the_models_rate_session_on_the_offline_output():
    from qasr import resample as rs
    m = plain.model('static')
    m.reserve(None, None)
    ep = ec.facade_endpointing()
    x, lens = rs_cpu.facade_pcm(RATE, 1, lens_s=(1.9, 5.6))
    assert x.dtype == np.int16
    y, yl = rs.resample_host(x, lens, rs.ResamplePlan(RATE, 16000, m.resample_quality), 1)
    want, _, _ = ec.play_ep_session(m, np.ascontiguousarray(y, dtype=np.float32), [int(v) for v in yl], 11000, ep, device='cuda', **KW)
    assert all(len(want[i]) > 1 for i in want)
    got, _, _ = ec.play_ep_session(m, x, lens, int(0.7 * RATE), ep, device='cuda', input_rate=RATE, **KW)
    assert got == want
    assert m._reserve is None
