"""EncDecCTCModel.stream(spot=) on an MI355X: on the static engine, with a caller's reservation and on the dynamic path the
hits, their detection times and the unchanged updates and hypotheses equal the host composition (the qasr.stream and
qasr.stream_spot twins over the same model's per-window forwards); it composes with endpoint= and with input_rate=8000;
full-window steps replay without engine allocations; a session without spot launches nothing of the spotter's and gives what
stream_cases.check_against_composition asks of it."""
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
import stream_spot_cases as pc  # noqa: E402
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
def test_hits_updates_and_hypotheses_equal_the_host_composition(mode):
    m = plain.model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(2, 3.0) if mode == 'reserved' else m.reserve(None, None)
    before = m._reserve
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    sspot = pc.facade_spot()
    try:
        slots, ups, hyps, got, pend, sess = pc.play_spot_session(m, audio, lens, 11000, sspot, device='cuda', **KW)
        assert m._reserve == before and sess.steps == 11 + 2
        plan, steps, want = pc.compose_hits(m, audio, lens, sspot, device='cuda', **KW)
        assert got == want                                           # hits, scores and detected_s
        assert all(len(want[i]) > 3 for i in want) and any(p[s] for p in pend for s in p)
        sc.check_against_composition(m, slots, ups, hyps, steps, lens)
    finally:
        m.reserve(None, None)


def test_with_endpointing_both_queues_equal_their_compositions():
    m = plain.model('static')
    m.reserve(None, None)
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    sspot, ep = pc.facade_spot(), ec.facade_endpointing()
    utts = []
    slots, ups, hyps, got, _, sess = pc.play_spot_session(m, audio, lens, 11000, sspot, device='cuda', endpoint=ep,
                                                          wrap=lambda s: utts.append(s), **KW)
    _, _, want = pc.compose_hits(m, audio, lens, sspot, device='cuda', **KW)
    assert got == want and all(len(want[i]) > 3 for i in want)
    taken = utts[0].take_utterances()
    assert len(taken) > 6 and {u.reason for u in taken} >= {'end'}
    for s, h in zip(slots, hyps):                                    # close() returns the END utterance's Hypothesis, as without spot
        last = [u for u in taken if u.slot == s][-1]
        assert last.reason == 'end' and last.hypothesis is h


def test_input_rate_session_equals_the_models_rate_session_on_the_offline_output():
    from qasr import resample as rs
    m = plain.model('static')
    m.reserve(None, None)
    sspot = pc.facade_spot()
    x, lens = rs_cpu.facade_pcm(RATE, 1, lens_s=(1.9, 5.6))
    y, yl = rs.resample_host(x, lens, rs.ResamplePlan(RATE, 16000, m.resample_quality), 1)
    want = pc.play_spot_session(m, np.ascontiguousarray(y, dtype=np.float32), [int(v) for v in yl], 11000, sspot, device='cuda', **KW)[3]
    assert all(len(want[i]) > 1 for i in want)
    got = pc.play_spot_session(m, x, lens, int(0.7 * RATE), sspot, device='cuda', input_rate=RATE, **KW)[3]
    assert got == want and m._reserve is None


def test_full_window_steps_replay_without_allocating():
    m = plain.model('static')
    m.reserve(None, None)
    audio = torch.from_numpy(sc.facade_audio()).cuda()
    n_hits = 0
    with m.stream(max_streams=2, spot=pc.facade_spot(), **KW) as sess:
        C = sess.plan.C
        slot = sess.open()
        stats = []
        for k in range(90000 // C):
            assert len(sess.push([slot], audio[1:2, k * C:(k + 1) * C])) == 1
            n_hits += len(sess.take_hits())
            if k >= 1:                                               # the first step has run: nothing is allocated from here on
                stats.append(m._ragged_engine.ragged_stats())
        sess.close(slot)
        n_hits += len(sess.take_hits())
    assert len(stats) >= 9 and n_hits > 3
    assert stats[-1]['device_allocs'] == stats[0]['device_allocs'] and stats[-1]['device_frees'] == stats[0]['device_frees']


def test_a_session_without_spot_is_the_session_it_was(monkeypatch):
    """no spot state, no k_star and no k_stream_spot launch, the forward without log-probabilities, and the updates and
    hypotheses that stream_cases.check_against_composition asks for"""
    from qasr import engine
    m = plain.model('static')
    m.reserve(None, None)

    def never(*a, **kw):
        raise AssertionError('a session without spot launched the spotter')

    monkeypatch.setattr(engine, 'ctc_star', never)
    monkeypatch.setattr(engine, 'stream_spot', never)
    monkeypatch.setattr(engine, 'stream_spot_state', never)
    decodes = []
    fwd = m._forward
    monkeypatch.setattr(m, '_forward', lambda *a, **kw: (decodes.append(kw.get('decode')), fwd(*a, **kw))[1])
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    slots, ups, hyps, steps = sc.play_session(m, audio, lens, 11000, device='cuda', **KW)
    assert steps == 11 + 2 and set(decodes) == {'frames'}
    monkeypatch.setattr(m, '_forward', fwd)
    plan, want = sc.compose_on_host(m, audio, lens, device='cuda', **KW)
    sc.check_against_composition(m, slots, ups, hyps, want, lens)
