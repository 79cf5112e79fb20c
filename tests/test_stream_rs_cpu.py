"""Streaming at any sample rate on the CPU (qasr.stream_rs): however a stream is sliced, what push_rs_host puts into the ring is
resample_host of the whole stream on every byte; the edges of the rule; the history bound of every plan; the façade on CPU
tensors against a session at the model's rate fed the offline resampler's output; the refusals."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_cases as rc  # noqa: E402
import stream_cases as sc  # noqa: E402
import stream_rs_cases as cases  # noqa: E402
from qasr import resample as rs, stream as st, stream_rs as srs  # noqa: E402

SP = cases.SP


def test_plans_are_what_the_cases_say():
    got = {n: (cases.rplan(n).L, cases.rplan(n).M, cases.rplan(n).W) for n in cases.PLANS}
    assert got['8000_best'] == (2, 1, 68) and got['48000_best'] == (1, 3, 203) and got['44100_fast'] == (160, 441, 52)
    assert got['12000_fast'][:2] == (4, 3) and cases.rplan('16000_equal').equal and cases.splan('16000_equal', 2).W == 0
    assert all(cases.staged(cases.rplan(n)) for n in cases.PLANS) and not cases.staged(cases.rplan(cases.DIRECT[0]))
    p = cases.splan('48000_best', 1)
    assert (p.Ain, p.hcap) == (1920, 2328) and 2 * p.W > SP.C * p.M // p.L // 8
    assert p.ready(p.W) == 0 and p.ready(p.W + 1) == 1 and p.ready(p.W + 3) == 1 and p.ready(p.W + 4) == 2 and p.out_len(4) == 2
    assert abs(cases.splan('8000_best', 1).latency_s() - 0.0085) < 1e-12


@pytest.mark.parametrize('name,dtype,ch', cases.combos())
def test_every_slicing_gives_the_offline_bytes(name, dtype, ch):
    """pieces of 1 and 7 frames cost one twin call per piece, so they run on the first 2 W + 3 M + 50 frames of the long
    stream (the start-up, the first final outputs of every phase group and the flush); the other slicings on all of it"""
    p = cases.splan(name, ch)
    xs, lens = cases.streams(name, dtype, ch)
    for x, n in zip(xs, lens):
        want = cases.offline(p, x, n)
        for sl, pieces in cases.slicings(p, n).items():
            if sl in ('1', '7') and n > 2 * p.W + 3 * p.M + 50:
                continue
            got, state, rss = cases.play_stream(p, x, n, pieces)
            assert state.received(0) == p.out_len(n) == len(want) and rss.in_received(0) == n
            assert got.tobytes() == want.tobytes(), (name, dtype, ch, n, sl)
    x, n = xs[0], min(lens[0], 2 * p.W + 3 * p.M + 50)
    want = cases.offline(p, x[:n * ch], n)
    for sl in ('1', '7'):
        got, state, _ = cases.play_stream(p, x[:n * ch], n, cases.slicings(p, n)[sl])
        assert got.tobytes() == want.tobytes() and state.received(0) == len(want), (name, dtype, ch, sl)


@pytest.mark.parametrize('name,dtype,ch', [('8000_best', 'int16', 2), ('44100_fast', 'float32', 3), ('48000_best', 'int16', 1),
                                           ('16000_equal', 'int16', 2), (cases.DIRECT[0], 'float32', 1)])
def test_the_schedule_keeps_finality(name, dtype, ch):
    """rows joining and leaving, clamped and refused rows: every slot's outputs are the offline bytes of the frames it took"""
    seen, last = set(), None
    for call in cases.schedule(name, dtype, ch):
        if call.get('done'):
            last = call
        else:
            seen |= set(call['status'].tolist())
            assert (call['n_taken'] <= np.maximum(call['n_in'], 0)).all()
    assert {0, 1, 2} <= seen                                                     # the history-full clamp and a bad slot occurred
    p = last['plan']
    for s, got in last['outs'].items():
        n = last['taken'][s]
        want = cases.offline(p, last['data'][s][:n * ch], n)
        assert len(got) <= len(want) and got.tobytes() == want[:len(got)].tobytes(), (name, s)
        if s in last['ended']:
            assert len(got) > 0
    assert any(len(last['outs'][s]) == p.out_len(last['taken'][s]) > 0 for s in last['ended'])     # a flushed stream is complete


def _one(p, dtype='int16', S=2):
    return st.StreamState(S, SP), srs.ResampleState(S, p)


def test_edges_of_the_rule():
    name, ch = '8000_best', 2
    p = cases.splan(name, ch)
    rng = np.random.default_rng(5)
    n = p.hcap * 2
    x = cases.signal(rng, 'int16', n, ch)
    want = cases.offline(p, x, n)
    state, rss = _one(p)
    push = lambda flag, k, lim, off=0, slot=0: srs.push_rs_host(state, rss, [slot], [flag], [k], [lim], x[None, off * ch:(off + max(k, 1)) * ch])
    # out_limit = 0 appends only; n_in = 0 produces only; a limit below the ready count leaves the rest for the next call
    nt, no, stt = push(st.BEGIN, 200, 0)
    assert (nt[0], no[0], stt[0]) == (200, 0, 0) and state.received(0) == 0 and rss.in_received(0) == 200 and rss.fmt(0) == srs.PCM_S16
    nt, no, stt = push(0, 0, 100)
    assert (nt[0], no[0]) == (0, 100) and rss.in_received(0) == 200
    a = cases.read_ring(state, 0, 100)
    nt, no, stt = push(0, 0, 2 ** 30)
    assert no[0] == p.ready(200) - 100 == 164
    b = cases.read_ring(state, 0, 164)
    assert np.concatenate([a, b]).tobytes() == want[:264].tobytes()
    assert push(0, 0, 2 ** 30)[1][0] == 0                                        # nothing ready any more
    # a slot out of range: no byte of either state changes
    before = (state.block.tobytes(), state.ring.tobytes(), rss.block.tobytes(), rss.hist.tobytes())
    for bad in (-1, 2):
        nt, no, stt = push(0, 50, 50, slot=bad)
        assert (nt[0], no[0], stt[0]) == (0, 0, srs.STATUS_SLOT)
    assert before == (state.block.tobytes(), state.ring.tobytes(), rss.block.tobytes(), rss.hist.tobytes())
    # the other sample format on an open slot: nothing appended, status 3
    nt, no, stt = srs.push_rs_host(state, rss, [0], [0], [10], [0], np.zeros((1, 10 * ch), np.float32))
    assert (nt[0], stt[0]) == (0, srs.STATUS_FORMAT) and rss.in_received(0) == 200
    # appending without producing until the history is full: the clamp drops frames, no needed frame is overwritten
    off, statuses = 200, []
    while off < n and 1 not in statuses:
        nt, no, stt = push(0, p.Ain, 0, off)
        off += int(nt[0])
        statuses.append(int(stt[0]))
    assert statuses[-1] == 1 and nt[0] < p.Ain and off == p.keep(264) + p.hcap
    got = [a, b]
    while True:
        nt, no, stt = push(srs.FLUSH, 0, SP.C)
        if no[0] == 0:
            break
        got.append(cases.read_ring(state, 0, int(no[0])))
    full = cases.offline(p, x[:off * ch], off)
    assert np.concatenate(got).tobytes() == full.tobytes() and state.received(0) == p.out_len(off)
    # FLUSH twice is idempotent
    before = (state.block.tobytes(), state.ring.tobytes(), rss.block.tobytes(), rss.hist.tobytes())
    assert push(srs.FLUSH, 0, SP.C)[1][0] == 0
    assert before == (state.block.tobytes(), state.ring.tobytes(), rss.block.tobytes(), rss.hist.tobytes())
    # BEGIN on a used slot forgets both blocks
    state.block[0, 2:8] = 7
    nt, no, stt = push(st.BEGIN, 3, 5)
    assert rss.in_received(0) == 3 and state.received(0) == 0 and not state.block[0, 2:].any() and not rss.block[0, 3:].any()


def test_hcap_is_enough_for_every_plan():
    """the walk inside StreamResamplePlan asserts; here it is asked for its count, for every accepted plan of the resampler's
    own cases and the plans above, and for two stream plans"""
    names = set()
    for r in rc.RATES:
        names |= {(r, q) for q in rc.QUALITIES}
    for name in list(cases.PLANS) + [cases.DIRECT[0]]:
        names.add((cases.rplan(name).sr_in, cases.rplan(name).quality))
    for r in (8000, 11025, 12000, 22050, 32000, 44100, 48000, 96000, 16001, 15999):
        names |= {(r, 'best'), (r, 'fast')}
    checked, sps = 0, (SP, st.StreamPlan())
    for sr_in, quality in sorted(names):
        try:
            rp = rs.ResamplePlan(sr_in, 16000, quality)
        except ValueError:
            continue
        for sp in sps:
            p = srs.StreamResamplePlan(sp, rp, 1)
            assert p._walk() == 0 and p.hcap % 4 == 0 and 2 * p.W + p.Ain <= p.hcap < 2 * p.W + p.Ain + 4
            small = srs.StreamResamplePlan.__new__(srs.StreamResamplePlan)
            small.__dict__.update(p.__dict__)
            small.hcap = 2 * p.W + p.Ain - 2
            assert p.W == 0 or small._walk() > 0                                 # two entries fewer and frames would be dropped
            checked += 1
    assert checked >= 30


def test_the_argument_struct_has_the_size_of_the_header(tmp_path):
    """tests/test_abi.py probes the older structs; this one is probed here, with the same gcc-compiled program"""
    import ctypes
    import subprocess
    from qasr import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probe = tmp_path / 'probe.c'
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qasr.h"\nint main(){printf("%zu %zu %zu %d\\n",'
                     'sizeof(qasr_stream_rs_push_args),offsetof(qasr_stream_rs_push_args, state),'
                     'offsetof(qasr_stream_rs_push_args, pitch),(int)QASR_STREAM_FLUSH);return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(root, 'include'), str(probe), '-o', str(exe)], check=True)
    sizes = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    A = engine.StreamRsPushArgs
    assert sizes == [ctypes.sizeof(A), A.state.offset, A.pitch.offset, srs.FLUSH]


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


def facade_pcm(rate, ch, lens_s=(1.9, 3.1), seed=8):
    """int16 PCM [2][S * ch] at `rate`: the synthetic speech-like audio of the plain façade tests, resampled down or up by
    the offline twin's own `best` plan where the rate differs, then spread over the channels with different gains"""
    from qasr import synth
    a = synth.make_audio(2, int(max(lens_s) * 16000), seed=seed)
    lens = [int(s * rate) for s in lens_s]
    S = max(lens)
    t = np.arange(S) * (16000.0 / rate)
    mono = np.stack([np.interp(t, np.arange(a.shape[1]), a[i]) for i in range(2)])
    x = np.zeros((2, S, ch), dtype=np.int16)
    for c in range(ch):
        x[:, :, c] = np.clip(mono * (0.9 - 0.2 * c) * 32767, -32768, 32767).astype(np.int16)
    return x.reshape(2, S * ch), lens


def play(m, x, lens, piece, ch=1, device='cpu', **kw):
    """both streams side by side in pieces of `piece` frames; returns (hypotheses, updates per stream incl. those of close())"""
    sess = m.stream(max_streams=2, **KW, **kw)
    slots = [sess.open() for _ in lens]
    ups = {s: [] for s in slots}
    xt = torch.from_numpy(x).to(device)
    for off in range(0, max(lens), piece):
        live = [j for j in range(len(lens)) if off < lens[j]]
        n = [min(piece, lens[j] - off) for j in live]
        for u in sess.push([slots[j] for j in live], xt[live, off * ch:(off + max(n)) * ch], torch.tensor(n)):
            ups[u.slot].append(u)
    hyps = []
    for s in slots:
        hyps.append(sess.close(s))
        ups[s] += sess.closing_updates
    sess.close_all()
    return [dataclasses.astuple(h) for h in hyps], [[dataclasses.astuple(u) for u in ups[s]] for s in slots]


@pytest.mark.parametrize('mode,rate,ch', [('host', 8000, 1), ('dynamic', 8000, 1), ('host', 48000, 2)])
def test_facade_equals_the_session_at_the_models_rate_on_the_offline_output(mode, rate, ch):
    torch.set_grad_enabled(False)
    m = _model(mode)
    x, lens = facade_pcm(rate, ch)
    plan = rs.ResamplePlan(rate, 16000, m.resample_quality)
    y, yl = rs.resample_host(x, lens, plan, ch)
    want = play(m, y, [int(v) for v in yl], 7000)
    assert sum(len(h[0]) for h in want[0]) > 0                                   # at least one label is emitted
    for piece in (int(0.033 * rate), int(0.5 * rate), int(1.7 * rate)):
        got = play(m, x, lens, piece, ch=ch, input_rate=rate, channels=ch)
        assert got == want, piece


def test_the_models_rate_mono_is_todays_session():
    torch.set_grad_enabled(False)
    m = _model('host')
    audio, lens = sc.facade_audio(), sc.FACADE_LENS
    sess = m.stream(max_streams=2, input_rate=16000, channels=1, **KW)
    assert sess.rs_plan is None
    sess.close_all()
    assert play(m, audio, lens, 9000, input_rate=16000, channels=1) == play(m, audio, lens, 9000)


def test_refusals_by_name():
    torch.set_grad_enabled(False)
    m = _model('host')
    with pytest.raises(ValueError, match='input_rate 500'):
        m.stream(input_rate=500)
    with pytest.raises(ValueError, match='input_rate 16001.*table'):
        m.stream(input_rate=16001)
    with pytest.raises(ValueError, match='channels'):
        m.stream(input_rate=8000, channels=9)
    with pytest.raises(ValueError, match='channels'):
        m.stream(channels=2)
    with pytest.raises(ValueError, match='sample_rate.*input_rate='):
        m.stream(sample_rate=8000)
    sess = m.stream(max_streams=2, input_rate=8000, channels=2, **KW)
    s = sess.open()
    assert sess.push([s], torch.zeros(1, 200, dtype=torch.int16), torch.tensor([100])) == []
    with pytest.raises(ValueError, match='sample format'):
        sess.push([s], torch.zeros(1, 200), torch.tensor([100]))
    with pytest.raises(ValueError, match='channels'):
        sess.push([s], torch.zeros(1, 201, dtype=torch.int16), torch.tensor([100]))
    with pytest.raises(ValueError, match='lengths'):
        sess.push([s], torch.zeros(1, 200, dtype=torch.int16), torch.tensor([101]))
    t = sess.open()
    assert sess.push([t], torch.zeros(1, 200), torch.tensor([100])) == []       # another slot may carry the other format
    from qasr import ctc
    assert isinstance(sess.close(s), ctc.Hypothesis) and isinstance(sess.close(t), ctc.Hypothesis)
    sess.close_all()
