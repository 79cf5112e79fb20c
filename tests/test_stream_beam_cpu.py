"""The streaming beam search on the host (qasr.stream_beam): any slicing of a stream equals the whole-stream statement on
every byte; with a lag beyond the stream it is qasr.beam's offline search; with one candidate per frame the committed
labels are the greedy collapse; the committed text is a prefix of every later beam; ring and pitches hold over the walked
protocol; and an independent float64 lagged search holds the twin's best string."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_beam_cases as cases  # noqa: E402
from qasr import beam as qb  # noqa: E402
from qasr import ctc as qc  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402

_lms = {}


def _lm(golden_dir, name):
    if name not in _lms:
        _lms[name] = cases.load_lm(golden_dir, name)
    return _lms[name]


def _cands(lp, N):
    cid, cq = qb.topn_host(lp[None], N)
    return cid[0], cq[0]


# (what, model, alpha, beta, classes): no model, a word-mode and a character-mode model
MODES = (('none', None, 0.0, 0.0), ('en3', 'en3', 0.7, 1.0), ('zh2', 'zh2', 1.5, 0.5))


def _stream(mode, seed, T, golden_dir):
    what, model, alpha, beta = mode
    if model is None:
        return cases.stream_logp(seed, T), None, 0.0, 0.0
    return cases.lm_stream_logp(model, seed, T), _lm(golden_dir, model), alpha, beta


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('W,N,lag', [(1, 20, 7), (3, 64, 0), (16, 20, 40), (16, 1, 7), (128, 20, 40)])
def test_any_slicing_equals_the_whole_stream(mode, W, N, lag, golden_dir):
    T = 200 if W == 128 else 300
    lp, lm, alpha, beta = _stream(mode, 7 + W + lag, T, golden_dir)
    blank = lp.shape[1] - 1
    cid, cq = _cands(lp, N)
    kw = dict(blank=blank, beam_width=W, n_best=min(W, 3), lm=lm, alpha=alpha, beta=beta, lag=lag)
    whole = sb.lagged_search_host(cid, cq, T, **kw)
    a = sb.lagged_search_host(cid, cq, T, cuts=cases.cuts_of(cases.STEP_LENS_A, T), **kw)
    b = sb.lagged_search_host(cid, cq, T, cuts=cases.cuts_of(cases.STEP_LENS_B, T), **kw)
    assert whole == a and whole == b
    assert whole.frames == sorted(set(whole.frames)) and len(whole.frames) == len(whole.labels)      # creation frames rise
    assert whole.hyps[0][0] == whole.labels and 0 < whole.commit_len_before_end <= len(whole.labels)


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('W,N', [(1, 20), (3, 20), (16, 64), (128, 20)])
def test_a_lag_beyond_the_stream_is_the_offline_search(mode, W, N, golden_dir):
    T = 200
    lp, lm, alpha, beta = _stream(mode, 31 + W, T, golden_dir)
    blank = lp.shape[1] - 1
    cid, cq = _cands(lp, N)
    off = qb.beam_search_host(cid[None], cq[None], None, blank, W, W, lm, alpha, beta)
    for lag in (T, T + 100):
        r = sb.lagged_search_host(cid, cq, T, blank, W, W, lm, alpha, beta, lag=lag, cuts=cases.cuts_of(cases.STEP_LENS_A, T))
        assert r.commit_len_before_end == 0 and len(r.hyps) == int(off.n_hyps[0])
        for h, (labs, sc, lmt) in enumerate(r.hyps):
            assert labs == off.labels[0, h, :off.n_labels[0, h]].tolist() and sc == int(off.score[0, h]), (lag, h)
            assert lm is None or lmt == int(off.lm_score[0, h])
    # the batch form: END rows on every byte (labels at pitch F, the rest equal as arrays)
    plan = sb.StreamBeamPlan(W, W, N, T, T)
    st = sb.StreamBeamState(1, plan)
    row = sb.advance_host(st, 0, cid, cq, 0, 0, T, True, True, blank, lm, *sb._weights(lm, alpha, beta, blank))
    assert [x[1] for x in row.end] == off.score[0, :len(row.end)].tolist()


@pytest.mark.parametrize('lag', [0, 7, 40, 400])
@pytest.mark.parametrize('W', [1, 16])
def test_one_candidate_per_frame_commits_the_greedy_collapse(W, lag):
    """N = 1: whatever the lag and the rounds do, the concatenated deltas are collapse_host of the final frames and the
    creation frames are the runs' first frames.  This check does not rest on the twin."""
    T = 300
    lp = cases.stream_logp(90 + lag, T)
    blank = lp.shape[1] - 1
    cid, cq = _cands(lp, 1)
    r = sb.lagged_search_host(cid, cq, T, blank, W, 1, lag=lag, cuts=cases.cuts_of(cases.STEP_LENS_B, T))
    want = qc.collapse_host(lp.argmax(1)[None].astype(np.int32), lp.max(1)[None], None, blank)
    n = int(want.n_labels[0])
    assert n > 20 and r.labels == want.labels[0, :n].tolist() and r.frames == want.start[0, :n].tolist()


def test_the_committed_text_is_a_prefix_of_every_later_beam():
    """stepped frame by frame so that every beam is seen; the ring (F = Lg + K rows) wraps more than four times"""
    W, N, lag, T = 16, 20, 7, 400
    lp = cases.stream_logp(5, T)
    blank = lp.shape[1] - 1
    cid, cq = _cands(lp, N)
    plan = sb.StreamBeamPlan(W, 4, N, lag, 1)
    assert T >= 4 * plan.F and plan.F == lag + sb.K_ROUND
    st = sb.StreamBeamState(1, plan)
    committed, lens = [], []
    for t in range(T):
        row = sb.advance_host(st, 0, cid, cq, 0, t, t + 1, t == 0, t == T - 1, blank)
        committed += row.labels
        assert row.commit_len == len(committed) and len(row.labels) <= plan.delta_pitch
        lens.append(row.commit_len)
        e, commit, done = st.load(0, None)
        assert done == t + 1 and len(e) == row.n_live >= 1
        for i in range(len(e)):                                     # the twin's own trail holds every node ever made
            full = sb._full_labels(st.trail[0], int(e.node[i]))
            assert full[:commit] == committed[:commit] and len(full) == int(e.ln[i]) and len(full) - commit <= plan.F
        if row.end is None:
            assert len(row.tail) <= plan.tail_pitch
        else:
            assert len(row.end) == 4 and all(len(x[0]) <= plan.end_pitch for x in row.end) and row.end[0][0] == row.labels
    assert lens == sorted(lens) and lens[-1] > lens[0]


def test_plan_sizes_and_refusals():
    p = sb.StreamBeamPlan(16, 2, 40, 200, 60)
    assert (p.F, p.end_pitch, p.tail_pitch, p.delta_pitch) == (232, 232, 232, 292)
    assert sb.state_bytes(5, 16, 232) == 5 * 4 * (16 + 20 * 16 + 2 * 232 * 16)
    from qasr import stream as qs
    sp = qs.StreamPlan(0.96, 4.0, 0.96)
    bp = sb.StreamBeamPlan.for_stream(sp, sb.StreamBeam())
    assert bp.Lg == 200 and bp.max_final_frames == sp.max_final_frames and bp.W == 16 and bp.N == 40
    for kw in (dict(width=0), dict(width=129), dict(cutoff_top_n=0), dict(cutoff_top_n=65), dict(n_best=0), dict(n_best=17),
               dict(lag_frames=-1), dict(max_final_frames=0), dict(K=0)):
        with pytest.raises(ValueError):
            sb.StreamBeamPlan(**kw)
    for lag in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            sb.StreamBeamPlan.for_stream(sp, sb.StreamBeam(lag_s=lag))


def test_statuses_leave_the_state_alone():
    from qasr import stream as qs
    sp = qs.StreamPlan(95 * 320 / 16000, 5 * 320 / 16000, 1 * 320 / 16000, 16000, 320)
    W, N = 3, 20
    bp = sb.StreamBeamPlan(W, 2, N, 7, sp.max_final_frames)
    S = 3
    ss, bs = qs.StreamState(S, sp), sb.StreamBeamState(S, bp)
    lp = cases.stream_logp(3, sp.Tw)
    cid, cq = _cands(lp, N)
    blank = lp.shape[1] - 1
    recv = lambda slot, r, done: (ss.block[slot, 0:2].view(np.int64).__setitem__(0, r), ss.block[slot].__setitem__(2, done))
    recv(0, 10 ** 6, 0), recv(1, 10 ** 6, 0), recv(2, 10 ** 6, 0)
    step = lambda slots, flags, enc, first: sb.step_batch_host(bs, ss, slots, flags, np.stack([cid] * len(slots)),
                                                               np.stack([cq] * len(slots)), enc, first, blank)
    o = step([0, 1], [qs.BEGIN, qs.BEGIN], [40, 40], [0, 0])
    assert o.status.tolist() == [0, 0] and bs.header(0)[2] == 40
    ss.block[0, 2] = ss.block[1, 2] = 40
    before = bs.block.copy()
    ss.block[1, 2] = 41                                             # the stream block ran ahead of the beam block
    o = step([7, 0, 1], [0, 0, 0], [40, 40, 60], [0, 41, 0])
    assert o.status.tolist() == [sb.STATUS_SLOT, sb.STATUS_GAP, sb.STATUS_SYNC] and bs.block.tobytes() == before.tobytes()
    assert o.n_new_labels.tolist() == [0, 0, 0] and (o.labels == blank).all() and (o.end_score == qb.NEG).all()
    big = sb.StreamBeamPlan(128, 1, N, 7, sp.max_final_frames)
    bs2 = sb.StreamBeamState(S, big)
    recv(2, 10 ** 12, 2 ** 24)                                       # hi * W passes 2^31 - 1
    bs2.block[2, 2], bs2.block[2, 3] = 2 ** 24, 1
    before = bs2.block.copy()
    o = sb.step_batch_host(bs2, ss, [2], [0], cid[None], cq[None], [40], [2 ** 24], blank)
    assert o.status.tolist() == [sb.STATUS_NODES] and bs2.block.tobytes() == before.tobytes()


def test_a_dead_beam_stays_dead():
    """a frame without a live candidate (every slot empty) kills the beam; END then reports no hypothesis, as offline"""
    W, N, T = 3, 20, 100
    lp = cases.stream_logp(4, T)
    blank = lp.shape[1] - 1
    cid, cq = _cands(lp, N)
    cid, cq = cid.copy(), cq.copy()
    cid[50], cq[50] = -1, qb.EMPTY_Q
    off = qb.beam_search_host(cid[None], cq[None], None, blank, W, W)
    r = sb.lagged_search_host(cid, cq, T, blank, W, W, lag=7, cuts=[40, 60])
    assert int(off.n_hyps[0]) == 0 and r.hyps == [] and len(r.labels) == r.commit_len_before_end > 0


@pytest.mark.parametrize('name', [s[0] for s in cases.ORACLE_LISTS])
def test_the_float64_oracle_holds_the_best_string(name):
    n_waived = 0
    for lp, blank, W, N, lag, best, gap in cases.checked_oracle_list(name):
        cid, cq = _cands(lp, N)
        r = sb.lagged_search_host(cid, cq, lp.shape[0], blank, W, 1, lag=lag, check=False)
        if tuple(r.hyps[0][0]) != tuple(best):
            assert gap < cases.GAP, (name, lag, gap)
            n_waived += 1
    assert n_waived <= cases.MAX_WAIVED * len(cases.checked_oracle_list(name))


# ---------------------------------------------------------------------------------------------------------- the façade
torch = pytest.importorskip('torch')
import stream_cases as sc  # noqa: E402

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


def _facade_lm(m):
    """a word-mode model over the synthetic model's own vocabulary (the English letters, in the decoder's order)"""
    from qasr import ngram
    import beam_lm_cases
    assert sorted(m.decoder.vocabulary) == sorted(beam_lm_cases.EN_VOCAB)
    return ngram.NgramLM.from_arpa(beam_lm_cases.model_path(cases.GOLDEN, 'en3'), m.decoder.vocabulary)


@pytest.mark.parametrize('mode,with_lm,n_best,lag_s', [('host', False, 1, 0.3), ('host', True, 3, 0.3), ('dynamic', False, 2, 100.0)])
def test_facade_on_cpu_tensors_is_the_composition(mode, with_lm, n_best, lag_s):
    torch.set_grad_enabled(False)
    m = _model(mode)
    lm = _facade_lm(m) if with_lm else None
    beam = sb.StreamBeam(width=8, n_best=n_best, cutoff_top_n=20, lm=lm, alpha=0.5, beta=0.5, lag_s=lag_s)
    audio, lens = sc.facade_audio()[:, :50000], [20000, 50000]                   # 6 chunks and END; rounds every 0.64 s
    plan, bplan, want = cases.compose_on_host(m, audio, lens, beam, **KW)
    results = []
    for piece in (1000, 15360, 50000):
        slots, ups, hyps, _, _ = cases.play_session(m, audio, lens, piece, beam, **KW)
        cases.check_against_composition(m, slots, ups, hyps, want, beam)
        results.append((repr(hyps), repr([ups[s] for s in slots])))
    assert results[0] == results[1] == results[2]                                # however the audio was sliced
    if lag_s < 1:
        assert any(int(w['n_new_labels']) > 0 for w in want[1][:-1])             # text was committed before END
    else:                                                                        # no round fires: decode(beam_width=) of the final frames
        assert all(int(w['n_new_labels']) == 0 for w in want[1][:-1])
    if with_lm:
        hyp = m.decode_stream(torch.from_numpy(audio), torch.tensor(lens), beam=beam, **KW)
        assert repr(hyp) == repr(hyps)


def test_facade_refusals():
    """beam_width= stays refused by name and now points to beam=; boost is refused by name; ranges are _beam_args's"""
    m = _model('host')
    with pytest.raises(ValueError, match='beam_width.*beam='):
        m.stream(beam_width=4)
    with pytest.raises(ValueError, match='boost'):
        m.stream(beam=sb.StreamBeam(), boost=object())
    for kw, name in ((dict(width=0), 'beam_width'), (dict(width=129), 'beam_width'), (dict(cutoff_top_n=65), 'cutoff_top_n'),
                     (dict(n_best=17), 'n_best'), (dict(lag_s=-1.0), 'lag_s'), (dict(lag_s=float('nan')), 'lag_s')):
        with pytest.raises(ValueError, match=name):
            m.stream(beam=sb.StreamBeam(**kw))
    with pytest.raises(ValueError, match='alpha|weights|0 ..'):
        m.stream(beam=sb.StreamBeam(lm=_facade_lm(m), alpha=17.0))
    with pytest.raises(ValueError, match='StreamBeam'):
        m.stream(beam=16)
