"""Streaming phrase boosting on the host (qasr.stream_beam with boost=, STREAM_BOOST_RULES): any slicing of a boosted stream
equals the whole-stream statement on every byte, the state block and the ring included; with a lag beyond the stream it is
qasr.beam's offline boosted search; boost_tot of every final hypothesis is the brute-force substring sum over its WHOLE text,
however much of it was committed early; weight 0 and set 0 are the unboosted search; sets are per slot; and the façade."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boost_cases  # noqa: E402
import stream_beam_cases as sbc  # noqa: E402
import stream_boost_cases as cases  # noqa: E402
from qasr import beam as qb  # noqa: E402
from qasr import boost as qboost  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402

_lms = {}


def _lm(golden_dir, name):
    if name not in _lms:
        _lms[name] = sbc.load_lm(golden_dir, name)
    return _lms[name]


def _cands(lp, N):
    cid, cq = qb.topn_host(lp[None], N)
    return cid[0], cq[0]


MODES = (('none', None, 0.0, 0.0), ('en3', 'en3', 0.7, 1.0), ('zh2', 'zh2', 1.5, 0.5))


def _stream(mode, seed, T, golden_dir):
    what, model, alpha, beta = mode
    if model is None:
        return sbc.stream_logp(seed, T), None, 0.0, 0.0
    return sbc.lm_stream_logp(model, seed, T), _lm(golden_dir, model), alpha, beta


def _space(blank):
    return boost_cases.EN_SPACE if blank == 28 else -1


# ------------------------------------------------------------------------------------------------------------- slicing
@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('lag', [0, 7, 40, 100])
@pytest.mark.parametrize('N', [1, 20])
@pytest.mark.parametrize('W', [1, 3, 16])
def test_any_slicing_of_a_boosted_stream_equals_the_whole_stream(W, N, lag, mode, golden_dir):
    """labels, frames, scores, boost_tot of the steps against lagged_search_host(boost=); the state block and the ring
    after every step against the run cut at the union of both schedules' edges (the twin's own assertions stay on); and
    boost_tot of every final hypothesis against the brute-force substring sum over its whole text"""
    T = 512
    lp, lm, alpha, beta = _stream(mode, 7 + W + lag, T, golden_dir)
    blank = lp.shape[1] - 1
    space = _space(blank)
    cid, cq = _cands(lp, N)
    nb = min(W, 3)
    ea, eb = (sbc.edges_of(sbc.cuts_of(s, T), T) for s in (sbc.STEP_LENS_A, sbc.STEP_LENS_B))
    n_sets = 0
    for kind in cases.SET_KINDS:
        ph, whole = cases.phrases_of(kind, 100 * W + lag, lp, blank, space)
        if ph is None:                                              # whole words without a space label: PhraseSet refuses
            assert space < 0
            with pytest.raises(ValueError, match='whole_words'):
                cases.make_set([((0, 1), 1.0)], True, blank, space)
            continue
        n_sets += 1
        bs = cases.make_set(ph, whole, blank, space)
        whole_r = sb.lagged_search_host(cid, cq, T, blank, W, nb, lm, alpha, beta, lag=lag, boost=bs, check=True)
        ref = cases.run_steps(cid, cq, T, sorted(set(ea) | set(eb)), blank, W, nb, lag, lm, alpha, beta, bs)
        for edges in (ea, eb):
            labels, frames, end, blocks, commits = cases.run_steps(cid, cq, T, edges, blank, W, nb, lag, lm, alpha, beta, bs)
            assert labels == whole_r.labels and frames == whole_r.frames
            head = labels[:whole_r.commit_len_before_end]
            assert [(head + x[0],) + tuple(x[1:]) for x in end] == whole_r.hyps
            for edge, blk in blocks.items():                        # header, entries (bst, boost_tot, pad) and ring
                assert blk.tobytes() == ref[3][edge].tobytes(), (kind, edge)
            assert commits == sorted(commits)
        brute = cases.brute_of(ph, whole, space)
        assert len(whole_r.hyps) >= 1
        for labs, sc, lmt, bt in whole_r.hyps:
            assert bt == brute.final(labs) == bs.score(labs), (kind, labs)
            assert lm is not None or lmt == 0
        if lag < 100:
            assert 0 < whole_r.commit_len_before_end                # text was committed before END
    assert n_sets == (3 if space >= 0 else 2)


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('W,N', [(1, 20), (3, 20), (16, 20)])
def test_a_lag_beyond_the_stream_is_the_offline_boosted_search(mode, W, N, golden_dir):
    T = 200
    lp, lm, alpha, beta = _stream(mode, 31 + W, T, golden_dir)
    blank = lp.shape[1] - 1
    space = _space(blank)
    cid, cq = _cands(lp, N)
    for kind in ('random', 'nested_plain'):
        ph, whole = cases.phrases_of(kind, 5 + W, lp, blank, space)
        bs = cases.make_set(ph, whole, blank, space)
        off = qb.beam_search_host(cid[None], cq[None], None, blank, W, W, lm, alpha, beta, boost=bs)
        for lag in (T, T + 100):
            r = sb.lagged_search_host(cid, cq, T, blank, W, W, lm, alpha, beta, lag=lag, cuts=sbc.cuts_of(sbc.STEP_LENS_A, T), boost=bs)
            assert r.commit_len_before_end == 0 and len(r.hyps) == int(off.n_hyps[0]) >= 1
            for h, (labs, sc, lmt, bt) in enumerate(r.hyps):
                assert labs == off.labels[0, h, :off.n_labels[0, h]].tolist(), (lag, h)
                assert sc == int(off.score[0, h]) and bt == int(off.boost_score[0, h])
                assert lmt == (0 if lm is None else int(off.lm_score[0, h]))


# --------------------------------------------------------------------------------------------------- independent checks
LAG_LISTS = ('en_t63_w16_n40', 'en_t250_w16_n20', 'zh_t63_w16_n40')
MAX_LAG_LOST = 1 / 8           # the share of cases in which a lag of 200 frames may lose the offline best (see below)


def test_the_float64_boosted_oracle_holds_the_best_string_at_lag_200():
    """boost_cases' float64 boosted search (no trie, no state, no fixed point) against the twin at a lag of 200 frames.
    A case whose float64 top-1 / top-2 gap is below GAP is waived as in test_boost_cpu (at most MAX_WAIVED of a list: the
    generator asserts that on the oracle alone).  A lag can lose the offline best: a round drops every entry whose old
    labels differ from the best entry's of that moment.  The lists of T = 63 see no round at all (the first is at frame
    223), the T = 250 list sees one, with the horizon at frame 23; the condition is that at most 1 case in 8 over all lists
    differs for that reason."""
    total = lost = 0
    for name in LAG_LISTS:
        waived = 0
        for lp, blank, W, N, phrases, whole, space, o, gap, plain in boost_cases.checked_case_list(name):
            bs = cases.make_set(phrases, whole, blank, space)
            cid, cq = _cands(lp, N)
            r = sb.lagged_search_host(cid, cq, lp.shape[0], blank, W, 1, lag=200, boost=bs, check=False)
            total += 1
            labs, sc, lmt, bt = r.hyps[0]
            assert bt == boost_cases.Brute(phrases, whole, space).final(labs)
            if tuple(labs) != tuple(o[0][0]):
                if gap < boost_cases.GAP:
                    waived += 1
                else:
                    lost += 1
        assert waived <= boost_cases.MAX_WAIVED * len(boost_cases.checked_case_list(name))
    assert total >= 20 and lost <= MAX_LAG_LOST * total, (lost, total)


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('W,N,lag', [(3, 20, 0), (16, 20, 40)])
def test_weight_0_and_set_0_are_the_unboosted_search(mode, W, N, lag, golden_dir):
    """every byte that the boosted layout shares with the plain one: header (but word 4), the eight 64-bit and four 32-bit
    arrays, the ring; the outputs; boost_tot, bst's terms and the pad are 0"""
    T = 300
    lp, lm, alpha, beta = _stream(mode, 77 + W, T, golden_dir)
    blank = lp.shape[1] - 1
    space = _space(blank)
    cid, cq = _cands(lp, N)
    edges = sbc.edges_of(sbc.cuts_of(sbc.STEP_LENS_B, T), T)
    plain = cases.run_steps(cid, cq, T, edges, blank, W, min(W, 3), lag, lm, alpha, beta, None)
    ph, whole = cases.phrases_of('random', 9, lp, blank, space)
    zero = cases.make_set([(p, 0.0) for p, _ in ph], whole, blank, space)
    hot = cases.make_set(ph, whole, blank, space)

    def shared(blk):
        hdr, ent = sb.HDR_WORDS, blk[0, sb.HDR_WORDS:sb.HDR_WORDS + 24 * W]
        return np.concatenate([blk[0, :4], blk[0, 5:hdr], ent[:16 * W], ent[18 * W:22 * W], blk[0, hdr + 24 * W:]])

    def plain_shared(blk):
        hdr = sb.HDR_WORDS
        return np.concatenate([blk[0, :4], blk[0, 5:hdr], blk[0, hdr:hdr + 20 * W], blk[0, hdr + 20 * W:]])

    # weight 0: the set's states move, every term is 0
    z = cases.run_steps(cid, cq, T, edges, blank, W, min(W, 3), lag, lm, alpha, beta, zero)
    assert z[0] == plain[0] and z[1] == plain[1] and [x[:3] for x in z[2]] == plain[2] and all(x[3] == 0 for x in z[2])
    for edge in edges[1:]:
        assert shared(z[3][edge]).tobytes() == plain_shared(plain[3][edge]).tobytes()
        ent = z[3][edge][0, sb.HDR_WORDS:sb.HDR_WORDS + 24 * W]
        assert not ent[16 * W:18 * W].any() and not ent[23 * W:].any() and z[3][edge][0, 4] == 1
    # set 0 (boost_set -1) in a boosted session: no state moves either
    plan = sb.StreamBeamPlan(W, min(W, 3), N, lag, T, boost=True)
    st = sb.StreamBeamState(1, plan)
    aq, bq = sb._weights(lm, alpha, beta, blank)
    labels, frames = [], []
    for i in range(len(edges) - 1):
        row = sb.advance_host(st, 0, cid, cq, 0, edges[i], edges[i + 1], i == 0, i == len(edges) - 2, blank, lm, aq, bq, [hot], -1)
        labels += row.labels
        frames += row.frames
        assert shared(st.block).tobytes() == plain_shared(plain[3][edges[i + 1]]).tobytes()
        ent = st.block[0, sb.HDR_WORDS:sb.HDR_WORDS + 24 * W]
        assert not ent[16 * W:18 * W].any() and not ent[22 * W:].any() and st.block[0, 4] == 0
    assert labels == plain[0] and frames == plain[1] and [x[:3] for x in row.end] == plain[2] and all(x[3] == 0 for x in row.end)


def test_a_boost_that_matters_crosses_a_commit():
    """The unboosted lagged search returns A; boosting a piece of a runner-up (boost_cases.differing_piece) makes it return B,
    which holds the phrase; the lag (3 frames) is shorter than the phrase's span in frames and a round commits SOME of the
    phrase's labels and not the rest, so the provisional pot crossed a commit - and boost_tot is still the exact
    brute-force sum at END."""
    T, W, N, lag, seed = 256, 16, 20, 3, 129
    lp = sbc.stream_logp(seed, T)
    blank = lp.shape[1] - 1
    cid, cq = _cands(lp, N)
    A = sb.lagged_search_host(cid, cq, T, blank, W, W, lag=lag)
    a = A.hyps[0][0]
    rng = np.random.Generator(np.random.PCG64(seed))
    piece = None
    for other in A.hyps[1:6]:
        piece = boost_cases.differing_piece(a, other[0], False, -1, rng)
        if piece and len(piece) >= 3:
            break
    assert piece and len(piece) >= 3
    phrases = [(piece, 3.0)]
    bs = cases.make_set(phrases, False, blank, -1)
    edges = list(range(0, T, sb.K_ROUND)) + [T]                      # a step per round: commit_len after every round
    labels, frames, end, blocks, commits = cases.run_steps(cid, cq, T, edges, blank, W, W, lag, boost=bs)
    B = sb.lagged_search_host(cid, cq, T, blank, W, W, lag=lag, boost=bs)
    assert labels == B.labels == B.hyps[0][0] and labels != a
    occ = [i for i in range(len(labels) - len(piece) + 1) if tuple(labels[i:i + len(piece)]) == tuple(piece)]
    assert occ and not any(tuple(a[i:i + len(piece)]) == tuple(piece) for i in occ)
    inside = [(i, c) for i in occ for c in commits[:-1] if i < c < i + len(piece)]
    assert inside, (occ, commits)                                    # a round fired inside an occurrence
    i = inside[0][0]
    assert frames[i + len(piece) - 1] - frames[i] > lag              # the phrase spans more frames than the lag
    brute = boost_cases.Brute(phrases, False, -1)
    for labs, sc, lmt, bt in B.hyps:
        assert bt == brute.final(labs)
    assert B.hyps[0][3] >= len(occ) * 3 * len(piece) * boost_cases.ONE > 0
    assert B.hyps[0][1] > A.hyps[0][1]                               # the boosted score carries the bonus


# ------------------------------------------------------------------------------------------------------- per-slot sets
def test_sets_per_slot_header_word_and_status_5():
    from qasr import stream as qs
    sp = qs.StreamPlan(95 * 320 / 16000, 5 * 320 / 16000, 1 * 320 / 16000, 16000, 320)
    W, N, lag = 3, 20, 7
    bp = sb.StreamBeamPlan(W, 2, N, lag, sp.max_final_frames, boost=True)
    assert bp.slot_words == 16 + 24 * W + 2 * bp.F * W == sb.slot_words(W, bp.F, True)
    assert sb.state_bytes(5, W, bp.F, True) == 5 * 4 * bp.slot_words and sb.state_bytes(5, W, bp.F) == 5 * 4 * (16 + 20 * W + 2 * bp.F * W)
    S = 4
    ss, bs = qs.StreamState(S, sp), sb.StreamBeamState(S, bp)
    lps = [sbc.stream_logp(40 + k, sp.Tw) for k in range(3)]
    blank = lps[0].shape[1] - 1
    space = boost_cases.EN_SPACE
    cands = [_cands(lp, N) for lp in lps]
    sets = [cases.make_set(*cases.phrases_of('nested_plain', 1, lps[0], blank, space), blank, space),
            cases.make_set(cases.phrases_of('random', 2, lps[1], blank, space)[0], True, blank, space)]
    recv = lambda slot, r, done: (ss.block[slot, 0:2].view(np.int64).__setitem__(0, r), ss.block[slot].__setitem__(2, done))  # noqa: E731
    for s in range(S):
        recv(s, 10 ** 6, 0)

    def step(slots, flags, enc, first, rows, bset):
        return sb.step_batch_host(bs, ss, slots, flags, np.stack([cands[r][0] for r in rows]), np.stack([cands[r][1] for r in rows]),
                                  enc, first, blank, boost=sets, boost_set=bset)

    # three slots in one batch with sets 0 / 1 / none, in two steps of 40 and 55 frames (the second one END)
    o1 = step([2, 0, 1], [qs.BEGIN] * 3, [40] * 3, [0] * 3, [0, 1, 2], [0, 1, -1])
    assert o1.status.tolist() == [0, 0, 0]
    assert [int(bs.block[s, 4]) for s in (2, 0, 1)] == [1, 2, 0]
    for s in (0, 1, 2):
        ss.block[s, 2] = 40
    o2 = step([2, 0, 1], [qs.END] * 3, [95] * 3, [0] * 3, [0, 1, 2], [5, -7, 1])     # not BEGIN: the input is ignored
    assert o2.status.tolist() == [0, 0, 0] and [int(bs.block[s, 4]) for s in (2, 0, 1)] == [1, 2, 0]
    for b, (slot, k) in enumerate(((2, 0), (0, 1), (1, None))):                    # each equals its single-stream run
        one = sb.StreamBeamState(1, bp)
        s1 = qs.StreamState(1, sp)
        s1.block[0, 0:2].view(np.int64)[0] = 10 ** 6
        kw = dict(boost=sets, boost_set=[-1 if k is None else k])
        a = sb.step_batch_host(one, s1, [0], [qs.BEGIN], cands[b][0][None], cands[b][1][None], [40], [0], blank, **kw)
        s1.block[0, 2] = 40
        z = sb.step_batch_host(one, s1, [0], [qs.END], cands[b][0][None], cands[b][1][None], [95], [0], blank, **kw)
        assert one.block[0].tobytes() == bs.block[slot].tobytes()
        for got, want in ((o1, a), (o2, z)):
            for name, v in vars(want).items():
                if v is not None:
                    assert np.array_equal(getattr(got, name)[b], v[0]), name
        if k is None:
            assert not z.end_boost_score.any()
    # BEGIN on a used slot changes the set; a boost_set out of range: status 5, the state untouched
    for s in (0, 1, 2):
        ss.block[s, 2] = 0
    before = bs.block.copy()
    o = step([0, 1, 2], [qs.BEGIN] * 3, [40] * 3, [0] * 3, [0, 1, 2], [2, -2, 8])
    assert o.status.tolist() == [sb.STATUS_SET] * 3 == [5, 5, 5] and bs.block.tobytes() == before.tobytes()
    assert o.n_new_labels.tolist() == [0, 0, 0] and (o.labels == blank).all() and (o.end_score == qb.NEG).all() and not o.end_boost_score.any()
    o = step([0, 1], [qs.BEGIN] * 2, [40] * 2, [0] * 2, [0, 1], [-1, 0])
    assert o.status.tolist() == [0, 0] and [int(bs.block[s, 4]) for s in (0, 1)] == [0, 1]
    with pytest.raises(ValueError, match='phrase sets'):
        sb.as_sets([sets[0]] * 9)
    with pytest.raises(ValueError, match='boost'):
        sb.step_batch_host(sb.StreamBeamState(1, sb.StreamBeamPlan(W, 2, N, lag, sp.max_final_frames)), ss, [0], [qs.BEGIN],
                           cands[0][0][None], cands[0][1][None], [40], [0], blank, boost=sets)


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
    from qasr import ngram
    import beam_lm_cases
    return ngram.NgramLM.from_arpa(beam_lm_cases.model_path(sbc.GOLDEN, 'en3'), m.decoder.vocabulary)


@pytest.mark.parametrize('mode,with_lm,n_best,lag_s,named', [('host', False, 1, 0.3, False), ('host', True, 3, 0.3, True),
                                                             ('dynamic', False, 2, 100.0, True)])
def test_facade_on_cpu_tensors_is_the_composition(mode, with_lm, n_best, lag_s, named):
    torch.set_grad_enabled(False)
    m = _model(mode)
    lm = _facade_lm(m) if with_lm else None
    audio, lens = sc.facade_audio()[:, :50000], [20000, 50000]
    words = cases.facade_phrases(m, audio, lens, **KW)
    if named:                                   # two named sets: stream 0 takes 'b' (index 1), stream 1 none
        boost = {'a': [(w, 2.0) for w in words[:2]], 'b': qboost.PhraseSet(words, m.decoder.vocabulary, weight=1.5, whole_words=False)}
        open_boost, set_of = ['b', None], [1, -1]
    else:                                       # one set: stream 0 uses it, stream 1 opts out
        boost, open_boost, set_of = [(w, 2.5) for w in words], [None, False], [0, -1]
    beam = sb.StreamBeam(width=8, n_best=n_best, cutoff_top_n=20, lm=lm, alpha=0.5, beta=0.5, lag_s=lag_s, boost=boost, boost_weight=0.5)
    sess = m.stream(max_streams=2, beam=beam, **KW)
    sets = list(sess.beam.boost.values())       # compiled against the model's vocabulary at stream() time
    assert all(isinstance(s, qboost.PhraseSet) for s in sets) and len(sets) == (2 if named else 1)
    sess.close_all()
    plan, bplan, want = cases.compose_on_host(m, audio, lens, sess.beam, sets, set_of, **KW)
    results = []
    for piece in (1000, 15360, 50000):
        slots, ups, hyps, _, _ = cases.play_session(m, audio, lens, piece, beam, open_boost, **KW)
        cases.check_against_composition(m, slots, ups, hyps, want, beam)
        cases.check_boost_scores(hyps, want, beam)
        results.append((repr(hyps), repr([ups[s] for s in slots])))
    assert results[0] == results[1] == results[2]                                # however the audio was sliced
    first = lambda h: h[0] if n_best > 1 else h                                   # noqa: E731
    assert first(hyps[0]).boost_score is not None and first(hyps[1]).boost_score == 0.0
    assert first(hyps[0]).boost_score > 0.0                                      # the phrases are words of the stream's own text
    if not named:                                                                # decode_stream: one set, every row uses it
        hyp = m.decode_stream(torch.from_numpy(audio), torch.tensor(lens), beam=beam, **KW)
        _, _, want_all = cases.compose_on_host(m, audio, lens, sess.beam, sets, [0, 0], **KW)
        cases.check_boost_scores(hyp, want_all, beam)
        assert repr(hyp[0]) == repr(hyps[0])


def test_facade_refusals():
    m = _model('host')
    ok = ['ab', ('cd', 2.0)]
    # the two pinned refusals still fire
    with pytest.raises(ValueError, match=r'boost.*StreamBeam\(boost='):
        m.stream(beam=sb.StreamBeam(), boost=ok)
    with pytest.raises(ValueError, match='boost'):
        m.stream(boost=ok)                                                       # boost without a beam
    from qasr import stream_ep as qse
    with pytest.raises(ValueError, match='beam= together with endpoint='):
        m.stream(beam=sb.StreamBeam(boost=ok), endpoint=qse.Endpointing())
    # the new ones, all before anything is launched, all carrying the offending name
    nine = {f's{k}': ok for k in range(9)}
    for boost, kw, name in ((nine, {}, r'stream: beam: boost: 9 phrase sets.*MAX_SETS = 8'), ({}, {}, 'stream: beam: boost: .*empty'),
                            (['a#b'], {}, "stream: beam: boost: phrase 0 .*'#'"), ([], {}, 'stream: beam: boost: .*empty'),
                            ({'x': ['ab'], 'y': [('ab', 17.0)]}, {}, r"stream: beam: boost: a weight.*\(set 'y'\)"),
                            ('ab', {}, 'stream: beam: boost: .*not one string'),
                            (ok, dict(boost_weight=16.5), 'stream: beam: boost_weight'), (ok, dict(boost_weight=-0.1), 'boost_weight'),
                            (ok, dict(boost_weight=float('nan')), 'boost_weight'), ({3: ok}, {}, 'stream: beam: boost: the name')):
        with pytest.raises(ValueError, match=name):
            m.stream(beam=sb.StreamBeam(boost=boost, **kw))
    other = qboost.PhraseSet([[0, 1]], n_labels=5)
    with pytest.raises(ValueError, match='stream: beam: boost: .*labels'):
        m.stream(beam=sb.StreamBeam(boost=other))
    # open(boost=)
    with m.stream(max_streams=4, beam=sb.StreamBeam(boost={'x': ok, 'y': ok}), **KW) as sess:
        with pytest.raises(ValueError, match="boost='z'.*no such phrase set"):
            sess.open(boost='z')
        assert [sess._open[sess.open(boost=b)]['boost_set'] for b in ('x', 'y', None, False)] == [0, 1, -1, -1]
    with m.stream(max_streams=2, beam=sb.StreamBeam(boost=ok), **KW) as sess:
        with pytest.raises(ValueError, match="boost='x'"):
            sess.open(boost='x')
        assert [sess._open[sess.open(boost=b)]['boost_set'] for b in (None, False)] == [0, -1]
    for beam in (sb.StreamBeam(), None):
        with m.stream(max_streams=2, beam=beam, **KW) as sess:
            with pytest.raises(ValueError, match="boost='x'.*no phrase set"):
                sess.open(boost='x')
            sess.open()
    # positional construction stays valid: the new fields are the last two
    b = sb.StreamBeam(4, 1, 20, None, 0.0, 0.0, 1.0)
    assert b.boost is None and b.boost_weight == 1.0
    assert [f for f in sb.StreamBeam.__dataclass_fields__][-2:] == ['boost', 'boost_weight']
