"""MBR re-ranking on the host: qasr.mbr.mbr_host against independent statements - edit_host and the metric's _levenshtein for the
distances, an MBR in float64 for the pick (inside the bound MBR_RULES derives), and identities that each pin one rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edit_cases as ec  # noqa: E402
import mbr_cases as mc  # noqa: E402
from qasr import edit, mbr  # noqa: E402

CASES = mc.small_cases()
W_ONE = 1 << 24


def _host(case, mode, scale=1.0, **kw):
    a = dict(case)
    a.update(kw)
    return mbr.mbr_host(a['labels'], a['n_labels'], a['score'], a['n_hyps'], a['C'], mode=mode, is_space=a['is_space'], scale=scale)


def test_weight_table_and_scale():
    t = mbr.weight_table()
    assert t.dtype == np.uint32 and t.shape == (16384,) and t[0] == W_ONE and t[1] == round(np.exp(-64 / 65536) * W_ONE)
    assert (np.diff(t.astype(np.int64)) <= 0).all() and t[-1] == round(np.exp(-64 * 16383 / 65536) * W_ONE) and t[-1] > 0
    assert mbr.check_scale(0, 't') == 0 and mbr.check_scale(1.0, 't') == 1 << 16 and mbr.check_scale(16, 't') == 16 << 16
    for bad in (-0.001, 16.001, float('nan'), None, 'x'):
        with pytest.raises(ValueError, match='mbr_scale must be a number in 0 .. 16'):
            mbr.check_scale(bad, 't')
    for rule in ('score > -2^61', 'x = (d * scale_q + 2^15) >> 16', 'risk ascending, score descending, k ascending', 'MBR_BOUND'):
        assert rule in mbr.MBR_RULES, rule


@pytest.mark.parametrize('mode', ['char', 'word'])
@pytest.mark.parametrize('name,case', CASES, ids=[n for n, _ in CASES])
def test_dist_equals_edit_host_and_the_metric(name, case, mode):
    from nemo.collections.asr.metrics.wer import _levenshtein
    res = _host(case, mode)
    B, K, L = case['labels'].shape
    assert res.dist.dtype == np.int32 and (res.ok == 1).all()
    for b in range(B):
        d = res.dist[b]
        assert (d == d.T).all() and (np.diag(d) == 0).all() and (d >= 0).all()
        for i in range(K):
            # hypothesis rows j against the reference row i, in one call
            e = edit.edit_host(case['labels'][b], case['n_labels'][b], case['labels'][b, i:i + 1], case['n_labels'][b, i:i + 1],
                               case['C'], mode=mode, is_space=case['is_space'], rows_per_ref=K)
            assert e.errors.tolist() == d[i].tolist(), (name, b, i)
        if mode == 'word' and case['C'] == 29:
            voc = ' abcdefghijklmnopqrstuvwxyz\'-'
            text = [''.join(voc[c] for c in case['labels'][b, k, :case['n_labels'][b, k]]).split() for k in range(K)]
            assert [[_levenshtein(text[i], text[j]) for j in range(K)] for i in range(K)] == d.tolist()


@pytest.mark.parametrize('mode', ['char', 'word'])
@pytest.mark.parametrize('scale', [0.0, 0.5, 1.0, 3.0])
def test_pick_against_float64_mbr_inside_the_derived_bound(mode, scale):
    """Seen on these cases: the largest excess is 0 at every scale and in both modes - the integers' pick is a float64 minimiser
    everywhere - against bounds between 1e-9 (an utterance of equal rows) and 0.09 errors (unnormalised, best row's weight 1);
    5 .. 28 of the 31 utterances are decided by their margin.  The test prints the figures."""
    worst, tightest, widest, decided = 0.0, np.inf, 0.0, 0
    sq = mbr.check_scale(scale, 't')
    for name, case in CASES:
        res = _host(case, mode, scale)
        for b in range(case['labels'].shape[0]):
            R, dmax, best = mc.float_mbr(case, b, mode, sq)
            bound = mbr.mbr_bound(R.min(), len(R), dmax) + 1e-9 * (1 + R.min())
            pick = int(res.pick[b])
            excess = R[pick] - R.min()
            worst, tightest, widest = max(worst, excess), min(tightest, bound), max(widest, bound)
            assert excess <= bound, (name, b, excess, bound)
            margin = np.partition(R, 1)[1] - R.min()
            if margin > bound:
                decided += 1
                assert pick == best, (name, b, pick, best, margin, bound)
            ee, post = mbr.expected_errors(res)
            assert abs(ee[b, pick] - R[pick] / np.exp((sq / 65536.0) * (case['score'][b] - case['score'][b].max()) / 65536.0).sum()) \
                <= 2e-3 * (1 + ee[b, pick])
            assert abs(post[b].sum() - 1) < 1e-12
    print(f'mode {mode} scale {scale}: largest excess {worst:.3g}, bounds {tightest:.3g} .. {widest:.3g}, {decided} utterances decided by margin')
    assert decided > 0


@pytest.mark.parametrize('mode', ['char', 'word'])
@pytest.mark.parametrize('name,case', CASES, ids=[n for n, _ in CASES])
def test_identities(name, case, mode):
    B, K, L = case['labels'].shape
    flat = _host(case, mode, 0.0)
    # scale 0: uniform weights, the pick is the medoid
    assert (flat.weight == W_ONE).all() and (flat.wsum == K * W_ONE).all()
    sums = flat.dist.astype(np.int64).sum(axis=2)
    assert (flat.risk == sums * W_ONE).all()
    for b in range(B):
        assert sums[b, flat.pick[b]] == sums[b].min()
    # a gap of more than 16 nats at scale 16 after widening the scores: the best row alone
    far = dict(case, score=case['score'] * 64 - np.arange(K) * (2 << 16))
    alone = _host(far, mode, 16.0)
    best = far['score'].argmax(axis=1)
    for b in range(B):
        assert alone.weight[b].tolist() == [W_ONE * int(k == best[b]) for k in range(K)] and alone.pick[b] == best[b]
        assert (alone.risk[b] == W_ONE * alone.dist[b, :, best[b]].astype(np.int64)).all()
    # the pick's expected errors never exceed row 0's
    for scale in (0.0, 1.0, 16.0):
        res = _host(case, mode, scale)
        ee, _ = mbr.expected_errors(res)
        assert (ee[np.arange(B), res.pick] <= ee[:, 0]).all()
        assert (np.sort(res.order, axis=1) == np.arange(K)).all()
        r = np.take_along_axis(res.risk, res.order.astype(np.int64), axis=1)
        assert (np.diff(r, axis=1) >= 0).all()


def test_equal_rows_order_by_score_then_k():
    row = [3, 4, 0, 5, 6, 0, 7]
    case = mc.from_lists([[row] * 5], [[-50000, -20000, -50000, -10000, -20000]])
    for mode in ('char', 'word'):
        res = _host(case, mode)
        assert (res.risk == 0).all() and (res.dist == 0).all() and res.order.tolist() == [[3, 1, 4, 0, 2]]


@pytest.mark.parametrize('mode', ['char', 'word'])
def test_permuted_and_unsorted_lists(mode):
    case = mc.nbest(71, 29, B=4, K=7, L=28, min_len=12, sort=False)
    res = _host(case, mode)
    g = np.random.default_rng(3)
    for perm in (g.permutation(7), np.argsort(-case['score'][0], kind='stable')):
        moved = dict(case, labels=case['labels'][:, perm], n_labels=case['n_labels'][:, perm], score=case['score'][:, perm])
        got = _host(moved, mode)
        assert (got.weight == res.weight[:, perm]).all() and (got.risk == res.risk[:, perm]).all() and (got.ok == res.ok[:, perm]).all()
        assert (got.dist == res.dist[:, perm][:, :, perm]).all() and (got.wsum == res.wsum).all()
        for b in range(4):
            keys = list(zip(res.risk[b].tolist(), case['score'][b].tolist()))
            if len(set(keys)) == 7:                                 # tie-free: the order maps through the permutation
                assert perm[got.order[b]].tolist() == res.order[b].tolist()


@pytest.mark.parametrize('mode', ['char', 'word'])
def test_present_row_rules(mode):
    case = mc.nbest(41, 29, B=6, K=4, L=20, min_len=6)
    full = _host(case, mode)
    # n_hyps: 0, 1, partial, all; None equals all
    nh = np.array([0, 1, 2, 4, 3, 4], dtype=np.int32)
    res = _host(case, mode, n_hyps=nh)
    assert res.ok.tolist() == [[1] * n + [2] * (4 - n) for n in nh.tolist()]
    assert res.pick.tolist()[:2] == [-1, 0] and res.wsum[0] == 0 and res.order[0].tolist() == [-1] * 4
    assert res.risk[1].tolist() == [0, -1, -1, -1] and res.dist[1].tolist() == [[0, -1, -1, -1]] + [[-1] * 4] * 3
    assert _host(case, mode, n_hyps=np.full(6, 4, dtype=np.int32)).risk.tobytes() == full.risk.tobytes()
    for b in range(6):                                              # the present rows: the call over them alone
        n = int(nh[b])
        if n:
            sub = dict(case, labels=case['labels'][b:b + 1, :n], n_labels=case['n_labels'][b:b + 1, :n], score=case['score'][b:b + 1, :n])
            alone = _host(sub, mode)
            assert (res.risk[b, :n] == alone.risk[0]).all() and (res.order[b, :n] == alone.order[0]).all()
            assert (res.dist[b, :n, :n] == alone.dist[0]).all() and (res.dist[b, n:] == -1).all() and (res.dist[b, :, n:] == -1).all()
    # invalid rows between valid ones: an id equal to C, a length of L + 1, a score of -2^62 inside n_hyps
    bad = dict(case, labels=case['labels'].copy(), n_labels=case['n_labels'].copy(), score=case['score'].copy())
    bad['labels'][0, 1, 0] = 29
    bad['n_labels'][0, 1] = max(bad['n_labels'][0, 1], 1)
    bad['n_labels'][1, 2] = 21
    bad['score'][2, 0] = -(1 << 62)
    bad['score'][3, 3] = -(1 << 61)                                 # the floor itself is refused, one above is not
    bad['score'][4, 3] = -(1 << 61) + 1
    bad['score'][5, :] = -(1 << 62)
    got = _host(bad, mode)
    assert got.ok.tolist() == [[1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0]]
    assert got.pick[5] == -1 and got.wsum[5] == 0 and (got.dist[5] == -1).all() and (got.risk[5] == -1).all()
    assert got.weight[4, 3] == 0 and got.risk[4, 3] >= 0
    for b, keep in ((0, [0, 2, 3]), (1, [0, 1, 3]), (2, [1, 2, 3]), (3, [0, 1, 2])):
        sub = dict(case, labels=case['labels'][b:b + 1, keep], n_labels=case['n_labels'][b:b + 1, keep], score=case['score'][b:b + 1, keep])
        alone = _host(sub, mode)
        assert (got.risk[b, keep] == alone.risk[0]).all() and (got.weight[b, keep] == alone.weight[0]).all()
        assert [keep[k] for k in alone.order[0]] == got.order[b, :3].tolist() and got.order[b, 3] == -1
        gone = [k for k in range(4) if k not in keep][0]
        assert got.risk[b, gone] == -1 and got.weight[b, gone] == 0 and (got.dist[b, gone] == -1).all() and (got.dist[b, :, gone] == -1).all()


def test_refusals_by_name():
    case = mc.nbest(1, 29, B=2, K=3, L=8)
    with pytest.raises(ValueError, match="mode must be 'char' or 'word'"):
        _host(case, 'phone')
    with pytest.raises(ValueError, match='word mode needs is_space'):
        _host(case, 'word', is_space=None)
    with pytest.raises(ValueError, match='mbr_scale'):
        _host(case, 'char', 17.0)
    with pytest.raises(ValueError, match='1 .. 128 rows'):
        mbr.mbr_host(np.zeros((1, 129, 4), dtype=np.int32), np.zeros((1, 129), dtype=np.int32), np.zeros((1, 129), dtype=np.int64), None, 29, 'char')
    with pytest.raises(ValueError, match='1 .. 65536 ids'):
        mbr.mbr_host(np.zeros((1, 2, 65537), dtype=np.int32), np.zeros((1, 2), dtype=np.int32), np.zeros((1, 2), dtype=np.int64), None, 29, 'char')
    with pytest.raises(ValueError, match='score must be'):
        _host(case, 'char', score=case['score'][:, :2])
    with pytest.raises(ValueError, match='wtab must have 16384 entries'):
        mbr.mbr_host(case['labels'], case['n_labels'], case['score'], None, 29, 'char', wtab=np.zeros(5, dtype=np.uint32))


def test_rerank_texts():
    nbest = [['the cat sat', 'the cat sad', 'a cat sat', 'the bat sat'], ['hello'], ['a b', 'a c', 'a c']]
    scores = [[-1.0, -1.1, -1.2, -1.3], [-0.5], [-1.0, -1.5, -1.5]]
    out = mbr.rerank_texts(nbest, scores)
    # utterance 2: two equal rows of weight exp(-0.5) each outvote the best one: 2 * 0.607 > 1
    assert [r.pick for r in out] == [0, 0, 1] and out[1].order == [0] and out[1].posterior == [1.0] and out[1].expected_errors == [0.0]
    assert sorted(out[0].order) == [0, 1, 2, 3] and abs(sum(out[0].posterior) - 1) < 1e-12
    p = np.exp(np.array(scores[0]) + 1.0)
    assert abs(out[0].expected_errors[0] - (p[1] + p[2] + p[3]) / p.sum()) < 2e-3
    flat = mbr.rerank_texts(nbest, scores, scale=0.0)
    assert flat[2].pick == 1 and flat[2].order == [1, 2, 0]      # two equal rows outvote the best one
    cer = mbr.rerank_texts(nbest, scores, use_cer=True)
    assert abs(cer[0].expected_errors[0] - (p[1] + 3 * p[2] + p[3]) / p.sum()) < 5e-3
    assert mbr.rerank_texts([], []) == []
    with pytest.raises(ValueError, match='same number of rows'):
        mbr.rerank_texts(nbest, scores[:2])
    with pytest.raises(ValueError, match='without a row'):
        mbr.rerank_texts([[]], [[]])
    with pytest.raises(ValueError, match='mbr_scale'):
        mbr.rerank_texts(nbest, scores, scale=-1)


def test_decode_mbr_on_the_host_modules():
    """decode(mbr=) with CPU tensors runs the twin: the lists are rerank_texts over decode(n_best=)'s texts and scores, beam_rank
    is a permutation, the refusals are by name"""
    torch = pytest.importorskip('torch')
    from nemo.collections.asr.models import EncDecCTCModel
    from qasr import synth
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')
    io = dict(processed_signal=torch.from_numpy(synth.make_features(3, 16, 96, 7)), processed_signal_length=torch.tensor([96, 61, 33]))
    with torch.no_grad():
        plain = m.decode(**io, beam_width=8, n_best=4)
        for mode, scale in (('word', 1.0), ('char', 0.0), ('char', 2.5)):
            got = m.decode(**io, beam_width=8, n_best=4, mbr=mode, mbr_scale=scale)
            want = mbr.rerank_texts([[h.text for h in row] for row in plain], [[h.utt_score for h in row] for row in plain],
                                    use_cer=mode == 'char', scale=scale)
            for row, base, w in zip(got, plain, want):
                assert [h.beam_rank for h in row] == w.order and sorted(w.order) == list(range(len(base))) and len(base) >= 2
                assert [h.text for h in row] == [base[k].text for k in w.order]
                assert [h.posterior for h in row] == [w.posterior[k] for k in w.order]
                assert [h.mbr_risk for h in row] == [w.expected_errors[k] for k in w.order]
                assert [h.utt_score for h in row] == [base[k].utt_score for k in w.order]
        assert all(h.posterior is None and h.beam_rank is None for row in plain for h in row)
        refs = [row[-1].text or 'a' for row in plain]
        rep = m.error_rate(**io, texts=refs, use_cer=True, beam_width=8, n_best=4, mbr='char', mbr_scale=2.5)
        assert rep.mbr_pick == [w.pick for w in want]
        from nemo.collections.asr.metrics.wer import _levenshtein
        assert rep.mbr_total.errors == sum(_levenshtein(list(row[0].text), list(r)) for row, r in zip(got, refs))
        assert rep.oracle_errors <= rep.mbr_total.errors and m.error_rate(**io, texts=refs, beam_width=8, n_best=4).mbr_total is None
        for kw, msg in ((dict(mbr='word'), 'mbr needs beam_width'), (dict(beam_width=8, mbr='word'), 'mbr needs n_best >= 2'),
                        (dict(beam_width=8, n_best=4, mbr='phone'), "mbr must be None, 'word' or 'char'"),
                        (dict(beam_width=8, n_best=4, mbr='char', mbr_scale=-1), 'mbr_scale must be a number in 0 .. 16')):
            with pytest.raises(ValueError, match=msg):
                m.decode(**io, **kw)
        with pytest.raises(ValueError, match='decode_long: mbr is not built for long recordings'):
            m.decode_long(torch.zeros(1, 16000), torch.tensor([16000]), beam_width=8, n_best=4, mbr='word')


def test_beam_search_decoder_with_lm_mbr_is_keyword_only_and_reorders():
    torch = pytest.importorskip('torch')
    import beam_cases
    from nemo.collections.asr.modules.beam_search_decoder import BeamSearchDecoderWithLM
    vocab = [' '] + list('abcdefghijklmnopqrstuvwxyz') + ["'"]
    rng = np.random.Generator(np.random.PCG64(5))
    lp = torch.from_numpy(np.stack([beam_cases.peaky_logp(rng, 50, 29, 28, blend=True) for _ in range(3)]))
    plain = BeamSearchDecoderWithLM(vocab, 6, 0, 0, None, 1, input_tensor=True)(lp)
    for mode, scale in (('char', 0.5), ('word', 1.0)):
        got = BeamSearchDecoderWithLM(vocab, 6, 0, 0, None, 1, input_tensor=True, mbr=mode, mbr_scale=scale)(lp)
        want = mbr.rerank_texts([[t for _, t in r] for r in plain], [[s for s, _ in r] for r in plain], use_cer=mode == 'char', scale=scale)
        assert got == [[r[k] for k in w.order] for r, w in zip(plain, want)]
    assert any(w.order != sorted(w.order) for w in want) or any(len(r) > 1 for r in plain)
    with pytest.raises(TypeError):
        BeamSearchDecoderWithLM(vocab, 6, 0, 0, None, 1, 1.0, 40, True, None, 1.0, 'word')       # the positional signature stays
    with pytest.raises(ValueError, match='mbr needs beam_width >= 2'):
        BeamSearchDecoderWithLM(vocab, 1, 0, 0, None, 1, mbr='word')
    with pytest.raises(ValueError, match="mbr must be None, 'word' or 'char'"):
        BeamSearchDecoderWithLM(vocab, 4, 0, 0, None, 1, mbr='phone')
    with pytest.raises(ValueError, match='mbr_scale'):
        BeamSearchDecoderWithLM(vocab, 4, 0, 0, None, 1, mbr='char', mbr_scale=20)

