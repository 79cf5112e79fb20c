"""CTC prefix beam search with phrase boosting on an MI355X: k_beam_boost (csrc/qasr_beam_boost.hip), without and with an
n-gram model, against its NumPy statement qasr.beam.beam_search_host(boost=) on every byte of labels, n_labels, score,
boost_score, n_hyps (and lm_score with a model), outputs pre-filled with 0x5a; weight 0 equals k_beam / k_beam_lm byte for
byte; refused arguments launch nothing; the launch replays from a captured graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_cases  # noqa: E402
import beam_lm_cases as lm_cases  # noqa: E402
import boost_cases as cases  # noqa: E402
from qasr import beam, boost, ngram  # noqa: E402

EN, ZH = lm_cases.EN_VOCAB, lm_cases.ZH_VOCAB
SP = EN.index(' ')
FILL32, FILL64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
_models = {}


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    torch.set_grad_enabled(False)
    return engine


def lm_of(golden_dir, name):
    if name not in _models:
        _models[name] = ngram.NgramLM.from_arpa(lm_cases.model_path(golden_dir, name), lm_cases.vocab_of(name))
    return _models[name]


def _filled_out(B, nb, T, blank, with_lm, with_boost=True):
    i32 = dict(dtype=torch.int32, device='cuda')
    i64 = dict(dtype=torch.int64, device='cuda')
    return beam.BeamResult(labels=torch.full((B, nb, T), FILL32, **i32), n_labels=torch.full((B, nb), FILL32, **i32),
                           score=torch.full((B, nb), FILL64, **i64), n_hyps=torch.full((B,), FILL32, **i32), blank=blank,
                           lm_score=torch.full((B, nb), FILL64, **i64) if with_lm else None,
                           boost_score=torch.full((B, nb), FILL64, **i64) if with_boost else None)


def _assert_equal(got, want, what, fields=None):
    fields = fields or (('labels', 'n_labels', 'score', 'boost_score', 'n_hyps') + (('lm_score',) if want.lm_score is not None else ()))
    for name in fields:
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


def _run_and_compare(eng, lp, lens, ps, W, N, what, n_best=(None,), lm=None, alpha=0.0, beta=0.0):
    """k_beam_boost on the candidates of topn_host against the twin, for each n_best; returns the twin's full result"""
    B, T, C_ = lp.shape
    blank = C_ - 1
    cid, cq = beam.topn_host(lp, N, None)
    cid_d, cq_d = torch.from_numpy(cid).cuda(), torch.from_numpy(cq).cuda()
    lens_d = None if lens is None else torch.from_numpy(lens).cuda()
    full = beam.beam_search_host(cid, cq, lens, blank, W, None, lm, alpha, beta, boost=ps)       # computed once
    for nb in n_best:
        k = W if nb is None else nb                        # the twin reports the first n_best rows of the same final beam
        want = beam.BeamResult(full.labels[:, :k], full.n_labels[:, :k], full.score[:, :k], np.minimum(full.n_hyps, k).astype(np.int32),
                               blank, None if lm is None else full.lm_score[:, :k], full.boost_score[:, :k])
        out = _filled_out(B, W if nb is None else nb, T, blank, lm is not None)
        eng.ctc_beam(cid_d, cq_d, lens_d, blank, W, nb, out=out, lm=lm, alpha=alpha, beta=beta, boost=ps)
        torch.cuda.synchronize()
        _assert_equal(out, want, (what, nb))
    return full


# ------------------------------------------------------------------------------------------------------------ the tiny alphabet
@pytest.mark.parametrize('whole', [False, True])
def test_tiny_alphabet_nested_set_every_byte(eng, whole):
    C_, T, B, W, N = 5, 24, 4, 8, 4
    rng = np.random.Generator(np.random.PCG64(40 + whole))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C_, C_ - 1, sharp=0.7) for _ in range(B)])
    lens = np.array([T, T - 5, 1, 0], dtype=np.int32)
    ph = [(p, w) for p, w in zip(cases.NESTED, (1.0, 0.5, 2.0, 0.25))]
    for tight in (False, True):
        ps = boost.PhraseSet(ph, n_labels=4, space=3 if whole else None, whole_words=whole, min_capacity=tight)
        want = _run_and_compare(eng, lp, lens, ps, W, N, ('tiny', whole, tight), n_best=(None, 1))
        assert want.boost_score[:2].any() and want.n_hyps[3] == 1 and want.boost_score[3, 0] == 0
        br = cases.Brute(ph, whole, 3)
        for b in range(B):
            for h in range(int(want.n_hyps[b])):
                assert want.boost_score[b, h] == br.final(want.labels[b, h, :want.n_labels[b, h]].tolist())


# ------------------------------------------------------------------------------------------------------------ En and Zh
@pytest.mark.parametrize('W,N', [(1, 20), (16, 40), (128, 64)])
def test_en_whole_words_every_byte(eng, W, N):
    T = 63
    rng = np.random.Generator(np.random.PCG64(50 + W))
    lp = np.stack([beam_cases.peaky_logp(rng, T, 29, 28) for _ in range(3)])
    lens = np.array([T, T // 2, 0], dtype=np.int32)
    ph = cases.gpu_phrases(rng, lp, lens, 28, True, SP)
    ps = boost.PhraseSet(ph, EN)
    assert ps.whole_words and ps.start != 0
    want = _run_and_compare(eng, lp, lens, ps, W, N, ('en', W, N), n_best=(None, 1) if W > 1 else (None,))
    assert want.boost_score[0, :want.n_hyps[0]].any() and want.n_hyps[2] == 1 and want.n_labels[2, 0] == 0
    if W == 16:
        sub = boost.PhraseSet(ph, EN, whole_words=False)
        _run_and_compare(eng, lp, None, sub, W, N, ('en, substrings, padded rows', W, N))


def test_zh_every_byte(eng):
    T, W, N = 63, 16, 40
    rng = np.random.Generator(np.random.PCG64(60))
    lp = np.stack([beam_cases.peaky_logp(rng, T, 5207, 5206) for _ in range(2)])
    lens = np.array([T, T // 2], dtype=np.int32)
    ps = boost.PhraseSet(cases.gpu_phrases(rng, lp, lens, 5206, False, -1), ZH)
    assert not ps.whole_words and ps.start == 0 and ps.space == -1
    want = _run_and_compare(eng, lp, lens, ps, W, N, 'zh', n_best=(None, W))
    assert want.boost_score[0, :want.n_hyps[0]].any()


# ------------------------------------------------------------------------------------------------------------ with a model
@pytest.mark.parametrize('model', ['en3', 'zh2'])
def test_with_a_model_every_byte(eng, golden_dir, model):
    lm = lm_of(golden_dir, model)
    T, W, N = 63, 16, 20
    lp, lens = lm_cases.batch_inputs(model, T, 3, 900)
    rng = np.random.Generator(np.random.PCG64(61))
    ph = cases.gpu_phrases(rng, lp, lens, lm.n_labels, lm.word_mode, lm.space)
    ps = boost.PhraseSet(ph, lm_cases.vocab_of(model))
    assert ps.whole_words == lm.word_mode
    want = _run_and_compare(eng, lp, lens, ps, W, N, ('model', model), n_best=(None, 1), lm=lm, alpha=1.25, beta=0.75)
    assert want.boost_score[0, :want.n_hyps[0]].any() and want.lm_score[0, :want.n_hyps[0]].any()
    assert want.n_hyps[2] == 1 and want.boost_score[2, 0] == 0 and want.lm_score[2, 0] == 0


# ------------------------------------------------------------------------------------------------------------ set variants
@pytest.mark.parametrize('variant', ['minimal_capacity', 'phrase_of_64', 'phrase_of_1', 'many_phrases'])
def test_set_variants_every_byte(eng, variant):
    T, W, N = 63, 16, 20
    rng = np.random.Generator(np.random.PCG64(70))
    lp = np.stack([beam_cases.peaky_logp(rng, T, 29, 28) for _ in range(2)])
    g = [c for c in beam_cases.greedy(lp[0], 28)]
    if variant == 'minimal_capacity':                     # substrings of the best path and random ones: a full table
        ph = [(g[a:a + k], 1.0 + 0.25 * k) for a in range(0, len(g) - 6, 2) for k in (2, 4, 6)]
        ph += [([int(c) for c in rng.integers(0, 28, size=5)], 2.0) for _ in range(40)]
        ps = boost.PhraseSet(ph, EN, whole_words=False, min_capacity=True)
        h = np.frombuffer(ps.pack()[:128], '<i4')
        assert h[8] >= 8 and h[8] > np.frombuffer(ps.pack(False)[:128], '<i4')[8]          # long probe runs
    elif variant == 'phrase_of_64':                       # the longest phrase, spelled label by label over 128 frames: it completes
        labs = [int(c) for c in rng.integers(0, 28, size=64)]
        toks = np.array([x for c in labs for x in (c, 28)])
        lp = np.stack([beam_cases.token_logp(toks, 29, 71), beam_cases.token_logp(np.roll(toks, 1), 29, 72)])
        ph = [(labs, 3.0), (labs[:3], 1.0), (labs[5:], 0.5)]
        ps = boost.PhraseSet(ph, EN, whole_words=False)
        assert ps.n_nodes >= 65 and ps.pot.max() == 60 * 3 * 65536          # behind the end node of its 3-label prefix
    elif variant == 'phrase_of_1':
        ph = [([g[1]], 2.0)]
        ps = boost.PhraseSet(ph, EN, whole_words=False)
        assert ps.n_nodes == 2
    else:                                                 # a thousand random phrases and the path's own words
        ph = [([int(c) for c in rng.integers(0, 28, size=int(rng.integers(1, 7)))], float(rng.uniform(0, 3))) for _ in range(1000)]
        ph += cases.gpu_phrases(rng, lp, None, 28, False, SP)
        ps = boost.PhraseSet(ph, EN, whole_words=False)
    want = _run_and_compare(eng, lp, None, ps, W, N, variant)
    assert want.boost_score[0, :want.n_hyps[0]].any()
    if variant == 'phrase_of_64':
        assert want.labels[0, 0, :64].tolist() == labs and want.boost_score[0, 0] >= 64 * 3 * 65536


# ------------------------------------------------------------------------------------------------------------ weight 0
def test_weight_zero_equals_k_beam_and_k_beam_lm_byte_for_byte(eng, golden_dir):
    for model, W, N in ((None, 16, 40), (None, 128, 64), ('en3', 16, 20), ('zh2', 16, 20)):
        lm = None if model is None else lm_of(golden_dir, model)
        if model is None:
            rng = np.random.Generator(np.random.PCG64(80 + W))
            lp = np.stack([beam_cases.peaky_logp(rng, 63, 29, 28) for _ in range(3)])
            lens = np.array([63, 31, 0], dtype=np.int32)
            vocab, whole, space = EN, True, SP
        else:
            lp, lens = lm_cases.batch_inputs(model, 63, 3, 901)
            vocab, whole, space = lm_cases.vocab_of(model), lm.word_mode, lm.space
        blank = lp.shape[2] - 1
        rng = np.random.Generator(np.random.PCG64(81))
        ps = boost.PhraseSet([(p, 0.0) for p, _ in cases.gpu_phrases(rng, lp, lens, blank, whole, space)], vocab)
        cid, cq = beam.topn_host(lp, N, None)
        cid_d, cq_d, lens_d = torch.from_numpy(cid).cuda(), torch.from_numpy(cq).cuda(), torch.from_numpy(lens).cuda()
        plain = _filled_out(3, W, 63, blank, lm is not None, with_boost=False)
        eng.ctc_beam(cid_d, cq_d, lens_d, blank, W, None, out=plain, lm=lm, alpha=1.2, beta=0.5)
        out = _filled_out(3, W, 63, blank, lm is not None)
        eng.ctc_beam(cid_d, cq_d, lens_d, blank, W, None, out=out, lm=lm, alpha=1.2, beta=0.5, boost=ps)
        torch.cuda.synchronize()
        for f in ('labels', 'n_labels', 'score', 'n_hyps') + (('lm_score',) if lm is not None else ()):
            assert torch.equal(getattr(out, f), getattr(plain, f)), (model, W, f)
        assert not out.boost_score.any()


# ------------------------------------------------------------------------------------------------------------ the chain
def test_k_topn_then_k_beam_boost_equal_the_host_search_and_sets_are_cached_per_set(eng):
    rng = np.random.Generator(np.random.PCG64(90))
    lp = np.stack([beam_cases.peaky_logp(rng, 100, 29, 28) for _ in range(2)])
    lens = np.array([100, 47], dtype=np.int32)
    ph = cases.gpu_phrases(rng, lp, lens, 28, True, SP)
    for weight in (0.5, 3.0):                             # a sweep of weights: a new set per weight, nothing stale
        ps = boost.PhraseSet([p for p, _ in ph], EN, weight=weight)
        got = eng.ctc_beam_search(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), None, 16, 5, 40, boost=ps)
        torch.cuda.synchronize()
        _assert_equal(got, beam.search_host(lp, lens, None, 16, 5, 40, boost=ps), ('chain', weight))
        assert eng.boost_device(ps, 'cuda') is eng.boost_device(ps, torch.device('cuda', torch.cuda.current_device()))
    plain = eng.ctc_beam_search(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), None, 16, 5, 40)
    assert plain.boost_score is None and plain.lm_score is None


# ------------------------------------------------------------------------------------------------------------ refusals
def test_k_beam_boost_refuses_bad_arguments_and_writes_nothing(eng, golden_dir):
    lib = eng.load_library()
    lm = lm_of(golden_dir, 'en3')
    ps = boost.PhraseSet(['cat', 'dog'], EN)
    B, T, N, W, nb, blank = 2, 8, 20, 16, 4, 28
    cid = torch.zeros(B, T, N, dtype=torch.int32, device='cuda')
    cq = torch.zeros(B, T, N, dtype=torch.int32, device='cuda')
    out = _filled_out(B, nb, T, blank, True)
    need = eng.ctc_beam_workspace_bytes(B, T, W)
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device='cuda')
    tab = eng.lae_table_device('cuda')
    lm_blob, blob = eng.lm_device(lm, 'cuda'), eng.boost_device(ps, 'cuda')

    def args(with_lm=True, **kw):
        a = eng.BeamBoostArgs()
        a.struct_size = C.sizeof(eng.BeamBoostArgs)
        a.B, a.T, a.N, a.beam_width, a.n_best, a.blank, a.lae_entries = B, T, N, W, nb, blank, beam.TAB_ENTRIES
        a.cand_id, a.cand_q, a.lae_table, a.workspace, a.workspace_bytes = cid.data_ptr(), cq.data_ptr(), tab.data_ptr(), ws.data_ptr(), need
        a.labels, a.n_labels, a.score, a.n_hyps = out.labels.data_ptr(), out.n_labels.data_ptr(), out.score.data_ptr(), out.n_hyps.data_ptr()
        if with_lm:
            a.lm, a.lm_bytes, a.alpha_q, a.beta_q, a.lm_score = lm_blob.data_ptr(), lm_blob.numel(), 65536, 0, out.lm_score.data_ptr()
        a.space, a.whole_words = SP, 1
        a.boost, a.boost_bytes, a.boost_score = blob.data_ptr(), blob.numel(), out.boost_score.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=C.sizeof(eng.BeamLmArgs)), dict(B=0), dict(T=0), dict(T=65537), dict(N=0), dict(N=65),
           dict(beam_width=0), dict(beam_width=129), dict(n_best=0), dict(n_best=W + 1), dict(blank=-1), dict(lae_entries=4096),
           dict(workspace_bytes=need - 1), dict(lm_bytes=0), dict(lm_bytes=127), dict(lm=lm_blob.data_ptr() + 4), dict(alpha_q=-1),
           dict(alpha_q=16 * 65536 + 1), dict(beta_q=16 * 65536 + 1), dict(beta_q=-16 * 65536 - 1), dict(space=-2), dict(space=blank),
           dict(boost_bytes=0), dict(boost_bytes=127), dict(boost=blob.data_ptr() + 4), dict(space=-1), dict(with_lm=False, space=-1),
           dict(with_lm=False, space=blank)]
    bad += [{k: None} for k in ('cand_id', 'cand_q', 'lae_table', 'workspace', 'labels', 'n_labels', 'score', 'n_hyps', 'lm_score',
                                'boost', 'boost_score')]
    bad += [dict(with_lm=False, boost=None), dict(with_lm=False, boost_score=None)]
    for kw in bad:
        assert lib.qasr_ctc_beam_boost(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_beam_boost(s, None) == 1
    for kw in (dict(lm=lm, alpha=-1.0), dict(lm=lm, beta=17.0)):            # the binding refuses before it launches
        with pytest.raises(ValueError):
            eng.ctc_beam(cid, cq, None, blank, W, nb, out=out, boost=ps, **kw)
    with pytest.raises(ValueError, match='labels'):
        eng.ctc_beam(cid, cq, None, blank + 1, W, nb, out=out, boost=ps)
    torch.cuda.synchronize()
    for t in (out.labels, out.n_labels, out.n_hyps):
        assert (t == FILL32).all()
    assert (out.score == FILL64).all() and (out.lm_score == FILL64).all() and (out.boost_score == FILL64).all() and (ws == 0x5a).all()
    # a header that does not fit the bytes given, or a whole_words flag that is not the header's: the search ends empty, in bounds
    for kw in (dict(boost_bytes=blob.numel() - 16), dict(whole_words=0), dict(with_lm=False, boost_bytes=blob.numel() - 16),
               dict(lm_bytes=lm_blob.numel() - 16)):
        assert lib.qasr_ctc_beam_boost(s, C.byref(args(**kw))) == 0
        torch.cuda.synchronize()
        assert (out.n_hyps == 0).all() and (out.score == beam.NEG).all() and (out.labels == blank).all() and not out.boost_score.any()
    out.lm_score.fill_(FILL64)
    assert lib.qasr_ctc_beam_boost(s, C.byref(args(with_lm=False))) == 0     # without a model: accepted, lm_score is not touched
    torch.cuda.synchronize()
    assert (out.n_hyps.cpu().numpy() == nb).all() and (out.lm_score == FILL64).all()
    assert lib.qasr_ctc_beam_boost(s, C.byref(args())) == 0                   # and the full block unchanged is accepted
    torch.cuda.synchronize()
    assert (out.n_hyps.cpu().numpy() == nb).all() and not (out.lm_score == FILL64).any()
    with pytest.raises(eng.QasrError, match='phrase set'):
        eng.boost_check(ps.pack()[:-4], ps.n_labels)


# ------------------------------------------------------------------------------------------------------------ graph replay
def test_k_beam_boost_is_capturable(eng):
    """nothing is allocated and no length is read on the host: the launch replays from a graph on new inputs"""
    T, B, W, N, blank = 40, 2, 8, 20, 28
    rng = np.random.Generator(np.random.PCG64(95))
    lps = [np.stack([beam_cases.peaky_logp(rng, T, 29, blank) for _ in range(B)]) for _ in range(2)]
    lens = [np.array([T, 17], dtype=np.int32), np.array([9, T], dtype=np.int32)]
    ps = boost.PhraseSet(cases.gpu_phrases(rng, np.concatenate(lps), None, blank, True, SP), EN)
    cands = [beam.topn_host(lp, N, None) for lp in lps]
    cid_d, cq_d = torch.from_numpy(cands[0][0]).cuda(), torch.from_numpy(cands[0][1]).cuda()
    lens_d = torch.from_numpy(lens[0]).cuda()
    out = _filled_out(B, W, T, blank, False)
    ws = torch.empty(eng.ctc_beam_workspace_bytes(B, T, W), dtype=torch.uint8, device='cuda')
    eng.lae_table_device('cuda'), eng.boost_device(ps, 'cuda')          # uploaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_beam(cid_d, cq_d, lens_d, blank, W, None, workspace=ws, out=out, boost=ps)
    for (cid, cq), ln in zip(cands, lens):
        cid_d.copy_(torch.from_numpy(cid)), cq_d.copy_(torch.from_numpy(cq)), lens_d.copy_(torch.from_numpy(ln))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(out, beam.beam_search_host(cid, cq, ln, blank, W, None, boost=ps), 'replay')
