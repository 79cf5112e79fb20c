"""CTC prefix beam search with an n-gram language model on an MI355X: k_beam_lm (csrc/qasr_beam.hip) against its NumPy
statement qasr.beam.beam_search_host(lm=), every byte of labels, n_labels, score, lm_score and n_hyps; refused arguments
launch nothing; BeamSearchDecoderWithLM and decode(lm=) on CUDA tensors equal their host results."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_cases  # noqa: E402
import beam_lm_cases as cases  # noqa: E402
from qasr import beam, ngram  # noqa: E402

FIELDS = ('labels', 'n_labels', 'score', 'lm_score', 'n_hyps')
_models = {}


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    torch.set_grad_enabled(False)
    return engine


def lm_of(golden_dir, name, tight=False):
    if (name, tight) not in _models:
        _models[name, tight] = ngram.NgramLM.from_arpa(cases.model_path(golden_dir, name), cases.vocab_of(name), min_capacity=tight)
    return _models[name, tight]


def _filled_out(B, nb, T, blank):
    i32 = dict(dtype=torch.int32, device='cuda')
    i64 = dict(dtype=torch.int64, device='cuda')
    return beam.BeamResult(labels=torch.full((B, nb, T), 0x5a5a5a5a, **i32), n_labels=torch.full((B, nb), 0x5a5a5a5a, **i32),
                           score=torch.full((B, nb), 0x5a5a5a5a5a5a5a5a, **i64), n_hyps=torch.full((B,), 0x5a5a5a5a, **i32),
                           blank=blank, lm_score=torch.full((B, nb), 0x5a5a5a5a5a5a5a5a, **i64))


def _assert_equal(got, want, what):
    for name in FIELDS:
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


def _run_and_compare(eng, lp, lens, lm, W, N, alpha, beta, what, n_best=(None,)):
    """k_beam_lm on the candidates of topn_host against the twin, for each n_best; returns the twin's full result"""
    B, T, C_ = lp.shape
    blank = C_ - 1
    cid, cq = beam.topn_host(lp, N, None)                # candidates on every frame, so that lens decides where to stop
    cid_d, cq_d = torch.from_numpy(cid).cuda(), torch.from_numpy(cq).cuda()
    lens_d = None if lens is None else torch.from_numpy(lens).cuda()
    want = None
    for nb in n_best:
        want = beam.beam_search_host(cid, cq, lens, blank, W, nb, lm, alpha, beta)
        out = _filled_out(B, W if nb is None else nb, T, blank)
        eng.ctc_beam(cid_d, cq_d, lens_d, blank, W, nb, out=out, lm=lm, alpha=alpha, beta=beta)
        torch.cuda.synchronize()
        _assert_equal(out, want, (what, nb))
    return want


# ------------------------------------------------------------------------------------------------------------ En, word mode
@pytest.mark.parametrize('T', [1, 63, 65])
@pytest.mark.parametrize('W', [1, 16, 128])
def test_en_word_mode_every_byte(eng, golden_dir, W, T):
    lm = lm_of(golden_dir, 'en3')
    for N in (20, 64):
        lp, lens = cases.batch_inputs('en3', T, 3, 500 + 10 * T + W + N)
        assert lens.tolist() == [T, T // 2, 0] and lp.shape == (3, T, 29)
        want = _run_and_compare(eng, lp, lens, lm, W, N, 1.25, 0.75, ('en', T, W, N), n_best=(None, 1, min(W, 3)))
        assert want.n_hyps[2] == 1 and want.n_labels[2, 0] == 0 and want.lm_score[2, 0] == 0
        if T > 1 and W > 1:
            assert want.lm_score[0, :want.n_hyps[0]].any()                    # the model took part
        _run_and_compare(eng, lp, None, lm, W, N, 1.25, 0.75, ('en, padded rows', T, W, N))


# ------------------------------------------------------------------------------------------------------------ Zh, character mode
@pytest.mark.parametrize('W', [16, 128])
def test_zh_character_mode_every_byte(eng, golden_dir, W):
    lm = lm_of(golden_dir, 'zh2')
    lp, lens = cases.batch_inputs('zh2', 63, 3, 600 + W)
    assert lp.shape == (3, 63, 5207)
    want = _run_and_compare(eng, lp, lens, lm, W, 40, 0.8, 1.5, ('zh', W), n_best=(None, 2))
    assert (want.lm_score[0, :want.n_hyps[0]] != 0).all()


# ------------------------------------------------------------------------------------------------------------ model variants
@pytest.mark.parametrize('variant', ['order1', 'order3', 'order5', 'tight3', 'tight5', 'all_oov', 'alpha0', 'negative_beta'])
def test_model_variants_every_byte(eng, golden_dir, variant):
    name = {'order1': 'en1', 'order5': 'en5', 'tight5': 'en5'}.get(variant, 'en3')
    tight = variant.startswith('tight')
    lm = lm_of(golden_dir, name, tight)
    alpha, beta = {'alpha0': (0.0, 0.75), 'negative_beta': (16.0, -16.0)}.get(variant, (1.5, 0.5))
    if tight:                                             # the smallest capacity: probe chains reach the stored bound
        hdr = np.frombuffer(lm.pack()[:128], '<i4')
        assert hdr[6] == ngram._pow2_above(len(lm.trans)) and hdr[7] >= 64
    T, W, N = 63, 16, 20
    if variant == 'all_oov':                              # random labels: no word of the strings is one of the model's
        rng = np.random.Generator(np.random.PCG64(9))
        lp = np.stack([beam_cases.peaky_logp(rng, T, 29, 28, sharp=3.0) for _ in range(3)])
        lens = np.array([T, T // 2, 0], dtype=np.int32)
    else:
        lp, lens = cases.batch_inputs(name, T, 3, 700)
    want = _run_and_compare(eng, lp, lens, lm, W, N, alpha, beta, variant, n_best=(None, 5))
    if variant == 'all_oov':
        t_oov = ngram.term(ngram.OOV_Q, *ngram.fixed_weights(alpha, beta))
        best = want.lm_score[:2, 0]
        assert (best <= t_oov).all()                                      # at least the last word is none of the model's
    if variant == 'alpha0':
        assert (want.lm_score[0, :want.n_hyps[0]] % 49152 == 0).all() and want.lm_score[0].any()      # word counts times beta
    assert want.lm_score[:2].any()


# ------------------------------------------------------------------------------------------------------------ ties
def test_ties_at_the_cut_with_a_model(eng, golden_dir):
    """rows of few distinct values (beam_cases.tie_rows): many candidates share the score at the W-th place - letters inside
    a word add no term - and the candidate index decides, with the model's terms among the scores"""
    lp = np.stack([beam_cases.tie_rows(31 + b, 40, 29) for b in range(3)])
    lp[2, :, 26] = np.float32(-0.25)                      # a space among the tied values on every frame
    for name, W in (('en3', 1), ('en3', 2), ('en3', 16), ('en3', 128), ('en1', 16)):
        _run_and_compare(eng, lp, None, lm_of(golden_dir, name), W, 20, 1.0, 0.5, ('ties', name, W))
    zlp = np.stack([beam_cases.tie_rows(41 + b, 30, 5207) for b in range(2)])
    for W in (16, 128):
        _run_and_compare(eng, zlp, None, lm_of(golden_dir, 'zh2'), W, 40, 1.0, 0.5, ('ties zh', W))


# ------------------------------------------------------------------------------------------------------------ the chain
def test_k_topn_then_k_beam_lm_equal_the_host_search(eng, golden_dir):
    for name, W, nb, N in (('en3', 16, 5, 40), ('zh2', 16, 5, 40), ('en5', 128, None, 29)):
        lm = lm_of(golden_dir, name)
        lp, lens = cases.batch_inputs(name, 120, 2, 800)
        got = eng.ctc_beam_search(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), None, W, nb, N, lm=lm, alpha=0.7, beta=1.0)
        torch.cuda.synchronize()
        _assert_equal(got, beam.search_host(lp, lens, None, W, nb, N, lm, 0.7, 1.0), ('chain', name))
        again = eng.ctc_beam_search(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), None, W, nb, N, lm=lm, alpha=2.0, beta=0.0)
        torch.cuda.synchronize()                          # a sweep: the same upload, other weights
        _assert_equal(again, beam.search_host(lp, lens, None, W, nb, N, lm, 2.0, 0.0), ('chain, second weights', name))
        assert eng.lm_device(lm, 'cuda') is eng.lm_device(lm, torch.device('cuda', torch.cuda.current_device()))
        plain = eng.ctc_beam_search(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), None, W, nb, N)
        assert plain.lm_score is None


# ------------------------------------------------------------------------------------------------------------ refusals
def test_k_beam_lm_refuses_bad_arguments_and_writes_nothing(eng, golden_dir):
    lib = eng.load_library()
    lm = lm_of(golden_dir, 'en3')
    B, T, N, W, nb, blank = 2, 8, 20, 16, 4, 28
    cid = torch.zeros(B, T, N, dtype=torch.int32, device='cuda')
    cq = torch.zeros(B, T, N, dtype=torch.int32, device='cuda')
    out = _filled_out(B, nb, T, blank)
    need = eng.ctc_beam_workspace_bytes(B, T, W)
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device='cuda')
    tab = eng.lae_table_device('cuda')
    blob = eng.lm_device(lm, 'cuda')

    def args(**kw):
        a = eng.BeamLmArgs()
        a.struct_size = C.sizeof(eng.BeamLmArgs)
        a.B, a.T, a.N, a.beam_width, a.n_best, a.blank, a.lae_entries = B, T, N, W, nb, blank, beam.TAB_ENTRIES
        a.cand_id, a.cand_q, a.lae_table, a.workspace, a.workspace_bytes = cid.data_ptr(), cq.data_ptr(), tab.data_ptr(), ws.data_ptr(), need
        a.labels, a.n_labels, a.score, a.n_hyps = out.labels.data_ptr(), out.n_labels.data_ptr(), out.score.data_ptr(), out.n_hyps.data_ptr()
        a.lm, a.lm_bytes, a.alpha_q, a.beta_q, a.space, a.lm_score = blob.data_ptr(), blob.numel(), 65536, 0, lm.space, out.lm_score.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=C.sizeof(eng.BeamArgs)), dict(B=0), dict(T=0), dict(T=65537), dict(N=0), dict(N=65),
           dict(beam_width=0), dict(beam_width=129), dict(n_best=0), dict(n_best=W + 1), dict(blank=-1), dict(lae_entries=4096),
           dict(workspace_bytes=need - 1), dict(lm_bytes=0), dict(lm_bytes=127), dict(lm=blob.data_ptr() + 4), dict(alpha_q=-1),
           dict(alpha_q=16 * 65536 + 1), dict(beta_q=16 * 65536 + 1), dict(beta_q=-16 * 65536 - 1), dict(space=-2), dict(space=blank)]
    bad += [{k: None} for k in ('cand_id', 'cand_q', 'lae_table', 'workspace', 'labels', 'n_labels', 'score', 'n_hyps', 'lm', 'lm_score')]
    for kw in bad:
        assert lib.qasr_ctc_beam_lm(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_beam_lm(s, None) == 1
    for kw in (dict(alpha=-1.0), dict(alpha=16.5), dict(beta=17.0)):       # the binding refuses before it launches
        with pytest.raises(ValueError):
            eng.ctc_beam(cid, cq, None, blank, W, nb, out=out, lm=lm, **kw)
    with pytest.raises(ValueError, match='labels'):
        eng.ctc_beam(cid, cq, None, blank + 1, W, nb, out=out, lm=lm)
    torch.cuda.synchronize()
    for t in (out.labels, out.n_labels, out.n_hyps):
        assert (t == 0x5a5a5a5a).all()
    assert (out.score == 0x5a5a5a5a5a5a5a5a).all() and (out.lm_score == 0x5a5a5a5a5a5a5a5a).all() and (ws == 0x5a).all()
    # a model whose mode disagrees with `space`, or fewer bytes than its header says: the search ends empty, in bounds
    for kw in (dict(space=-1), dict(lm_bytes=blob.numel() - 16)):
        assert lib.qasr_ctc_beam_lm(s, C.byref(args(**kw))) == 0
        torch.cuda.synchronize()
        assert (out.n_hyps == 0).all() and (out.score == beam.NEG).all() and (out.labels == blank).all()
    assert lib.qasr_ctc_beam_lm(s, C.byref(args())) == 0                   # and the same block unchanged is accepted
    torch.cuda.synchronize()
    assert (out.n_hyps.cpu().numpy() == nb).all()
    with pytest.raises(eng.QasrError, match='language model'):
        eng.lm_check(lm.pack()[:-4], lm.n_labels)


# ------------------------------------------------------------------------------------------------------------ the facade
def test_module_and_decode_on_cuda_equal_the_host(eng, golden_dir):
    from nemo.collections.asr.models import EncDecCTCModel
    from nemo.collections.asr.modules import BeamSearchDecoderWithLM
    path = cases.model_path(golden_dir, 'en3')
    lp, lens = cases.batch_inputs('en3', 80, 3, 70)
    dec = BeamSearchDecoderWithLM(cases.EN_VOCAB, 8, 1.5, 0.5, path, 1, cutoff_top_n=20, input_tensor=True)
    host = dec(torch.from_numpy(lp), torch.from_numpy(lens))
    assert dec(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda()) == host
    res = dec.search(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), n_best=2)
    _assert_equal(res, beam.search_host(lp, lens, 28, 8, 2, 20, dec.scorer, 1.5, 0.5), 'module')
    zlp, zlens = cases.batch_inputs('zh2', 40, 2, 71)
    zdec = BeamSearchDecoderWithLM(cases.ZH_VOCAB, 4, 1.0, 0.0, cases.model_path(golden_dir, 'zh2'), 1, cutoff_top_n=20, input_tensor=True)
    assert zdec(torch.from_numpy(zlp).cuda(), torch.from_numpy(zlens).cuda()) == zdec(torch.from_numpy(zlp), torch.from_numpy(zlens))
    # decode(lm=) on the dynamic device path: the hypotheses of the twin on the same log-probabilities
    import nemo.quantization.utils.quantize_model as qm
    from qasr import synth
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.evaluate(m)
    qm.set_dynamic(m, True)
    x = torch.from_numpy(synth.make_features(4, 16, 96, 7)).cuda()
    xl = torch.tensor([96, 90, 61, 12]).cuda()
    vocab = m.decoder.vocabulary
    lm = ngram.NgramLM.from_arpa(path, vocab)
    logp, enc_len, _ = m(processed_signal=x, processed_signal_length=xl)
    torch.cuda.synchronize()
    want = beam.to_hypotheses(beam.search_host(logp.cpu().numpy(), enc_len.cpu().numpy(), len(vocab), 16, 3, 40, lm, 0.8, 1.0), vocab)
    many = m.decode(processed_signal=x, processed_signal_length=xl, beam_width=16, n_best=3, lm=path, alpha=0.8, beta=1.0)
    key = lambda h: (h.text, h.labels, h.utt_score, h.lm_score)     # noqa: E731
    assert [[key(h) for h in hs] for hs in many] == [[key(h) for h in w] for w in want]
    one = m.decode(processed_signal=x, processed_signal_length=xl, beam_width=16, lm=lm, alpha=0.8, beta=1.0)
    assert [key(h) for h in one] == [key(w[0]) for w in want] and all(isinstance(h.lm_score, float) for h in one)
    assert all(h.lm_score is None for h in m.decode(processed_signal=x, processed_signal_length=xl, beam_width=16))


def test_cli_refuses_model_arguments_without_their_switch(eng):
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'q-asr_amd', 'examples', 'asr', 'quantization',
                       'inference.py')
    base = [sys.executable, cli, '--asr_model', 'QuartzNet15x5Base-En', '--dataset', 'none.json']
    for extra, why in ((['--lm_path', 'lm.arpa'], '--beam_width'), (['--beam_width', '4', '--alpha', '1.0'], '--lm_path'),
                       (['--beam_width', '4', '--lm_path', 'lm.arpa', '--alpha', '17'], '0 .. 16')):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)      # refused before a model is built
        assert out.returncode == 2 and why in out.stderr, out.stderr[-500:]
