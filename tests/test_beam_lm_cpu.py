"""The beam search with an n-gram language model on the host: the packed model (qasr/ngram.py) against an independent float64
ARPA reader, the fixed-point twin (qasr.beam with lm=) against the float64 search of tests/beam_lm_cases.py, the cases
where the model decides, the word-mode edges, qasr_lm_check, and BeamSearchDecoderWithLM / decode(lm=) on the host."""
import gzip
import json
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_cases  # noqa: E402
import beam_lm_cases as cases  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from nemo.collections.asr.modules import BeamSearchDecoderWithLM  # noqa: E402
from qasr import beam, ngram  # noqa: E402

torch.set_grad_enabled(False)
EN, ZH = cases.EN_VOCAB, cases.ZH_VOCAB
SP = EN.index(' ')
_models = {}


def lm_of(golden_dir, name):
    if name not in _models:
        _models[name] = ngram.NgramLM.from_arpa(cases.model_path(golden_dir, name), cases.vocab_of(name))
    return _models[name]


def _term_bound(order, alpha):
    """What one fixed-point term may be off by, in nats: each of the at most `order` summands of raw is rounded once (half
    a unit of 2^-16), the product with alpha is rounded once more, and so is beta."""
    return (order * alpha + 2.0) / 131072.0


def _bound(T, n_terms, order, alpha):
    """the bound of test_beam_cpu.py on the search itself, plus the terms a hypothesis can have collected"""
    return 100.0 * T / 65536.0 + n_terms * _term_bound(order, alpha)


def _ids(text):
    return [EN.index(ch) for ch in text]


def _text(res, b=0, h=0, vocab=EN):
    return ''.join(vocab[i] for i in res.labels[b, h, :res.n_labels[b, h]])


# -------------------------------------------------------------------------------------------------- 0. the fixtures
def test_committed_models_are_what_the_generator_writes(golden_dir):
    for spec in cases.MODELS:
        path = cases.model_path(golden_dir, spec[0])
        assert os.path.getsize(path) < 64 * 1024
        with (gzip.open if path.endswith('.gz') else open)(path, 'rt', encoding='utf-8') as f:
            assert f.read() == cases.model_text(spec[0]), spec[0]
    assert [lm_of(golden_dir, n).order for n in ('en3', 'en1', 'en5', 'zh2')] == [3, 1, 5, 2]
    assert [lm_of(golden_dir, n).word_mode for n in ('en3', 'en1', 'en5', 'zh2')] == [True, True, True, False]
    assert 200 <= (lm_of(golden_dir, 'zh2').label_to_word >= 0).sum() <= 400


def test_recorded_twin_outputs(golden_dir):
    d = np.load(os.path.join(golden_dir, 'beam_lm.npz'))
    meta = json.loads(str(d['meta']))['cases']
    assert [c['name'] for c in meta] == [s[0] for s in cases.FIXTURE_LISTS]
    for c in meta:
        lp, lens = cases.batch_inputs(c['model'], c['T'], c['utterances'], c['seed'])
        res = beam.search_host(lp, lens, lp.shape[2] - 1, c['W'], None, c['N'], lm_of(golden_dir, c['model']), c['alpha'], c['beta'])
        for f in ('labels', 'n_labels', 'score', 'lm_score', 'n_hyps'):
            assert np.array_equal(getattr(res, f), d[f'{f}_{c["name"]}']), (c['name'], f)
            assert getattr(res, f).dtype == d[f'{f}_{c["name"]}'].dtype


# -------------------------------------------------------------------------------------------------- 1. look-ups
@pytest.mark.parametrize('name', ['en3', 'en1', 'en5', 'zh2'])
def test_lookups_against_the_float64_reader(golden_dir, name):
    lm, ref = lm_of(golden_dir, name), cases.OracleLM(cases.model_path(golden_dir, name))
    assert lm.order == ref.order
    rng = np.random.Generator(np.random.PCG64(50 + lm.order))
    words = [w for w in lm.words if w not in ('<s>', '</s>', '<unk>')]
    grams = [g for g in ref.prob if len(g) > 1]
    worst, n_seen, n_back = 0.0, 0, 0
    for q in range(3000):
        kind = q % 4
        if kind == 0 and grams:                          # a context the model has seen, with a word it has seen after it
            g = grams[rng.integers(len(grams))]
            hist, w = list(g[:-1]), g[-1]
            if w == '<s>':
                continue
        else:                                           # random words: mostly unseen contexts, any length up to order + 2
            hist = [words[i] for i in rng.integers(0, len(words), size=int(rng.integers(0, lm.order + 3)))]
            w = words[rng.integers(len(words))]
            if kind == 2:
                hist = ['<s>'] + hist[:int(rng.integers(0, 3))]
            if kind == 3 and w == '</s>':
                continue
        ctx = lm.context_of([lm.words.index(x) for x in hist])
        raw, nxt = lm.raw(ctx, lm.words.index(w))
        want = ref.cond(tuple(hist), w)
        worst = max(worst, abs(raw / 65536.0 - want))
        assert abs(raw / 65536.0 - want) <= lm.order / 131072.0, (hist, w)
        assert nxt == lm.context_of([lm.words.index(x) for x in hist + [w]])
        n_seen += tuple(hist[-(lm.order - 1):] if lm.order > 1 else []) + (w,) in ref.prob
        n_back += 1
    assert lm.order == 1 or 0 < n_seen < n_back                     # hits of the full order and back-offs both occurred
    assert lm.raw(lm.start, -1) == (ngram.OOV_Q, 0) and ngram.OOV_Q == -1000 * 65536
    if lm.order > 1:
        assert lm.start == lm.context_of([lm.words.index('<s>')]) != 0
    print(f'{name}: largest |raw / 2^16 - float64| = {worst:.3e} (bound {lm.order / 131072.0:.3e})')


def test_word_hash_table_and_oov(golden_dir):
    lm = lm_of(golden_dir, 'en3')
    for w in lm.words:
        if w in ('<s>', '</s>', '<unk>'):
            assert all(lm.word_of_hash.get(h) != lm.words.index(w) for h in lm.word_of_hash)     # cannot be spelled: left out
        else:
            assert lm.lookup_word(ngram.word_hash(_ids(w))) == lm.words.index(w)
    assert lm.lookup_word(ngram.word_hash(_ids('zzzzzzz'))) == -1
    assert ngram.term(-65536, 65536, 0) == -65536 and ngram.term(-3, 1 << 15, 7) == -1 + 7 and ngram.term(ngram.OOV_Q, 0, 5) == 5
    assert ngram.fixed_weights(0.5, -1.5) == (32768, -98304)
    for bad in ((-0.1, 0), (16.5, 0), (1, 17), (1, -16.5), (float('nan'), 0)):
        with pytest.raises(ValueError):
            ngram.fixed_weights(*bad)


# -------------------------------------------------------------------------------------------------- 2. alpha = beta = 0
@pytest.mark.parametrize('name,T,W,N', [('en3', 63, 16, 20), ('en5', 40, 128, 40), ('zh2', 63, 16, 40)])
def test_zero_weights_equal_the_search_without_a_model(golden_dir, name, T, W, N):
    lp, lens = cases.batch_inputs(name, T, 3, 60)
    blank = lp.shape[2] - 1
    a = beam.search_host(lp, lens, blank, W, None, N)
    b = beam.search_host(lp, lens, blank, W, None, N, lm_of(golden_dir, name), 0.0, 0.0)
    for f in ('labels', 'n_labels', 'score', 'n_hyps'):
        assert np.array_equal(getattr(a, f), getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, f
    assert a.lm_score is None and b.lm_score.dtype == np.int64 and not b.lm_score.any()


# -------------------------------------------------------------------------------------------------- 3. twin against oracle
@pytest.mark.parametrize('name', [s[0] for s in cases.CASE_LISTS])
def test_twin_against_the_float64_search(golden_dir, name):
    _, model, T, W, N, alpha, beta, n, seed, sharp = next(s for s in cases.CASE_LISTS if s[0] == name)
    lm = lm_of(golden_dir, model)
    waived = differ = 0
    worst = 0.0
    for lp, want, gap in cases.checked_case_list(name, golden_dir):
        blank = lp.shape[1] - 1
        res = beam.search_host(lp[None], None, blank, W, None, N, lm, alpha, beta)
        best = tuple(res.labels[0, 0, :res.n_labels[0, 0]].tolist())
        score, lms = res.score[0, 0] / 65536.0, res.lm_score[0, 0] / 65536.0
        in_beam = {p: (s, l) for p, s, l in want}
        tol = _bound(T, len(best) + 1, lm.order, alpha)
        assert best in in_beam, name
        assert abs(score - in_beam[best][0]) <= tol and abs(lms - in_beam[best][1]) <= tol
        worst = max(worst, abs(score - in_beam[best][0]))
        if gap < cases.GAP:
            waived += 1
        else:
            assert best == want[0][0], (name, gap)
        no_lm = beam.search_host(lp[None], None, blank, W, None, N)
        differ += tuple(no_lm.labels[0, 0, :no_lm.n_labels[0, 0]].tolist()) != best
    print(f'{name}: gap < {cases.GAP}: {waived}, best string differs from the search without a model: {differ}, '
          f'largest |score - float64| {worst:.5f}')
    assert waived <= cases.MAX_WAIVED * n, 'sharpen the input of this list; the cap and the gap stay'
    assert differ > 0 or W == 1


# -------------------------------------------------------------------------------------------------- 4. the model decides
def _spell(rows, T=None):
    """log-probabilities [1, T, 29] from rows of {char: probability}; '_' is the blank, the rest is spread evenly"""
    out = np.zeros((len(rows), 29))
    for t, r in enumerate(rows):
        rest = (1.0 - sum(r.values())) / (29 - len(r))
        out[t] = rest
        for ch, p in r.items():
            out[t, 28 if ch == '_' else EN.index(ch)] = p
    return np.log(out).astype(np.float32)[None]


def _known_and_unknown(lm):
    """a word of the model of >= 3 letters, and a spelling one letter off that the model does not have"""
    for w in lm.words:
        if len(w) >= 3 and w.isalpha():
            for ch in 'etaoinshr':
                o = w[:-1] + ch
                if o != w and o not in lm.words and w[-1] != w[-2] and ch != w[-2]:
                    return w, o
    raise AssertionError('no such pair')


def test_the_model_changes_the_answer(golden_dir):
    lm = lm_of(golden_dir, 'en3')
    w, o = _known_and_unknown(lm)
    rows = []
    for ch in w[:-1]:
        rows += [{ch: 0.9999}, {'_': 0.9999}]
    rows += [{o[-1]: 0.5, w[-1]: 0.4}, {'_': 0.9999}, {' ': 0.9999}, {'_': 0.9999}]
    lp = _spell(rows)
    # (W = 64: the space costs the word's term at once, the 27 other continuations of the frame pay only at the end)
    plain = beam.search_host(lp, None, 28, 64, None, 20)
    with_lm = beam.search_host(lp, None, 28, 64, None, 20, lm, 1.0, 0.0)
    assert _text(plain) == o + ' ' and ''.join(EN[i] for i in beam_cases.greedy(lp[0], 28)) == o + ' '
    assert _text(with_lm) == w + ' '
    raw = lm.raw(lm.start, lm.words.index(w))[0]
    assert with_lm.lm_score[0, 0] == raw and raw > -20 * 65536
    ref = cases.oracle_beam_lm(lp[0], 64, 20, 28, cases.OracleLM(cases.model_path(golden_dir, 'en3')), EN, 1.0, 0.0)
    assert ref[0][0] == tuple(_ids(w + ' ')) and abs(ref[0][2] - raw / 65536.0) <= _term_bound(3, 1.0)
    assert abs(with_lm.score[0, 0] / 65536.0 - ref[0][1]) <= _bound(len(rows), 1, 3, 1.0)


# -------------------------------------------------------------------------------------------------- 5. word-mode edges
def test_word_mode_edges(golden_dir):
    lm = lm_of(golden_dir, 'en3')
    ref = cases.OracleLM(cases.model_path(golden_dir, 'en3'))
    w, o = _known_and_unknown(lm)
    wid = lm.words.index(w)
    t_w = ngram.term(lm.raw(lm.start, wid)[0], 65536, 32768)                 # alpha 1, beta 0.5
    letters = [r for ch in w for r in ({ch: 0.9999}, {'_': 0.9999})]
    # a leading space scores nothing and keeps <s>; a doubled space scores once
    for rows, text, n_terms in (([{' ': 0.9999}, {'_': 0.9999}] + letters + [{' ': 0.9999}], ' ' + w + ' ', 1),
                                (letters + [{' ': 0.9999}, {'_': 0.9999}, {' ': 0.9999}], w + '  ', 1),
                                ([{' ': 0.9999}, {'_': 0.9999}, {' ': 0.9999}], '  ', 0)):
        res = beam.search_host(_spell(rows), None, 28, 4, None, 20, lm, 1.0, 0.5)
        assert _text(res) == text and res.lm_score[0, 0] == n_terms * t_w, text
        want = cases.oracle_beam_lm(_spell(rows)[0], 4, 20, 28, ref, EN, 1.0, 0.5)
        assert want[0][0] == tuple(_ids(text)) and abs(want[0][2] - res.lm_score[0, 0] / 65536.0) <= _term_bound(3, 1.0)
    # the utterance ends inside a word: before the end pass the unknown spelling leads, the end pass re-orders the beam
    rows = letters[:-2] + [{o[-1]: 0.5, w[-1]: 0.4}]
    lp = _spell(rows)
    plain = beam.search_host(lp, None, 28, 4, 2, 20)
    res = beam.search_host(lp, None, 28, 4, 2, 20, lm, 1.0, 0.5)
    assert [_text(plain, h=h) for h in (0, 1)] == [o, w]
    assert [_text(res, h=h) for h in (0, 1)] == [w, o]
    assert res.lm_score[0].tolist() == [t_w, ngram.term(ngram.OOV_Q, 65536, 32768)]
    assert (res.score[0] - res.lm_score[0]).tolist() == plain.score[0, ::-1].tolist()       # the acoustic part is untouched
    want = cases.oracle_beam_lm(lp[0], 4, 20, 28, ref, EN, 1.0, 0.5)
    assert [p for p, _, _ in want[:2]] == [tuple(_ids(w)), tuple(_ids(o))]
    # two known words: the second is scored in the context of the first
    w2 = next(g[1] for g in ref.prob if len(g) == 2 and g[0] == w and g[1] not in ('</s>',))
    rows = letters + [{' ': 0.9999}] + [r for ch in w2 for r in ({ch: 0.9999}, {'_': 0.9999})]
    res = beam.search_host(_spell(rows), None, 28, 4, None, 20, lm, 1.0, 0.5)
    raw2, _ = lm.raw(lm.raw(lm.start, wid)[1], lm.words.index(w2))
    assert _text(res) == w + ' ' + w2 and res.lm_score[0, 0] == t_w + ngram.term(raw2, 65536, 32768)
    assert abs(raw2 / 65536.0 - ref.cond(('<s>', w), w2)) <= 3 / 131072.0 and (w, w2) in ref.prob
    # an utterance of length 0: the empty hypothesis, nothing scored
    res = beam.search_host(_spell(rows), np.array([0]), 28, 4, None, 20, lm, 1.0, 0.5)
    assert res.n_hyps.tolist() == [1] and res.n_labels[0, 0] == 0 and res.score[0, 0] == 0 and res.lm_score[0, 0] == 0
    assert (res.score[0, 1:] == beam.NEG).all() and not res.lm_score[0, 1:].any()


# -------------------------------------------------------------------------------------------------- 6. qasr_lm_check
def _check(blob, n_labels):
    from qasr import engine
    lib = engine.load_library()
    return lib.qasr_lm_check(bytes(blob), len(blob), n_labels)


def _corruptions(lm, blob):
    """(what, corrupted blob): single-field corruptions of a valid blob, each of which qasr_lm_check must refuse"""
    h = np.frombuffer(blob[:128], '<i4')
    n_nodes, tcap, wcap, n_words, n_labels = int(h[4]), int(h[6]), int(h[9]), int(h[11]), int(h[8])
    t_off, w_off = 128, 128 + 16 * tcap
    n_off = w_off + 16 * wcap
    l_off = n_off + 8 * n_nodes

    def put(off, v):
        b = bytearray(blob)
        b[off:off + 4] = struct.pack('<i', v)
        return bytes(b)

    out = []
    for i, vals in ((0, (0, h[0] ^ 1)), (1, (0, 2)), (2, (0, 7, -1)), (3, (2, -1)), (4, (0, n_nodes + 1, n_nodes - 1)),
                    (5, (-1, n_nodes)), (6, (0, tcap + 1, tcap * 2, tcap // 2)), (7, (0, 1025, tcap + 1)),
                    (8, (0, n_labels + 1)), (9, (0, wcap * 2, wcap + 1)), (10, (0, 1025)), (11, (0, -5)),
                    (12, (len(blob) + 4, 0)), (13, (1,)), (14, (0, 2)), (20, (n_nodes - 1, n_nodes + 1)), (21, (1,)), (31, (9,))):
        out += [(f'header[{i}] = {v}', put(4 * i, int(v))) for v in vals]
    if lm.order > 1:
        out.append((f'level[{lm.order}] short of n_nodes', put(4 * (13 + lm.order), n_nodes - 1)))
        out.append(('level[2] below level[1]', put(4 * 15, 0)))
    rng = np.random.Generator(np.random.PCG64(77))
    trans = np.frombuffer(blob[t_off:w_off], '<i4').reshape(-1, 4)
    used = np.flatnonzero(trans[:, 0] >= 0)
    for s in rng.choice(used, size=4, replace=False):
        out += [(f'trans[{s}].node past the nodes', put(t_off + 16 * s, n_nodes)), (f'trans[{s}].node = -2', put(t_off + 16 * s, -2)),
                (f'trans[{s}].word past the words', put(t_off + 16 * s + 4, n_words)),
                (f'trans[{s}].prob beyond 2^30', put(t_off + 16 * s + 8, -(1 << 30) - 1)),
                (f'trans[{s}].next past the nodes', put(t_off + 16 * s + 12, n_nodes)),
                (f'trans[{s}].next = -1', put(t_off + 16 * s + 12, -1))]
    far = [s for s in used if (s - ngram.trans_slot(trans[s, 0], trans[s, 1], tcap)) % tcap > 0]
    if far:                                              # a key that sits behind others: emptying its home cuts it off
        s = far[0]
        home = ngram.trans_slot(trans[s, 0], trans[s, 1], tcap)
        out.append((f'trans[{home}] emptied before trans[{s}]', put(t_off + 16 * home, -1)))
        out.append(('probe bound below the longest chain', put(4 * 7, 1)))
    for i in rng.choice(np.arange(1, n_nodes), size=min(4, n_nodes - 1), replace=False) if n_nodes > 1 else ():
        out += [(f'suffix cycle at node {i}', put(n_off + 8 * i + 4, int(i))), (f'suffix of node {i} past the nodes', put(n_off + 8 * i + 4, n_nodes)),
                (f'back-off of node {i} beyond 2^30', put(n_off + 8 * i, (1 << 30) + 1))]
    out.append(('suffix of the empty context', put(n_off + 4, 1)))
    if lm.order > 2:                                    # a two-word node whose suffix is a two-word node: no descent
        out.append(('suffix on the same level', put(n_off + 8 * int(h[15]) + 4, int(h[15]) + 1)))
    out += [('label_to_word past the words', put(l_off, n_words)), ('label_to_word = -2', put(l_off + 4 * (n_labels - 1), -2))]
    wt = np.frombuffer(blob[w_off:n_off], '<i4').reshape(-1, 4)
    for s in np.flatnonzero(wt[:, 2] >= 0)[:2]:
        out += [(f'words[{s}].id past the words', put(w_off + 16 * s + 8, n_words)), (f'words[{s}].id = -2', put(w_off + 16 * s + 8, -2))]
    out += [(f'truncated to {n}', blob[:n]) for n in (0, 3, 100, 128, len(blob) - 4, len(blob) - 1)] + [('one byte more', blob + b'\0')]
    return out


@pytest.mark.parametrize('name', ['en3', 'en1', 'en5', 'zh2'])
def test_lm_check(golden_dir, name):
    lm = lm_of(golden_dir, name)
    for tight in (False, True):
        blob = lm.pack(min_capacity=tight)
        assert _check(blob, lm.n_labels) == 0
        assert _check(blob, lm.n_labels + 1) != 0
        n = 0
        for what, bad in _corruptions(lm, blob):
            assert bad != blob, what
            assert _check(bad, lm.n_labels) != 0, (name, tight, what)
            n += 1
        assert n >= 40
    hdr = np.frombuffer(lm.pack(True)[:128], '<i4')
    assert hdr[6] == ngram._pow2_above(len(lm.trans)) and hdr[7] <= ngram.MAX_PROBE      # the smallest capacity
    assert name == 'en1' or hdr[7] > np.frombuffer(lm.pack()[:128], '<i4')[7]


# -------------------------------------------------------------------------------------------------- 7. the facade
def test_module_with_a_model_on_the_host_both_input_forms(golden_dir):
    path = cases.model_path(golden_dir, 'en3')
    lp, lens = cases.batch_inputs('en3', 80, 3, 70)
    lm = lm_of(golden_dir, 'en3')
    want = beam.to_hypotheses(beam.search_host(lp, lens, 28, 8, None, 20, lm, 1.5, 0.5), EN)
    dec = BeamSearchDecoderWithLM(EN, 8, 1.5, 0.5, path, 1, cutoff_top_n=20, input_tensor=True)
    assert isinstance(dec.scorer, ngram.NgramLM) and dec.scorer.order == 3 and dec.scorer.word_mode
    got = dec(torch.from_numpy(lp), torch.from_numpy(lens))
    assert got == [[(h.utt_score, h.text) for h in w] for w in want] and got[2] == [(0.0, '')]
    assert all(h.lm_score is not None and h.lm_score <= 8 * 0.5 for w in want for h in w)
    plain = BeamSearchDecoderWithLM(EN, 8, 1.5, 0.5, None, 1, cutoff_top_n=20, input_tensor=True)(torch.from_numpy(lp), torch.from_numpy(lens))
    assert plain[0][0][1] != got[0][0][1] and plain[0][0][0] > got[0][0][0]
    res = dec.search(torch.from_numpy(lp), torch.from_numpy(lens))
    assert res.lm_score is not None and res.lm_score.shape == res.score.shape
    dec2 = BeamSearchDecoderWithLM(EN, 8, 1.5, 0.5, path, 1, cutoff_top_n=20)
    probs = [np.exp(lp[b, :lens[b]].astype(np.float64)).astype(np.float32) for b in range(2)]
    got2 = dec2(probs, None)
    want2 = beam.to_hypotheses(beam.search_host(np.stack([np.log(np.pad(p, ((0, 80 - len(p)), (0, 0)), constant_values=1.0)) for p in probs]),
                                                lens[:2], 28, 8, None, 20, lm, 1.5, 0.5), EN)
    assert got2 == [[(h.utt_score, h.text) for h in w] for w in want2]
    # the Zh form: a vocabulary without a space makes the model character-based
    zlp, zlens = cases.batch_inputs('zh2', 40, 2, 71)
    zdec = BeamSearchDecoderWithLM(ZH, 4, 1.0, 0.0, cases.model_path(golden_dir, 'zh2'), 1, cutoff_top_n=20, input_tensor=True)
    assert not zdec.scorer.word_mode and zdec.scorer.space == -1
    zwant = beam.to_hypotheses(beam.search_host(zlp, zlens, 5206, 4, None, 20, lm_of(golden_dir, 'zh2'), 1.0, 0.0), ZH)
    assert zdec(torch.from_numpy(zlp), torch.from_numpy(zlens)) == [[(h.utt_score, h.text) for h in w] for w in zwant]


def test_refusals(golden_dir, tmp_path):
    path = cases.model_path(golden_dir, 'en3')
    ok = dict(vocab=EN, beam_width=8, alpha=1.0, beta=0.0, lm_path=path, num_cpus=1)
    BeamSearchDecoderWithLM(**ok)
    for kw in (dict(alpha=-0.5), dict(alpha=16.5), dict(beta=17.0), dict(beta=-16.5)):
        with pytest.raises(ValueError, match='alpha|beta'):
            BeamSearchDecoderWithLM(**dict(ok, **kw))
    with pytest.raises(ValueError, match='1.0'):
        BeamSearchDecoderWithLM(**ok, cutoff_prob=0.9)
    binary = tmp_path / 'model.arpa'
    binary.write_bytes(b'mmap lm http://kheafield.com/code format version 5\n\0' + bytes(200))
    for p in (str(binary), 'lm.binary'):
        with pytest.raises(ModuleNotFoundError, match='ARPA'):
            BeamSearchDecoderWithLM(**dict(ok, lm_path=p))
    with pytest.raises(ValueError, match='space'):                    # a word model, a vocabulary without a space
        BeamSearchDecoderWithLM(**dict(ok, vocab=EN[:26] + ["'"]))
    with pytest.raises(ValueError, match='labels'):
        beam.search_host(np.zeros((1, 4, 20), np.float32), None, 19, 4, None, 10, lm_of(golden_dir, 'en3'), 1.0, 0.0)
    seven = tmp_path / 'seven.arpa'
    seven.write_text('\\data\\\nngram 1=1\nngram 7=1\n\n\\1-grams:\n-1.0\ta\n\n\\7-grams:\n-1.0\ta a a a a a a\n\n\\end\\\n')
    with pytest.raises(ValueError, match='1 .. 6'):
        ngram.NgramLM.from_arpa(str(seven), EN)
    with pytest.raises(ValueError, match='ARPA'):
        (tmp_path / 'junk.arpa').write_text('hello\n')
        ngram.NgramLM.from_arpa(str(tmp_path / 'junk.arpa'), EN)


def test_facade_decode_with_a_model_on_the_host_modules(golden_dir):
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')
    from qasr import synth
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7))
    lens = torch.tensor([96, 61, 12])
    vocab = m.decoder.vocabulary
    assert sorted(vocab) == sorted(EN)                     # the same labels in the model's own order (space first)
    path = cases.model_path(golden_dir, 'en3')
    lm = ngram.NgramLM.from_arpa(path, vocab)
    logp, enc_len, _ = m(processed_signal=x, processed_signal_length=lens)
    want = beam.to_hypotheses(beam.search_host(logp.numpy(), enc_len.numpy(), len(vocab), 8, 3, 40, lm, 0.8, 1.0), vocab)
    one = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, lm=path, alpha=0.8, beta=1.0)
    many = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, n_best=3, lm=lm, alpha=0.8, beta=1.0)
    assert [(h.text, h.utt_score, h.lm_score) for h in one] == [(w[0].text, w[0].utt_score, w[0].lm_score) for w in want]
    assert [[(h.text, h.labels, h.utt_score, h.lm_score) for h in hs] for hs in many] == \
        [[(h.text, h.labels, h.utt_score, h.lm_score) for h in w] for w in want]
    assert all(isinstance(h.lm_score, float) for h in one)
    assert all(h.lm_score is None for h in m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8))
    assert len(m._lm_cache) == 1
    m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, lm=path, alpha=0.2)
    assert len(m._lm_cache) == 1                            # a sweep loads once

    def no_forward(*a, **k):
        raise AssertionError('a refused argument must not cost a forward')
    m._forward = no_forward
    for kw in (dict(beam_width=4, lm=path, alpha=17.0), dict(beam_width=4, lm=path, beta=-20.0), dict(lm=path),
               dict(beam_width=4, lm=lm_of(golden_dir, 'zh2'))):
        with pytest.raises(ValueError):
            m.decode(processed_signal=x, processed_signal_length=lens, **kw)
