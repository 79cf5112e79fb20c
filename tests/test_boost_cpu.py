"""Phrase boosting on the host (no GPU): the automaton of qasr/boost.py against a brute-force substring sum, the packed
form, the NumPy twin (qasr.beam with boost=) against an independent float64 search, its invariants and edges,
qasr_boost_check, the refusals, and decode(boost=) / BeamSearchDecoderWithLM(boost=) / the CLI's phrase file on the host
(the CLI itself needs a GPU: tests/test_gpu_boost_facade.py)."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_cases  # noqa: E402
import beam_lm_cases as lm_cases  # noqa: E402
import boost_cases as cases  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from nemo.collections.asr.modules import BeamSearchDecoderWithLM  # noqa: E402
from qasr import beam, boost, ngram  # noqa: E402

torch.set_grad_enabled(False)
EN, ZH = lm_cases.EN_VOCAB, lm_cases.ZH_VOCAB
SP = EN.index(' ')
_models = {}


def lm_of(golden_dir, name):
    if name not in _models:
        _models[name] = ngram.NgramLM.from_arpa(lm_cases.model_path(golden_dir, name), lm_cases.vocab_of(name))
    return _models[name]


def _set(phrases, whole, space=3, n_labels=4, **kw):
    return boost.PhraseSet(phrases, n_labels=n_labels, space=space if whole else None, whole_words=whole, **kw)


def _rows(res, b):
    return [tuple(res.labels[b, h, :res.n_labels[b, h]].tolist()) for h in range(int(res.n_hyps[b]))]


def _same(a, b):
    for f in ('labels', 'n_labels', 'score', 'n_hyps'):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    return True


# ------------------------------------------------------------------------------------- 0. the fixture
def test_recorded_twin_outputs(golden_dir):
    """tests/golden/boost.npz: what the twin and the packer gave when the fixture was written (gen_golden_boost.py)"""
    sys.path.insert(0, golden_dir)
    import gen_golden_boost as gen
    d = np.load(os.path.join(golden_dir, 'boost.npz'))
    assert [c['name'] for c in __import__('json').loads(str(d['meta']))['cases']] == [s[0] for s in cases.FIXTURE_LISTS]
    for spec in cases.FIXTURE_LISTS:
        res, ps = gen.run(spec, golden_dir)
        for f in ('labels', 'n_labels', 'score', 'boost_score', 'n_hyps') + (('lm_score',) if spec[1] else ()):
            assert np.array_equal(getattr(res, f), d[f'{f}_{spec[0]}']), (spec[0], f)
        assert ps.pack() == d[f'blob_{spec[0]}'].tobytes(), spec[0]
        assert res.boost_score.any()


# ------------------------------------------------------------------------------------- 1. the automaton and its packing
@pytest.mark.parametrize('whole', [False, True])
def test_running_sum_equals_the_brute_force_substring_sum(whole):
    rng = np.random.Generator(np.random.PCG64(900 + whole))
    n = 0
    for it in range(400):
        ph = [(p, 1.0) for p in cases.NESTED] if it == 0 else cases.random_set(rng, 4, whole, 3)
        ps, br = _set(ph, whole), cases.Brute(ph, whole, 3)
        assert ps.pot[ps.start] == 0 and ps.bank[ps.start] == 0
        for _ in range(6):
            y = [int(c) for c in rng.integers(0, 4, size=int(rng.integers(0, 13)))]
            s, tot = ps.start, 0
            for c in y:
                tm, s = ps.term(s, c)
                tot += tm
            assert tot == br.running(y) == br.running_fast(y), (ph, y)          # not finalised
            assert tot + ps.finish(s) == ps.score(y) == br.final(y), (ph, y)    # finalised
            n += 1
    assert n == 2400


def test_nested_set_by_hand():
    """ab, abab, bab, b at 1 nat per label in 'abab': ab twice (2 each), abab behind its prefix ab (2), bab behind its
    prefix b (2), b twice (1 each)"""
    ps = _set([(p, 1.0) for p in cases.NESTED], False)
    assert ps.score([0, 1, 0, 1]) == 10 * 65536 and ps.score([0]) == 0 and ps.score([0, 0, 1]) == 3 * 65536
    heavy = _set([((0, 1), 1.0), ((0, 1, 0), 3.0), ((0, 1), 2.0)], False)      # duplicates and shared prefixes: the max rule
    assert heavy.score([0, 1]) == 6 * 65536 and heavy.score([0, 1, 0]) == 9 * 65536


@pytest.mark.parametrize('whole', [False, True])
def test_pack_unpack_and_delta_equal_the_dict_automaton(whole):
    rng = np.random.Generator(np.random.PCG64(910 + whole))
    longer = 0
    for it in range(60):
        ph = cases.random_set(rng, 4, whole, 3)
        ps = _set(ph, whole)
        for tight in (False, True):
            blob = ps.pack(min_capacity=tight)
            v = boost.PackedView(blob)
            h = np.frombuffer(blob[:128], '<i4')
            assert (v.n_nodes, v.n_labels, v.start, v.whole_words) == (ps.n_nodes, 4, ps.start, whole)
            assert h[2] == len(blob) and h[7] & (h[7] - 1) == 0 and 1 <= h[8] <= ngram.MAX_PROBE and not h[9:].any()
            assert np.array_equal(v.pot, ps.pot) and np.array_equal(v.bank, ps.bank)
            for s in range(ps.n_nodes):
                for c in range(-1, 6):
                    assert v.delta(s, c) == ps.delta(s, c)
            stored = v.table[v.table[:, 0] >= 0]
            assert all(int(e[0]) != 0 and int(e[2]) != int(v.root_next[e[1]]) for e in stored)    # only what differs from the root row
        longer += np.frombuffer(ps.pack(True)[:128], '<i4')[8] > np.frombuffer(ps.pack()[:128], '<i4')[8]
    assert longer > 0                                       # the minimal capacity does make longer probe runs


# ------------------------------------------------------------------------------------- 2. the twin against the float64 oracle
@pytest.mark.parametrize('name', [s[0] for s in cases.CASE_LISTS])
def test_twin_against_the_float64_search(name):
    """Best strings equal except where the oracle's top-1 / top-2 gap is below beam_cases.GAP (at most MAX_WAIVED of a list,
    asserted in the generator on the oracle alone); scores within the bound of test_beam_cpu.py (100 T / 2^16) plus half a
    unit of 2^-16 per phrase weight; boost_score of the best string exact against the brute-force sum."""
    lst = cases.checked_case_list(name)
    changed = waived = 0
    for lp, blank, W, N, phrases, whole, space, o, gap, plain in lst:
        vocab = cases.vocab_for(lp.shape[1])
        ps = boost.PhraseSet(phrases, vocab)
        assert ps.whole_words == whole
        res = beam.search_host(lp[None], None, blank, W, None, N, boost=ps)
        got = _rows(res, 0)[0]
        br = cases.Brute(phrases, whole, space)
        assert res.boost_score[0, 0] == br.final(got)
        if got != o[0][0]:
            assert gap < cases.GAP, (name, gap)
            waived += 1
            continue
        assert abs(res.score[0, 0] / 65536.0 - o[0][1]) <= 100.0 * lp.shape[0] / 65536.0 + len(phrases) * 64 / 131072.0
        assert abs(res.boost_score[0, 0] / 65536.0 - o[0][2]) < 1e-9
        changed += got != plain
    print(f'{name}: {changed} of {len(lst)} best strings differ from the unboosted search, {waived} waived')
    assert waived <= cases.MAX_WAIVED * len(lst)
    assert changed >= 1


# ------------------------------------------------------------------------------------- 3. invariants of the twin
def test_weight_zero_is_the_plain_search_on_every_byte(golden_dir):
    for C, T, W, N, seed in ((29, 63, 16, 40, 1), (29, 63, 1, 20, 2), (5207, 40, 8, 20, 3)):
        rng = np.random.Generator(np.random.PCG64(seed))
        lp = np.stack([beam_cases.peaky_logp(rng, T, C, C - 1) for _ in range(3)])
        lens = np.array([T, T // 2, 0])
        vocab = cases.vocab_for(C)
        ph = [(p, 0.0) for p, _ in cases.gpu_phrases(rng, lp, lens, C - 1, C == 29, SP)]
        ps = boost.PhraseSet(ph, vocab)
        plain = beam.search_host(lp, lens, C - 1, W, None, N)
        res = beam.search_host(lp, lens, C - 1, W, None, N, boost=ps)
        assert _same(plain, res) and res.lm_score is None and not res.boost_score.any()
    for model, T in (('en3', 63), ('zh2', 40)):
        lm = lm_of(golden_dir, model)
        lp, lens = lm_cases.batch_inputs(model, T, 3, 55)
        rng = np.random.Generator(np.random.PCG64(5))
        ph = [(p, 0.0) for p, _ in cases.gpu_phrases(rng, lp, lens, lm.n_labels, lm.word_mode, lm.space)]
        ps = boost.PhraseSet(ph, lm_cases.vocab_of(model))
        plain = beam.search_host(lp, lens, lm.n_labels, 8, None, 20, lm, 1.2, 0.5)
        res = beam.search_host(lp, lens, lm.n_labels, 8, None, 20, lm, 1.2, 0.5, boost=ps)
        assert _same(plain, res) and np.array_equal(plain.lm_score, res.lm_score) and not res.boost_score.any()


@pytest.mark.parametrize('model', [None, 'en3', 'zh2'])
def test_boost_score_of_every_row_is_the_brute_force_sum(golden_dir, model):
    lm = None if model is None else lm_of(golden_dir, model)
    if model is None:
        rng = np.random.Generator(np.random.PCG64(31))
        lp = np.stack([beam_cases.peaky_logp(rng, 63, 29, 28) for _ in range(3)])
        lens = np.array([63, 31, 0])
        vocab, whole, space = EN, True, SP
    else:
        lp, lens = lm_cases.batch_inputs(model, 63, 3, 56)
        vocab, whole, space = lm_cases.vocab_of(model), lm.word_mode, lm.space
    rng = np.random.Generator(np.random.PCG64(32))
    ph = cases.gpu_phrases(rng, lp, lens, len(vocab), whole, space)
    ps, br = boost.PhraseSet(ph, vocab), cases.Brute(ph, whole, space)
    res = beam.search_host(lp, lens, len(vocab), 16, None, 20, lm, 0.7, 0.3, boost=ps)
    assert res.boost_score.any()
    for b in range(3):
        rows = _rows(res, b)
        assert len(rows) == len(set(rows)) >= 1
        for h, y in enumerate(rows):
            assert res.boost_score[b, h] == br.final(y), (b, h)
        assert (np.diff(res.score[b, :len(rows)]) <= 0).all()               # the one re-ordering left the beam sorted
        assert not res.boost_score[b, len(rows):].any()
    assert res.n_hyps[2] == 1 and res.n_labels[2, 0] == 0 and res.score[2, 0] == 0 and res.boost_score[2, 0] == 0


def test_score_minus_the_shares_is_the_acoustic_score_where_the_beam_is_the_same(golden_dir):
    """W = 1: the beam is one prefix per frame, so 'the same beam' can be checked - the labels after every frame count t
    agree with the plain search's.  Then score - lm_score - boost_score is the plain score of that prefix, exactly: every
    contribution to pb and pnb of the single entry carries the same sum of terms, and lae(a + k, b + k) = lae(a, b) + k."""
    lm = lm_of(golden_dir, 'en3')
    lp, _ = lm_cases.batch_inputs('en3', 48, 2, 57)
    T = lp.shape[1]
    plain_full = beam.search_host(lp, None, 28, 1, None, 20)
    n_same = 0
    for b in range(2):
        y0 = list(_rows(plain_full, b)[0])
        words = [w for w in ''.join(EN[c] for c in y0).split(' ') if w]
        ps = boost.PhraseSet([(w, 0.25) for w in words[:4]], EN)          # pieces of the plain path itself, gently
        lens_all = np.arange(1, T + 1)
        rep = np.repeat(lp[b:b + 1], T, axis=0)
        plain = beam.search_host(rep, lens_all, 28, 1, None, 20)
        res = beam.search_host(rep, lens_all, 28, 1, None, 20, lm, 0.05, 0.0, boost=ps)
        same = all(_rows(plain, t) == _rows(res, t) for t in range(T))
        if same:
            n_same += 1
            assert np.array_equal(res.score - res.lm_score - res.boost_score, plain.score)
            assert res.boost_score[T - 1, 0] > 0
    assert n_same >= 1


def _spell(rows):
    out = np.zeros((len(rows), 29))
    for t, r in enumerate(rows):
        out[t] = (1.0 - sum(r.values())) / (29 - len(r))
        for ch, p in r.items():
            out[t, 28 if ch == '_' else EN.index(ch)] = p
    return np.log(out).astype(np.float32)[None]


def _letters(text):
    rows, prev = [], None
    for ch in text:
        if ch == prev:
            rows.append({'_': 0.9999})
        rows.append({ch: 0.9999})
        prev = ch
    return rows


def _text(res, b=0, h=0):
    return ''.join(EN[i] for i in res.labels[b, h, :res.n_labels[b, h]])


def test_edges(golden_dir):
    w = 65536
    ps = boost.PhraseSet(['cat', ('dog', 2.0), 'at'], EN)
    # a phrase at the utterance's start and one at its end count (the virtual spaces); 'at' inside 'cat' is no whole word
    res = beam.search_host(_spell(_letters('cat and dog')), None, 28, 4, None, 20, boost=ps)
    assert _text(res) == 'cat and dog' and res.boost_score[0, 0] == 3 * w + 6 * w
    # a doubled space ends one word and starts the next; leading and trailing spaces change nothing
    res = beam.search_host(_spell(_letters(' cat  dog ')), None, 28, 4, None, 20, boost=ps)
    assert _text(res) == ' cat  dog ' and res.boost_score[0, 0] == 9 * w
    # an unfinished match earns nothing: 'do' and 'cats' hold no phrase
    res = beam.search_host(_spell(_letters('cats do')), None, 28, 4, None, 20, boost=ps)
    assert _text(res) == 'cats do' and res.boost_score[0, 0] == 0
    # without whole words the same phrases match inside words
    sub = boost.PhraseSet(['cat', ('dog', 2.0), 'at'], EN, whole_words=False)
    res = beam.search_host(_spell(_letters('cats do')), None, 28, 4, None, 20, boost=sub)
    assert res.boost_score[0, 0] == 3 * w + 2 * w
    # lens = 0 and lens < T
    lp = np.repeat(_spell(_letters('cat dog')), 3, axis=0)
    res = beam.search_host(lp, np.array([0, 5, 99]), 28, 4, None, 20, boost=ps)
    assert res.n_hyps[0] == 1 and res.n_labels[0, 0] == 0 and res.score[0, 0] == 0 and res.boost_score[0, 0] == 0
    assert (res.score[0, 1:] == beam.NEG).all()
    assert _text(res, 1) == 'cat d' and res.boost_score[1, 0] == 3 * w
    assert _text(res, 2) == 'cat dog' and res.boost_score[2, 0] == 9 * w
    # boosting changes the answer: 'cab' leads acoustically, the phrase 'cat' wins - but only once the word has ended
    rows = _letters('ca') + [{'b': 0.5, 't': 0.4}]
    plain = beam.search_host(_spell(rows), None, 28, 4, 2, 20)
    res = beam.search_host(_spell(rows), None, 28, 4, 2, 20, boost=ps)
    assert [_text(plain, h=h) for h in (0, 1)] == ['cab', 'cat'] and [_text(res, h=h) for h in (0, 1)] == ['cat', 'cab']
    assert res.boost_score[0].tolist() == [3 * w, 0]
    assert (res.score[0] - res.boost_score[0]).tolist() == plain.score[0, ::-1].tolist()
    # with a word-mode model the model's unfinished-word term and the boost's correction share the ONE re-ordering pass
    lm = lm_of(golden_dir, 'en3')
    known = next(x for x in lm.words if len(x) >= 3 and x.isalpha() and x[-1] != x[-2])
    other = next(known[:-1] + ch for ch in 'etaoinshr' if known[:-1] + ch not in lm.words and ch != known[-2])
    rows = _letters(known[:-1]) + [{known[-1]: 0.5, other[-1]: 0.4}]
    t_known = ngram.term(lm.raw(lm.start, lm.words.index(known))[0], 65536, 0)
    t_oov = ngram.term(ngram.OOV_Q, 65536, 0)
    # the phrase backs the unknown spelling with less than the model takes from it: the model's word stays first ...
    gain = min((t_known - t_oov) // (2 * len(other)), 16 * w)
    ps2 = boost.PhraseSet([(other, gain / w)], EN)
    plain = beam.search_host(_spell(rows), None, 28, 4, 2, 20)
    res = beam.search_host(_spell(rows), None, 28, 4, 2, 20, lm, 1.0, 0.0, boost=ps2)
    assert [_text(res, h=h) for h in (0, 1)] == [known, other]
    assert res.lm_score[0].tolist() == [t_known, t_oov] and res.boost_score[0].tolist() == [0, ps2.score([EN.index(c) for c in other])]
    assert (res.score[0] - res.lm_score[0] - res.boost_score[0]).tolist() == plain.score[0].tolist()
    # ... and with alpha 0 the same phrase alone turns the order round
    res = beam.search_host(_spell(rows), None, 28, 4, 2, 20, lm, 0.0, 0.0, boost=ps2)
    assert [_text(res, h=h) for h in (0, 1)] == [other, known] and not res.lm_score.any()


# ------------------------------------------------------------------------------------- 4. the validator and the refusals
def _check(blob, n_labels):
    from qasr import engine
    lib = engine.load_library()
    rc = lib.qasr_boost_check(bytes(blob), len(blob), n_labels)
    return rc, lib.qasr_last_error().decode()


def test_boost_check_refuses_single_field_corruptions():
    rng = np.random.Generator(np.random.PCG64(77))
    ph = [(p, 1.0) for p in cases.NESTED] + cases.random_set(rng, 4, False) + [((0, 1, 2, 3, 0, 1, 2), 2.0), ((2, 3, 0, 1), 1.5)]
    ps = _set(ph, False)
    n = 0
    for tight in (False, True):
        blob = ps.pack(min_capacity=tight)
        assert _check(blob, 4)[0] == 0
        assert _check(blob, 5)[0] == 2
        h = np.frombuffer(blob[:128], '<i4')
        n_nodes, cap = int(h[3]), int(h[7])
        t_off, n_off = 128, 128 + 16 * cap
        r_off = n_off + 8 * n_nodes

        def put(off, v):
            b = bytearray(blob)
            b[off:off + 4] = struct.pack('<i', int(v))
            return bytes(b)

        bad = []
        for i, vals, word in ((0, (0, h[0] ^ 1), 'magic'), (1, (0, 2), 'version'), (2, (len(blob) + 4, 0), 'bytes'),
                              (3, (0, n_nodes + 1, n_nodes - 1), ''), (4, (0, 5), 'labels'), (5, (-1, n_nodes), 'start'),
                              (6, (2, -1), 'whole_words'), (7, (0, cap + 1, cap * 2, cap // 2, 3 * cap // 2), ''),
                              (8, (0, 1025, cap + 1), 'probe'), (9, (1,), 'reserved'), (31, (9,), 'reserved')):
            bad += [(f'header[{i}] = {v}', put(4 * i, v), word) for v in vals]
        table = np.frombuffer(blob[t_off:n_off], '<i4').reshape(-1, 4)
        used = np.flatnonzero(table[:, 0] >= 0)
        assert len(used) >= 4
        for s in used[:3]:
            bad += [(f'table[{s}].next past the nodes', put(t_off + 16 * s + 8, n_nodes), 'next'),
                    (f'table[{s}].next = -1', put(t_off + 16 * s + 8, -1), 'next'),
                    (f'table[{s}].node past the nodes', put(t_off + 16 * s, n_nodes), 'node'),
                    (f'table[{s}].node = root', put(t_off + 16 * s, 0), 'node'),
                    (f'table[{s}].label past the labels', put(t_off + 16 * s + 4, 4), 'label'),
                    (f'table[{s}] pad word', put(t_off + 16 * s + 12, 1), 'slot')]
        far = [s for s in used if (s - ngram.trans_slot(table[s, 0], table[s, 1], cap)) % cap > 0]
        if tight:
            assert far                                     # the minimal capacity displaces slots
        if far:
            s = far[0]
            home = ngram.trans_slot(table[s, 0], table[s, 1], cap)
            bad += [(f'table[{home}] emptied before table[{s}]', put(t_off + 16 * home, -1), 'cut off'),
                    ('a probe bound too small for a displaced slot', put(4 * 8, 1), 'probe bound')]
        bad += [('pot beyond the bound', put(n_off + 8 * 2, (1 << 30) + 1), 'pot'), ('a negative pot', put(n_off + 8, -1), 'pot'),
                ('bank beyond the bound', put(n_off + 8 * 2 + 4, (1 << 30) + 1), 'bank'),
                ('root_next past the nodes', put(r_off, n_nodes), 'root_next'), ('root_next = -1', put(r_off + 12, -1), 'root_next')]
        bad += [(f'truncated to {k}', blob[:k], '') for k in (0, 3, 100, 128, len(blob) - 4, len(blob) - 1)] + [('one byte more', blob + b'\0', '')]
        for what, b, word in bad:
            assert b != blob, what
            rc, msg = _check(b, 4)
            assert rc == 2 and msg.startswith('boost_check:') and word in msg, (tight, what, rc, msg)
            n += 1
    assert n >= 80
    from qasr import engine
    with pytest.raises(engine.QasrError, match='magic'):
        engine.boost_check(b'\0' * 256, 4)


def test_refusals_of_the_python_layer():
    for bad, why in (([], 'empty'), ([''], 'empty'), (['  '], 'empty'), (['café'], 'vocabulary'), (['a' * 65], '64'),
                     ([[28]], 'blank'), ([[3, -1]], 'label'), ([('cat', -0.5)], 'weight'), ([('cat', 16.5)], 'weight'),
                     ('cat', 'list')):
        with pytest.raises(ValueError, match=why):
            boost.PhraseSet(bad, EN)
    with pytest.raises(ValueError, match='weight'):
        boost.PhraseSet(['cat'], EN, weight=17)
    with pytest.raises(ValueError, match='space'):
        boost.PhraseSet(['一'], ZH, whole_words=True)
    assert boost.PhraseSet(['a' * 64], EN).n_nodes == 67 and not boost.PhraseSet(['一丁'], ZH).whole_words
    assert boost.PhraseSet([' cat ', 'cat', ('cat', 0.5)], EN).compiled == boost.PhraseSet(['cat'], EN).compiled      # duplicates merge
    with pytest.raises(ValueError, match='2\\^30'):         # the 64 suffixes of 64 distinct labels at 16 nats: 16 * 2080 nats end at once
        boost.PhraseSet([(''.join(ZH[k:64]), 16.0) for k in range(64)], ZH)
    assert boost.PhraseSet([(''.join(ZH[k:64]), 7.0) for k in range(64)], ZH).bank.max() == 7 * 2080 * 65536
    ps = boost.PhraseSet(['cat'], EN)
    lp = np.zeros((1, 4, 20), np.float32)
    with pytest.raises(ValueError, match='labels'):
        beam.search_host(lp, None, 19, 4, None, 10, boost=ps)
    with pytest.raises(ValueError, match='labels'):
        boost.as_phrase_set(ps, ZH)
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)

    def no_forward(*a, **k):
        raise AssertionError('a refused argument must not cost a forward')
    m._forward = no_forward
    x, lens = torch.zeros(1, 16, 32), torch.tensor([32])
    for kw in (dict(boost=['cat']), dict(beam_width=4, boost=[]), dict(beam_width=4, boost=['café']),
               dict(beam_width=4, boost=['cat'], boost_weight=17.0), dict(beam_width=4, boost=boost.PhraseSet(['一'], ZH))):
        with pytest.raises(ValueError):
            m.decode(processed_signal=x, processed_signal_length=lens, **kw)
    with pytest.raises(ValueError, match='vocabulary'):
        BeamSearchDecoderWithLM(EN, 8, 0.0, 0.0, None, 1, boost=['café'])
    with pytest.raises(TypeError):                          # keyword-only: the positional signature is the reference's
        BeamSearchDecoderWithLM(EN, 8, 0.0, 0.0, None, 1, 1.0, 40, False, ['cat'])


# ------------------------------------------------------------------------------------- 5. the host surface
def test_module_and_facade_on_the_host(golden_dir, tmp_path):
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')
    from qasr import synth
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7))
    lens = torch.tensor([96, 61, 12])
    vocab = m.decoder.vocabulary
    logp, enc_len, _ = m(processed_signal=x, processed_signal_length=lens)
    plain = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, n_best=3)
    assert all(h.boost_score is None for hs in plain for h in hs)
    words = [w for hs in plain for h in hs[1:] for w in h.text.split(' ') if w][:6] or ['a']
    phrases = [words[0]] + [(w, 2.5) for w in words[1:]]
    ps = boost.PhraseSet(phrases, vocab, weight=1.5)
    want = beam.to_hypotheses(beam.search_host(logp.numpy(), enc_len.numpy(), len(vocab), 8, 3, 40, boost=ps), vocab)
    many = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, n_best=3, boost=phrases, boost_weight=1.5)
    one = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, boost=ps)
    key = lambda h: (h.text, h.labels, h.utt_score, h.boost_score, h.lm_score)      # noqa: E731
    assert [[key(h) for h in hs] for hs in many] == [[key(h) for h in w] for w in want]
    assert [key(h) for h in one] == [key(w[0]) for w in want]
    assert all(isinstance(h.boost_score, float) and h.lm_score is None for h in one) and any(h.boost_score > 0 for hs in many for h in hs)
    timed = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, boost=ps, timestamps=True)
    assert [key(h) for h in timed] == [key(h) for h in one]
    assert all(len(h.start_s) == len(h.labels) for h in timed) and any(h.start_s for h in timed)
    # with a model as well
    path = lm_cases.model_path(golden_dir, 'en3')
    lm = ngram.NgramLM.from_arpa(path, vocab)
    want = beam.to_hypotheses(beam.search_host(logp.numpy(), enc_len.numpy(), len(vocab), 8, 1, 40, lm, 0.8, 1.0, ps), vocab)
    both = m.decode(processed_signal=x, processed_signal_length=lens, beam_width=8, lm=lm, alpha=0.8, beta=1.0, boost=ps)
    assert [key(h) for h in both] == [key(w[0]) for w in want] and all(h.lm_score is not None for h in both)
    # the module: tensors and the reference's list form
    dec = BeamSearchDecoderWithLM(vocab, 8, 0.0, 0.0, None, 1, cutoff_top_n=40, input_tensor=True, boost=phrases, boost_weight=1.5)
    full = beam.to_hypotheses(beam.search_host(logp.numpy(), enc_len.numpy(), len(vocab), 8, None, 40, boost=ps), vocab)
    assert dec(logp, enc_len) == [[(h.utt_score, h.text) for h in w] for w in full]
    assert dec.search(logp, enc_len).boost_score is not None
    dec_lm = BeamSearchDecoderWithLM(vocab, 8, 0.8, 1.0, lm, 1, cutoff_top_n=40, input_tensor=True, boost=ps)
    assert [r[0] for r in dec_lm(logp, enc_len)] == [(w[0].utt_score, w[0].text) for w in want]
    # the phrase file of the CLI
    f = tmp_path / 'phrases.txt'
    f.write_text('# names\n\nnew york\t2.5\nboston\n  \nsan jose\t0\n', encoding='utf-8')
    assert boost.read_phrase_file(str(f)) == [('new york', 2.5), 'boston', ('san jose', 0.0)]
    f.write_text('boston\theavy\n', encoding='utf-8')
    with pytest.raises(ValueError, match='phrases.txt:1'):
        boost.read_phrase_file(str(f))

