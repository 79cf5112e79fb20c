"""qasr.edit on the host: the twin edit_host against the existing metric (its Levenshtein distance, word_error_rate, the
reference's known answers), against a full-matrix DP with a back-trace that shares no code with it, and the rules around it -
word cutting, totals, oracle, absent and invalid rows, refusals - and the two facades on CPU tensors."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edit_cases as ec  # noqa: E402
from nemo.collections.asr.metrics import wer as W  # noqa: E402
from qasr import edit  # noqa: E402

CASES = ec.small_cases()
IDS = [n for n, _ in CASES]
WIDE = chr(0x3000)                      # the ideographic space: str.isspace() and str.split() know it
ALPHABET = [' ', '\t', WIDE] + list("abcdefghijklmnopqrstuvwxyz'") + list('GPUB')


def _host(case, mode, **kw):
    return edit.edit_host(case['hyp'], case['hyp_lens'], case['ref'], case['ref_lens'], case['C'], mode=mode,
                          is_space=case['is_space'], rows_per_ref=case['K'], **kw)


def _units(case, p, mode):
    b = p // case['K']
    return (ec.units(case['hyp'][p], case['hyp_lens'][p], mode, case['is_space']),
            ec.units(case['ref'][b], case['ref_lens'][b], mode, case['is_space']))


@pytest.mark.parametrize('mode', ['char', 'word'])
@pytest.mark.parametrize('name,case', CASES, ids=IDS)
def test_errors_equal_the_metrics_levenshtein_and_the_split_a_backtrace(name, case, mode):
    res = _host(case, mode)
    assert res.rows.dtype == np.int32 and res.rows.shape == (len(case['hyp']), 8)
    for p in range(len(case['hyp'])):
        h, r = _units(case, p, mode)
        e, S, D, I, nr, nh, ok, z = (int(x) for x in res.rows[p])
        assert ok == 1 and z == 0
        assert e == W._levenshtein(h, r), (name, p)
        assert (e, S, D, I) == ec.full_matrix(h, r), (name, p)
        assert (nr, nh) == (len(r), len(h))
        hits = nr - S - D
        assert S + D + I == e and hits + S + D == nr and hits + S + I == nh and hits >= 0


def test_ties_take_the_diagonal_then_the_deletion_then_the_insertion():
    by = dict(CASES)
    assert _host(by['swap'], 'word').rows[0, :4].tolist() == [2, 2, 0, 0]          # two substitutions, not a deletion and an insertion
    assert _host(by['repeated'], 'word').rows[0, :4].tolist() == [2, 0, 0, 2]
    assert _host(by['one_of_repeated'], 'word').rows[0, :4].tolist() == [2, 0, 2, 0]
    # "a" against "a a a": the back-trace takes the diagonal at the LAST occurrence, the two deletions lie in front of it
    assert ec.full_matrix([1], [1, 1, 1]) == (2, 0, 2, 0)
    assert _host(by['last_id_differs'], 'word').rows[0, :4].tolist() == [1, 1, 0, 0]


@pytest.mark.parametrize('use_cer', [False, True])
def test_rates_equal_word_error_rate_on_the_joined_strings(use_cer):
    g = np.random.default_rng(3)
    vocab = ALPHABET
    texts = [''.join(vocab[i] for i in g.choice([0, 0, 0, 1, 2] + list(range(3, 12)), int(n))) for n in g.integers(0, 40, 24)]
    hyps, refs = texts[:12], texts[12:]
    case = ec.from_lists(ec.encode(hyps, vocab), ec.encode(refs, vocab), len(vocab), is_space=edit.space_mask(vocab))
    res = _host(case, 'char' if use_cer else 'word')
    t = res.totals
    want = W.word_error_rate(hyps, refs, use_cer=use_cer)
    assert t[edit.T_ERRORS] / t[edit.T_REF] == want
    assert edit.error_counts(hyps, refs, use_cer=use_cer).rate == want
    assert W.word_error_rate(hyps, refs, use_cer=use_cer, device='cpu') == want
    for p, (h, r) in enumerate(zip(hyps, refs)):
        units = (list(h), list(r)) if use_cer else (h.split(), r.split())
        assert res.rows[p, 0] == W._levenshtein(*units) and res.rows[p, 4] == len(units[1]) and res.rows[p, 5] == len(units[0])


def test_the_references_known_answers(golden_dir):
    entries = json.load(open(os.path.join(golden_dir, 'wer.json')))
    assert len(entries) == 6
    for e in entries:
        assert edit.error_counts(e['hyp'], e['ref']).rate == e['wer'] == W.word_error_rate(e['hyp'], e['ref'])
        assert W.word_error_rate(e['hyp'], e['ref'], device='cpu') == e['wer']
        vocab = sorted(set(''.join(e['hyp'] + e['ref']) + ' '))
        case = ec.from_lists(ec.encode(e['hyp'], vocab), ec.encode(e['ref'], vocab), len(vocab), is_space=edit.space_mask(vocab))
        t = _host(case, 'word').totals
        assert t[edit.T_ERRORS] / t[edit.T_REF] == e['wer']


@pytest.mark.parametrize('text', ['', ' ', '  \t ', 'ab', ' ab', 'ab ', 'a  b', f'\ta{WIDE}{WIDE}b \t', f'a{WIDE}b\tc d', ' a b  c   '])
def test_word_cutting_is_str_split(text):
    vocab = ALPHABET
    mask = edit.space_mask(vocab)
    ids = ec.encode([text], vocab)[0]
    got = edit._row_units(np.array(ids + [0], dtype=np.int32), len(ids), 1, mask)
    assert [''.join(vocab[c] for c in w) for w in got] == text.split()
    case = ec.from_lists([ids], [ids], len(vocab), is_space=mask)
    row = _host(case, 'word').rows[0]
    assert row[:4].tolist() == [0, 0, 0, 0] and row[4] == row[5] == len(text.split())
    assert _host(case, 'char').rows[0, 4] == len(text)


@pytest.mark.parametrize('name,case', CASES, ids=IDS)
def test_totals_are_the_sum_of_the_rows_and_the_oracle_the_minimum(name, case):
    start = np.arange(100, 116, dtype=np.int64)
    res = _host(case, 'word', totals=start)
    assert start[0] == 100                                          # the caller's block is not written
    K = case['K']
    rows = res.rows.astype(np.int64).reshape(-1, K, 8)
    first = rows[:, 0]
    want = [first[:, 0].sum(), first[:, 4].sum(), first[:, 1].sum(), first[:, 2].sum(), first[:, 3].sum(), first[:, 5].sum(),
            len(first), rows[:, :, 0].min(axis=1).sum(), 0] + [0] * 7
    assert (res.totals - start).tolist() == [int(x) for x in want]
    assert res.totals[edit.T_ORACLE] - start[edit.T_ORACLE] <= res.totals[edit.T_ERRORS] - start[edit.T_ERRORS]


def test_absent_and_invalid_rows():
    case = ec.random_rows(9, 29, B=4, K=3, max_hyp=20, max_ref=16, min_ref=4)
    n_hyps = np.array([3, 1, 0, 2], dtype=np.int32)
    case['hyp'][0, 0] = 29                                          # b 0, k 0: an id == C inside the length
    case['hyp_lens'][0] = max(case['hyp_lens'][0], 1)
    case['hyp_lens'][10] = 21                                       # b 3, k 1: a length outside the row
    full = _host(case, 'char')
    res = _host(case, 'char', n_hyps=n_hyps)
    ok = res.rows[:, 6].reshape(4, 3)
    assert ok.tolist() == [[0, 1, 1], [1, 2, 2], [2, 2, 2], [1, 0, 2]]
    assert not res.rows[res.rows[:, 6] != 1][:, :6].any()
    scored = res.rows[:, 6] == 1
    assert np.array_equal(res.rows[scored], full.rows[scored])
    t, e = res.totals, res.rows[:, 0].astype(np.int64)
    assert t[edit.T_ROWS] == 2 and t[edit.T_ERRORS] == e[3] + e[9] and t[edit.T_INVALID] == 2
    assert t[edit.T_ORACLE] == min(e[1], e[2]) + e[3] + e[9]
    # an invalid reference takes all of its rows; a negative length likewise
    case['ref'][1, 0] = -1
    case['ref_lens'][3] = -1
    res = _host(case, 'char')
    assert res.rows[:, 6].reshape(4, 3).tolist() == [[0, 1, 1], [0, 0, 0], [1, 1, 1], [0, 0, 0]]
    # ids behind the length are not looked at; without lengths the padded row is
    case = ec.from_lists([[1, 2]], [[1, 3]], 29, pad=77)
    case['hyp'] = np.array([[1, 2, 77]], dtype=np.int32)
    assert _host(case, 'char').rows[0, 6] == 1
    assert edit.edit_host(case['hyp'], None, case['ref'], None, 29).rows[0, 6] == 0
    assert edit.edit_host(case['hyp'][:, :2], None, case['ref'], None, 29).rows[0].tolist() == [1, 1, 0, 0, 2, 2, 1, 0]


def test_refusals_by_name():
    h, r = np.zeros((2, 4), dtype=np.int32), np.zeros((2, 4), dtype=np.int32)
    with pytest.raises(ValueError, match="mode must be 'char' or 'word'"):
        edit.edit_host(h, None, r, None, 5, mode='phone')
    with pytest.raises(ValueError, match='word mode needs is_space'):
        edit.edit_host(h, None, r, None, 5, mode='word')
    with pytest.raises(ValueError, match='one entry per class'):
        edit.edit_host(h, None, r, None, 5, mode='word', is_space=np.zeros(4, dtype=np.uint8))
    with pytest.raises(ValueError, match='rows per reference'):
        edit.edit_host(h, None, r, None, 5, rows_per_ref=3)
    with pytest.raises(ValueError, match='hyp_lens must have 2 entries'):
        edit.edit_host(h, np.zeros(3, dtype=np.int32), r, None, 5)
    with pytest.raises(ValueError, match=r'1 \.\. 1048576 ids'):
        edit.edit_host(np.zeros((2, 0), dtype=np.int32), None, r, None, 5)
    with pytest.raises(ValueError, match='n_classes'):
        edit.edit_host(h, None, r, None, 0)
    with pytest.raises(ValueError, match="single characters, entry 2 is 'th'"):
        edit.space_mask([' ', 'a', 'th'])
    with pytest.raises(ValueError, match='single characters'):
        W.WER(vocabulary=[' ', 'a', '##ing'], device=True)
    with pytest.raises(ValueError, match='same number of elements'):
        edit.error_counts(['a'], ['a', 'b'])


@pytest.mark.parametrize('use_cer', [False, True])
def test_wer_device_on_cpu_tensors_equals_the_default_metric(use_cer):
    torch = pytest.importorskip('torch')
    vocab = [' '] + list('abcdefghijklmnopqrstuvwxyz') + ["'"]
    blank = len(vocab)
    g = torch.Generator().manual_seed(4)
    plain, dev = W.WER(vocabulary=vocab, use_cer=use_cer), W.WER(vocabulary=vocab, use_cer=use_cer, device=True)
    for B, T, L in ((5, 40, 12), (3, 25, 9)):
        pred = torch.randint(0, blank + 1, (B, T), generator=g)
        pred[torch.rand(B, T, generator=g) < 0.3] = 0
        tg = torch.randint(0, blank, (B, L), generator=g)
        tg[torch.rand(B, L, generator=g) < 0.25] = 0
        tl = torch.randint(0, L + 1, (B,), generator=g)
        plain.update(pred, tg, tl)
        dev.update(pred, tg, tl)
    a, b = plain.compute(), dev.compute()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[2]) > 0
    c = dev.counts()
    assert (c.errors, c.ref_units) == (int(a[1]), int(a[2])) and c.substitutions + c.deletions + c.insertions == c.errors
    assert c.rate == float(a[1]) / float(a[2])
    dev.reset()
    assert dev.counts().errors == 0


def test_model_error_rate_on_the_host_modules_equals_word_error_rate_over_decodes_texts():
    torch = pytest.importorskip('torch')
    from nemo.collections.asr.models import EncDecCTCModel
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
    m.set_quant_mode('none')
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    vocab = list(m.decoder.vocabulary)
    g = np.random.default_rng(5)
    x = torch.from_numpy((0.1 * g.standard_normal((3, 16000))).astype(np.float32))
    io = dict(input_signal=x, input_signal_length=torch.tensor([16000, 9000, 12345]))
    tg = g.integers(0, len(vocab), (3, 30)).astype(np.int32)
    tg[g.random((3, 30)) < 0.25] = vocab.index(' ')
    tl = np.array([30, 11, 0], dtype=np.int32)
    refs = [''.join(vocab[c] for c in row[:n]) for row, n in zip(tg, tl)]
    texts = [h.text for h in m.decode(**io)]
    for use_cer in (False, True):
        rep = m.error_rate(**io, targets=torch.from_numpy(tg), target_lengths=torch.from_numpy(tl), use_cer=use_cer)
        assert rep.total.rate == W.word_error_rate(texts, refs, use_cer=use_cer) and rep.invalid == 0 and rep.total.errors > 0
        assert rep.oracle_errors == rep.total.errors == sum(c.errors for c in rep.per_utterance)
        assert m.error_rate(**io, texts=refs, use_cer=use_cer) == rep
    nbest = m.decode(**io, beam_width=6, n_best=3)
    rep = m.error_rate(**io, texts=refs, beam_width=6, n_best=3)
    assert rep.total.rate == W.word_error_rate([row[0].text for row in nbest], refs)
    assert rep.oracle_errors == sum(min(W._levenshtein(h.text.split(), r.split()) for h in row) for row, r in zip(nbest, refs))
    with pytest.raises(ValueError, match='targets .* or as texts'):
        m.error_rate(**io)
    with pytest.raises(ValueError, match='not in the vocabulary'):
        m.error_rate(**io, texts=['#', '', ''])
