"""qasr.edit's edit path on the host: the twin trace_host against edit_host (the rows, every byte), against a full-matrix
back-trace that shares no code with it, against the counts and a replay of the path; the rules around it - the sentinel behind
n_ops, absent and invalid rows, refusals, the workspace cap - and the helpers that turn a path into listings and confusions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edit_cases as ec  # noqa: E402
import edit_trace_cases as tc  # noqa: E402
from qasr import ctc, edit  # noqa: E402

CASES = ec.small_cases()
IDS = [n for n, _ in CASES]
SENTINEL = 0xEE


def _trace(case, mode, extra=3, **kw):
    md = edit.MODES[mode]
    units = edit.unit_bound(case['hyp'].shape[1], md) + edit.unit_bound(case['ref'].shape[1], md)
    ops = np.full((case['hyp'].shape[0], units + extra), SENTINEL, dtype=np.uint8)
    res = edit.trace_host(case['hyp'], case['hyp_lens'], case['ref'], case['ref_lens'], case['C'], mode=mode,
                          is_space=case['is_space'], rows_per_ref=case['K'], ops=ops, **kw)
    assert res.ops is ops and res.n_ops.dtype == np.int32 and res.n_ops.shape == (len(ops),)
    return res


def _units(case, p, mode):
    b = p // case['K']
    return (ec.units(case['hyp'][p], case['hyp_lens'][p], mode, case['is_space']),
            ec.units(case['ref'][b], case['ref_lens'][b], mode, case['is_space']))


@pytest.mark.parametrize('mode', ['char', 'word'])
@pytest.mark.parametrize('name,case', CASES, ids=IDS)
def test_path_equals_an_independent_backtrace_the_counts_and_a_replay(name, case, mode):
    res = _trace(case, mode)
    want = edit.edit_host(case['hyp'], case['hyp_lens'], case['ref'], case['ref_lens'], case['C'], mode=mode,
                          is_space=case['is_space'], rows_per_ref=case['K'])
    assert res.rows.dtype == want.rows.dtype and res.rows.tobytes() == want.rows.tobytes() and res.rows_per_ref == case['K']
    for p in range(len(case['hyp'])):
        h, r = _units(case, p, mode)
        e, S, D, I, nr, nh, ok, _ = (int(x) for x in res.rows[p])
        n = int(res.n_ops[p])
        ops = res.ops[p, :n].tolist()
        path, cost = tc.full_matrix_ops(h, r)
        assert ok == 1 and cost == e and ops == path, (name, p, ops, path)
        assert (ops.count(1), ops.count(2), ops.count(3), ops.count(0)) == (S, D, I, nr - S - D), (name, p)
        assert n == nr + I and n <= nh + nr
        rebuilt, used = tc.apply(ops, h, tc.ref_fill(ops, r))
        assert rebuilt == r and used == nh, (name, p)
        assert (res.ops[p, n:] == SENTINEL).all()                   # bytes at and behind n_ops are left as they are


def test_ties_heavy_binary_alphabet_has_every_op_and_many_ties():
    """the C = 2 batch: among its cells many have predecessors of equal cost, and the paths use all four codes"""
    case = dict(CASES)['binary_ties']
    res = _trace(case, 'char')
    seen = set()
    for p in range(len(case['hyp'])):
        seen |= set(res.ops[p, :res.n_ops[p]].tolist())
    assert seen == {0, 1, 2, 3}


def test_structured_rows_by_hand():
    c = dict(CASES)
    ops = lambda name, mode, p=0: (lambda r: r.ops[p, :r.n_ops[p]].tolist())(_trace(c[name], mode))
    assert ops('swap', 'word') == [1, 1]                            # "a b" against "b a": two substitutions, the diagonal first
    assert ops('swap', 'char') == [1, 0, 1]
    assert ops('repeated', 'word') == [3, 3, 0]                     # "a a a" against "a": the diagonal is taken at the last cell
    assert ops('one_of_repeated', 'word') == [2, 2, 0]
    assert [ops('empty_rows', 'word', p) for p in range(3)] == [[2], [3, 3], []]
    assert [ops('empty_rows', 'char', p) for p in range(3)] == [[2, 2], [3, 3, 3], []]
    assert [ops('only_space', 'word', p) for p in range(2)] == [[2], [3]]
    assert ops('edges_of_space', 'word') == [0, 0]
    assert ops('last_id_differs', 'word') == [1, 0]


@pytest.mark.parametrize('mode', ['char', 'word'])
def test_absent_and_invalid_rows_have_no_ops(mode):
    case = ec.random_rows(77, 29, B=6, K=3, max_hyp=30, max_ref=24, min_ref=8)
    n_hyps = np.array([3, 1, 0, 3, 2, 3], dtype=np.int32)
    case['hyp'][4, 2] = 29                                          # b 1, k 1: absent, its bad id is not looked at
    case['hyp'][10, 0] = -1                                         # b 3, k 1: invalid between valid rows
    case['hyp_lens'][10] = max(case['hyp_lens'][10], 1)
    case['hyp_lens'][12] = 31                                       # b 4, k 0: a length outside the row
    case['ref'][5, 1] = 29                                          # b 5: an invalid reference takes its three rows
    res = _trace(case, mode, n_hyps=n_hyps)
    want = edit.edit_host(case['hyp'], case['hyp_lens'], case['ref'], case['ref_lens'], 29, mode=mode, is_space=case['is_space'],
                          rows_per_ref=3, n_hyps=n_hyps)
    assert res.rows.tobytes() == want.rows.tobytes()
    assert res.rows[:, 6].reshape(6, 3).tolist() == [[1, 1, 1], [1, 2, 2], [2, 2, 2], [1, 0, 1], [0, 1, 2], [0, 0, 0]]
    for p in range(18):
        if res.rows[p, 6] != 1:
            assert res.n_ops[p] == 0 and (res.ops[p] == SENTINEL).all()
        else:
            assert res.n_ops[p] == res.rows[p, 4] + res.rows[p, 3]


def test_default_ops_have_the_least_pitch_and_missing_lengths_mean_the_padded_rows():
    case = ec.from_lists([[1, 0, 2, 0], [3, 3, 0, 0]], [[1, 0, 2], [0, 0, 0]], 29, pad=0)
    res = edit.trace_host(case['hyp'], None, case['ref'], None, 29, mode='word', is_space=case['is_space'])
    assert res.ops.shape == (2, 2 + 2) and res.ops.dtype == np.uint8
    assert res.n_ops.tolist() == [2, 1] and res.ops[0, :2].tolist() == [0, 0] and res.ops[1, :1].tolist() == [3]
    res = edit.trace_host(case['hyp'], None, case['ref'], None, 29, mode='char')
    assert res.ops.shape == (2, 4 + 3) and res.n_ops.tolist() == [4, 4]


# ---------------------------------------------------------------------------------------------- listings and confusions
def _alignment(ops, ref, hyp):
    ri, hi, i, j = [], [], 0, 0
    for c in ops:
        ri.append(None if c == 'I' else j), hi.append(None if c == 'D' else i)
        i, j = i + (c != 'D'), j + (c != 'I')
    e = sum(c != 'C' for c in ops)
    return ctc.Alignment(ops, ref, hyp, ri, hi, ctc.ErrorCounts(e, ops.count('S'), ops.count('D'), ops.count('I'), len(ref), len(hyp),
                                                              e / len(ref) if ref else float('inf')))


def test_listing_against_literal_text():
    a = _alignment('CCSCDC', 'the cat sat on the mat'.split(), 'the cat sit on mat'.split())
    assert edit.listing(a) == ('REF: the cat SAT on THE mat\n'
                               'HYP: the cat SIT on *** mat')
    a = _alignment('SICI', 'hello world'.split(), 'help big world again'.split())
    assert edit.listing(a) == ('REF: HELLO *** world *****\n'
                               'HYP: HELP  BIG world AGAIN')
    a = _alignment('CDCSI', list('a bc'), list('abxy'))             # characters: a whitespace unit shows as _
    assert edit.listing(a) == ('REF: a _ b C *\n'
                               'HYP: a * b X Y')
    assert edit.listing(_alignment('', [], [])) == 'REF:\nHYP:'


def test_align_texts_by_hand_and_its_counts_equal_error_counts():
    hyps = ['the cat sit on mat', 'help big world again', '', 'ab', 'same  words here']
    refs = ['the cat sat on the mat', 'hello world', 'two words', 'a bc', 'same words\there']
    al = edit.align_texts(hyps, refs)
    assert [a.ops for a in al] == ['CCSCDC', 'ISCI', 'DD', 'DS', 'CCC']
    assert edit.listing(al[0]) == 'REF: the cat SAT on THE mat\nHYP: the cat SIT on *** mat'
    assert al[0].ref_index == [0, 1, 2, 3, 4, 5] and al[0].hyp_index == [0, 1, 2, 3, None, 4]
    assert al[1].ref_index == [None, 0, 1, None] and al[1].hyp_index == [0, 1, 2, 3]
    assert al[1].ref_units == ['hello', 'world'] and al[1].hyp_units == ['help', 'big', 'world', 'again']
    for use_cer in (False, True):
        al = edit.align_texts(hyps, refs, use_cer=use_cer)
        total = edit.error_counts(hyps, refs, use_cer=use_cer)
        for f in ('errors', 'substitutions', 'deletions', 'insertions', 'ref_units', 'hyp_units'):
            assert sum(getattr(a.counts, f) for a in al) == getattr(total, f), (use_cer, f)
        for a, h, r in zip(al, hyps, refs):
            assert a.counts == edit.error_counts([h], [r], use_cer=use_cer)
            assert a.ref_units == (list(r) if use_cer else r.split()) and a.hyp_units == (list(h) if use_cer else h.split())
            assert (a.ops.count('S'), a.ops.count('D'), a.ops.count('I')) == (a.counts.substitutions, a.counts.deletions, a.counts.insertions)
    assert edit.align_texts([], []) == []


def test_confusions_against_a_brute_force_count():
    g = np.random.default_rng(3)
    words = ['a', 'b', 'cc', 'dd', 'e']
    refs = [' '.join(g.choice(words, int(g.integers(0, 9)))) for _ in range(40)]
    hyps = [' '.join(g.choice(words, int(g.integers(0, 9)))) for _ in range(40)]
    al = edit.align_texts(hyps, refs) + [None]
    sub, dele, ins = {}, {}, {}
    for a in al[:-1]:
        i = j = 0
        for c in a.ops:
            if c == 'S':
                sub[(a.ref_units[j], a.hyp_units[i])] = sub.get((a.ref_units[j], a.hyp_units[i]), 0) + 1
            if c == 'D':
                dele[a.ref_units[j]] = dele.get(a.ref_units[j], 0) + 1
            if c == 'I':
                ins[a.hyp_units[i]] = ins.get(a.hyp_units[i], 0) + 1
            i, j = i + (c != 'D'), j + (c != 'I')
    got = edit.confusions(al)
    for have, want in zip(got, (sub, dele, ins)):
        assert dict(have) == want and len(have) == len(want) > 2
        assert [n for _, n in have] == sorted((n for _, n in have), reverse=True)
        assert all(a[0] < b[0] for a, b in zip(have, have[1:]) if a[1] == b[1])     # equal counts: in the order of the units
    top = edit.confusions(al, top=2)
    assert [x[:2] for x in got] == [list(x) for x in top]


# ------------------------------------------------------------------------------------------------------------- façade
def test_model_error_rate_alignments_on_the_host_modules_equal_align_texts_over_decodes_texts():
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
        plain = m.error_rate(**io, texts=refs, use_cer=use_cer)
        assert plain.alignments is None
        rep = m.error_rate(**io, targets=torch.from_numpy(tg), target_lengths=torch.from_numpy(tl), use_cer=use_cer, alignments=True)
        assert rep.alignments == edit.align_texts(texts, refs, use_cer=use_cer)
        assert [a.counts for a in rep.alignments] == rep.per_utterance
        rep.alignments = None
        assert rep == plain                                         # the totals and the oracle are those without alignments
    nbest = m.decode(**io, beam_width=6, n_best=3)
    plain = m.error_rate(**io, texts=refs, beam_width=6, n_best=3)
    rep = m.error_rate(**io, texts=refs, beam_width=6, n_best=3, alignments=True)
    assert rep.alignments == edit.align_texts([row[0].text for row in nbest], refs)
    assert (rep.total, rep.oracle_errors, rep.per_utterance, rep.invalid) == (plain.total, plain.oracle_errors, plain.per_utterance, plain.invalid)
    with pytest.raises(ValueError, match=r'trace_host: .* needs a workspace of \d+ bytes, above max_workspace_bytes = 64'):
        m.error_rate(**io, texts=refs, alignments=True, max_workspace_bytes=64)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name():
    case = ec.random_rows(1, 29, B=2, K=2, max_hyp=9, max_ref=8)
    a = (case['hyp'], case['hyp_lens'], case['ref'], case['ref_lens'], 29)
    with pytest.raises(ValueError, match="mode must be 'char' or 'word'"):
        edit.trace_host(*a, mode='phone', rows_per_ref=2)
    with pytest.raises(ValueError, match='word mode needs is_space'):
        edit.trace_host(*a, mode='word', rows_per_ref=2)
    with pytest.raises(ValueError, match='rows per reference'):
        edit.trace_host(*a, rows_per_ref=3)
    with pytest.raises(ValueError, match='n_hyps must have 2 entries'):
        edit.trace_host(*a, rows_per_ref=2, n_hyps=np.zeros(3, dtype=np.int32))
    for bad in (np.zeros((4, 16), dtype=np.uint8), np.zeros((3, 17), dtype=np.uint8), np.zeros((4, 17), dtype=np.int8), np.zeros(68, dtype=np.uint8)):
        with pytest.raises(ValueError, match=r'trace_host: ops must be a uint8 array \[4, >= 17\]'):
            edit.trace_host(*a, rows_per_ref=2, ops=bad)
    edit.trace_host(*a, rows_per_ref=2, ops=np.zeros((4, 17), dtype=np.uint8))
    need = edit.trace_workspace_bytes(4, 9, 8, 'char')
    assert need == 64 + 4 * 72 * 64                                 # the info block, then 4 planes of 9 + 63 steps of 64 bytes
    with pytest.raises(ValueError, match=f'trace_host: .* needs a workspace of {need} bytes, above max_workspace_bytes = {need - 1}'):
        edit.trace_host(*a, rows_per_ref=2, max_workspace_bytes=need - 1)
    edit.trace_host(*a, rows_per_ref=2, max_workspace_bytes=need)
    # the sizes the rules quote: 32 x 250 characters, an hour in words, an hour in characters (two of them: above the default cap)
    assert edit.trace_workspace_bytes(32, 250, 250, 'char') == 512 + 32 * 313 * 64
    assert 20e6 < edit.trace_workspace_bytes(1, 18000, 18000, 'word') < 22e6
    assert 0.7e9 < edit.trace_workspace_bytes(1, 54000, 54000, 'char') < 0.75e9 < edit.MAX_WORKSPACE == 1 << 30
    assert edit.trace_workspace_bytes(2, 54000, 54000, 'char') > edit.MAX_WORKSPACE
    with pytest.raises(ValueError, match='needs a workspace of'):
        edit.align_texts(['a' * 54000] * 2, ['b' * 54000] * 2, use_cer=True)
    with pytest.raises(ValueError, match='must have the same number of elements'):
        edit.align_texts(['a'], [])
    assert 'diagonal first' in edit.TRACE_RULES and 'FORWARD' in edit.TRACE_RULES
