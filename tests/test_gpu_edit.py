"""Edit distance on an MI355X: k_edit_cut / k_edit / k_edit_totals (csrc/qasr_edit.hip) against qasr.edit.edit_host - every byte of
the per-problem rows and of the totals block, outputs pre-filled with 0x5a, no tolerance; refused arguments launch nothing; the
chain k_ctc -> k_edit replays from a graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edit_cases as ec  # noqa: E402
from qasr import ctc, edit  # noqa: E402

FILL32, FILL64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
START = np.arange(1000, 1016, dtype=np.int64) * 3                  # a totals block that starts non-zero


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide(a, extra, fill):
    """the matrix inside rows of a larger pitch, the pad filled with ids that would be refused"""
    big = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.int32, device='cuda')
    big[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return big[:, :a.shape[1]]


def _run(eng, case, mode, lens=True, n_hyps=None, wide=False, what=''):
    """one call against the twin on every byte of rows and totals"""
    hl, rl = (case['hyp_lens'], case['ref_lens']) if lens else (None, None)
    want = edit.edit_host(case['hyp'], hl, case['ref'], rl, case['C'], mode=mode, is_space=case['is_space'], rows_per_ref=case['K'],
                          n_hyps=n_hyps, totals=START)
    P = case['hyp'].shape[0]
    out = torch.full((P, 8), FILL32, dtype=torch.int32, device='cuda')
    totals = _cuda(START.copy())
    hyp = _wide(case['hyp'], 5, case['C'] + 9) if wide else _cuda(case['hyp'])
    ref = _wide(case['ref'], 3, -7) if wide else _cuda(case['ref'])
    got = eng.edit_distance(hyp, _cuda(hl), ref, _cuda(rl), case['C'], mode=mode, is_space=_cuda(case['is_space']),
                            rows_per_ref=case['K'], n_hyps=_cuda(n_hyps), totals=totals, out=out)
    torch.cuda.synchronize()
    rows, tot = got.rows.cpu().numpy(), got.totals.cpu().numpy()
    assert rows.dtype == want.rows.dtype and tot.dtype == want.totals.dtype
    bad = np.flatnonzero((rows != want.rows).any(axis=1))
    assert len(bad) == 0, f'{what} {mode}: rows {bad[:8].tolist()} differ: got {rows[bad[:4]].tolist()} want {want.rows[bad[:4]].tolist()}'
    assert rows.tobytes() == want.rows.tobytes() and tot.tobytes() == want.totals.tobytes(), (what, mode, tot.tolist(), want.totals.tolist())
    return want


def _char_batch(seed, m, C_=29, rows=5):
    """references of m ids (the last one 3 shorter) against hypotheses of 0, 1, fewer, more and as many units, made from them
    by random edits: four different lengths share a work-group"""
    g = np.random.default_rng(seed)
    base = ec.random_rows(seed, C_, B=rows, K=1, max_hyp=m + 7, max_ref=max(m, 1), min_ref=max(m, 1))
    base['ref_lens'][:] = m
    if m >= 3:
        base['ref_lens'][-1] = m - 3
    hl = base['hyp_lens']
    for p, n in enumerate([0, 1, max(m - 5, 0), m + 7, m][:rows]):
        have = int(hl[p])
        if n > have:
            base['hyp'][p, have:n] = g.integers(0, C_, n - have)
        hl[p] = n
    return base


# reference units at which k_edit<NC> changes: 64 NC - 1, 64 NC, 64 NC + 1 for NC = 1, 4, 16 (the width picks NC), then two and three strips
@pytest.mark.parametrize('m', [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_k_edit_equals_edit_host_every_byte_char(eng, m):
    want = _run(eng, _char_batch(100 + m, m), 'char', what=f'm={m}')
    assert (want.rows[:, 6] == 1).all() and want.rows[:, 4].tolist()[:4] == [m] * 4


def test_three_strips(eng):
    case = _char_batch(7, 2049, rows=3)
    case['hyp_lens'][:] = [2056, 1500, 2049]
    case['hyp'] = np.where(case['hyp'] >= 29, 3, case['hyp']).astype(np.int32)
    want = _run(eng, case, 'char', what='three strips')
    assert (want.rows[:, 6] == 1).all() and want.rows[0, 0] > 0


def _word_batch(seed, n_words, max_len, C_=29, rows=4):
    """references of n_words words of 1 .. max_len ids against edited hypotheses of no word, one word, fewer and more words.
    max_len 1: one whitespace id between the words, so that the reference width 2 n_words (- 1) makes n_words the largest unit
    count the launch can see, which picks NC; otherwise one or two whitespace ids"""
    g = np.random.default_rng(seed)
    sp = np.flatnonzero(ec.space_mask(C_))
    letters = np.setdiff1d(np.arange(C_), sp)
    hyps, refs = [], []
    for b in range(rows):
        words = [list(g.choice(letters[:6], int(g.integers(1, max_len + 1)))) for _ in range(n_words - (3 if b == rows - 1 and n_words >= 3 else 0))]
        hw = []
        for w in words:
            u = g.random()
            if u < 0.05:
                continue
            hw.append(list(g.choice(letters[:6], len(w))) if u < 0.1 else (w[:-1] + [int(letters[7])] if u < 0.15 else w))
            if u > 0.95:
                hw.append([int(letters[8])])
        hw = [[], hw[:1], hw[:max(len(hw) - 5, 0)], hw + [[int(letters[9])]] * 4][b % 4] if b < 4 else hw
        join = lambda ws: [int(c) for i, w in enumerate(ws)
                           for c in ([int(sp[0])] * int(i > 0) * (1 + (max_len > 1 and i % 7 == 3)) + [int(x) for x in w])]
        hyps.append(join(hw) + [int(sp[-1])] * (b % 2))
        refs.append([int(sp[0])] * (b % 2) + join(words))
    return ec.from_lists(hyps, refs, C_)


@pytest.mark.parametrize('n_words,max_len', [(n, 1) for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)] +
                         [(65, 3), (700, 3), (1025, 3)])
def test_k_edit_equals_edit_host_every_byte_word(eng, n_words, max_len):
    case = _word_batch(200 + n_words, n_words, max_len)
    if max_len == 1:
        assert (case['ref'].shape[1] + 1) // 2 == max(n_words, 1)
    want = _run(eng, case, 'word', what=f'words={n_words}')
    assert (want.rows[:, 6] == 1).all() and want.rows[0, 4] == n_words and want.rows[0, 5] == 0


def test_words_and_chunk_boundaries(eng):
    """a word across the 64-id chunk boundary, a word of more than 64 ids, whitespace at ids 63 and 64, two words of equal length
    with a common prefix that differ in the last id"""
    sp, a, b, c = 0, 1, 2, 3
    long_word = [a, b] * 50
    refs = [[a] * 3 + [sp] + [b] * 58 + [sp] + [c] * 10 + [sp, a],                # ids 61 .. 71 are one word
            long_word + [sp] + long_word[:-1] + [c] + [sp, b],                   # two 100-id words that differ in the last id
            [a] * 63 + [sp, sp] + [b] * 5 + [sp],                                # whitespace at ids 63 and 64
            [a] * 62 + [sp] + [b] + [c] * 3 + [sp, a, b, c, a, sp, a, b, c, b],  # a word that starts at id 63; equal prefixes
            [sp] * 64 + [a] + [sp] * 63 + [b],                                   # words that start at ids 64 and 128
            [a] * 64,                                                            # one word that ends with the chunk
            [a] * 128 + [sp] + [b]]
    hyps = [[a] * 3 + [sp] + [b] * 58 + [sp] + [c] * 9 + [b, sp, a],
            long_word[:-1] + [c] + [sp] + long_word[:-1] + [c] + [sp, sp, b],
            [a] * 63 + [sp] + [a] + [b] * 5,
            [a] * 62 + [sp, sp] + [b] + [c] * 3 + [sp, a, b, c, b, sp, a, b, c, a],
            [a, sp, b],
            [a] * 63,
            [a] * 128 + [b]]
    case = ec.from_lists(hyps, refs, 29)
    want = _run(eng, case, 'word', what='boundaries')
    assert want.rows[:, 0].tolist() == [1, 1, 1, 2, 0, 1, 2] and want.rows[:, 4].tolist() == [4, 3, 2, 4, 2, 1, 2]
    _run(eng, case, 'char', what='boundaries')
    _run(eng, case, 'word', wide=True, what='boundaries, wide rows')


@pytest.mark.parametrize('C_', ec.CLASSES)
@pytest.mark.parametrize('mode', ['char', 'word'])
def test_classes_pitches_and_missing_lengths(eng, C_, mode):
    case = ec.random_rows(40 + C_, C_, B=9, K=1, max_hyp=150, max_ref=130, min_ref=20)
    _run(eng, case, mode, wide=True, what=f'C={C_} wide')
    # without length vectors the padded row is walked: pads that are valid ids count, here the whitespace id 0
    for k in ('hyp', 'ref'):
        case[k] = np.where(case[k] >= C_, 0, case[k]).astype(np.int32)
    want = _run(eng, case, mode, lens=False, wide=True, what=f'C={C_} no lengths')
    assert (want.rows[:, 6] == 1).all()
    if mode == 'char':
        assert (want.rows[:, 4] == 130).all() and (want.rows[:, 5] == 150).all()


@pytest.mark.parametrize('mode', ['char', 'word'])
def test_nbest_rows_absent_and_invalid_rows_between_valid_ones(eng, mode):
    case = ec.random_rows(77, 29, B=6, K=3, max_hyp=90, max_ref=80, min_ref=30)
    n_hyps = np.array([3, 1, 0, 3, 2, 3], dtype=np.int32)
    case['hyp'][4, 2] = 29                                          # b 1, k 1: absent, its bad id is not looked at
    case['hyp'][10, 0] = -1                                         # b 3, k 1: invalid between valid rows
    case['hyp_lens'][10] = max(case['hyp_lens'][10], 1)
    case['hyp_lens'][12] = 91                                       # b 4, k 0: a length outside the row
    case['ref'][5, 1] = 29                                          # b 5: an invalid reference takes its three rows
    want = _run(eng, case, mode, n_hyps=n_hyps, what='n-best')
    assert want.rows[:, 6].reshape(6, 3).tolist() == [[1, 1, 1], [1, 2, 2], [2, 2, 2], [1, 0, 1], [0, 1, 2], [0, 0, 0]]
    assert want.totals[edit.T_INVALID] - START[edit.T_INVALID] == 5 and want.totals[edit.T_ROWS] - START[edit.T_ROWS] == 3
    _run(eng, case, mode, what='n-best, all present')


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_launch_nothing(eng):
    lib = eng.load_library()
    B, K, C_, MH, MR = 2, 3, 29, 12, 10
    hyp = torch.ones(B * K, MH, dtype=torch.int32, device='cuda')
    ref = torch.ones(B, MR, dtype=torch.int32, device='cuda')
    sp = torch.zeros(C_, dtype=torch.uint8, device='cuda')
    rows = torch.full((B * K, 8), FILL32, dtype=torch.int32, device='cuda')
    totals = torch.full((16,), FILL64, dtype=torch.int64, device='cuda')
    need = eng.edit_workspace_bytes(B * K, MH, MR, 'word')
    assert need > 0 and eng.edit_workspace_bytes(B * K, MH, MR, 'char') > 0
    ws = torch.full((need + 16,), 0x5a, dtype=torch.uint8, device='cuda')
    size = C.sizeof(eng.EditArgs)

    def args(**kw):
        a = eng.EditArgs()
        a.struct_size, a.mode, a.B, a.K, a.C, a.max_hyp, a.max_ref, a.hyp_pitch, a.ref_pitch = size, 1, B, K, C_, MH, MR, MH, MR
        a.hyp, a.ref, a.is_space, a.rows, a.totals = hyp.data_ptr(), ref.data_ptr(), sp.data_ptr(), rows.data_ptr(), totals.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    # the struct in another size is refused, an older (shorter) one included, as every entry point with one struct size does
    bad = [dict(struct_size=8), dict(struct_size=size + 8), dict(struct_size=size - 8)]
    bad += [{f: None} for f in ('hyp', 'ref', 'rows', 'totals', 'workspace', 'is_space')]
    bad += [dict(mode=2), dict(mode=-1), dict(B=0), dict(K=0), dict(C=0), dict(B=1 << 13, K=(1 << 11) + 1), dict(max_hyp=0), dict(max_ref=0),
            dict(max_hyp=(1 << 20) + 1, hyp_pitch=1 << 21), dict(max_ref=(1 << 20) + 1, ref_pitch=1 << 21), dict(hyp_pitch=MH - 1),
            dict(ref_pitch=MR - 1), dict(workspace_bytes=need - 1), dict(workspace=ws.data_ptr() + 8), dict(rows=rows.data_ptr() + 4),
            dict(totals=totals.data_ptr() + 4)]
    for kw in bad:
        assert lib.qasr_edit_distance(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_edit_distance(s, None) == 1
    for shape in ((0, MH, MR, 1), (4, 0, MR, 0), (4, MH, (1 << 20) + 1, 0), (4, MH, MR, 2), ((1 << 24) + 1, MH, MR, 0)):
        assert lib.qasr_edit_workspace_bytes(*shape) == 0, shape
    with pytest.raises(ValueError, match='mode'):
        eng.edit_distance(hyp, None, ref, None, C_, mode='phone', rows_per_ref=K)
    with pytest.raises(ValueError, match='word mode needs is_space'):
        eng.edit_distance(hyp, None, ref, None, C_, mode='word', rows_per_ref=K)
    with pytest.raises(ValueError, match='rows per reference'):
        eng.edit_distance(hyp, None, ref, None, C_, rows_per_ref=2)
    with pytest.raises(ValueError, match='ref_lens must have 2 entries'):
        eng.edit_distance(hyp, None, ref, torch.zeros(3, dtype=torch.int32, device='cuda'), C_, rows_per_ref=3)
    torch.cuda.synchronize()
    assert (rows == FILL32).all() and (totals == FILL64).all() and (ws == 0x5a).all()
    # the same arguments, unbroken, are taken; char mode needs no mask
    for kw in (dict(), dict(mode=0, is_space=None)):
        totals.zero_()
        assert lib.qasr_edit_distance(s, C.byref(args(**kw))) == 0, kw
        torch.cuda.synchronize()
        want = edit.edit_host(hyp.cpu().numpy(), None, ref.cpu().numpy(), None, C_, mode='char' if kw else 'word',
                              is_space=np.zeros(C_, dtype=np.uint8), rows_per_ref=K)
        assert rows.cpu().numpy().tobytes() == want.rows.tobytes() and totals.cpu().numpy().tobytes() == want.totals.tobytes()


# ---------------------------------------------------------------------------------------------------------------- graph
def test_k_ctc_then_k_edit_is_capturable(eng):
    """nothing is allocated and nothing is read on the host: qasr_ctc_collapse -> qasr_edit_distance replays from a graph on new
    tokens and references in the same buffers, and equals the twins on every byte"""
    B, T, L, C_ = 6, 180, 70, 29
    blank = C_
    g = np.random.default_rng(21)
    mask = ec.space_mask(C_)

    def batch():
        tok = g.integers(0, C_ + 1, (B, T)).astype(np.int32)
        tok[g.random((B, T)) < 0.4] = blank
        tok[g.random((B, T)) < 0.15] = 0
        ref = g.integers(0, C_, (B, L)).astype(np.int32)
        ref[g.random((B, L)) < 0.2] = 0
        return tok, ref, g.integers(0, L + 1, B).astype(np.int32)
    first = batch()
    tok_d, ref_d, rl_d = (_cuda(x) for x in first)
    res = eng.ctc_buffers(B, T, 'cuda', scores=False, blank=blank)
    rows = torch.full((B, 8), FILL32, dtype=torch.int32, device='cuda')
    totals = torch.zeros(16, dtype=torch.int64, device='cuda')
    ws = torch.empty(eng.edit_workspace_bytes(B, T, L, 'word'), dtype=torch.uint8, device='cuda')
    sp_d = _cuda(mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.ctc_collapse(tok_d, lens=None, blank=blank, out=res)
            eng.edit_distance(res.labels, res.n_labels, ref_d, rl_d, C_, mode='word', is_space=sp_d, totals=totals, workspace=ws, out=rows)
    want_totals = np.zeros(16, dtype=np.int64)
    for tok, ref, rl in (batch(), first, batch()):
        tok_d.copy_(torch.from_numpy(tok)), ref_d.copy_(torch.from_numpy(ref)), rl_d.copy_(torch.from_numpy(rl))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        host = ctc.collapse_host(tok, lens=None, blank=blank)
        want = edit.edit_host(host.labels, host.n_labels, ref, rl, C_, mode='word', is_space=mask, totals=want_totals)
        want_totals = want.totals
        assert want.rows[:, 0].sum() > 0 and (want.rows[:, 6] == 1).all()
        assert rows.cpu().numpy().tobytes() == want.rows.tobytes()
        assert totals.cpu().numpy().tobytes() == want_totals.tobytes()           # the block keeps adding across replays
