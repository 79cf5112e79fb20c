"""The edit path on an MI355X: k_edit_cut / k_edit_trace (csrc/qasr_edit.hip) against qasr.edit.trace_host - every byte of the
per-problem rows, of n_ops and of the sentinel-filled ops, no tolerance; refused arguments launch nothing; the chain
k_ctc -> k_edit_trace replays from a graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edit_cases as ec  # noqa: E402
import test_gpu_edit as te  # noqa: E402  (its batch builders: the shapes at which k_edit, and so k_edit_trace, changes path)
from qasr import ctc, edit  # noqa: E402

FILL32, SENTINEL = 0x5a5a5a5a, 0xEE
_cuda = te._cuda


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _units(case, mode):
    md = edit.MODES[mode]
    return edit.unit_bound(case['hyp'].shape[1], md) + edit.unit_bound(case['ref'].shape[1], md)


def _run(eng, case, mode, lens=True, n_hyps=None, wide=False, extra=5, what=''):
    """one call against the twin on every byte of rows, n_ops and ops (pre-filled with a sentinel, `extra` bytes of pitch above
    the least)"""
    hl, rl = (case['hyp_lens'], case['ref_lens']) if lens else (None, None)
    P, pitch = case['hyp'].shape[0], _units(case, mode) + extra
    want = edit.trace_host(case['hyp'], hl, case['ref'], rl, case['C'], mode=mode, is_space=case['is_space'], rows_per_ref=case['K'],
                           n_hyps=n_hyps, ops=np.full((P, pitch), SENTINEL, dtype=np.uint8))
    assert eng.edit_trace_workspace_bytes(P, case['hyp'].shape[1], case['ref'].shape[1], mode) == \
        edit.trace_workspace_bytes(P, case['hyp'].shape[1], case['ref'].shape[1], mode)
    out = torch.full((P, 8), FILL32, dtype=torch.int32, device='cuda')
    n_ops = torch.full((P,), FILL32, dtype=torch.int32, device='cuda')
    big = torch.full((P, pitch + (7 if wide else 0)), SENTINEL, dtype=torch.uint8, device='cuda')
    ops = big[:, :pitch]
    hyp = te._wide(case['hyp'], 5, case['C'] + 9) if wide else _cuda(case['hyp'])
    ref = te._wide(case['ref'], 3, -7) if wide else _cuda(case['ref'])
    got = eng.edit_trace(hyp, _cuda(hl), ref, _cuda(rl), case['C'], mode=mode, is_space=_cuda(case['is_space']),
                         rows_per_ref=case['K'], n_hyps=_cuda(n_hyps), ops=ops, n_ops=n_ops, out=out)
    torch.cuda.synchronize()
    assert got.ops is ops and got.rows_per_ref == case['K']
    rows, cnt, path = got.rows.cpu().numpy(), got.n_ops.cpu().numpy(), big.cpu().numpy()
    assert rows.dtype == want.rows.dtype and cnt.dtype == want.n_ops.dtype
    bad = np.flatnonzero((rows != want.rows).any(axis=1))
    assert len(bad) == 0, f'{what} {mode}: rows {bad[:8].tolist()} differ: got {rows[bad[:4]].tolist()} want {want.rows[bad[:4]].tolist()}'
    assert cnt.tolist() == want.n_ops.tolist(), (what, mode)
    bad = np.flatnonzero((path[:, :pitch] != want.ops).any(axis=1))
    assert len(bad) == 0, f'{what} {mode}: ops of problems {bad[:8].tolist()} differ, first at {np.flatnonzero(path[bad[0], :pitch] != want.ops[bad[0]])[:4].tolist()}'
    assert rows.tobytes() == want.rows.tobytes() and cnt.tobytes() == want.n_ops.tobytes() and path[:, :pitch].tobytes() == want.ops.tobytes()
    assert (path[:, pitch:] == SENTINEL).all()                      # the bytes of the pitch behind the row
    return want


# reference units at which k_edit_trace<NC> changes: 64 NC - 1, 64 NC, 64 NC + 1 for NC = 1, 4, 16 (the width picks NC); 1025: two strips
@pytest.mark.parametrize('m', [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_k_edit_trace_equals_trace_host_every_byte_char(eng, m):
    """hypotheses of 0, 1, fewer, more and as many units inside one work-group"""
    want = _run(eng, te._char_batch(100 + m, m), 'char', what=f'm={m}')
    assert (want.rows[:, 6] == 1).all() and want.rows[:, 4].tolist()[:4] == [m] * 4
    assert want.n_ops[0] == m and want.n_ops[3] >= m + 7


def test_three_strips(eng):
    case = te._char_batch(7, 2049, rows=3)
    case['hyp_lens'][:] = [2056, 1500, 2049]
    case['hyp'] = np.where(case['hyp'] >= 29, 3, case['hyp']).astype(np.int32)
    want = _run(eng, case, 'char', what='three strips')
    assert (want.rows[:, 6] == 1).all() and want.rows[0, 0] > 0 and {0, 1, 2, 3} <= set(want.ops[1, :want.n_ops[1]].tolist())


@pytest.mark.parametrize('n_words,max_len', [(n, 1) for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)] +
                         [(65, 3), (700, 9), (1025, 5)])
def test_k_edit_trace_equals_trace_host_every_byte_word(eng, n_words, max_len):
    case = te._word_batch(200 + n_words, n_words, max_len)
    if max_len == 1:
        assert (case['ref'].shape[1] + 1) // 2 == max(n_words, 1)
    want = _run(eng, case, 'word', what=f'words={n_words}')
    assert (want.rows[:, 6] == 1).all() and want.rows[0, 4] == n_words and want.rows[0, 5] == 0 and want.n_ops[0] == n_words


@pytest.mark.parametrize('C_', ec.CLASSES)
@pytest.mark.parametrize('mode', ['char', 'word'])
def test_classes_pitches_and_missing_lengths(eng, C_, mode):
    case = ec.random_rows(40 + C_, C_, B=9, K=1, max_hyp=150, max_ref=130, min_ref=20)
    _run(eng, case, mode, wide=True, what=f'C={C_} wide')
    _run(eng, case, mode, extra=0, what=f'C={C_} least ops pitch')
    for k in ('hyp', 'ref'):                                        # without length vectors the padded row is walked
        case[k] = np.where(case[k] >= C_, 0, case[k]).astype(np.int32)
    want = _run(eng, case, mode, lens=False, wide=True, what=f'C={C_} no lengths')
    assert (want.rows[:, 6] == 1).all()


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
    assert ((want.n_ops == 0) == (want.rows[:, 6] != 1)).all()      # such rows: nothing written, the sentinel stays
    _run(eng, case, mode, what='n-best, all present')


@pytest.mark.parametrize('mode', ['char', 'word'])
def test_binary_alphabet_ties(eng, mode):
    """C = 2, half of the ids edited: most cells have predecessors of equal cost, so the tie order decides the path"""
    case = ec.random_rows(5, 2, B=8, K=2, max_hyp=330, max_ref=300, space_p=0.3, edit_p=0.5, min_ref=200)
    want = _run(eng, case, mode, what='binary')
    assert {0, 1, 2, 3} <= set(want.ops[0, :want.n_ops[0]].tolist())


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_launch_nothing(eng):
    lib = eng.load_library()
    B, K, C_, MH, MR = 2, 3, 29, 12, 10
    hyp = torch.ones(B * K, MH, dtype=torch.int32, device='cuda')
    ref = torch.ones(B, MR, dtype=torch.int32, device='cuda')
    sp = torch.zeros(C_, dtype=torch.uint8, device='cuda')
    rows = torch.full((B * K, 8), FILL32, dtype=torch.int32, device='cuda')
    n_ops = torch.full((B * K,), FILL32, dtype=torch.int32, device='cuda')
    units = (MH + 1) // 2 + (MR + 1) // 2
    ops = torch.full((B * K, MH + MR), SENTINEL, dtype=torch.uint8, device='cuda')
    need = eng.edit_trace_workspace_bytes(B * K, MH, MR, 'word')
    assert need == edit.trace_workspace_bytes(B * K, MH, MR, 'word') > eng.edit_workspace_bytes(B * K, MH, MR, 'word')
    need_char = eng.edit_trace_workspace_bytes(B * K, MH, MR, 'char')
    assert need_char == edit.trace_workspace_bytes(B * K, MH, MR, 'char') > 0
    ws = torch.full((max(need, need_char) + 16,), 0x5a, dtype=torch.uint8, device='cuda')
    size = C.sizeof(eng.EditTraceArgs)

    def args(**kw):
        a = eng.EditTraceArgs()
        a.struct_size, a.mode, a.B, a.K, a.C, a.max_hyp, a.max_ref, a.hyp_pitch, a.ref_pitch = size, 1, B, K, C_, MH, MR, MH, MR
        a.hyp, a.ref, a.is_space, a.rows = hyp.data_ptr(), ref.data_ptr(), sp.data_ptr(), rows.data_ptr()
        a.ops, a.n_ops, a.ops_pitch = ops.data_ptr(), n_ops.data_ptr(), MH + MR
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=size + 8), dict(struct_size=size - 8)]
    bad += [{f: None} for f in ('hyp', 'ref', 'rows', 'ops', 'n_ops', 'workspace', 'is_space')]
    bad += [dict(mode=2), dict(mode=-1), dict(B=0), dict(K=0), dict(C=0), dict(B=1 << 13, K=(1 << 11) + 1), dict(max_hyp=0), dict(max_ref=0),
            dict(max_hyp=(1 << 20) + 1, hyp_pitch=1 << 21), dict(max_ref=(1 << 20) + 1, ref_pitch=1 << 21), dict(hyp_pitch=MH - 1),
            dict(ref_pitch=MR - 1), dict(workspace_bytes=need - 1), dict(workspace=ws.data_ptr() + 8), dict(rows=rows.data_ptr() + 4),
            dict(ops_pitch=units - 1), dict(mode=0, workspace_bytes=need_char, ops_pitch=MH + MR - 1),
            dict(mode=0, workspace_bytes=need_char - 1), dict(ops_pitch=0), dict(ops_pitch=-1)]
    for kw in bad:
        assert lib.qasr_edit_trace(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_edit_trace(s, None) == 1
    assert lib.qasr_edit_trace(s, C.byref(args(ops_pitch=units - 1))) == 1 and b'ops_pitch' in lib.qasr_last_error()
    for shape in ((0, MH, MR, 1), (4, 0, MR, 0), (4, MH, (1 << 20) + 1, 0), (4, MH, MR, 2), ((1 << 24) + 1, MH, MR, 0)):
        assert lib.qasr_edit_trace_workspace_bytes(*shape) == 0, shape
    with pytest.raises(ValueError, match='mode'):
        eng.edit_trace(hyp, None, ref, None, C_, mode='phone', rows_per_ref=K)
    with pytest.raises(ValueError, match='word mode needs is_space'):
        eng.edit_trace(hyp, None, ref, None, C_, mode='word', rows_per_ref=K)
    with pytest.raises(ValueError, match='rows per reference'):
        eng.edit_trace(hyp, None, ref, None, C_, rows_per_ref=2)
    with pytest.raises(ValueError, match='edit_trace: ops must be a cuda uint8'):
        eng.edit_trace(hyp, None, ref, None, C_, rows_per_ref=K, ops=ops[:, :MH + MR - 1])
    with pytest.raises(ValueError, match=f'edit_trace: .* needs a workspace of {edit.trace_workspace_bytes(6, MH, MR, "char")} bytes, above max_workspace_bytes = 1000'):
        eng.edit_trace(hyp, None, ref, None, C_, rows_per_ref=K, max_workspace_bytes=1000)
    torch.cuda.synchronize()
    assert (rows == FILL32).all() and (n_ops == FILL32).all() and (ops == SENTINEL).all() and (ws == 0x5a).all()
    # the same arguments, unbroken, are taken - the least ops pitch of word mode included; char mode needs no mask
    for kw in (dict(ops_pitch=units), dict(mode=0, is_space=None, workspace_bytes=need_char)):
        assert lib.qasr_edit_trace(s, C.byref(args(**kw))) == 0, kw
        torch.cuda.synchronize()
        pitch = units if 'ops_pitch' in kw else MH + MR
        want = edit.trace_host(hyp.cpu().numpy(), None, ref.cpu().numpy(), None, C_, mode='char' if 'mode' in kw else 'word',
                               is_space=np.zeros(C_, dtype=np.uint8), rows_per_ref=K)
        assert rows.cpu().numpy().tobytes() == want.rows.tobytes() and n_ops.cpu().numpy().tobytes() == want.n_ops.tobytes()
        got = ops.cpu().numpy().reshape(-1)
        for p in range(B * K):
            n = int(want.n_ops[p])
            assert got[p * pitch:p * pitch + n].tolist() == want.ops[p, :n].tolist()


# ---------------------------------------------------------------------------------------------------------------- graph
def test_k_ctc_then_k_edit_trace_is_capturable(eng):
    """nothing is allocated and nothing is read on the host: qasr_ctc_collapse -> qasr_edit_trace replays from a graph on new
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
    n_ops = torch.full((B,), FILL32, dtype=torch.int32, device='cuda')
    pitch = (T + 1) // 2 + (L + 1) // 2
    ops = torch.empty((B, pitch), dtype=torch.uint8, device='cuda')
    ws = torch.empty(eng.edit_trace_workspace_bytes(B, T, L, 'word'), dtype=torch.uint8, device='cuda')
    sp_d = _cuda(mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.ctc_collapse(tok_d, lens=None, blank=blank, out=res)
            eng.edit_trace(res.labels, res.n_labels, ref_d, rl_d, C_, mode='word', is_space=sp_d, ops=ops, n_ops=n_ops, workspace=ws, out=rows)
    for tok, ref, rl in (batch(), first, batch()):
        tok_d.copy_(torch.from_numpy(tok)), ref_d.copy_(torch.from_numpy(ref)), rl_d.copy_(torch.from_numpy(rl))
        ops.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        host = ctc.collapse_host(tok, lens=None, blank=blank)
        want = edit.trace_host(host.labels, host.n_labels, ref, rl, C_, mode='word', is_space=mask,
                               ops=np.full((B, pitch), SENTINEL, dtype=np.uint8))
        assert want.rows[:, 0].sum() > 0 and (want.rows[:, 6] == 1).all() and want.n_ops.max() > 10
        assert rows.cpu().numpy().tobytes() == want.rows.tobytes() and n_ops.cpu().numpy().tobytes() == want.n_ops.tobytes()
        assert ops.cpu().numpy().tobytes() == want.ops.tobytes()
