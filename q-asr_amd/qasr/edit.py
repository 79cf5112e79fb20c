"""Word and character error counts as an edit distance over label ids: the host statement of k_edit (csrc/qasr_edit.hip,
include/qasr.h) and the step from strings or label rows to counts.  NumPy only: no GPU, no native library.

`edit_host` is the CPU path of error_counts, WER(device=True) on CPU tensors and EncDecCTCModel.error_rate with the host
modules, and the yardstick the GPU tests compare k_edit with, byte for byte.  Its distance is the Levenshtein distance of
nemo/collections/asr/metrics/wer.py over the same units; what it adds is the substitution / deletion / insertion split under
one stated tie order, and the oracle over n-best rows."""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

MAX_IDS = 1 << 20                       # QASR_EDIT_MAX_IDS: ids per row
MODES = {'char': 0, 'word': 1}          # QASR_EDIT_CHAR / QASR_EDIT_WORD
ROW_WORDS = 8                           # int32 per problem: errors, S, D, I, ref_units, hyp_units, ok, 0
TOTAL_WORDS = 16                        # int64 of a totals block
T_ERRORS, T_REF, T_SUB, T_DEL, T_INS, T_HYP, T_ROWS, T_ORACLE, T_INVALID = range(9)

EDIT_RULES = """Edit distance between hypothesis rows and reference rows of label ids, with the substitution / deletion / insertion split.
Rows: hyp int32 [B * K, max_hyp] with hyp_lens int32 [B * K] or None, ref int32 [B, max_ref] with ref_lens int32 [B] or None.  A
length vector of None means the padded row: every one of the max_hyp (max_ref) ids of the row.  Problem p = b * K + k scores
hypothesis row p against reference row b (K rows per reference: the n-best layout).  n_hyps int32 [B] or None: rows
k >= n_hyps[b] are absent.  A row holds at most MAX_IDS = 2^20 ids.
Units.  mode 'char': a unit is one label id, whitespace labels included - what list(text) gives word_error_rate(use_cer=True).
mode 'word': a unit is a maximal run of ids c with is_space[c] == 0 (is_space uint8 [C], the caller's vocabulary[c].isspace());
with a vocabulary of single characters the units of a row are ''.join(...).split() of that row.  Two words are equal when their
id sequences are equal, exactly (the device compares length and a 64-bit hash first and verifies the ids on a match).
Validity: ok[p] = 2 for an absent row; otherwise 0 when the hypothesis row's or the reference row's length is outside
0 .. max_hyp (max_ref) or one of the ids inside the length is outside [0, C); otherwise 1.  The checks come before any use of
an id.  Rows with ok != 1 have every count 0.
Recurrence: D[i][j] over the first i hypothesis units and the first j reference units, unit costs.  D[0][j] = j deletions,
D[i][0] = i insertions.  D[i][j] takes the cheapest of: the diagonal D[i-1][j-1] + (hyp unit i != ref unit j) - a hit or a
substitution -, the deletion D[i][j-1] + 1 and the insertion D[i-1][j] + 1; among predecessors of equal cost the diagonal first,
then the deletion, then the insertion.  Every cell carries (cost, S, D) of the path this picks, so no back-pointer is kept:
I = cost - S - D and hits = j - S - D.
Per problem, int32 [P, 8]: errors, S, D, I, ref_units, hyp_units, ok, 0.
Totals: int64 [16] that every call ADDS to (the caller zeroes it): [0] errors, [1] ref_units, [2] S, [3] D, [4] I, [5] hyp_units
and [6] the number of rows, each over the rows with ok == 1 and k == 0; [7] the oracle: over b, the smallest errors of b's rows
with ok == 1 (nothing for a b without one); [8] the number of rows with ok == 0; [9 .. 15] reserved, left as they are."""


@dataclass
class EditResult:
    """Outputs of EDIT_RULES (arrays: NumPy on the host, torch tensors from the device binding): rows int32 [P, 8], totals
    int64 [16]; rows_per_ref = K."""
    rows: object
    totals: object
    rows_per_ref: int = 1

    errors = property(lambda s: s.rows[:, 0])
    substitutions = property(lambda s: s.rows[:, 1])
    deletions = property(lambda s: s.rows[:, 2])
    insertions = property(lambda s: s.rows[:, 3])
    ref_units = property(lambda s: s.rows[:, 4])
    hyp_units = property(lambda s: s.rows[:, 5])
    ok = property(lambda s: s.rows[:, 6])


TRACE_RULES = """The edit path behind EDIT_RULES: which hypothesis unit met which reference unit.  Rows, units, validity, recurrence and the
per-problem int32 [P, 8] are EDIT_RULES', byte for byte; there is no totals block.
The path runs from cell (n, m) - n hypothesis units, m reference units - back to (0, 0).  At i == 0 the step is a deletion, at
j == 0 an insertion; otherwise it goes to the predecessor the recurrence picked for the cell: the diagonal first, then the deletion
(i, j - 1) only when strictly cheaper, then the insertion (i - 1, j) only when strictly cheaper than that - the order in which
EDIT_RULES' cells took their (cost, S, D).
ops uint8 [P, ops_pitch], ops_pitch >= HU + RU (the unit bounds of the two widths: width in char mode, (width + 1) // 2 in word
mode), in FORWARD order, first unit first.  Codes: 0 a hit and 1 a substitution, each consuming one unit of each row; 2 a
deletion, consuming a reference unit; 3 an insertion, consuming a hypothesis unit.  n_ops int32 [P]: the path's length.  Bytes at
and behind n_ops[p] are left as they are; a caller's ops array is written into.  Rows with ok != 1 have n_ops = 0 and nothing
written.
Invariants: the numbers of codes 1 / 2 / 3 in ops[p, :n_ops[p]] are rows[p, 1 / 2 / 3] (S / D / I), the number of code 0 is
ref_units - S - D, and n_ops = ref_units + I <= hyp_units + ref_units.
Workspace of the device call (trace_workspace_bytes): the choices of all cells, 2 bits each, about HU * RU / 4 bytes per problem
(64 HU when RU <= 64); entry points refuse a shape that needs more than max_workspace_bytes, naming the bytes."""
OP_CODES = 'CSDI'                       # ops code -> the letter of Alignment.ops: correct, substitution, deletion, insertion
MAX_WORKSPACE = 1 << 30                 # max_workspace_bytes of the Python entry points


def check_mode(mode, who) -> int:
    if mode not in MODES:
        raise ValueError(f"{who}: mode must be 'char' or 'word', got {mode!r}")
    return MODES[mode]


def check_widths(max_hyp, max_ref, who):
    for n, w in (('hypothesis', max_hyp), ('reference', max_ref)):
        if not 1 <= int(w) <= MAX_IDS:
            raise ValueError(f'{who}: {n} rows must hold 1 .. {MAX_IDS} ids, got {int(w)}')


def space_mask(vocabulary: Sequence[str], who='space_mask') -> np.ndarray:
    """is_space uint8 [C] of a vocabulary of single characters; an entry of another length is refused by name (word mode
    cuts at labels: a word piece has no place in it)"""
    for c, s in enumerate(vocabulary):
        if not isinstance(s, str) or len(s) != 1:
            raise ValueError(f'{who}: word mode needs a vocabulary of single characters, entry {c} is {s!r}')
    return np.array([s.isspace() for s in vocabulary], dtype=np.uint8)


def _row_units(row, n, mode, is_space):
    """the units of one valid row as a list of hashable values (ids, or tuples of ids)"""
    ids = [int(x) for x in row[:n]]
    if mode == 0:
        return ids
    out, cur = [], []
    for c in ids:
        if is_space[c]:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(c)
    if cur:
        out.append(tuple(cur))
    return out


def _triple(hu, ru):
    """(cost, S, D) of EDIT_RULES at the last cell for unit arrays hu [n], ru [m] (int64), one anti-diagonal at a time: the
    cells with i + j = d need those of d - 1 (deletion, insertion) and d - 2 (diagonal) only"""
    n, m = len(hu), len(ru)
    if n == 0 or m == 0:
        return (n + m, 0, m)                                        # n insertions, or m deletions
    z = lambda: np.zeros(n + 1, dtype=np.int64)
    c2, s2, d2 = z(), z(), z()                                      # diagonal 0: the cell (0, 0)
    c1, s1, d1 = z(), z(), z()                                      # diagonal 1: (0, 1) = one deletion, (1, 0) = one insertion
    c1[0], d1[0], c1[1] = 1, 1, 1
    for d in range(2, n + m + 1):
        c0, s0, d0 = z(), z(), z()
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)             # the cells with i >= 1 and j = d - i >= 1
        if len(i):
            neq = (hu[i - 1] != ru[d - i - 1]).astype(np.int64)
            cost, S, D = c2[i - 1] + neq, s2[i - 1] + neq, d2[i - 1].copy()
            t = c1[i] + 1 < cost                                    # the deletion, from (i, j - 1): only when strictly cheaper
            cost[t], S[t], D[t] = c1[i][t] + 1, s1[i][t], d1[i][t] + 1
            t = c1[i - 1] + 1 < cost                                # the insertion, from (i - 1, j)
            cost[t], S[t], D[t] = c1[i - 1][t] + 1, s1[i - 1][t], d1[i - 1][t]
            c0[i], s0[i], d0[i] = cost, S, D
        if d <= m:
            c0[0], d0[0] = d, d
        if d <= n:
            c0[d] = d
        c2, s2, d2, c1, s1, d1 = c1, s1, d1, c0, s0, d0
    return int(c1[n]), int(s1[n]), int(d1[n])


def edit_host(hyp, hyp_lens, ref, ref_lens, n_classes, mode='char', is_space=None, rows_per_ref=1, n_hyps=None,
              totals=None) -> EditResult:
    """EDIT_RULES on the host.  hyp [B * K, max_hyp], ref [B, max_ref] integer arrays; totals: an int64 [16] block to add to
    (None: a zeroed one)."""
    who = 'edit_host'
    md = check_mode(mode, who)
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    K, Cn = int(rows_per_ref), int(n_classes)
    if hyp.ndim != 2 or ref.ndim != 2:
        raise ValueError(f'{who}: hyp and ref must be matrices [rows, ids]')
    P, B = hyp.shape[0], ref.shape[0]
    if K < 1 or B < 1 or P != B * K:
        raise ValueError(f'{who}: {P} hypothesis rows are not {B} references * {K} rows per reference')
    if Cn < 1:
        raise ValueError(f'{who}: n_classes must be at least 1, got {Cn}')
    check_widths(hyp.shape[1], ref.shape[1], who)
    if md == 1:
        if is_space is None:
            raise ValueError(f'{who}: word mode needs is_space')
        is_space = np.asarray(is_space)
        if is_space.shape != (Cn,):
            raise ValueError(f'{who}: is_space must have one entry per class ({Cn}), got shape {is_space.shape}')
    for name, v, n in (('hyp_lens', hyp_lens, P), ('ref_lens', ref_lens, B), ('n_hyps', n_hyps, B)):
        if v is not None and np.asarray(v).shape != (n,):
            raise ValueError(f'{who}: {name} must have {n} entries')
    tot = np.zeros(TOTAL_WORDS, dtype=np.int64) if totals is None else np.array(totals, dtype=np.int64)
    if tot.shape != (TOTAL_WORDS,):
        raise ValueError(f'{who}: totals must be int64 [{TOTAL_WORDS}]')

    def valid(mat, lens, r):
        n = mat.shape[1] if lens is None else int(lens[r])
        if not 0 <= n <= mat.shape[1]:
            return False, 0
        row = mat[r, :n]
        return bool(((row >= 0) & (row < Cn)).all()), n

    rows = np.zeros((P, ROW_WORDS), dtype=np.int32)
    ref_units = {}
    ids = {}                                                        # unit -> a number, so the diagonals compare integers
    number = lambda units: np.array([ids.setdefault(u, len(ids)) for u in units], dtype=np.int64)
    for p in range(P):
        b, k = divmod(p, K)
        if n_hyps is not None and k >= int(n_hyps[b]):
            rows[p, 6] = 2
            continue
        okh, nh = valid(hyp, hyp_lens, p)
        okr, nr = valid(ref, ref_lens, b)
        if not (okh and okr):
            continue
        if b not in ref_units:
            ref_units[b] = number(_row_units(ref[b], nr, md, is_space))
        hu, ru = number(_row_units(hyp[p], nh, md, is_space)), ref_units[b]
        cost, S, D = _triple(hu, ru)
        rows[p] = (cost, S, D, cost - S - D, len(ru), len(hu), 1, 0)
    r64 = rows.astype(np.int64).reshape(B, K, ROW_WORDS)
    good = r64[:, :, 6] == 1
    first = r64[:, 0][good[:, 0]]
    for w, col in ((T_ERRORS, 0), (T_REF, 4), (T_SUB, 1), (T_DEL, 2), (T_INS, 3), (T_HYP, 5)):
        tot[w] += first[:, col].sum()
    tot[T_ROWS] += len(first)
    any_good = good.any(axis=1)
    tot[T_ORACLE] += np.where(good, r64[:, :, 0], np.iinfo(np.int64).max).min(axis=1)[any_good].sum()
    tot[T_INVALID] += int((r64[:, :, 6] == 0).sum())
    return EditResult(rows, tot, K)


@dataclass
class TraceResult:
    """Outputs of TRACE_RULES (NumPy on the host, torch tensors from the device binding): rows int32 [P, 8], ops uint8
    [P, ops_pitch], n_ops int32 [P]; rows_per_ref = K."""
    rows: object
    ops: object
    n_ops: object
    rows_per_ref: int = 1


def unit_bound(width, mode) -> int:
    """the most units a row of `width` ids holds (edit_units of qasr_edit.hip); mode: 0 char / 1 word"""
    return (int(width) + 1) // 2 if mode == 1 else int(width)


def trace_workspace_bytes(P, max_hyp, max_ref, mode) -> int:
    """qasr_edit_trace_workspace_bytes, stated on the host (mode: 'char' / 'word'): qasr_edit_distance's workspace, then per
    problem a plane of one word per lane and step - strips of 64 NC reference units, HU + 63 steps each, NC = 1 / 4 / 16 from RU"""
    md = check_mode(mode, 'trace_workspace_bytes')
    up16 = lambda x: (x + 15) & ~15
    P, HU, RU = int(P), unit_bound(max_hyp, md), unit_bound(max_ref, md)
    at = up16(P * 16)
    if md == 1:
        at += P * HU * 16 + P * RU * 16
    if RU > 64 * 16:
        at += up16(P * 3 * (HU + 1) * 4)
    nc = 1 if RU <= 64 else (4 if RU <= 256 else 16)
    strips = (RU + 64 * nc - 1) // (64 * nc)
    return up16(at) + P * up16(strips * (HU + 63) * 64 * (4 if nc == 16 else 1))


def check_trace_workspace(P, max_hyp, max_ref, mode, max_workspace_bytes, who):
    need = trace_workspace_bytes(P, max_hyp, max_ref, mode)
    if need > int(max_workspace_bytes):
        raise ValueError(f'{who}: the edit path of {int(P)} problems of {int(max_hyp)} x {int(max_ref)} ids needs a workspace of '
                         f'{need} bytes, above max_workspace_bytes = {int(max_workspace_bytes)}')
    return need


def _path(hu, ru):
    """the forward op list (uint8) of TRACE_RULES for unit arrays hu [n], ru [m] (int64) and the last cell's cost: _triple's
    anti-diagonals with the pick of every cell kept in a plane [n + 1, m + 1], then the walk back"""
    n, m = len(hu), len(ru)
    if n == 0 or m == 0:
        return np.full(n + m, 2 if n == 0 else 3, dtype=np.uint8), n + m
    pick = np.zeros((n + 1, m + 1), dtype=np.uint8)
    c2 = np.zeros(n + 1, dtype=np.int64)                            # diagonal 0: the cell (0, 0)
    c1 = np.zeros(n + 1, dtype=np.int64)                            # diagonal 1
    c1[0], c1[1] = 1, 1
    for d in range(2, n + m + 1):
        c0 = np.zeros(n + 1, dtype=np.int64)
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)             # the cells with i >= 1 and j = d - i >= 1
        if len(i):
            neq = (hu[i - 1] != ru[d - i - 1]).astype(np.int64)
            cost, op = c2[i - 1] + neq, neq.astype(np.uint8)
            t = c1[i] + 1 < cost                                    # the deletion, from (i, j - 1): only when strictly cheaper
            cost[t], op[t] = c1[i][t] + 1, 2
            t = c1[i - 1] + 1 < cost                                # the insertion, from (i - 1, j)
            cost[t], op[t] = c1[i - 1][t] + 1, 3
            c0[i], pick[i, d - i] = cost, op
        if d <= m:
            c0[0] = d
        if d <= n:
            c0[d] = d
        c2, c1 = c1, c0
    back, i, j = [], n, m
    while i > 0 or j > 0:
        op = 2 if i == 0 else (3 if j == 0 else int(pick[i, j]))
        back.append(op)
        i, j = i - (op != 2), j - (op != 3)
    return np.array(back[::-1], dtype=np.uint8), int(c1[n])


def trace_host(hyp, hyp_lens, ref, ref_lens, n_classes, mode='char', is_space=None, rows_per_ref=1, n_hyps=None, ops=None,
               max_workspace_bytes=MAX_WORKSPACE) -> TraceResult:
    """TRACE_RULES on the host: edit_host's arguments and rows; ops: a uint8 [P, >= HU + RU] array to write into (None: a
    zeroed one of the least pitch)."""
    who = 'trace_host'
    md = check_mode(mode, who)
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    if hyp.ndim == 2 and ref.ndim == 2:                             # the cap before any work; edit_host refuses the other shapes
        check_trace_workspace(hyp.shape[0], hyp.shape[1], ref.shape[1], mode, max_workspace_bytes, who)
    res = edit_host(hyp, hyp_lens, ref, ref_lens, n_classes, mode=mode, is_space=is_space, rows_per_ref=rows_per_ref, n_hyps=n_hyps)
    P, K = hyp.shape[0], int(rows_per_ref)
    units = unit_bound(hyp.shape[1], md) + unit_bound(ref.shape[1], md)
    if ops is None:
        ops = np.zeros((P, units), dtype=np.uint8)
    if not isinstance(ops, np.ndarray) or ops.dtype != np.uint8 or ops.ndim != 2 or ops.shape[0] != P or ops.shape[1] < units:
        raise ValueError(f'{who}: ops must be a uint8 array [{P}, >= {units}] (the unit bounds of the two widths)')
    n_ops = np.zeros(P, dtype=np.int32)
    ids = {}
    number = lambda us: np.array([ids.setdefault(u, len(ids)) for u in us], dtype=np.int64)
    sp = None if is_space is None else np.asarray(is_space)
    for p in range(P):
        if res.rows[p, 6] != 1:
            continue
        b = p // K
        nh = hyp.shape[1] if hyp_lens is None else int(hyp_lens[p])
        nr = ref.shape[1] if ref_lens is None else int(ref_lens[b])
        path, cost = _path(number(_row_units(hyp[p], nh, md, sp)), number(_row_units(ref[b], nr, md, sp)))
        assert cost == res.rows[p, 0] and len(path) == res.rows[p, 4] + res.rows[p, 3], (p, cost, len(path))
        ops[p, :len(path)], n_ops[p] = path, len(path)
    return TraceResult(res.rows, ops, n_ops, K)


def trace_device(hyp, hyp_lens, ref, ref_lens, n_classes, mode='char', is_space=None, rows_per_ref=1, n_hyps=None, ops=None,
                 workspace=None, out=None, stream=None, max_workspace_bytes=MAX_WORKSPACE) -> TraceResult:
    """TRACE_RULES on the device (qasr_edit_trace: two launches on the current stream, nothing read back): cuda matrices as for
    edit_device; ops: a cuda uint8 [P, >= HU + RU] to write into.  Returns a TraceResult of cuda tensors."""
    from . import engine
    return engine.edit_trace(hyp, hyp_lens, ref, ref_lens, n_classes, mode=mode, is_space=is_space, rows_per_ref=rows_per_ref,
                             n_hyps=n_hyps, ops=ops, workspace=workspace, out=out, stream=stream,
                             max_workspace_bytes=max_workspace_bytes)


def alignments_of(trace, hyp, hyp_lens, ref, ref_lens, vocabulary, mode='char', is_space=None):
    """One qasr.ctc.Alignment per problem of a TraceResult from host copies (NumPy) of its arrays and of the label rows it was
    made from; None for a problem with ok != 1.  A unit's text is the vocabulary entries of its ids, joined."""
    from .ctc import Alignment
    md = check_mode(mode, 'alignments_of')
    rows, ops, n_ops = np.asarray(trace.rows), np.asarray(trace.ops), np.asarray(trace.n_ops)
    hyp, ref, K = np.asarray(hyp), np.asarray(ref), int(trace.rows_per_ref)
    sp = None if is_space is None else np.asarray(is_space)
    text = (lambda u: vocabulary[u]) if md == 0 else (lambda u: ''.join(vocabulary[c] for c in u))
    out = []
    for p in range(rows.shape[0]):
        if rows[p, 6] != 1:
            out.append(None)
            continue
        b = p // K
        nh = hyp.shape[1] if hyp_lens is None else int(hyp_lens[p])
        nr = ref.shape[1] if ref_lens is None else int(ref_lens[b])
        hu = [text(u) for u in _row_units(hyp[p], nh, md, sp)]
        ru = [text(u) for u in _row_units(ref[b], nr, md, sp)]
        codes = ops[p, :int(n_ops[p])].tolist()
        ri, hi, i, j = [], [], 0, 0
        for c in codes:
            ri.append(j if c != 3 else None)
            hi.append(i if c != 2 else None)
            i, j = i + (c != 2), j + (c != 3)
        if i != len(hu) or j != len(ru):
            raise RuntimeError(f'alignments_of: the ops of problem {p} consume {i} x {j} units, its rows hold {len(hu)} x {len(ru)}')
        r = rows[p]
        out.append(Alignment(''.join(OP_CODES[c] for c in codes), ru, hu, ri, hi, counts_of(r[0], r[1], r[2], r[3], r[4], r[5])))
    return out


def listing(alignment) -> str:
    """The two-line listing of an Alignment as sclite prints it: one column per op, padded to equal width and joined by one
    blank; substituted, deleted and inserted units in upper case, correct ones as they are; `*` fillers of the unit's length
    opposite an insertion or a deletion; a whitespace unit (character mode) shows as `_`."""
    show = lambda u: ''.join('_' if ch.isspace() else ch for ch in u)
    top, bot = [], []
    for op, ri, hi in zip(alignment.ops, alignment.ref_index, alignment.hyp_index):
        r = show(alignment.ref_units[ri]) if ri is not None else None
        h = show(alignment.hyp_units[hi]) if hi is not None else None
        if op == 'C':
            a, b = r, h
        elif op == 'S':
            a, b = r.upper(), h.upper()
        elif op == 'D':
            a, b = r.upper(), '*' * len(r)
        else:
            a, b = '*' * len(h), h.upper()
        w = max(len(a), len(b))
        top.append(a.ljust(w)), bot.append(b.ljust(w))
    return ('REF: ' + ' '.join(top)).rstrip() + '\n' + ('HYP: ' + ' '.join(bot)).rstrip()


def confusions(alignments, top=None):
    """(substitutions, deletions, insertions) over Alignments (None entries skipped): lists of ((ref, hyp), count), (unit, count)
    and (unit, count), the most frequent first and equal counts in the order of the units; top: at most that many of each."""
    sub, dele, ins = {}, {}, {}
    for a in alignments:
        if a is None:
            continue
        for op, ri, hi in zip(a.ops, a.ref_index, a.hyp_index):
            if op == 'S':
                k = (a.ref_units[ri], a.hyp_units[hi])
                sub[k] = sub.get(k, 0) + 1
            elif op == 'D':
                dele[a.ref_units[ri]] = dele.get(a.ref_units[ri], 0) + 1
            elif op == 'I':
                ins[a.hyp_units[hi]] = ins.get(a.hyp_units[hi], 0) + 1
    order = lambda d: sorted(d.items(), key=lambda kv: (-kv[1], kv[0]))[:top]
    return order(sub), order(dele), order(ins)


def counts_of(errors, S, D, I, ref_units, hyp_units):
    """an ErrorCounts with word_error_rate's rate: errors / ref_units, inf for no reference unit"""
    from .ctc import ErrorCounts
    e, r = int(errors), int(ref_units)
    return ErrorCounts(e, int(S), int(D), int(I), r, int(hyp_units), 1.0 * e / r if r != 0 else float('inf'))


def totals_counts(totals):
    """the ErrorCounts of a totals block (an int64 [16] array, read from the device by the caller)"""
    t = [int(x) for x in totals]
    return counts_of(t[T_ERRORS], t[T_SUB], t[T_DEL], t[T_INS], t[T_REF], t[T_HYP])


def report_of(rows, totals, rows_per_ref=1):
    """an ErrorReport from host copies of a result's rows [B * K, 8] and totals [16]: per_utterance is row k = 0 of each b"""
    from .ctc import ErrorReport
    rows = np.asarray(rows).reshape(-1, int(rows_per_ref), ROW_WORDS)
    per = [counts_of(r[0], r[1], r[2], r[3], r[4], r[5]) for r in rows[:, 0].tolist()]
    return ErrorReport(totals_counts(totals), int(totals[T_ORACLE]), per, int(totals[T_INVALID]))


def edit_device(hyp, hyp_lens, ref, ref_lens, n_classes, mode='char', is_space=None, rows_per_ref=1, n_hyps=None, totals=None,
                workspace=None, out=None, stream=None) -> EditResult:
    """EDIT_RULES on the device (qasr_edit_distance: at most three launches on the current stream, nothing read back): cuda int32
    matrices as for edit_host; totals: a cuda int64 [16] block to add to (None: a zeroed one).  Returns an EditResult of cuda
    tensors."""
    from . import engine
    return engine.edit_distance(hyp, hyp_lens, ref, ref_lens, n_classes, mode=mode, is_space=is_space, rows_per_ref=rows_per_ref,
                                n_hyps=n_hyps, totals=totals, workspace=workspace, out=out, stream=stream)


def _pack(texts: Sequence[str], table):
    n = max(1, max((len(t) for t in texts), default=0))
    mat = np.zeros((len(texts), n), dtype=np.int32)
    lens = np.zeros(len(texts), dtype=np.int32)
    for r, t in enumerate(texts):
        mat[r, :len(t)] = [table.setdefault(ch, len(table)) for ch in t]
        lens[r] = len(t)
    return mat, lens


def align_texts(hyps: List[str], refs: List[str], use_cer=False, device: Optional[str] = None,
                max_workspace_bytes=MAX_WORKSPACE):
    """One Alignment per (hypothesis, reference) pair of strings, packed as error_counts packs them: through k_edit_trace on
    device='cuda' (or a cuda device), where only ops and n_ops are read back beside the rows, and through the twin otherwise."""
    if len(hyps) != len(refs):
        raise ValueError("In word error rate calculation, hypotheses and reference lists must have the same "
                         "number of elements. But I got:{0} and {1} correspondingly".format(len(hyps), len(refs)))
    if not hyps:
        return []
    table = {}
    h, hl = _pack(hyps, table)
    r, rl = _pack(refs, table)
    chars = sorted(table, key=table.get) or [' ']
    mask = np.array([ch.isspace() for ch in chars], dtype=np.uint8)
    mode = 'char' if use_cer else 'word'
    if device is not None and str(device).startswith('cuda'):
        import torch
        t = lambda a: torch.from_numpy(a).to(device)
        res = trace_device(t(h), t(hl), t(r), t(rl), len(chars), mode=mode, is_space=t(mask), max_workspace_bytes=max_workspace_bytes)
        res = TraceResult(res.rows.cpu().numpy(), res.ops.cpu().numpy(), res.n_ops.cpu().numpy(), 1)
    else:
        res = trace_host(h, hl, r, rl, len(chars), mode=mode, is_space=mask, max_workspace_bytes=max_workspace_bytes)
    if (res.rows[:, 6] != 1).any():
        raise RuntimeError('align_texts: the edit distance refused a row it packed itself')
    return alignments_of(res, h, hl, r, rl, chars, mode=mode, is_space=mask)


def error_counts(hyps: List[str], refs: List[str], use_cer=False, device: Optional[str] = None):
    """The counts behind word_error_rate(hyps, refs, use_cer) as an ErrorCounts, for callers that only have strings: the
    characters are numbered by a table of this call, the whitespace mask is str.isspace of each, and the rows go through
    k_edit on device='cuda' (or a cuda device) and through the twin otherwise."""
    if len(hyps) != len(refs):
        raise ValueError("In word error rate calculation, hypotheses and reference lists must have the same "
                         "number of elements. But I got:{0} and {1} correspondingly".format(len(hyps), len(refs)))
    if not hyps:
        return counts_of(0, 0, 0, 0, 0, 0)
    table = {}
    h, hl = _pack(hyps, table)
    r, rl = _pack(refs, table)
    chars = sorted(table, key=table.get) or [' ']
    mask = np.array([ch.isspace() for ch in chars], dtype=np.uint8)
    mode = 'char' if use_cer else 'word'
    if device is not None and str(device).startswith('cuda'):
        import torch
        t = lambda a: torch.from_numpy(a).to(device)
        res = edit_device(t(h), t(hl), t(r), t(rl), len(chars), mode=mode, is_space=t(mask))
        totals = res.totals.cpu().numpy()
    else:
        totals = edit_host(h, hl, r, rl, len(chars), mode=mode, is_space=mask).totals
    if int(totals[T_INVALID]):
        raise RuntimeError('error_counts: the edit distance refused a row it packed itself')
    return totals_counts(totals)
