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
