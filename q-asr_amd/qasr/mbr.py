"""Minimum Bayes risk re-ranking of n-best lists: the host statement of k_mbr_pair and k_mbr_pick (csrc/qasr_mbr.hip,
include/qasr.h) and the step from strings to a re-ranked list.  NumPy only: no GPU, no native library.

The beam hands back the row with the highest path score, the maximum-a-posteriori string.  MBR picks, among the K rows of
an utterance, the one whose expected edit distance to the others is smallest, the others weighted by their posterior.
`mbr_host` is the CPU path of rerank_texts and of decode(mbr=) on CPU tensors and the host modules, and the yardstick the
GPU tests compare the kernels with, byte for byte."""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .edit import _row_units, check_mode

MAX_ROWS = 128                          # QASR_BEAM_MAX_WIDTH: rows per utterance
MAX_IDS = 65536                         # QASR_BEAM_MAX_FRAMES: ids per row
MAX_PAIRS = 1 << 24                     # QASR_EDIT_MAX_PROBLEMS: B * K * (K - 1) / 2, and B * K
WTAB_ENTRIES = 16384                    # QASR_MBR_TABLE_ENTRIES
WTAB_STEP = 64                          # score units (2^-16 nat) per table entry
W_ONE = 1 << 24                         # the weight of the best row
MAX_SCALE = 16.0
SCORE_FLOOR = -(1 << 61)                # a row at or below it is not a hypothesis (the beam's empty slots lie far below)
D_CAP = 1 << 40

MBR_RULES = """Minimum Bayes risk order of the K rows of each of B utterances.
Inputs.  labels int32 [B, K, L] (rows of any pitch >= L), n_labels int32 [B, K], score int64 [B, K] in the beam's fixed point
(2^-16 nat), n_hyps int32 [B] or None, n_classes C, mode 'char' | 'word' with is_space uint8 [C]: units and the equality of
words are EDIT_RULES' (qasr/edit.py), exactly.  scale_q = rint(scale * 2^16) with scale in 0 .. 16.  A weight table wtab uint32
[16384], wtab[i] = rint(exp(-(64 i) / 2^16) * 2^24), built in float64 by weight_table(); the device call takes it in device
memory.  K in 1 .. 128, L in 1 .. 65536, B * K and B * K * (K - 1) / 2 at most 2^24.
Present rows.  Row k of utterance b is ABSENT when n_hyps is given and k >= n_hyps[b]: ok = 2, nothing of it is read.  Otherwise
it is VALID when its length lies in 0 .. L, every id inside the length lies in [0, C) and score > -2^61: ok = 1; else ok = 0.
The checks come before any use of an id.  A row is present when ok == 1.  Rows that are not present take no part, neither as
candidates nor as evidence: the outputs of the present rows are those of the call without the others.
Weights.  smax = the largest score among the present rows of b (the list need not be sorted).  d = min(smax - score, 2^40);
x = (d * scale_q + 2^15) >> 16; w = 0 when x >= 16 * 2^16, else wtab[x >> 6].  The best row has w = 2^24, so wsum = the sum of
w over the present rows is > 0 wherever a row is present.  scale = 0: every present row has 2^24.  Rows that are not present
have w = 0; an utterance without a present row has wsum = 0.
Distances.  dist int32 [B, K, K]: dist[b][i][j] = the EDIT_RULES cost (unit costs: the Levenshtein distance) between the units
of rows i and j; symmetric, zero on the diagonal; -1 wherever either row is not present (the diagonal included).
Risk and order.  risk[b][i] = sum over present j of w[j] * dist[i][j], int64: below 2^52, for w <= 2^24, dist < 2^21 (a row
holds at most 2^16 units) and K <= 2^7.  risk = -1 for a row that is not present.  order int32 [B, K]: the present rows by
(risk ascending, score descending, k ascending), then -1.  pick = order[:, 0]; -1 for an utterance without a present row.
Every comparison is on integers.  The division happens once, on the host, in float64: expected_errors = risk / wsum (errors in
the mode's units), posterior = w / wsum.
Against MBR in real numbers.  Let p[j] = exp(-scale_q d[j] / 2^32) (the best row: 1) and R(i) = sum_j p[j] dist[i][j].  The
exponent is rounded to a score unit (half a unit) and floored to the table's step (at most 63 units), so a tabled weight is
within a factor exp(64 / 2^16) = 1 + delta of p[j], delta = 9.77e-4; the table rounds to 2^-24 (2^-25), and a row cut off at
x >= 16 * 2^16 loses p[j] <= exp(-16 + 2^-17) < 2^-23 = eps.  So |w[j] / 2^24 - p[j]| <= delta p[j] + eps, and the risks differ by
at most delta R(i) + E, E = eps (K - 1) Dmax, Dmax the largest distance of the utterance.  The row t the integers pick
therefore has R(t) - min R <= (2 delta min R + 2 E) / (1 - delta) = MBR_BOUND; wherever the second smallest R exceeds the
smallest by more than that, the picks are equal."""
DELTA = float(np.expm1(WTAB_STEP / 65536.0))
EPS = 2.0 ** -23


def mbr_bound(min_risk, K, max_dist) -> float:
    """MBR_BOUND of MBR_RULES: how far the unnormalised real-number risk (best row's weight 1) of the integers' pick may lie
    above the smallest one"""
    return (2 * DELTA * float(min_risk) + 2 * EPS * (int(K) - 1) * float(max_dist)) / (1 - DELTA)


@dataclass
class MbrResult:
    """Outputs of MBR_RULES (NumPy on the host, torch tensors from the device binding): dist int32 [B, K, K], weight int32
    [B, K], wsum int64 [B], risk int64 [B, K], order int32 [B, K], ok int32 [B, K]."""
    dist: object
    weight: object
    wsum: object
    risk: object
    order: object
    ok: object

    pick = property(lambda s: s.order[:, 0])


def weight_table() -> np.ndarray:
    """wtab uint32 [16384] of MBR_RULES, in float64"""
    i = np.arange(WTAB_ENTRIES, dtype=np.float64)
    return np.rint(np.exp(-(WTAB_STEP * i) / 65536.0) * W_ONE).astype(np.uint32)


def check_scale(scale, who) -> int:
    """scale_q of MBR_RULES; a scale outside 0 .. 16 (or not a number) is refused by name"""
    try:
        s = float(scale)
    except (TypeError, ValueError):
        s = float('nan')
    if not 0.0 <= s <= MAX_SCALE:
        raise ValueError(f'{who}: mbr_scale must be a number in 0 .. {MAX_SCALE:g}, got {scale!r}')
    return int(np.rint(s * 65536.0))


def check_shape(B, K, L, who):
    B, K, L = int(B), int(K), int(L)
    if B < 1 or not 1 <= K <= MAX_ROWS:
        raise ValueError(f'{who}: needs at least one utterance and 1 .. {MAX_ROWS} rows per utterance, got [{B}, {K}]')
    if not 1 <= L <= MAX_IDS:
        raise ValueError(f'{who}: rows must hold 1 .. {MAX_IDS} ids, got {L}')
    if B * K > MAX_PAIRS or B * K * (K - 1) // 2 > MAX_PAIRS:
        raise ValueError(f'{who}: {B} utterances of {K} rows are more than {MAX_PAIRS} rows or pairs')


def _distances(units: List[np.ndarray]) -> np.ndarray:
    """the Levenshtein distance of every pair of the unit arrays (int64 each), one row of the cost matrix at a time for all
    pairs at once: t[j] = min(above-left + differs, above + 1), then D[j] = min over k <= j of t[k] + (j - k), a running
    minimum of t - j"""
    n = len(units)
    out = np.zeros((n, n), dtype=np.int32)
    if n < 2:
        return out
    ia, ib = np.triu_indices(n, 1)
    lens = np.array([len(u) for u in units], dtype=np.int64)
    W = max(1, int(lens.max()))
    mat = np.full((n, W), -1, dtype=np.int64)
    for r, u in enumerate(units):
        mat[r, :len(u)] = u
    A, Bm = mat[ia], np.where(mat[ib] < 0, -2, mat[ib])             # pads differ from every unit and from each other
    na, nb = lens[ia], lens[ib]
    ar = np.arange(W + 1, dtype=np.int64)
    prev = np.broadcast_to(ar, (len(ia), W + 1)).copy()
    rows = np.arange(len(ia))
    res = np.where(na == 0, nb, 0)
    for i in range(1, int(na.max()) + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        cur[:, 1:] = np.minimum(prev[:, :-1] + (A[:, i - 1, None] != Bm), prev[:, 1:] + 1)
        cur = np.minimum.accumulate(cur - ar, axis=1) + ar
        hit = na == i
        res[hit] = cur[rows[hit], nb[hit]]
        prev = cur
    out[ia, ib] = res
    out[ib, ia] = res
    return out


def mbr_host(labels, n_labels, score, n_hyps, n_classes, mode='word', is_space=None, scale=1.0, wtab=None) -> MbrResult:
    """MBR_RULES on the host.  labels [B, K, L], n_labels [B, K], score [B, K] integer arrays, n_hyps [B] or None; wtab: the
    table (None: weight_table())."""
    who = 'mbr_host'
    md = check_mode(mode, who)
    labels, n_labels, score = np.asarray(labels), np.asarray(n_labels), np.asarray(score)
    if labels.ndim != 3:
        raise ValueError(f'{who}: labels must be [utterances, rows, ids]')
    B, K, L = labels.shape
    check_shape(B, K, L, who)
    Cn = int(n_classes)
    if Cn < 1:
        raise ValueError(f'{who}: n_classes must be at least 1, got {Cn}')
    if md == 1:
        if is_space is None:
            raise ValueError(f'{who}: word mode needs is_space')
        is_space = np.asarray(is_space)
        if is_space.shape != (Cn,):
            raise ValueError(f'{who}: is_space must have one entry per class ({Cn}), got shape {is_space.shape}')
    for name, v, shape in (('n_labels', n_labels, (B, K)), ('score', score, (B, K))):
        if v.shape != shape:
            raise ValueError(f'{who}: {name} must be {list(shape)}')
    if n_hyps is not None and np.asarray(n_hyps).shape != (B,):
        raise ValueError(f'{who}: n_hyps must have {B} entries')
    scale_q = check_scale(scale, who)
    wtab = weight_table() if wtab is None else np.asarray(wtab)
    if wtab.shape != (WTAB_ENTRIES,):
        raise ValueError(f'{who}: wtab must have {WTAB_ENTRIES} entries')

    dist = np.full((B, K, K), -1, dtype=np.int32)
    weight = np.zeros((B, K), dtype=np.int32)
    wsum = np.zeros(B, dtype=np.int64)
    risk = np.full((B, K), -1, dtype=np.int64)
    order = np.full((B, K), -1, dtype=np.int32)
    ok = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        ids = {}                                                    # unit -> a number, so the rows compare integers
        rows, units = [], []
        for k in range(K):
            if n_hyps is not None and k >= int(n_hyps[b]):
                ok[b, k] = 2
                continue
            n = int(n_labels[b, k])
            if not 0 <= n <= L:
                continue
            row = labels[b, k, :n]
            if not bool(((row >= 0) & (row < Cn)).all()) or int(score[b, k]) <= SCORE_FLOOR:
                continue
            ok[b, k] = 1
            rows.append(k)
            units.append(np.array([ids.setdefault(u, len(ids)) for u in _row_units(row, n, md, is_space)], dtype=np.int64))
        if not rows:
            continue
        rows = np.array(rows)
        d = _distances(units)
        dist[b][np.ix_(rows, rows)] = d
        sc = [int(score[b, k]) for k in rows]
        smax = max(sc)
        w = []
        for s in sc:
            x = (min(smax - s, D_CAP) * scale_q + (1 << 15)) >> 16
            w.append(0 if x >= (16 << 16) else int(wtab[x >> 6]))
        w = np.array(w, dtype=np.int64)
        r = d.astype(np.int64) @ w
        weight[b, rows], wsum[b], risk[b, rows] = w, int(w.sum()), r
        by = sorted(range(len(rows)), key=lambda t: (int(r[t]), -sc[t], int(rows[t])))
        order[b, :len(rows)] = rows[by]
    return MbrResult(dist, weight, wsum, risk, order, ok)


def mbr_device(labels, n_labels, score, n_hyps, n_classes, mode='word', is_space=None, scale=1.0, wtab=None, dist=None,
               workspace=None, out=None, stream=None) -> MbrResult:
    """MBR_RULES on the device (qasr_ctc_mbr: three launches on the current stream, nothing read back): cuda tensors as for
    mbr_host, as the beam leaves them.  Returns an MbrResult of cuda tensors."""
    from . import engine
    return engine.mbr_rerank(labels, n_labels, score, n_hyps, n_classes, mode=mode, is_space=is_space, scale=scale, wtab=wtab,
                             dist=dist, workspace=workspace, out=out, stream=stream)


def expected_errors(res: MbrResult):
    """(expected_errors, posterior) float64 [B, K] from host copies of a result: risk / wsum and weight / wsum; NaN for rows
    that are not present"""
    risk, w = np.asarray(res.risk, dtype=np.float64), np.asarray(res.weight, dtype=np.float64)
    ws = np.asarray(res.wsum, dtype=np.float64)[:, None]
    present = np.asarray(res.ok) == 1
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(present, risk / ws, np.nan), np.where(present, w / ws, np.nan)


def score_q(scores) -> np.ndarray:
    """log-probabilities in nats as the beam's fixed point: rint(score * 2^16), int64"""
    return np.rint(np.asarray(scores, dtype=np.float64) * 65536.0).astype(np.int64)


@dataclass
class Reranked:
    """One utterance of rerank_texts: order lists the rows of the n-best list in MBR order, pick = order[0]; posterior and
    expected_errors are per row of the list as it was given."""
    order: List[int]
    posterior: List[float]
    expected_errors: List[float]

    pick = property(lambda s: s.order[0])


def rerank_texts(nbest: Sequence[Sequence[str]], scores: Sequence[Sequence[float]], use_cer=False, scale=1.0,
                 device: Optional[str] = None) -> List[Reranked]:
    """MBR over lists of strings: nbest[b] holds the rows of utterance b (lists may differ in length, none may be empty),
    scores[b] their log-probabilities in nats.  The characters are numbered by a table of this call and the whitespace mask is
    str.isspace of each, as error_counts does; the rows go through qasr_ctc_mbr on device='cuda' (or a cuda device) and through
    the twin otherwise."""
    who = 'rerank_texts'
    if len(nbest) != len(scores) or any(len(n) != len(s) for n, s in zip(nbest, scores)):
        raise ValueError(f'{who}: nbest and scores must hold the same number of rows for every utterance')
    if not nbest:
        return []
    if any(len(n) < 1 for n in nbest):
        raise ValueError(f'{who}: an utterance without a row cannot be re-ranked')
    scale_q = check_scale(scale, who)
    B, K = len(nbest), max(len(n) for n in nbest)
    L = max(1, max(len(t) for n in nbest for t in n))
    check_shape(B, K, L, who)
    table = {}
    labels = np.zeros((B, K, L), dtype=np.int32)
    n_labels = np.zeros((B, K), dtype=np.int32)
    sc = np.zeros((B, K), dtype=np.int64)
    n_hyps = np.array([len(n) for n in nbest], dtype=np.int32)
    for b, (rows, ss) in enumerate(zip(nbest, scores)):
        sc[b, :len(rows)] = score_q(ss)
        for k, t in enumerate(rows):
            labels[b, k, :len(t)] = [table.setdefault(ch, len(table)) for ch in t]
            n_labels[b, k] = len(t)
    chars = sorted(table, key=table.get) or [' ']
    mask = np.array([ch.isspace() for ch in chars], dtype=np.uint8)
    mode = 'char' if use_cer else 'word'
    if device is not None and str(device).startswith('cuda'):
        import torch
        t = lambda a: torch.from_numpy(a).to(device)
        res = mbr_device(t(labels), t(n_labels), t(sc), t(n_hyps), len(chars), mode=mode, is_space=t(mask), scale=scale_q / 65536.0)
        res = MbrResult(None, res.weight.cpu().numpy(), res.wsum.cpu().numpy(), res.risk.cpu().numpy(), res.order.cpu().numpy(),
                        res.ok.cpu().numpy())
    else:
        res = mbr_host(labels, n_labels, sc, n_hyps, len(chars), mode=mode, is_space=mask, scale=scale_q / 65536.0)
    if (res.ok == 0).any():
        raise RuntimeError(f'{who}: the re-ranking refused a row it packed itself')
    ee, post = expected_errors(res)
    return [Reranked([int(k) for k in res.order[b, :n]], post[b, :n].tolist(), ee[b, :n].tolist()) for b, n in enumerate(n_hyps.tolist())]
