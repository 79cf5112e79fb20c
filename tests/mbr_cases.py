"""Case builders for the MBR tests (qasr.mbr, k_mbr_pair, k_mbr_pick): n-best lists of seeded random id rows made from one
hidden row by random edits, with scores in the beam's fixed point, and an MBR in float64 that shares no code with the twin."""
import numpy as np

import edit_cases as ec

CLASSES = ec.CLASSES
space_mask = ec.space_mask


def nbest(seed, C, B, K, L, min_len=0, space_p=0.2, edit_p=0.2, spread=3.0, sort=True, lengths=None):
    """labels int32 [B, K, L] (pads: an id that would be refused), n_labels [B, K], score int64 [B, K]: per utterance K edited
    copies of one random row of min_len .. L ids (lengths: a list of K lengths per utterance instead), scores spread over about `spread` nats, the best first when sort"""
    g = np.random.default_rng(seed)
    sp = np.flatnonzero(space_mask(C))
    labels = np.full((B, K, L), C + 5, dtype=np.int32)
    n_labels = np.zeros((B, K), dtype=np.int32)
    score = np.zeros((B, K), dtype=np.int64)

    def ids(n):
        x = g.integers(0, C, n)
        s = g.random(n) < space_p
        x[s] = g.choice(sp, int(s.sum()))
        return x

    for b in range(B):
        base = ids(int(g.integers(min_len, L + 1)) if lengths is None else L)
        for k in range(K):
            out = []
            for c in base:
                u = g.random()
                if u < edit_p / 3:
                    continue
                out.append(int(ids(1)[0]) if u < 2 * edit_p / 3 else int(c))
                if u > 1 - edit_p / 3:
                    out.append(int(ids(1)[0]))
            if lengths is not None:
                n = int(lengths[b][k])
                out = (out + [int(x) for x in ids(max(n - len(out), 0))])[:n]
            out = out[:L]
            labels[b, k, :len(out)], n_labels[b, k] = out, len(out)
        s = np.rint(-g.random(K) * spread * 65536 - 65536 * 20).astype(np.int64)
        score[b] = np.sort(s)[::-1] if sort else s
    return dict(labels=labels, n_labels=n_labels, score=score, n_hyps=None, C=C, is_space=space_mask(C))


def words_case(seed, word_counts, C=29, max_len=1):
    """rows of the given numbers of words (a list of K counts per utterance), words of 1 .. max_len ids over six letters,
    one whitespace id between them (max_len 1: the width 2 n - 1 makes the largest count the unit bound), edited copies of one
    row so that hits and all three operations occur"""
    g = np.random.default_rng(seed)
    sp = int(np.flatnonzero(space_mask(C))[0])
    letters = np.setdiff1d(np.arange(C), np.flatnonzero(space_mask(C)))[:6]
    B, K = len(word_counts), len(word_counts[0])
    rows = []
    for counts in word_counts:
        base = [list(g.choice(letters, int(g.integers(1, max_len + 1)))) for _ in range(max(max(counts), 1))]
        for n in counts:
            ws = []
            for w in base:
                u = g.random()
                if u < 0.05:
                    continue
                ws.append([int(g.choice(letters))] if u < 0.1 else (w[:-1] + [int(letters[(list(letters).index(w[-1]) + 1) % 6])] if u < 0.15 else w))
            ws = (ws + base)[:n]
            rows.append([int(c) for i, w in enumerate(ws) for c in ([sp] * int(i > 0) + [int(x) for x in w])])
    L = max(1, max(len(r) for r in rows))
    labels = np.full((B, K, L), C + 5, dtype=np.int32)
    n_labels = np.zeros((B, K), dtype=np.int32)
    for p, r in enumerate(rows):
        labels[p // K, p % K, :len(r)], n_labels[p // K, p % K] = r, len(r)
    score = np.sort(np.rint(-g.random((B, K)) * 3 * 65536 - 65536 * 9).astype(np.int64), axis=1)[:, ::-1].copy()
    return dict(labels=labels, n_labels=n_labels, score=score, n_hyps=None, C=C, is_space=space_mask(C))


def from_lists(rows, scores, C=29, L=None):
    """one utterance per list of id lists"""
    B, K = len(rows), max(len(r) for r in rows)
    L = L or max(1, max(len(x) for r in rows for x in r))
    labels = np.full((B, K, L), C + 5, dtype=np.int32)
    n_labels = np.zeros((B, K), dtype=np.int32)
    score = np.full((B, K), -(1 << 62), dtype=np.int64)
    for b, r in enumerate(rows):
        for k, x in enumerate(r):
            labels[b, k, :len(x)], n_labels[b, k] = x, len(x)
        score[b, :len(r)] = scores[b]
    return dict(labels=labels, n_labels=n_labels, score=score, n_hyps=np.array([len(r) for r in rows], dtype=np.int32), C=C,
                is_space=space_mask(C))


def levenshtein(a, b):
    """the textbook two-row distance, written apart from the twin's"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]


def float_mbr(case, b, mode, scale_q, rows=None):
    """MBR of utterance b in float64 over the rows given (default: all K, which must be valid): (R [n] the risks with the best
    row's weight 1, the largest distance, the argmin)"""
    K = case['labels'].shape[1]
    rows = list(range(K)) if rows is None else list(rows)
    units = [ec.units(case['labels'][b, k], int(case['n_labels'][b, k]), mode, case['is_space']) for k in rows]
    s = np.array([int(case['score'][b, k]) for k in rows], dtype=np.float64)
    p = np.exp((scale_q / 65536.0) * (s - s.max()) / 65536.0)
    D = np.array([[levenshtein(x, y) for y in units] for x in units], dtype=np.float64)
    R = D @ p
    return R, float(D.max()), int(np.argmin(R))


def small_cases():
    """(name, case) pairs for the CPU tests: every class count, K = 2 .. 8, sorted and unsorted lists, a tie-heavy alphabet"""
    out = []
    for C in CLASSES:
        out.append((f'random_c{C}', nbest(11 + C, C, B=3, K=5, L=30, min_len=8)))
        out.append((f'unsorted_c{C}', nbest(31 + C, C, B=2, K=8, L=24, min_len=6, sort=False)))
    out.append(('binary_ties', nbest(5, 2, B=4, K=6, L=16, min_len=4, space_p=0.3, edit_p=0.5, spread=0.5)))
    out.append(('pairs', nbest(9, 29, B=5, K=2, L=20)))
    out.append(('flat_scores', nbest(13, 29, B=3, K=7, L=26, min_len=10, spread=0.01)))
    out.append(('far_scores', nbest(17, 29, B=3, K=4, L=26, min_len=10, spread=40.0)))
    return out
