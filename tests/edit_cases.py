"""Case builders for the edit-distance tests (qasr.edit, k_edit): seeded random id rows over 2 / 29 / 5207 classes, structured rows,
and a full-matrix Levenshtein with an explicit back-trace that shares no code with the twin."""
import numpy as np

CLASSES = (2, 29, 5207)


def space_mask(C):
    """is_space uint8 [C]: class 0 always (the space of the 29-class alphabet), two more in the wide alphabet"""
    m = np.zeros(C, dtype=np.uint8)
    m[0] = 1
    if C > 5000:
        m[[17, 5000]] = 1
    return m


def random_rows(seed, C, B, K, max_hyp, max_ref, space_p=0.2, edit_p=0.15, min_ref=0):
    """B reference rows and B * K hypothesis rows made from them by random substitutions, deletions and insertions, so that hits,
    ties and all three operations occur; lengths vary from row to row; pads hold an id that would be refused (C + 5)"""
    g = np.random.default_rng(seed)
    sp = np.flatnonzero(space_mask(C))
    ref = np.full((B, max_ref), C + 5, dtype=np.int32)
    hyp = np.full((B * K, max_hyp), C + 5, dtype=np.int32)
    rl, hl = np.zeros(B, dtype=np.int32), np.zeros(B * K, dtype=np.int32)

    def ids(n):
        x = g.integers(0, C, n)
        s = g.random(n) < space_p
        x[s] = g.choice(sp, int(s.sum()))
        return x

    for b in range(B):
        n = int(g.integers(min_ref, max_ref + 1))
        r = ids(n)
        ref[b, :n], rl[b] = r, n
        for k in range(K):
            out = []
            for c in r:
                u = g.random()
                if u < edit_p / 3:
                    continue
                out.append(int(ids(1)[0]) if u < 2 * edit_p / 3 else int(c))
                if u > 1 - edit_p / 3:
                    out.append(int(ids(1)[0]))
            out = out[:max_hyp]
            hyp[b * K + k, :len(out)], hl[b * K + k] = out, len(out)
    return dict(hyp=hyp, hyp_lens=hl, ref=ref, ref_lens=rl, C=C, K=K, is_space=space_mask(C))


def from_lists(hyps, refs, C, K=1, is_space=None, pad=None, hyp_width=None, ref_width=None):
    """rows from lists of id lists (hyps: B * K lists), padded with `pad` (default: an id that would be refused)"""
    pad = C + 5 if pad is None else pad
    hw = hyp_width or max(1, max(len(h) for h in hyps))
    rw = ref_width or max(1, max(len(r) for r in refs))
    hyp = np.full((len(hyps), hw), pad, dtype=np.int32)
    ref = np.full((len(refs), rw), pad, dtype=np.int32)
    for i, h in enumerate(hyps):
        hyp[i, :len(h)] = h
    for i, r in enumerate(refs):
        ref[i, :len(r)] = r
    return dict(hyp=hyp, hyp_lens=np.array([len(h) for h in hyps], dtype=np.int32), ref=ref,
                ref_lens=np.array([len(r) for r in refs], dtype=np.int32), C=C, K=K,
                is_space=space_mask(C) if is_space is None else np.asarray(is_space, dtype=np.uint8))


def encode(texts, vocabulary):
    """strings over a vocabulary of single characters as id lists"""
    at = {ch: i for i, ch in enumerate(vocabulary)}
    return [[at[ch] for ch in t] for t in texts]


def units(row, n, mode, is_space):
    """the units of a row, written apart from the twin's: ids, or the id tuples between whitespace ids"""
    row = [int(x) for x in row[:n]]
    if mode == 'char':
        return row
    words, i = [], 0
    while i < len(row):
        if is_space[row[i]]:
            i += 1
            continue
        j = i
        while j < len(row) and not is_space[row[j]]:
            j += 1
        words.append(tuple(row[i:j]))
        i = j
    return words


def full_matrix(h, r):
    """(errors, S, D, I) of the whole (len(h) + 1) x (len(r) + 1) cost matrix and a back-trace from its last cell that prefers the
    diagonal, then the deletion (i, j - 1), then the insertion (i - 1, j) among the predecessors that give the cell's cost"""
    n, m = len(h), len(r)
    M = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        M[0][j] = j
    for i in range(1, n + 1):
        M[i][0] = i
        for j in range(1, m + 1):
            M[i][j] = min(M[i - 1][j - 1] + (h[i - 1] != r[j - 1]), M[i][j - 1] + 1, M[i - 1][j] + 1)
    i, j, S, D, I = n, m, 0, 0, 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and M[i][j] == M[i - 1][j - 1] + (h[i - 1] != r[j - 1]):
            S += h[i - 1] != r[j - 1]
            i, j = i - 1, j - 1
        elif j > 0 and M[i][j] == M[i][j - 1] + 1:
            D += 1
            j -= 1
        else:
            assert i > 0 and M[i][j] == M[i - 1][j] + 1
            I += 1
            i -= 1
    return M[n][m], S, D, I


def small_cases():
    """(name, case) pairs for the CPU tests: every class count, K = 1 and 3, short rows with many ties, structured rows"""
    out = []
    for C in CLASSES:
        out.append((f'random_c{C}', random_rows(11 + C, C, B=6, K=1, max_hyp=40, max_ref=36)))
        out.append((f'nbest_c{C}', random_rows(23 + C, C, B=4, K=3, max_hyp=30, max_ref=24)))
    out.append(('binary_ties', random_rows(5, 2, B=8, K=2, max_hyp=24, max_ref=20, space_p=0.3, edit_p=0.5)))
    a, b, sp = 1, 2, 0
    out.append(('swap', from_lists([[a, sp, b]], [[b, sp, a]], 29)))                        # "a b" against "b a"
    out.append(('repeated', from_lists([[a, sp, a, sp, a]], [[a]], 29)))                    # a repeated word against one occurrence
    out.append(('one_of_repeated', from_lists([[a]], [[a, sp, a, sp, a]], 29)))
    out.append(('empty_rows', from_lists([[], [a, sp, b], []], [[a, b], [], []], 29)))
    out.append(('only_space', from_lists([[sp, sp, sp], [a]], [[a], [sp, sp]], 29)))
    out.append(('edges_of_space', from_lists([[sp, a, b, sp, sp, b, sp]], [[a, b, sp, b]], 29)))
    out.append(('last_id_differs', from_lists([[3, 4, 5, 6, sp, 7]], [[3, 4, 5, 8, sp, 7]], 29)))
    return out
