"""Helpers for the edit-path tests (qasr.edit.trace_host, k_edit_trace): a full-matrix Levenshtein that returns the op list under
the stated tie order, written apart from the twin (edit_cases.full_matrix returns the counts only), and a replay of a path."""
HIT, SUB, DEL, INS = 0, 1, 2, 3


def full_matrix_ops(h, r):
    """the forward op list of the whole (len(h) + 1) x (len(r) + 1) cost matrix: every cell remembers the predecessor it took -
    the diagonal, the deletion (i, j - 1) only when strictly cheaper, the insertion (i - 1, j) only when strictly cheaper than
    that - and the walk from the last cell follows what the cells remember; on the borders a deletion (i == 0) or an insertion"""
    n, m = len(h), len(r)
    M = [[0] * (m + 1) for _ in range(n + 1)]
    took = [[None] * (m + 1) for _ in range(n + 1)]
    for j in range(1, m + 1):
        M[0][j], took[0][j] = j, DEL
    for i in range(1, n + 1):
        M[i][0], took[i][0] = i, INS
        for j in range(1, m + 1):
            differ = h[i - 1] != r[j - 1]
            best, op = M[i - 1][j - 1] + differ, SUB if differ else HIT
            if M[i][j - 1] + 1 < best:
                best, op = M[i][j - 1] + 1, DEL
            if M[i - 1][j] + 1 < best:
                best, op = M[i - 1][j] + 1, INS
            M[i][j], took[i][j] = best, op
    ops, i, j = [], n, m
    while i or j:
        op = took[i][j]
        ops.append(op)
        if op != DEL:
            i -= 1
        if op != INS:
            j -= 1
    return ops[::-1], M[n][m]


def apply(ops, hyp_units, ref_fill):
    """replays a path over the hypothesis units: a hit keeps the unit, a substitution and a deletion take the next of ref_fill
    (the reference units the path names, in order), an insertion drops the unit.  Returns the rebuilt reference and how many
    hypothesis units were used."""
    out, i, fill = [], 0, iter(ref_fill)
    for op in ops:
        if op == HIT:
            out.append(hyp_units[i])
            i += 1
        elif op == SUB:
            out.append(next(fill))
            i += 1
        elif op == DEL:
            out.append(next(fill))
        else:
            assert op == INS, op
            i += 1
    assert next(fill, None) is None
    return out, i


def ref_fill(ops, ref_units):
    """the reference units a path substitutes or deletes, in order"""
    out, j = [], 0
    for op in ops:
        if op in (SUB, DEL):
            out.append(ref_units[j])
        if op != INS:
            j += 1
    return out
