"""Seeded token matrices for the greedy-CTC tests and their fixture generator (tests/golden/gen_golden_ctc.py): rows
with the run structure of real CTC output plus the rows that break a chunked implementation.  Data only, NumPy only."""
import numpy as np

FIXTURE_T = (1, 63, 64, 65, 250, 1000)
FIXTURE_VOCAB = (28, 5206)          # labels; blank = the vocabulary size (29 / 5207 classes)


def realistic_row(rng, T, blank, first_emits=False, last_emits=False):
    """Long blank stretches, label runs of 1-4 frames, a label repeated across ONE blank (two emissions), a label
    repeated without a blank (one emission), other labels back to back."""
    out = []
    if not first_emits:
        out += [blank] * int(rng.integers(1, 12))
    prev = None
    while len(out) < T:
        lab = int(rng.integers(0, blank))
        kind = rng.random()
        if prev is not None and kind < 0.15:
            out += [blank, prev] if out[-1] != blank else [prev]     # same label again behind a single blank
            lab = prev
        elif prev is not None and kind < 0.30:
            lab = prev                                               # same label, no blank between: the run goes on
        out += [lab] * int(rng.integers(1, 5))
        prev = lab
        if rng.random() < 0.7:
            out += [blank] * int(rng.geometric(0.25))
    row = np.array(out[:T], dtype=np.int32)
    if first_emits and row[0] == blank:
        row[0] = int(rng.integers(0, blank))
    if last_emits and row[-1] == blank:
        row[-1] = int(rng.integers(0, blank))
    return row


def adversarial_rows(rng, T, blank):
    """all blank; one non-blank run over the whole row; every frame emits (no two neighbours equal, no blank); first and
    last frame emit"""
    lab = int(rng.integers(0, blank))
    alt = np.empty(T, dtype=np.int32)
    a, b = int(rng.integers(0, blank)), int(rng.integers(0, blank - 1))
    b = b + 1 if b >= a else b                                      # b != a
    alt[0::2], alt[1::2] = a, b
    walk = rng.integers(0, blank, size=T).astype(np.int32)
    for t in range(1, T):                                            # random labels, neighbours forced apart
        if walk[t] == walk[t - 1]:
            walk[t] = (walk[t] + 1) % blank
    return [np.full(T, blank, dtype=np.int32), np.full(T, lab, dtype=np.int32), alt, walk,
            realistic_row(rng, T, blank, first_emits=True, last_emits=True)]


def token_matrix(seed, T, n_labels, n_realistic=4):
    """[n_realistic + 5, T] int32: realistic rows, then adversarial_rows"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = [realistic_row(rng, T, n_labels) for _ in range(n_realistic)] + adversarial_rows(rng, T, n_labels)
    return np.stack(rows)


def frame_scores(seed, shape):
    """log-probability-like float32 values <= 0 with exact zeros and repeated values mixed in (ties inside a run)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = -rng.gamma(0.5, 0.7, size=shape).astype(np.float32)
    x[rng.random(shape) < 0.1] = 0.0
    x = np.where(rng.random(shape) < 0.2, np.float32(-0.25), x)
    return np.ascontiguousarray(x, dtype=np.float32)


def vocabulary(n_labels):
    from qasr import topology
    if n_labels == 28:
        return list(topology.VOCABULARY)
    return topology.zh_placeholder_vocabulary(n_labels)
