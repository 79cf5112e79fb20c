"""Reserved engines (qasr_engine_reserve, include/qasr.h): the bucket policy, restated in Python.

A reserved engine rounds every batch up to a bucket - all `max_batch` rows, frames up to a bucket edge - and keeps one
captured graph per bucket.  The policy is a pure function of the envelope; csrc/qasr_ragged.hip states it in C
(`qasr_ragged_bucket_frames`), tests/test_ragged_cpu.py holds the two together.

    envelope_frames  the envelope in frames: the larger of max_frames and the front-end's frame count of max_samples,
                     rounded up to a whole number of TILE-frame tiles
    step             envelope / TILE tiles are cut into at most max_graphs equal steps of whole tiles
    bucket_frames    the smallest multiple of the step that holds T, capped at the envelope

Every edge is a multiple of TILE (128 frames: the largest frame tile of the separable-layer kernels, so a bucket never
ends inside a tile) and therefore of every pad_to that divides 128.
"""

TILE = 128
HOP = 160
DEFAULT_MAX_GRAPHS = 16


def frontend_frames(samples, pad_to=16):
    """qasr_frontend_frames: STFT frames of a padded row of `samples`, rounded up to a multiple of pad_to"""
    n = 1 + samples // HOP
    if pad_to > 0 and n % pad_to:
        n += pad_to - n % pad_to
    return n


def envelope_frames(max_samples=0, max_frames=0, pad_to=16):
    """qasr_ragged_envelope_frames; -1 for arguments the engine refuses"""
    pad_to = pad_to or 16
    if pad_to < 1 or TILE % pad_to or max_samples < 0 or max_frames < 0 or (max_samples == 0 and max_frames == 0):
        return -1
    if max_samples > (1 << 28) or max_frames > (1 << 24):
        return -1
    m = max_frames
    if max_samples > 0:
        m = max(m, frontend_frames(max_samples, pad_to))
    return (m + TILE - 1) // TILE * TILE


def step_frames(max_frames, max_graphs=DEFAULT_MAX_GRAPHS):
    units = max_frames // TILE
    return (units + max_graphs - 1) // max_graphs * TILE


def bucket_frames(max_frames, max_graphs, T):
    """qasr_ragged_bucket_frames: the bucket edge of a batch of T frames, -1 outside the envelope"""
    if max_frames < 1 or max_graphs < 1 or T < 1 or max_frames % TILE or T > max_frames:
        return -1
    step = step_frames(max_frames, max_graphs)
    return min((T + step - 1) // step * step, max_frames)


def bucket_edges(max_frames, max_graphs=DEFAULT_MAX_GRAPHS):
    """every bucket edge of an envelope, ascending (at most max_graphs of them)"""
    step = step_frames(max_frames, max_graphs)
    return sorted({min(e, max_frames) for e in range(step, max_frames + step, step)})
