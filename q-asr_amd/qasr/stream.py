"""Streaming recognition, buffered: the plan, the rule for which frames are final and the host statement of k_stream_push /
k_stream_window / k_stream_emit (csrc/qasr_stream.hip, include/qasr.h).  NumPy only: no GPU, no native library.

The models are not causal and normalise per utterance, so a step re-runs a window [left context | new chunk | look-ahead]
of the stream's most recent samples through the whole model (NeMo's buffered streaming, the FrameBatchASR idea) and only the
chunk's frames become final, one look-ahead late.  `push_host`, `window_host` and `emit_host` are the CPU path of
EncDecCTCModel.stream and the yardstick the GPU tests compare the kernels with, byte for byte, the state block included.
Normalisation and every other per-utterance statistic of the model is per WINDOW."""
from dataclasses import dataclass
from typing import List

import numpy as np

from .ctc import _order_key

BEGIN, END = 1, 2                       # row flags: push forgets the slot first / emit closes the stream
STATE_WORDS = 80                        # one slot's state block: 16 header words + 64 float32 partial sums
_W_RECV, _W_DONE, _W_OPEN, _W_FIRST, _W_MAX, _W_NLAB, _W_PART = 0, 2, 3, 4, 5, 6, 16
STATUS_OK, STATUS_GAP, STATUS_SLOT = 0, 1, 2

STREAM_RULES = """State of a slot: 80 32-bit words.  Words 0-1: received (int64, samples pushed since BEGIN); 2: frames_done (global
frames already final); 3: the open run's token + 1 (0: no run is open); 4: its first global frame; 5: its running maximum
frame score as ctc._order_key; 6: n_labels committed so far; 7-15: zero; 16-79: float32 part[0..63].  A zeroed block is a
fresh stream.  Behind the S blocks lie S rings of cap = (Wl + C rounded up to a multiple of 4) float32; sample i of a
stream lives at ring[i % cap].

push   n = n_new clamped to 0 .. min(pitch, C); a BEGIN row zeroes its block first; samples received .. received + n - 1 are
       written (int16 as float32(x) / 32768), then received += n.  A slot outside 0 .. S - 1 is skipped.
window r = received; start = max(0, spf * ceil((r - Wl) / spf)); len = r - start; the row is samples [start, r) and zeros
       up to Wl; first = start / spf: local frame j of the window is global frame first + j.
emit   lo = frames_done, e = enc_len clamped to 0 .. Tw, top = first + e;
       hi = max(lo, top) on an END row, else max(lo, min(top, floor((r - Rr) / spf))).  Frames [lo, hi) become final.
       lo < first (frames were lost: more than L + C samples between two steps): status 1, the state is not touched and
       the row's outputs are those of an empty step.  A slot outside 0 .. S - 1: status 2, likewise.
       Walking t = lo .. hi - 1: a frame whose token equals the open run's extends it (maximum in _order_key order);
       any other frame closes the open run - it is appended to the step's delta as (label, first frame, frames, best
       score) - and opens a new one unless it is blank.  The run that reaches hi - 1 stays open: whether it has ended
       is decided by a later FINAL frame.  part[t % 64] += frame_score[t] in float32, t global, in increasing t.
       END closes the open run, utt_score = part[0] + ... + part[63] summed in index order from 0.0f (utt_score_host's
       order; 0 on other rows).  total_frames = hi on every row.  A delta has at most P entries (StreamPlan.emit_pitch:
       the plan proves that no step of a session emits more); entries past P are dropped and n_new_labels stops at P, the
       state's n_labels counts them all.
tail   labels only, state untouched: the open run's token first (if one is open after the step), then every token of
       the frames [hi, top) that differs from its predecessor (the open run's token for frame hi) and is not blank; at
       most Ptail = Rr / spf + 2, the rest is dropped.  Rows behind a count hold blank (labels) and zeros."""


class StreamPlan:
    """chunk_s / left_s / right_s rounded to multiples of samples_per_frame (spf): C, L, Rr samples; Wl = L + C + Rr.

    A session steps a stream whenever it has received another C samples, and once more (END) when it closes.
    frames_of: samples -> the encoded frames of a window that long (default n // spf + 1; a model passes its own, as
    _long_plan does).  Tw = frames_of(Wl) is the row pitch of the windows' outputs.
    max_final_frames: the most frames one such step makes final, found by walking the rule over every stream length up
    to the point where it repeats (Wl + 2 C samples) - not guessed; emit_pitch P = max_final_frames + 1: every final
    frame can close one run, and the END step also closes the last.  tail_pitch = Rr / spf + 2."""

    def __init__(self, chunk_s=0.96, left_s=4.0, right_s=0.96, sample_rate=16000, samples_per_frame=320, frames_of=None):
        spf, rate = int(samples_per_frame), int(sample_rate)
        if spf < 1 or rate < 1:
            raise ValueError(f'StreamPlan: sample_rate {sample_rate} and samples_per_frame {samples_per_frame} must be positive')
        for name, v in (('chunk_s', chunk_s), ('left_s', left_s), ('right_s', right_s)):
            if not np.isfinite(float(v)):
                raise ValueError(f'StreamPlan: {name} {v} is not finite')
        to_frames = lambda s: int(round(float(s) * rate / spf))
        cf, lf, rf = to_frames(chunk_s), to_frames(left_s), to_frames(right_s)
        if cf < 1:
            raise ValueError(f'StreamPlan: chunk_s {chunk_s} rounds to {cf} frames, it must be at least one frame ({spf} samples)')
        if lf < 0:
            raise ValueError(f'StreamPlan: left_s {left_s} must not be negative')
        if rf < 0:
            raise ValueError(f'StreamPlan: right_s {right_s} must not be negative')
        self.sample_rate, self.samples_per_frame = rate, spf
        self.chunk_frames, self.left_frames, self.right_frames = cf, lf, rf
        self.C, self.L, self.Rr = cf * spf, lf * spf, rf * spf
        self.Wl = self.L + self.C + self.Rr
        if self.Wl + self.C >= 2 ** 31 - 4:
            raise ValueError('StreamPlan: the window is too long for int32 sample offsets')
        self.cap = (self.Wl + self.C + 3) // 4 * 4
        self.frames_of = frames_of if frames_of is not None else (lambda n: n // spf + 1)
        self.Tw = int(self.frames_of(self.Wl))
        self.tail_pitch = rf + 2
        self.max_final_frames = self._max_final()
        self.emit_pitch = self.max_final_frames + 1

    def seconds_per_frame(self):
        return self.samples_per_frame / float(self.sample_rate)

    def window_of(self, r):
        """(start, len, first) of the window of a stream that has received r samples"""
        spf = self.samples_per_frame
        start = max(0, spf * -(-(r - self.Wl) // spf))
        return start, r - start, start // spf

    def final_range(self, r, frames_done, first, enc_len, end):
        """(lo, hi) of STREAM_RULES; enc_len already clamped"""
        lo, top = int(frames_done), int(first) + int(enc_len)
        if end:
            return lo, max(lo, top)
        return lo, max(lo, min(top, (r - self.Rr) // self.samples_per_frame))

    def _max_final(self):
        """Walks a session's steps - one at every multiple of C, then END at every length in between - with the encoded
        length frames_of gives.  Beyond r = Wl + C the window slides by whole chunks and the counts repeat."""
        C, most = self.C, 0
        done, k = 0, 0                                  # frames_done after the step at r = k C
        while k * C <= self.Wl + 2 * C:
            if k:
                start, ln, first = self.window_of(k * C)
                lo, hi = self.final_range(k * C, done, first, min(int(self.frames_of(ln)), self.Tw), False)
                most, done = max(most, hi - lo), hi
            for d in range(C):                          # END at r = k C + d
                start, ln, first = self.window_of(k * C + d)
                lo, hi = self.final_range(k * C + d, done, first, min(int(self.frames_of(ln)), self.Tw), True)
                most = max(most, hi - lo)
            k += 1
        return most


class StreamState:
    """S slots as the device holds them: block int32 [S][80] and ring float32 [S][cap]."""

    def __init__(self, S, plan: StreamPlan):
        self.S, self.plan = int(S), plan
        self.block = np.zeros((self.S, STATE_WORDS), dtype=np.int32)
        self.ring = np.zeros((self.S, plan.cap), dtype=np.float32)

    def received(self, slot):
        return int(self.block[slot, _W_RECV:_W_RECV + 2].view(np.int64)[0])

    def frames_done(self, slot):
        return int(self.block[slot, _W_DONE])

    def n_labels(self, slot):
        return int(self.block[slot, _W_NLAB])

    def part(self, slot):
        return self.block[slot, _W_PART:].view(np.float32)


def state_bytes(S, plan: StreamPlan):
    """qasr_stream_state_bytes(S, Wl, C)"""
    return int(S) * (4 * STATE_WORDS + 4 * plan.cap)


def _to_f32(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) / np.float32(32768.0)
    if x.dtype != np.float32:
        raise ValueError(f'stream: int16 or float32 samples, got {x.dtype}')
    return x


def push_host(state: StreamState, slots, flags, n_new, chunk):
    """chunk float32 or int16 [B][pitch]; slots / flags / n_new int [B].  See STREAM_RULES."""
    plan = state.plan
    x = np.asarray(chunk)
    if x.ndim != 2:
        raise ValueError(f'push: chunk must be [B][pitch], got {x.shape}')
    x = _to_f32(x)
    for b, slot in enumerate(np.asarray(slots).reshape(-1).tolist()):
        if not 0 <= slot < state.S:
            continue
        n = max(0, min(int(n_new[b]), x.shape[1], plan.C))
        if int(flags[b]) & BEGIN:
            state.block[slot] = 0
        r = max(state.received(slot), 0)
        pos = (r + np.arange(n, dtype=np.int64)) % plan.cap
        state.ring[slot, pos] = x[b, :n]
        state.block[slot, _W_RECV:_W_RECV + 2].view(np.int64)[0] = r + n


def window_host(state: StreamState, slots):
    """-> (windows float32 [B][Wl], zeros behind each length; window_lens int32 [B]; first_frame int32 [B])"""
    plan = state.plan
    sl = np.asarray(slots).reshape(-1).tolist()
    win = np.zeros((len(sl), plan.Wl), dtype=np.float32)
    wl = np.zeros(len(sl), dtype=np.int32)
    first = np.zeros(len(sl), dtype=np.int32)
    for b, slot in enumerate(sl):
        if not 0 <= slot < state.S:
            continue
        r = max(state.received(slot), 0)
        start, ln, f = plan.window_of(r)
        win[b, :ln] = state.ring[slot, (start + np.arange(ln, dtype=np.int64)) % plan.cap]
        wl[b], first[b] = ln, f
    return win, wl, first


@dataclass
class StepRow:
    """What one emit step gives for one row: the delta (arrays of n_new entries), the provisional tail and the scalars."""
    labels: np.ndarray
    start: np.ndarray
    nframes: np.ndarray
    score: np.ndarray
    n_new: int
    status: int
    total_frames: int
    utt_score: np.float32
    tail: np.ndarray
    lo: int = 0
    hi: int = 0


def _unkey(k):
    k = np.int32(k)
    return (k ^ ((k >> 31) & np.int32(0x7fffffff))).view(np.float32)


def emit_host(tokens_row, frame_score_row, enc_len, first, state: StreamState, slot, end, blank, session=False) -> StepRow:
    """One row of one step under STREAM_RULES: tokens_row int [Tw], frame_score_row float32 [Tw], enc_len and first as
    the window's forward and window_host gave them.  Updates state.block[slot]; the delta is NOT cut to emit_pitch here
    (emit_batch_host does that, as the kernel does); session=True asserts the plan's bound, which holds for the steps a
    session makes."""
    plan = state.plan
    tok = np.asarray(tokens_row).astype(np.int32).reshape(-1)
    fs = np.ascontiguousarray(frame_score_row, dtype=np.float32).reshape(-1)
    Tw = len(tok)
    empty = lambda dt: np.zeros(0, dtype=dt)
    if not 0 <= slot < state.S:
        return StepRow(empty(np.int32), empty(np.int32), empty(np.int32), empty(np.float32), 0, STATUS_SLOT, 0, np.float32(0), empty(np.int32))
    blk = state.block[slot]
    r = max(state.received(slot), 0)
    first = int(first)
    e = max(0, min(int(enc_len), Tw))
    lo, hi = plan.final_range(r, blk[_W_DONE], first, e, bool(end))
    if lo < first or first < 0:
        return StepRow(empty(np.int32), empty(np.int32), empty(np.int32), empty(np.float32), 0, STATUS_GAP, 0, np.float32(0), empty(np.int32), lo, lo)
    assert not session or hi - lo <= plan.max_final_frames, (lo, hi, plan.max_final_frames)
    top = first + e
    open_tok = int(blk[_W_OPEN]) - 1                    # -1: none
    open_first, open_max = int(blk[_W_FIRST]), int(blk[_W_MAX])
    part = state.part(slot)
    keys = _order_key(fs)
    out = []
    for t in range(lo, hi):
        k, key = int(tok[t - first]), int(keys[t - first])
        if open_tok >= 0 and k == open_tok:
            open_max = max(open_max, key)
        else:
            if open_tok >= 0:
                out.append((open_tok, open_first, t - open_first, open_max))
            open_tok, open_first, open_max = (k, t, key) if k != blank else (-1, 0, 0)
        part[t % 64] = np.float32(part[t % 64] + fs[t - first])
    utt = np.float32(0.0)
    if end:
        if open_tok >= 0:
            out.append((open_tok, open_first, hi - open_first, open_max))
        open_tok, open_first, open_max = -1, 0, 0
        for l in range(64):
            utt = np.float32(utt + part[l])
    blk[_W_DONE], blk[_W_OPEN], blk[_W_FIRST], blk[_W_MAX] = hi, open_tok + 1, open_first, open_max
    blk[_W_NLAB] += len(out)
    tail = [open_tok] if open_tok >= 0 else []
    prev = open_tok if open_tok >= 0 else blank
    for t in range(hi, top):
        k = int(tok[t - first])
        if k != blank and k != prev:
            tail.append(k)
        prev = k
    return StepRow(np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.int32),
                   np.array([o[2] for o in out], dtype=np.int32),
                   np.array([_unkey(o[3]) for o in out], dtype=np.float32), len(out), STATUS_OK, hi, utt,
                   np.array(tail[:plan.tail_pitch], dtype=np.int32), lo, hi)


@dataclass
class StepBatch:
    """k_stream_emit's outputs, pitch P (labels / start / nframes / score) and Ptail (tail_labels)."""
    labels: np.ndarray
    start: np.ndarray
    nframes: np.ndarray
    score: np.ndarray
    n_new_labels: np.ndarray
    status: np.ndarray
    total_frames: np.ndarray
    utt_score: np.ndarray
    tail_labels: np.ndarray
    tail_n: np.ndarray


def emit_batch_host(state: StreamState, slots, flags, tokens, frame_score, enc_lens, first_frame, blank, P=None) -> StepBatch:
    """The twin of one k_stream_emit launch: tokens int32 [B][Tw], frame_score float32 [B][Tw], enc_lens / first_frame /
    slots / flags (END) int [B]."""
    plan = state.plan
    P = plan.emit_pitch if P is None else int(P)
    tok = np.asarray(tokens)
    B, Pt = tok.shape[0], plan.tail_pitch
    o = StepBatch(np.full((B, P), blank, np.int32), np.zeros((B, P), np.int32), np.zeros((B, P), np.int32),
                  np.zeros((B, P), np.float32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32),
                  np.zeros(B, np.float32), np.full((B, Pt), blank, np.int32), np.zeros(B, np.int32))
    for b in range(B):
        s = emit_host(tok[b], frame_score[b], int(enc_lens[b]), int(first_frame[b]), state, int(slots[b]), int(flags[b]) & END, blank)
        n = min(s.n_new, P)
        o.labels[b, :n], o.start[b, :n], o.nframes[b, :n], o.score[b, :n] = s.labels[:n], s.start[:n], s.nframes[:n], s.score[:n]
        o.n_new_labels[b], o.status[b], o.total_frames[b], o.utt_score[b] = n, s.status, s.total_frames, s.utt_score
        o.tail_labels[b, :len(s.tail)] = s.tail
        o.tail_n[b] = len(s.tail)
    return o


def split_pushes(pending: int, n: int, C: int) -> List[int]:
    """How a session cuts n arriving samples for a stream that holds `pending` samples of an unfinished chunk: pieces that
    each end at a multiple of C (a step follows each of those) and a rest shorter than C."""
    out = []
    while n > 0:
        k = min(n, C - pending)
        out.append(k)
        n -= k
        pending = (pending + k) % C
    return out
