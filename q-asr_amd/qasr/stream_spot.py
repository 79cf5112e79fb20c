"""Streaming keyword spotting: the rule that carries a keyword's lattice across the steps of a streaming session, its plan and
the host statement of k_stream_spot (csrc/qasr_stream_spot.hip, include/qasr.h).  NumPy only: no GPU, no native library.

A keyword's whole lattice under qasr.spot.SPOT_RULES is one Viterbi row of pairs (D int64, start int32) and one open hit, so
that is what a stream keeps between two steps.  `spot_step_host` / `spot_batch_host` are the CPU path of
EncDecCTCModel.stream(spot=) and the yardstick the GPU tests compare the kernel with, byte for byte, the state block included;
`spot_whole_host` is the same statement over a whole stream in one pass, which any slicing into steps has to reproduce.
quantize and NEG are qasr.beam's; the frame step, the candidate rule and the overlap rule are SPOT_RULES' and are restated here
for one keyword at a time only because the state has to be cut at any frame."""
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .beam import NEG, quantize
from .spot import MAX_LABELS, check_max_span
from .stream import BEGIN, END, StreamPlan, StreamState

HEADER_WORDS = 8
_W_DONE, _W_STEPPED, _W_OPEN, _W_HSTART, _W_HEND, _W_COUNT, _W_HD = 0, 1, 2, 3, 4, 5, 6
STATUS_OK, STATUS_GAP, STATUS_SLOT, STATUS_RANGE = 0, 1, 2, 3

STREAM_SPOT_RULES = """Keyword spotting (qasr.spot.SPOT_RULES) over the frames that a streaming session makes final, step by step.
Problems: K keywords are shared by all streams of a session (targets int32 [K, ML], target_lens int32 [K], ML <= 127); problem
p = row * K + k of a step; its state lives at (slot, k), slot = slots[row].
State of a (slot, keyword): a block of 8 + 3 SP 32-bit words, SP = 64 NS the state pitch, NS = 1 / 2 / 4 by 2 ML + 1 <= 64 / 128 /
256.  Word 0: frames_done of THIS block (global frames the lattice has walked); 1: stepped (0: fresh); 2: 1 if a hit is open;
3: its start; 4: its end (global frames, inclusive); 5: count, the hits emitted since BEGIN; 6-7: its score D as int64.  Behind
the header D int64 [SP] and then start int32 [SP]: the Viterbi row after frame frames_done - 1.  State 0 and the states above
F = 2L - 1 are stored dead (NEG, -1).  A block with stepped == 0 is a fresh stream whatever else it holds: zeroed memory is S
fresh streams; a fresh stream has every state dead, no open hit, count 0 and frames_done 0.  frames_done and stepped are per
keyword block, not per slot: no word is written by one wave and read by another.

The step runs AFTER the emit step (qasr.stream.STREAM_RULES) of the same rows and reads the stream block read-only:
hi = its frames_done as emit left it.  It sees the window's log-probabilities [B][Tw][C], the plane star [B][Tw] (qasr.align.
star_host(log_probs, enc_lens, 0.0) over the same window), enc_lens (e = enc_len clamped to 0 .. Tw), first_frame, slots, flags
and emit's status.
ok     ok[p] is SPOT_RULES' validity of keyword k (1 <= L <= ML, L <= 127, every label in [0, C) and not the blank).  A problem
       with ok = 0 writes no state and an empty step; its status is 2 or 1 where those hold, else 0.
status 2: the slot is outside 0 .. S - 1.  1: emit's status of the row is not 0 (frames were lost).  3: with lo = this block's
       frames_done (0 when fresh or on a BEGIN row): lo > hi, lo < first_frame, lo < hi and hi > first_frame + e (the range
       would leave the window's encoded frames), or hi - lo > max_final_frames (more than a step of the plan walks).  Checked
       in this order.  A problem with a status leaves its block untouched (a BEGIN row too) and writes an empty step.
BEGIN  makes the block fresh first.
walk   t = lo .. hi - 1 in increasing order, the row of frame t taken at window index t - first_frame.  The frame step is
       SPOT_RULES' on every point - states, predecessors, skip rule, tie order, emission min(q(logp) - q(star), 0), the fresh
       start (0, t) with t GLOBAL - and so are the candidate rule (a live F with n = t - start + 1 <= max_span and
       D >= threshold_q * n) and the overlap rule (a candidate with start <= open.end replaces the open hit iff D * n_open >
       D_open * n, else it is dropped; one that does not overlap closes the open hit and opens a new one).
close  Offline an open hit closes when a candidate that does not overlap arrives, or at the row's end; on a stream that may be
       never.  So after frame t, behind the candidate rule, the open hit closes and is emitted UNLESS some state 1 <= s <= F is
       live with start[s] <= open.end and (t + 1) - start[s] + 1 <= max_span.  Why that changes nothing: a candidate at a later
       frame t' > t carries a start that it inherited from a state that is live now, or a fresh start > t >= open.end.  A fresh
       start cannot overlap.  An inherited start[s] overlaps only if start[s] <= open.end, and its span at t' is at least
       (t + 1) - start[s] + 1, which has to be <= max_span for a candidate.  With no such state no later candidate overlaps the
       open hit: it can never be replaced, and the next candidate would close it unchanged.  The emitted list is therefore
       SPOT_RULES' list of the whole stream, on every byte, for any slicing.
END    row: after its last frame the open hit closes.
Every closed hit is emitted as (start, end, D, detect): detect is the global frame after which it closed, hi - 1 on END (-1 when
the stream has no frame).  A step stores the first PH of them, in order, in hit_start / hit_end / hit_detect int32 [P][PH] and
hit_score int64 [P][PH], tails 0; n_new_hits counts every hit closed in the step, n_hits_total is the block's count.
open_start / open_end (int32) and open_score (int64): the open hit after the step, -1 / -1 / 0 if none is open: the
provisional, immediate detection.  An empty step: no hits, n_new_hits = n_hits_total = 0, open -1 / -1 / 0.
Finally word 0 = hi, word 1 = 1.
PH     A frame closes at most two hits: one by a candidate that does not overlap, and the new one at once when its span equals
       max_span (no later candidate can then carry its start).  END closes one more.  So PH = 2 * max_final_frames + 1 holds
       every hit of a step (StreamSpotPlan.hit_pitch)."""


@dataclass
class StreamSpot:
    """The keywords of a streaming session (EncDecCTCModel.stream(spot=)): exactly one of keywords (strings) and labels (one
    sequence of label ids each), as EncDecCTCModel.spot takes them; threshold: the lowest mean a hit may have, -16 .. 0 nats per
    frame; max_span_s: the longest hit - and, on blank-dominated audio, how long a final hit can trail its end.  BOTH DEFAULTS
    ARE UNTRIED ON SPEECH; a wake-word caller sets max_span_s near the keyword's longest plausible duration."""
    keywords: Optional[Sequence] = None
    labels: Optional[Sequence] = None
    threshold: float = -1.0
    max_span_s: float = 10.0


def state_lanes(ML):
    """NS of k_spot / k_stream_spot for a row pitch of ML labels"""
    states = 2 * int(ML) + 1
    return 1 if states <= 64 else (2 if states <= 128 else 4)


class StreamSpotPlan:
    """The keywords as the kernel takes them (targets int32 [K, ML], target_lens int32 [K]), threshold_q and max_span in frames,
    the state pitch SP = 64 NS, the words of one block and the row pitch of the hit outputs, hit_pitch = 2 * max_final_frames +
    1 (STREAM_SPOT_RULES, PH): derived from the stream's plan, not guessed."""

    def __init__(self, plan: StreamPlan, targets, target_lens, threshold_q, max_span):
        tg, tl = np.asarray(targets), np.asarray(target_lens)
        if tg.ndim != 2 or tg.shape[0] < 1 or tl.shape != (tg.shape[0],):
            raise ValueError(f'StreamSpotPlan: targets must be [K, max_labels] with K >= 1 and one length each, got {tg.shape} / {tl.shape}')
        K, ML = tg.shape
        if not 1 <= ML <= MAX_LABELS:
            raise ValueError(f'StreamSpotPlan: max_labels (the row pitch of targets) must be 1 .. {MAX_LABELS}, got {ML}')
        thr = int(threshold_q)
        if not -16 * 65536 <= thr <= 0:
            raise ValueError(f'StreamSpotPlan: threshold_q must be {-16 * 65536} .. 0, got {threshold_q!r}')
        self.plan = plan
        self.targets, self.target_lens = np.ascontiguousarray(tg, dtype=np.int32), np.ascontiguousarray(tl, dtype=np.int32)
        self.K, self.ML = int(K), int(ML)
        self.threshold_q, self.max_span = thr, check_max_span(max_span, 'StreamSpotPlan')
        self.NS = state_lanes(ML)
        self.SP = 64 * self.NS
        self.block_words = HEADER_WORDS + 3 * self.SP
        self.max_final_frames = int(plan.max_final_frames)
        self.hit_pitch = 2 * self.max_final_frames + 1


def spot_state_bytes(S, K, ML):
    """qasr_stream_spot_state_bytes(S, K, max_labels)"""
    if int(S) < 1 or int(K) < 1 or not 1 <= int(ML) <= MAX_LABELS:
        return 0
    return int(S) * int(K) * 4 * (HEADER_WORDS + 3 * 64 * state_lanes(ML))


class SpotState:
    """S slots of K keyword blocks as the device holds them: block int32 [S][K][8 + 3 SP]."""

    def __init__(self, S, splan: StreamSpotPlan):
        self.S, self.splan = int(S), splan
        self.block = np.zeros((self.S, splan.K, splan.block_words), dtype=np.int32)

    def D(self, slot, k):
        sp = self.splan.SP
        return self.block[slot, k, HEADER_WORDS:HEADER_WORDS + 2 * sp].view(np.int64)

    def start(self, slot, k):
        return self.block[slot, k, HEADER_WORDS + 2 * self.splan.SP:]

    def h_d(self, slot, k):
        return self.block[slot, k, _W_HD:_W_HD + 2].view(np.int64)


def keyword_ok(y_row, L, ML, C, blank):
    """SPOT_RULES' validity of one keyword"""
    L = int(L)
    if L < 1 or L > ML or L > MAX_LABELS:
        return False
    y = np.asarray(y_row[:L])
    return bool(y.min() >= 0 and y.max() < C and not (y == blank).any())


def _lattice(y, SP, blank):
    """(lab int64 [SP], skip bool [SP], F) of one valid keyword; the states above F carry the blank and are never live"""
    L = len(y)
    lab = np.full(SP, blank, dtype=np.int64)
    skip = np.zeros(SP, dtype=bool)
    ya = np.asarray(y, dtype=np.int64)
    lab[1:2 * L:2] = ya
    if L > 1:
        skip[3:2 * L:2] = ya[1:] != ya[:-1]
    return lab, skip, 2 * L - 1


class _Walk:
    """One keyword's row and open hit, and the walk of STREAM_SPOT_RULES over frames: the state as Python / NumPy values"""

    def __init__(self, lab, skip, F, thr, max_span, D=None, B=None, hit=None, count=0):
        SP = len(lab)
        self.lab, self.skip, self.F, self.thr, self.max_span = lab, skip, int(F), int(thr), int(max_span)
        self.D = np.full(SP, NEG, np.int64) if D is None else np.array(D, dtype=np.int64)
        self.B = np.full(SP, -1, np.int32) if B is None else np.array(B, dtype=np.int32)
        self.hit, self.count = hit, int(count)               # hit: None or (start, end, D)
        self.closed = []                                     # (start, end, D, detect)
        self.early = []                                      # the detect frames of the hits that the early close closed

    def _close(self, t):
        self.closed.append(self.hit + (t,))
        self.hit, self.count = None, self.count + 1

    def frame(self, t, q_row, q_star):
        """global frame t with the quantised row q_row int [C] and q_star int"""
        D, B, F = self.D, self.B, self.F
        e = np.minimum(q_row[self.lab].astype(np.int64) - np.int64(q_star), 0)
        a1, s1 = np.concatenate([[NEG], D[:-1]]), np.concatenate([[-1], B[:-1]]).astype(np.int32)
        a1[1], s1[1] = 0, t                                  # the fresh start
        a2 = np.where(self.skip, np.concatenate([[NEG, NEG], D[:-2]]), NEG)
        s2 = np.concatenate([[-1, -1], B[:-2]]).astype(np.int32)
        best, bs = D, B
        m = a1 > best
        best, bs = np.where(m, a1, best), np.where(m, s1, bs)
        m = a2 > best
        best, bs = np.where(m, a2, best), np.where(m, s2, bs)
        live = best != NEG
        live[0] = False
        live[F + 1:] = False
        self.D = D = np.where(live, np.where(live, best, 0) + e, NEG)
        self.B = B = np.where(live, bs, -1).astype(np.int32)
        fd, fs = int(D[F]), int(B[F])
        if fd != NEG:
            n = t - fs + 1
            if n <= self.max_span and fd >= self.thr * n:   # a candidate
                if self.hit is not None and fs <= self.hit[1]:
                    if fd * (self.hit[1] - self.hit[0] + 1) > self.hit[2] * n:
                        self.hit = (fs, t, fd)
                else:
                    if self.hit is not None:
                        self._close(t)
                    self.hit = (fs, t, fd)
        if self.hit is not None:                             # the early close
            s = slice(1, F + 1)
            keep = (D[s] != NEG) & (B[s] <= self.hit[1]) & ((t + 2) - B[s].astype(np.int64) <= self.max_span)
            if not keep.any():
                self._close(t)
                self.early.append(t)

    def end(self, t_last):
        if self.hit is not None:
            self._close(t_last)


@dataclass
class SpotRow:
    """What one step gives for one problem: the closed hits int64 [n][4] (start, end, D, detect; not cut to PH), the open hit
    (start, end, D) or None, the block's count, ok and status."""
    hits: np.ndarray
    open: Optional[tuple]
    total: int
    ok: int
    status: int
    lo: int = 0
    hi: int = 0
    early: tuple = ()         # the detect frames of the hits that the early close closed (a diagnostic of the twin)


_NONE = np.zeros((0, 4), dtype=np.int64)


def spot_step_host(state: SpotState, sstate: StreamState, slot, k, flags, q_rows, q_star, enc_len, first, emit_status, C, blank,
                   session=False) -> SpotRow:
    """One problem of one step under STREAM_SPOT_RULES, after emit_host of the same row: q_rows int32 [Tw][C] and q_star int32
    [Tw] are quantize() of the window's log-probabilities and of its plane, enc_len and first as emit saw them.  Updates
    state.block[slot, k]; the hits are NOT cut to hit_pitch here (spot_batch_host does that, as the kernel does); session=True
    asserts the plan's bound."""
    sp = state.splan
    slot_ok = 0 <= slot < state.S and 0 <= slot < sstate.S
    status = STATUS_SLOT if not slot_ok else (STATUS_GAP if int(emit_status) != 0 else STATUS_OK)
    L = int(sp.target_lens[k])
    if not keyword_ok(sp.targets[k], L, sp.ML, C, blank):
        return SpotRow(_NONE, None, 0, 0, status)
    if status:
        return SpotRow(_NONE, None, 0, 1, status)
    Tw = len(q_star)
    blk = state.block[slot, k]
    begin, end = bool(int(flags) & BEGIN), bool(int(flags) & END)
    fresh = begin or int(blk[_W_STEPPED]) == 0
    hi = sstate.frames_done(slot)
    lo, first = (0 if fresh else int(blk[_W_DONE])), int(first)
    e = max(0, min(int(enc_len), Tw))
    if lo > hi or lo < first or (lo < hi and hi > first + e) or hi - lo > sp.max_final_frames:
        return SpotRow(_NONE, None, 0, 1, STATUS_RANGE, lo, hi)
    lab, skip, F = _lattice(sp.targets[k, :L], sp.SP, blank)
    if fresh:
        w = _Walk(lab, skip, F, sp.threshold_q, sp.max_span)
    else:
        hit = (int(blk[_W_HSTART]), int(blk[_W_HEND]), int(state.h_d(slot, k)[0])) if int(blk[_W_OPEN]) else None
        w = _Walk(lab, skip, F, sp.threshold_q, sp.max_span, state.D(slot, k), state.start(slot, k), hit, int(blk[_W_COUNT]))
    for t in range(lo, hi):
        w.frame(t, q_rows[t - first], int(q_star[t - first]))
    if end:
        w.end(hi - 1)
    blk[:HEADER_WORDS] = 0
    blk[_W_DONE], blk[_W_STEPPED], blk[_W_COUNT] = hi, 1, w.count
    if w.hit is not None:
        blk[_W_OPEN], blk[_W_HSTART], blk[_W_HEND] = 1, w.hit[0], w.hit[1]
        state.h_d(slot, k)[0] = w.hit[2]
    state.D(slot, k)[:] = w.D
    state.start(slot, k)[:] = w.B
    hits = np.array(w.closed, dtype=np.int64).reshape(-1, 4)
    assert not session or len(hits) <= 2 * (hi - lo) + (1 if end else 0) <= sp.hit_pitch, (lo, hi, len(hits), sp.hit_pitch)
    return SpotRow(hits, w.hit, w.count, 1, STATUS_OK, lo, hi, tuple(w.early))


@dataclass
class SpotStepBatch:
    """k_stream_spot's outputs, P = B * K problems, p = row * K + k: hit_start / hit_end / hit_detect int32 [P][PH], hit_score
    int64 [P][PH], n_new_hits / n_hits_total / open_start / open_end int32 [P], open_score int64 [P], ok / status int32 [P]."""
    hit_start: np.ndarray
    hit_end: np.ndarray
    hit_detect: np.ndarray
    hit_score: np.ndarray
    n_new_hits: np.ndarray
    n_hits_total: np.ndarray
    open_start: np.ndarray
    open_end: np.ndarray
    open_score: np.ndarray
    ok: np.ndarray
    status: np.ndarray


FIELDS = ('hit_start', 'hit_end', 'hit_detect', 'hit_score', 'n_new_hits', 'n_hits_total', 'open_start', 'open_end', 'open_score',
          'ok', 'status')
FIELD_DTYPES = dict(hit_score=np.int64, open_score=np.int64)


def spot_batch_host(state: SpotState, sstate: StreamState, slots, flags, log_probs, star, enc_lens, first_frame, emit_status, blank,
                    PH=None, rows_out=None) -> SpotStepBatch:
    """The twin of one k_stream_spot launch, after emit_batch_host of the same rows: log_probs float32 [B][Tw][C], star float32
    [B][Tw] (star_host(log_probs, enc_lens, 0.0)), enc_lens / first_frame / slots / flags / emit_status int [B].  rows_out: a
    list that receives every problem's SpotRow."""
    sp = state.splan
    PH = sp.hit_pitch if PH is None else int(PH)
    lp = np.asarray(log_probs, dtype=np.float32)
    st = np.asarray(star, dtype=np.float32)
    B, Tw, C = lp.shape
    assert st.shape == (B, Tw), (st.shape, lp.shape)
    P, K = B * sp.K, sp.K
    z = lambda *s: np.zeros(s, dtype=np.int32)
    o = SpotStepBatch(z(P, PH), z(P, PH), z(P, PH), np.zeros((P, PH), np.int64), z(P), z(P), np.full(P, -1, np.int32),
                      np.full(P, -1, np.int32), np.zeros(P, np.int64), z(P), z(P))
    for b in range(B):
        q_rows, q_star = None, None
        for k in range(K):
            p = b * K + k
            if q_rows is None:
                q_rows, q_star = quantize(lp[b]), quantize(st[b])
            r = spot_step_host(state, sstate, int(slots[b]), k, int(flags[b]), q_rows, q_star, int(enc_lens[b]), int(first_frame[b]),
                               int(emit_status[b]), C, int(blank))
            if rows_out is not None:
                rows_out.append(r)
            n = min(len(r.hits), PH)
            o.hit_start[p, :n], o.hit_end[p, :n], o.hit_score[p, :n], o.hit_detect[p, :n] = r.hits[:n].T
            o.n_new_hits[p], o.n_hits_total[p], o.ok[p], o.status[p] = len(r.hits), r.total, r.ok, r.status
            if r.open is not None:
                o.open_start[p], o.open_end[p], o.open_score[p] = r.open
    return o


def spot_whole_host(log_probs, star, y, blank, threshold_q, max_span) -> np.ndarray:
    """The whole-stream statement: one pass over ALL final frames of a stream (log_probs float32 [T][C], star float32 [T]) for
    one valid keyword y, no steps, END behind the last frame -> the emitted hits int64 [n][4] (start, end, D, detect).  Its
    first three columns are spot_host's hits of that row (STREAM_SPOT_RULES, close)."""
    lp = np.asarray(log_probs, dtype=np.float32)
    T = lp.shape[0]
    y = [int(c) for c in y]
    lab, skip, F = _lattice(y, 64 * state_lanes(len(y)), blank)
    w = _Walk(lab, skip, F, threshold_q, check_max_span(max_span, 'spot_whole_host'))
    q_rows, q_star = quantize(lp), quantize(np.asarray(star, dtype=np.float32))
    for t in range(T):
        w.frame(t, q_rows[t], int(q_star[t]))
    w.end(T - 1)
    return np.array(w.closed, dtype=np.int64).reshape(-1, 4)


def to_stream_hits(batch: SpotStepBatch, slots, keywords, seconds_per_frame):
    """The stored hits of one step as qasr.ctc.StreamHit(slot, KeywordHit in seconds of the stream, detected_s: the end of the
    frame after which the hit closed), and the open hits per slot as KeywordHits"""
    from .ctc import KeywordHit, StreamHit
    from .spot import ONE
    spf, K = float(seconds_per_frame), len(keywords)
    hs, he, hd, sc, nn = (np.asarray(getattr(batch, n)) for n in ('hit_start', 'hit_end', 'hit_detect', 'hit_score', 'n_new_hits'))
    os_, oe, od = np.asarray(batch.open_start), np.asarray(batch.open_end), np.asarray(batch.open_score)
    final, pending = [], {}
    for b, slot in enumerate(slots):
        pending[slot] = []
        for k in range(K):
            p = b * K + k
            for i in range(min(int(nn[p]), hs.shape[1])):
                a, e = int(hs[p, i]), int(he[p, i])
                n = e - a + 1
                final.append(StreamHit(slot, KeywordHit(keywords[k], k, a * spf, (e + 1) * spf, float(sc[p, i]) / ONE / n, n),
                                       (int(hd[p, i]) + 1) * spf))
            if int(os_[p]) >= 0:
                a, e = int(os_[p]), int(oe[p])
                n = e - a + 1
                pending[slot].append(KeywordHit(keywords[k], k, a * spf, (e + 1) * spf, float(od[p]) / ONE / n, n))
    return final, pending


def sort_hits(hits):
    """the order of StreamSession.take_hits: (detected_s, slot, start_s, index)"""
    return sorted(hits, key=lambda h: (h.detected_s, h.slot, h.hit.start_s, h.hit.index))
