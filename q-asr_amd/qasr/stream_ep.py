"""Streaming endpointing, decoder-driven: the rule that cuts a stream into utterances, its plan and the host statement of
k_stream_endpoint (csrc/qasr_stream_ep.hip, include/qasr.h).  NumPy only: no GPU, no native library.

No acoustic model and no energy threshold: the model's own FINAL frames say where speech is - blank against non-blank
arg-max, and the frame score - and the rules are integer rules over global frames (Kaldi's endpoint rules in spirit:
trailing silence after speech, a time-out with no speech, a maximum utterance length).  `endpoint_host` /
`endpoint_batch_host` are the CPU path of EncDecCTCModel.stream(endpoint=) and the yardstick the GPU tests compare the
kernel with, byte for byte, the state block included; `endpoints_whole_host` is the same statement over a whole stream
in one pass, which any slicing into steps has to reproduce."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .stream import BEGIN, END, StreamPlan, StreamState

STATE_WORDS = 80                        # one slot's endpoint block: 16 header words + 64 float32 partial sums
_W_DONE, _W_INDEX, _W_FIRST, _W_SP0, _W_SP1, _W_NSP, _W_LDONE, _W_PART = 0, 1, 2, 3, 4, 5, 6, 16
STATUS_OK, STATUS_GAP, STATUS_SLOT, STATUS_RANGE = 0, 1, 2, 3
SILENCE, TIMEOUT, MAX, HARD, UTT_END = 1, 2, 3, 4, 5
REASONS = {SILENCE: 'silence', TIMEOUT: 'timeout', MAX: 'max', HARD: 'hard', UTT_END: 'end'}
REC_WORDS = 10                          # one record: 10 32-bit words
R_INDEX, R_FIRST, R_END, R_SP_FIRST, R_SP_LAST, R_SP_FRAMES, R_REASON, R_SCORE, R_LABEL_END = range(9)
MAX_RULE_FRAMES = 1 << 24

EP_RULES = """State of a slot: 80 32-bit words.  Word 0: frames_done of THIS block (global frames the rule has walked); 1: utt_index
(utterances cut so far); 2: utt_first (the global frame where the open utterance began); 3: its first speech frame + 1
(0: none yet); 4: its last speech frame + 1 (0: none); 5: its speech frames; 6: labels_done (the stream's label count at
the start of the open utterance); 7-15: zero; 16-79: float32 part[(t - utt_first) % 64].  A zeroed block is a fresh stream.

The step runs AFTER the emit step (qasr.stream.STREAM_RULES) of the same rows and reads the stream block read-only:
hi = its frames_done, n_labels = its label count, both as emit left them; and emit's outputs of the step: status,
n_new_labels (n, clamped to 0 .. P) and the delta's start / nframes.  The stream's label count BEFORE the step is
n_before = n_labels - n.  It sees emit's tokens, frame_score, enc_lens (e = enc_len clamped to 0 .. Tw), first_frame,
slots and flags.

status 2: the slot is outside 0 .. S - 1.  1: emit's status of the row is not 0 (frames were lost).  3: with lo = this
       block's frames_done (0 on a BEGIN row): lo > hi, lo < first_frame, or lo < hi and hi > first_frame + e (the range
       would leave the window's encoded frames).  Checked in this order.  A row with a status leaves its state untouched
       (a BEGIN row too) and writes no record.
BEGIN  zeroes the block first.
walk   t = lo .. hi - 1 in increasing order, token and score of frame t taken at window index t - first_frame:
       speech(t) = token != blank and frame_score >= min_logp, compared in float32 (NaN is not speech; min_logp = -inf
       when unset).  part[(t - utt_first) % 64] += frame_score in float32.  Speech sets word 3 if it is 0, sets word 4,
       counts in word 5.  trailing = t + 1 - (word 4 if speech was seen, else utt_first); length = t + 1 - utt_first.
       The first true of these fires, in this order: SILENCE (1) speech seen and trailing >= Fsil; TIMEOUT (2) no speech
       and trailing >= Fstart; MAX (3) length >= Fmax and the token is blank; HARD (4) length >= Fhard.
fire   at t writes one record of 10 words: index = utt_index, first = utt_first, end = t + 1, speech_first (the first
       speech frame, -1: none), speech_last (the last speech frame, -1: none), speech_frames, reason, score, label_end, 0.
       score = part[0] + ... + part[63] in index order from 0.0f: utt_score_host's order over frame_score[first:end].
       label_end = n_before + the entries j < n of the delta with start[j] + nframes[j] <= t: a label belongs to the
       utterance that is open when its run is CLOSED BY A FINAL FRAME AT OR BEFORE THE CUT.  Where the cut frame is blank
       (MAX always; SILENCE and TIMEOUT whenever min_logp is unset and no score is NaN) that is every label that starts
       before `end`, and the utterance's labels are the greedy collapse of its own frames.  HARD may cut inside a run
       (and so may SILENCE / TIMEOUT on a non-blank frame that min_logp rejects): a run that spans the cut goes to the
       NEXT utterance, whole, with its first frame before that utterance's `first`.
       Then utt_index += 1, utt_first = t + 1, words 3-5 and part are cleared, labels_done = label_end.
END    row: after its last frame one more record, reason END (5), covering [utt_first, hi) with label_end = n_labels (the
       END emit has closed the last run), written even when it is empty; the block is then reset as after any fire.
Finally word 0 = hi.  A step writes at most E records (EndpointPlan.max_records: the plan proves that no step of a
session fires more); records past E are dropped and n_records stops at E, the state advances all the same.  Rows behind
n_records hold zeros.  Two fires lie at least min(Fsil, Fstart, Fmax) frames apart (Fhard >= Fmax)."""


@dataclass
class Endpointing:
    """The rule's times in seconds of the stream.  ALL FIVE DEFAULTS ARE UNTRIED ON SPEECH (no checkpoint or corpus ships
    here): silence_s of non-speech after speech ends an utterance, start_timeout_s without any speech ends an empty one,
    max_utt_s ends one at the next blank frame, hard_max_s ends one wherever it stands; min_logp: a non-blank frame counts
    as speech only if its score is at least this (None: every non-blank frame)."""
    silence_s: float = 0.8
    start_timeout_s: float = 5.0
    max_utt_s: float = 30.0
    hard_max_s: float = 40.0
    min_logp: Optional[float] = None


class EndpointPlan:
    """Fsil, Fstart, Fmax, Fhard in frames, min_logp as float32, and max_records E: the most records one step of a session
    writes, found by walking the protocol as StreamPlan._max_final does - a step that makes n frames final fires at most
    1 + (n - 1) // m times, m = min(Fsil, Fstart, Fmax) the least distance of two fires (EP_RULES), and an END step writes
    one more."""

    def __init__(self, plan: StreamPlan, Fsil, Fstart, Fmax, Fhard, min_logp=None):
        for name, v in (('Fsil', Fsil), ('Fstart', Fstart), ('Fmax', Fmax)):
            if int(v) < 1:
                raise ValueError(f'EndpointPlan: {name} {v} must be at least one frame')
        if int(Fhard) < int(Fmax):
            raise ValueError(f'EndpointPlan: Fhard {Fhard} must not be below Fmax {Fmax}')
        for name, v in (('Fsil', Fsil), ('Fstart', Fstart), ('Fmax', Fmax), ('Fhard', Fhard)):
            if int(v) > MAX_RULE_FRAMES:
                raise ValueError(f'EndpointPlan: {name} {v} is above 2^24 frames')
        lp = -math.inf if min_logp is None else float(min_logp)
        if math.isnan(lp):
            raise ValueError(f'EndpointPlan: min_logp {min_logp} is NaN')
        self.plan = plan
        self.Fsil, self.Fstart, self.Fmax, self.Fhard = int(Fsil), int(Fstart), int(Fmax), int(Fhard)
        self.min_logp = np.float32(lp)
        self.min_gap = min(self.Fsil, self.Fstart, self.Fmax)
        self.max_records = self._max_records()

    @classmethod
    def for_stream(cls, plan: StreamPlan, ep: Endpointing):
        """The times of an Endpointing rounded to frames as StreamPlan rounds chunk_s / left_s / right_s."""
        rate, spf = plan.sample_rate, plan.samples_per_frame
        frames = []
        for name in ('silence_s', 'start_timeout_s', 'max_utt_s', 'hard_max_s'):
            v = float(getattr(ep, name))
            if not np.isfinite(v):
                raise ValueError(f'EndpointPlan: {name} {getattr(ep, name)} is not finite')
            f = int(round(v * rate / spf))
            if name != 'hard_max_s' and f < 1:
                raise ValueError(f'EndpointPlan: {name} {getattr(ep, name)} rounds to {f} frames, it must be at least one frame')
            if f > MAX_RULE_FRAMES:
                raise ValueError(f'EndpointPlan: {name} {getattr(ep, name)} rounds to {f} frames, above 2^24')
            frames.append(f)
        if frames[3] < frames[2]:
            raise ValueError(f'EndpointPlan: hard_max_s {ep.hard_max_s} ({frames[3]} frames) is below max_utt_s {ep.max_utt_s} '
                             f'({frames[2]} frames)')
        if ep.min_logp is not None and math.isnan(float(ep.min_logp)):
            raise ValueError(f'EndpointPlan: min_logp {ep.min_logp} is NaN')
        return cls(plan, *frames, ep.min_logp)

    def step_records(self, n, end):
        """the most records a step of n final frames writes"""
        return (1 + (n - 1) // self.min_gap if n > 0 else 0) + (1 if end else 0)

    def _max_records(self):
        """StreamPlan._max_final's walk - a step at every multiple of C, END at every length in between - counting records"""
        p, most = self.plan, 0
        C, done, k = p.C, 0, 0
        bound = lambda n: n // min(self.Fsil, self.Fstart, self.Fmax, self.Fhard) + 2
        while k * C <= p.Wl + 2 * C:
            if k:
                start, ln, first = p.window_of(k * C)
                lo, hi = p.final_range(k * C, done, first, min(int(p.frames_of(ln)), p.Tw), False)
                assert self.step_records(hi - lo, False) <= bound(p.max_final_frames)
                most, done = max(most, self.step_records(hi - lo, False)), hi
            for d in range(C):
                start, ln, first = p.window_of(k * C + d)
                lo, hi = p.final_range(k * C + d, done, first, min(int(p.frames_of(ln)), p.Tw), True)
                assert self.step_records(hi - lo, True) <= bound(p.max_final_frames)
                most = max(most, self.step_records(hi - lo, True))
            k += 1
        return most


class EpState:
    """S slots as the device holds them: block int32 [S][80]."""

    def __init__(self, S):
        self.S = int(S)
        self.block = np.zeros((self.S, STATE_WORDS), dtype=np.int32)

    def part(self, slot):
        return self.block[slot, _W_PART:].view(np.float32)


def ep_state_bytes(S):
    """qasr_stream_ep_state_bytes(S)"""
    return int(S) * 4 * STATE_WORDS


@dataclass
class EpRow:
    """What one endpoint step gives for one row: records int32 [n][10] (not cut to E) and the status."""
    records: np.ndarray
    status: int


def _record(index, first, end, sp0, sp1, nsp, reason, score, label_end):
    r = np.zeros(REC_WORDS, dtype=np.int32)
    r[:7] = index, first, end, sp0 - 1, sp1 - 1, nsp, reason
    r[R_SCORE:R_SCORE + 1].view(np.float32)[0] = score
    r[R_LABEL_END] = label_end
    return r


def _sum_part(part):
    acc = np.float32(0.0)
    for l in range(64):
        acc = np.float32(acc + part[l])
    return acc


def _fires(eplan, speech_seen, trailing, length, is_blank):
    if speech_seen and trailing >= eplan.Fsil:
        return SILENCE
    if not speech_seen and trailing >= eplan.Fstart:
        return TIMEOUT
    if length >= eplan.Fmax and is_blank:
        return MAX
    if length >= eplan.Fhard:
        return HARD
    return 0


def endpoint_host(state: EpState, sstate: StreamState, slot, flags, tokens_row, frame_score_row, enc_len, first,
                  emit_start, emit_nframes, emit_n_new, emit_status, blank, eplan: EndpointPlan, session=False) -> EpRow:
    """One row of one step under EP_RULES, after emit_host of the same row: tokens_row / frame_score_row [Tw], enc_len and
    first as emit saw them, emit_start / emit_nframes the delta's arrays with emit_n_new entries (already clamped to P).
    Updates state.block[slot]; the records are NOT cut to max_records here (endpoint_batch_host does that, as the kernel
    does); session=True asserts the plan's bound."""
    none = np.zeros((0, REC_WORDS), dtype=np.int32)
    if not 0 <= slot < state.S or not 0 <= slot < sstate.S:
        return EpRow(none, STATUS_SLOT)
    if int(emit_status) != 0:
        return EpRow(none, STATUS_GAP)
    tok = np.asarray(tokens_row).astype(np.int32).reshape(-1)
    fs = np.ascontiguousarray(frame_score_row, dtype=np.float32).reshape(-1)
    Tw = len(tok)
    blk = state.block[slot]
    begin, end = bool(int(flags) & BEGIN), bool(int(flags) & END)
    hi, n_labels = sstate.frames_done(slot), sstate.n_labels(slot)
    lo, first = (0 if begin else int(blk[_W_DONE])), int(first)
    e = max(0, min(int(enc_len), Tw))
    if lo > hi or lo < first or (lo < hi and hi > first + e):
        return EpRow(none, STATUS_RANGE)
    if begin:
        blk[:] = 0
    n = max(0, int(emit_n_new))
    closes = (np.asarray(emit_start)[:n].astype(np.int64) + np.asarray(emit_nframes)[:n].astype(np.int64))
    n_before = n_labels - n
    index, utt_first, sp0, sp1, nsp = (int(blk[w]) for w in (_W_INDEX, _W_FIRST, _W_SP0, _W_SP1, _W_NSP))
    labels_done = int(blk[_W_LDONE])
    part = state.part(slot)
    out = []

    def cut(t_end, reason, label_end):
        nonlocal index, utt_first, sp0, sp1, nsp, labels_done
        out.append(_record(index, utt_first, t_end, sp0, sp1, nsp, reason, _sum_part(part), label_end))
        index, utt_first, sp0, sp1, nsp, labels_done = index + 1, t_end, 0, 0, 0, label_end
        part[:] = 0

    for t in range(lo, hi):
        k, x = int(tok[t - first]), fs[t - first]
        i = (t - utt_first) % 64
        part[i] = np.float32(part[i] + x)
        if k != blank and bool(x >= eplan.min_logp):
            sp0 = sp0 or t + 1
            sp1 = t + 1
            nsp += 1
        reason = _fires(eplan, sp1 != 0, t + 1 - (sp1 if sp1 else utt_first), t + 1 - utt_first, k == blank)
        if reason:
            cut(t + 1, reason, n_before + int(np.count_nonzero(closes <= t)))
    if end:
        cut(hi, UTT_END, n_labels)
    blk[_W_DONE], blk[_W_INDEX], blk[_W_FIRST], blk[_W_SP0], blk[_W_SP1], blk[_W_NSP] = hi, index, utt_first, sp0, sp1, nsp
    blk[_W_LDONE] = labels_done
    assert not session or len(out) <= eplan.step_records(hi - lo, end) <= eplan.max_records, (lo, hi, len(out), eplan.max_records)
    return EpRow(np.stack(out) if out else none, STATUS_OK)


@dataclass
class EpStepBatch:
    """k_stream_endpoint's outputs: records int32 [B][E][10] (score: float32 bits in word 7), n_records, status int32 [B]."""
    records: np.ndarray
    n_records: np.ndarray
    status: np.ndarray


def endpoint_batch_host(state: EpState, sstate: StreamState, slots, flags, tokens, frame_score, enc_lens, first_frame, emit,
                        blank, eplan: EndpointPlan, E=None) -> EpStepBatch:
    """The twin of one k_stream_endpoint launch, after emit_batch_host of the same rows gave `emit` (a qasr.stream.StepBatch)."""
    E = eplan.max_records if E is None else int(E)
    tok = np.asarray(tokens)
    B = tok.shape[0]
    o = EpStepBatch(np.zeros((B, E, REC_WORDS), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32))
    P = np.asarray(emit.start).shape[1]
    for b in range(B):
        n = max(0, min(int(emit.n_new_labels[b]), P))
        r = endpoint_host(state, sstate, int(slots[b]), int(flags[b]), tok[b], frame_score[b], int(enc_lens[b]), int(first_frame[b]),
                          emit.start[b], emit.nframes[b], n, int(emit.status[b]), blank, eplan)
        k = min(len(r.records), E)
        o.records[b, :k] = r.records[:k]
        o.n_records[b], o.status[b] = k, r.status
    return o


def record_score(rec):
    """the float32 score of one record (or of an array of records)"""
    return np.ascontiguousarray(np.asarray(rec)[..., R_SCORE]).view(np.float32)


def endpoints_whole_host(tokens, frame_score, blank, eplan: EndpointPlan) -> np.ndarray:
    """The whole-stream statement: one pass over ALL final frames of a stream (tokens int [T], frame_score float32 [T]),
    no steps, END behind the last frame -> records int32 [n][10].  label_end counts the labels of the greedy collapse
    whose run is closed by a frame at or before the cut; the END record takes all."""
    from .ctc import collapse_host
    tok = np.asarray(tokens).astype(np.int32).reshape(-1)
    fs = np.ascontiguousarray(frame_score, dtype=np.float32).reshape(-1)
    T = len(tok)
    if T:
        ref = collapse_host(tok[None], blank=blank)
        n_all = int(ref.n_labels[0])
        closes = ref.start[0, :n_all].astype(np.int64) + ref.nframes[0, :n_all]
    else:
        n_all, closes = 0, np.zeros(0, dtype=np.int64)
    index = utt_first = sp0 = sp1 = nsp = 0
    part = np.zeros(64, dtype=np.float32)
    out = []
    for t in range(T):
        i = (t - utt_first) % 64
        part[i] = np.float32(part[i] + fs[t])
        if tok[t] != blank and bool(fs[t] >= eplan.min_logp):
            sp0 = sp0 or t + 1
            sp1 = t + 1
            nsp += 1
        reason = _fires(eplan, sp1 != 0, t + 1 - (sp1 if sp1 else utt_first), t + 1 - utt_first, tok[t] == blank)
        if reason:
            out.append(_record(index, utt_first, t + 1, sp0, sp1, nsp, reason, _sum_part(part), int(np.count_nonzero(closes <= t))))
            index, utt_first, sp0, sp1, nsp = index + 1, t + 1, 0, 0, 0
            part[:] = 0
    out.append(_record(index, utt_first, T, sp0, sp1, nsp, UTT_END, _sum_part(part), n_all))
    return np.stack(out)


def split_labels(deltas, base, label_end):
    """A session's accumulated deltas - a list of (labels, start, nframes, score) arrays whose first label is the stream's
    label number `base` - cut at the stream's label number label_end: (the four arrays of the labels before it,
    concatenated; the list of what remains)."""
    cat = [np.concatenate([d[i] for d in deltas] + [np.zeros(0, dtype=dt)]).astype(dt)
           for i, dt in enumerate((np.int32, np.int32, np.int32, np.float32))]
    k = int(label_end) - int(base)
    assert 0 <= k <= len(cat[0]), (base, label_end, len(cat[0]))
    rest = tuple(c[k:] for c in cat)
    return tuple(c[:k] for c in cat), ([rest] if len(rest[0]) else [])
