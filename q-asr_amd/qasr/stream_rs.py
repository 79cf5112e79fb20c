"""Streaming at any sample rate: the plan, the rule for which resampled samples are final and the host statement of
k_stream_rs_append / k_stream_rs_fir (csrc/qasr_stream_rs.hip, include/qasr.h).  NumPy only: no GPU, no native library.

The resampler of qasr.resample (RULES) runs in front of the sample ring of qasr.stream: PCM at the source's rate is appended
to a per-slot history of channel sums, and the outputs that can no longer change are written into the slot's ring, where
window / emit find them as if they had been pushed at the model's rate.  `push_rs_host` is the CPU path of
EncDecCTCModel.stream(input_rate=) and the yardstick the GPU tests compare the kernels with, byte for byte, both states
included.  What is pinned: however the pushes are sliced, the samples that reach the ring are resample_host of the whole
stream on every byte."""
import numpy as np

from . import resample as rs
from .stream import BEGIN, StreamPlan, StreamState, _W_RECV

FLUSH = 4                               # row flag: the frames behind the last one count as zeros, as at an utterance's end
RS_STATE_WORDS = 16                     # one slot's resampler block: in_received (int64), format + 1, zeros
_R_IN, _R_FMT = 0, 2
PCM_S16, PCM_F32 = 0, 1
STATUS_OK, STATUS_FULL, STATUS_SLOT, STATUS_FORMAT = 0, 1, 2, 3      # (4: the device table's header disagrees with the launch)
MAX_HCAP = 1 << 26

RS_STREAM_RULES = """Resampler state of a slot: 16 32-bit words.  Words 0-1: in_received (int64, input frames appended since BEGIN); 2: the
slot's sample format + 1 (1: int16, 2: float32; 0: none yet), set by the row that first touches the slot; 3-15: zero.  Behind
the S blocks lie S histories of hcap 8-byte entries; input frame k lives at hist[k % hcap] as the channel sum RULES defines:
an int64 for int16 input (the integer sum), a float64 for float32 input (the channels added in ascending order).  A zeroed
buffer is S fresh streams.  The stream state (block of 80 words, sample ring of cap floats) is STREAM_RULES', unchanged;
`received` counts the samples at the model's rate that have been written to the ring.

W is the resample plan's, and 0 for equal rates (the `equal` rule of RULES: no filter, output i is the channel mean of frame i).
final   output i reads frames q - W + 1 .. q + W, q = floor(i M / L); with n frames received it is final when q + W <= n - 1,
        i.e. floor(i M / L) < n - W, i.e. i < (n - W) L / M: ready(n) = max(0, ceil((n - W) L / M)).  At the end of the stream
        the missing frames are zeros and out_len(n) = ceil(n L / M) outputs exist.
row     a slot outside 0 .. S - 1: nothing is touched, n_taken = n_out = 0, status 2.  Else append, then produce:
append  a BEGIN row zeroes the slot's stream block and resampler block first.  want = n_in clamped to 0 .. min(pitch, Ain),
        Ain = max(1, floor(C M / L)) - and 0 with status 3 if the slot holds the other sample format.  The frames an output
        at or behind `received` still reads start at keep = max(0, floor(received M / L) - W + 1) (W = 0: keep = received,
        the frame output `received` is the mean of); frame k would overwrite frame k - hcap, so n = min(want, max(0, keep + hcap - in_received)); status 1 if n < want.  Frames in_received ..
        in_received + n - 1 are stored as channel sums, then in_received += n; n_taken = n.
produce target = out_len(in_received) on a FLUSH row, else ready(in_received); k = max(0, min(target - received, out_limit, C)).
        Outputs i = received .. received + k - 1 are RULES' with the utterance's length taken as in_received (frames below 0
        or at and behind it are zero), written to ring[i % cap]; received += k; n_out = k."""


class StreamResamplePlan:
    """The stream plan, the resample plan and the channel count of one session, and what follows from them: W (0 for equal
    rates), ready(n), out_len(n), Ain (the most input frames one append takes) and hcap (entries of a slot's history).

    hcap.  A session (EncDecCTCModel.stream) appends at most Ain frames per round and then produces and steps until no ready
    output is left, so before every append received = ready(n), n = in_received.  For n > W that is ceil((n - W) L / M), so
    received M / L >= n - W and keep = floor(received M / L) - W + 1 >= n - 2 W + 1; for n <= W, keep = 0 >= n - 2 W + 1 as
    well.  The append stores frames up to n + Ain - 1 and must leave frame keep alone: n + Ain - 1 - hcap < keep holds for
    every n when hcap >= 2 W + Ain - 1 (W = 0: keep = n and hcap >= Ain).  hcap = 2 W + Ain rounded up to a multiple of 4; _walk() plays the protocol over the
    lengths at which the counters' phases repeat and asserts that no append was cut - the bound is checked, not guessed."""

    def __init__(self, stream_plan: StreamPlan, resample_plan, channels=1):
        ch = int(channels)
        if not 1 <= ch <= rs.MAX_CHANNELS:
            raise ValueError(f'stream: channels must be 1 .. {rs.MAX_CHANNELS}, got {channels}')
        if resample_plan.sr_out != stream_plan.sample_rate:
            raise ValueError(f'stream: the resample plan ends at {resample_plan.sr_out} Hz, the stream plan runs at {stream_plan.sample_rate} Hz')
        self.stream_plan, self.resample_plan, self.channels = stream_plan, resample_plan, ch
        self.L, self.M = resample_plan.L, resample_plan.M
        self.W = 0 if resample_plan.equal else resample_plan.W
        self.C, self.cap = stream_plan.C, stream_plan.cap
        self.Ain = max(1, self.C * self.M // self.L)
        self.hcap = (2 * self.W + self.Ain + 3) // 4 * 4
        if self.hcap > MAX_HCAP:
            raise ValueError(f'stream: a history of {self.hcap} frames per stream is beyond {MAX_HCAP}')
        assert self._walk() == 0, 'the session protocol would drop frames: hcap is too small'

    def ready(self, n):
        n = int(n)
        return -((-(n - self.W) * self.L) // self.M) if n > self.W else 0

    def out_len(self, n):
        n = int(n)
        return -((-n * self.L) // self.M) if n > 0 else 0

    def keep(self, received):
        return max(0, int(received) * self.M // self.L - self.W + 1) if self.W else int(received)

    def room(self, received, in_received):
        """how many frames an append may still take"""
        return max(0, self.keep(received) + self.hcap - int(in_received))

    def latency_s(self):
        """what the filter adds to the stream's latency: W input frames"""
        return self.W / float(self.resample_plan.sr_in)

    def _walk(self):
        """Before every append of a session the counters are (received, in_received) = (ready(n), n).  n - keep(ready(n)) has
        the period M in n (ready(n + M) = ready(n) + L and keep(r + L) = keep(r) + M), so every n up to 2 W + 2 M covers all
        states; then the protocol itself is played with whole pieces until the history has wrapped twice.  Returns how many
        frames the append clamp would have dropped."""
        L, M, W = self.L, self.M, self.W
        n = np.arange(0, 2 * W + 2 * M + 2, dtype=np.int64)
        r = np.where(n > W, -((-(n - W) * L) // M), 0)
        room = (np.maximum(0, r * M // L - W + 1) if W else r) + self.hcap - n
        dropped = int(np.maximum(0, self.Ain - room).sum())
        for piece in sorted({self.Ain, max(1, self.Ain - 1), self.Ain // 2 + 1}):
            n = r = 0
            while n < 2 * self.hcap + 2 * piece:
                dropped += max(0, piece - self.room(r, n))
                n += piece
                r = self.ready(n)
        return dropped


class ResampleState:
    """S slots of the resampler state as the device holds them: block int32 [S][16], hist int64 [S][hcap] (float32 slots hold
    the bits of float64 sums)."""

    def __init__(self, S, plan: StreamResamplePlan):
        self.S, self.plan = int(S), plan
        self.block = np.zeros((self.S, RS_STATE_WORDS), dtype=np.int32)
        self.hist = np.zeros((self.S, plan.hcap), dtype=np.int64)

    def in_received(self, slot):
        return int(self.block[slot, _R_IN:_R_IN + 2].view(np.int64)[0])

    def fmt(self, slot):
        return int(self.block[slot, _R_FMT]) - 1


def rs_state_bytes(S, plan: StreamResamplePlan):
    """qasr_stream_rs_state_bytes(S, hcap)"""
    return int(S) * (4 * RS_STATE_WORDS + 8 * plan.hcap)


def _outputs(hist_row, fmt, n, plan: StreamResamplePlan, i0, i1):
    """outputs i0 .. i1 - 1 of a slot whose history holds the frames they read, the utterance's length taken as n"""
    rp, ch, hcap = plan.resample_plan, plan.channels, plan.hcap
    if i1 <= i0:
        return np.zeros(0, dtype=np.float32)
    if plan.W == 0:                                             # equal rates: the channel mean of frame i
        i = np.arange(i0, i1, dtype=np.int64)
        inside = i < n
        e = hist_row[i % hcap]
        if fmt == PCM_S16:
            y = e.astype(np.float32) * np.float32(2.0 ** -15)
            y = y / np.float32(ch) if ch > 1 else y
        else:
            s = e.view(np.float64)
            y = (s / np.float64(ch)).astype(np.float32) if ch > 1 else s.astype(np.float32)
        return np.where(inside, y, np.float32(0)).astype(np.float32)
    lo = max(0, i0 * rp.M // rp.L - rp.W + 1)
    hi = max(lo, min(n, (i1 - 1) * rp.M // rp.L + rp.W + 1))     # frames lo .. hi - 1 are the ones read
    t = lo // rp.M                                               # shifted by t periods (M frames, L outputs): same phases
    off, sh = t * rp.M, t * rp.L
    k = np.arange(lo, hi, dtype=np.int64)
    e = hist_row[k % hcap]
    if fmt == PCM_S16:
        xs = np.zeros(n - off, dtype=np.int64)
        xs[lo - off:hi - off] = e
        acc = rs._filter_row(xs, n - off, rp, rp.table.astype(np.int64), i0 - sh, i1 - sh)
        return (acc.astype(np.float64) / np.float64(ch * (1 << 45))).astype(np.float32)
    xs = np.zeros(n - off, dtype=np.float64)
    xs[lo - off:hi - off] = e.view(np.float64)
    acc = rs._filter_row(xs, n - off, rp, rp.table.astype(np.float64) * 2.0 ** -30, i0 - sh, i1 - sh)
    return (acc / np.float64(ch)).astype(np.float32)


def push_rs_host(state: StreamState, rs_state: ResampleState, slots, flags, n_in, out_limit, chunk):
    """The twin of one qasr_stream_rs_push: chunk int16 or float32 [B][pitch * channels] (interleaved); slots / flags / n_in /
    out_limit int [B].  Returns (n_taken, n_out, status) int32 [B].  See RS_STREAM_RULES."""
    plan = rs_state.plan
    x = np.asarray(chunk)
    if x.ndim != 2 or x.dtype not in (np.int16, np.float32):
        raise ValueError(f'push_rs: chunk must be int16 or float32 [B][pitch * channels], got {x.dtype} {x.shape}')
    ch = plan.channels
    if x.shape[1] % ch:
        raise ValueError(f'push_rs: a chunk row of {x.shape[1]} samples is no multiple of {ch} channels')
    pitch = x.shape[1] // ch
    call_fmt = PCM_S16 if x.dtype == np.int16 else PCM_F32
    sl = np.asarray(slots).reshape(-1).tolist()
    B = len(sl)
    n_taken, n_out, status = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, slot in enumerate(sl):
        if not 0 <= slot < state.S:
            status[b] = STATUS_SLOT
            continue
        blk, rsb, hist = state.block[slot], rs_state.block[slot], rs_state.hist[slot]
        if int(flags[b]) & BEGIN:
            blk[:] = 0
            rsb[:] = 0
        r = max(state.received(slot), 0)
        n0 = max(rs_state.in_received(slot), 0)
        fmt0 = int(rsb[_R_FMT])
        fmt_ok = fmt0 in (0, call_fmt + 1)
        fmt = fmt0 - 1 if fmt0 else call_fmt
        want = max(0, min(int(n_in[b]), pitch, plan.Ain)) if fmt_ok else 0
        n = min(want, plan.room(r, n0))
        if n:
            sums = rs._channel_sum(x[b], n, ch, np.int64 if fmt == PCM_S16 else np.float64)
            hist[(n0 + np.arange(n, dtype=np.int64)) % plan.hcap] = sums.view(np.int64)
        n1 = n0 + n
        rsb[_R_IN:_R_IN + 2].view(np.int64)[0] = n1
        rsb[_R_FMT] = fmt + 1
        target = plan.out_len(n1) if int(flags[b]) & FLUSH else plan.ready(n1)
        k = max(0, min(target - r, int(out_limit[b]), plan.C))
        if k:
            y = _outputs(hist, fmt, n1, plan, r, r + k)
            state.ring[slot, (r + np.arange(k, dtype=np.int64)) % plan.cap] = y
        blk[_W_RECV:_W_RECV + 2].view(np.int64)[0] = r + k
        n_taken[b], n_out[b] = n, k
        status[b] = STATUS_FORMAT if not fmt_ok else (STATUS_FULL if n < want else STATUS_OK)
    return n_taken, n_out, status
