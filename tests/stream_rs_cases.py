"""Shared cases of the tests of streaming at any sample rate (qasr.stream_rs): a small stream plan whose rings wrap within
half a second, the resample plans, the sample formats, three streams per case, the slicings, and a seeded schedule of calls
(rows joining and leaving, BEGIN on a used slot, an out-of-range slot, the history-full clamp, FLUSH twice) played on the twin
and recorded, so that a device can be driven with the same calls and compared on every byte."""
import numpy as np

import stream_cases as sc
from qasr import resample as rs, stream as st, stream_rs as srs

SP = sc.plan_frames(2, 2, 1)                        # C = 640 samples, cap = 2240: 0.14 s of ring
assert (SP.C, SP.cap) == (640, 2240)

# name -> (input rate, preset); what each is here for
PLANS = {
    '8000_best': (8000, 'best'),                    # L 2 / M 1, W 68: one input frame yields two outputs
    '48000_best': (48000, 'best'),                  # 1 / 3, W 203: the filter is longer than a chunk's worth of history
    '44100_fast': (44100, 'fast'),                  # 160 / 441, W 52: many phases
    '12000_fast': (12000, 'fast'),                  # 4 / 3
    '16000_equal': (16000, 'best'),                 # the equal rule (no filter; 2 or more channels, or int16)
}
DIRECT = ('256000_fast', (256000, 'fast'))          # 1 / 16, W 302: a tile's stretch, 255 * 16 + 1 + 604 frames, exceeds the stage
FORMATS = [('int16', 1), ('int16', 2), ('int16', 8), ('float32', 1), ('float32', 3)]
_plans = {}


def rplan(name):
    rate, quality = dict(PLANS, **{DIRECT[0]: DIRECT[1]})[name]
    if name not in _plans:
        _plans[name] = rs.ResamplePlan(rate, 16000, quality)
    return _plans[name]


def splan(name, channels):
    return srs.StreamResamplePlan(SP, rplan(name), channels)


def staged(rp):
    """the inequality by which the host picks the staged instantiation (resample_staged, csrc/qasr_resample.hip)"""
    return (255 * rp.M + rp.L - 1) // rp.L + 1 + 2 * rp.W <= 4096


def combos():
    out = []
    for name in PLANS:
        for dtype, ch in FORMATS:
            if name == '16000_equal' and dtype == 'float32' and ch == 1:
                continue                            # the model's rate, mono float: the plain session, no resampler
            out.append((name, dtype, ch))
    return out


def signal(rng, dtype, n, ch):
    """[n * ch] interleaved; int16 carries full-scale -32768 in every channel of some frames (the exactness bound)"""
    if dtype == 'int16':
        x = rng.integers(-32768, 32768, size=n * ch).astype(np.int16)
        if n:
            x.reshape(n, ch)[::37] = -32768
        return x
    return (rng.standard_normal(n * ch) * 0.3).astype(np.float32)


def streams(name, dtype, ch, seed=0):
    """three streams: 0.25 s, three frames fewer than W (every output comes at the flush; 5 frames for W = 0) and 0 frames"""
    p = splan(name, ch)
    rate = p.resample_plan.sr_in
    rng = np.random.default_rng(seed)
    lens = [int(0.25 * rate) + 3, max(p.W - 3, 5), 0]
    return [signal(rng, dtype, n, ch) for n in lens], lens


def slicings(p, n):
    """name -> the pieces (frames) a stream of n frames is offered in; pieces above Ain must be cut by the caller"""
    rng = np.random.default_rng(n)
    rnd, left = [], n
    while left > 0:
        k = int(rng.choice([0, 1, 7, max(p.W, 1), p.W + 1, p.Ain, int(rng.integers(1, p.Ain + 1))]))
        rnd.append(min(k, left))
        left -= rnd[-1]
    return {'1': [1] * n, '7': [7] * (n // 7) + [n % 7], 'W': [max(p.W, 1)] * (n // max(p.W, 1)) + [n % max(p.W, 1)],
            'W+1': [p.W + 1] * (n // (p.W + 1)) + [n % (p.W + 1)], 'Ain': [p.Ain] * (n // p.Ain) + [n % p.Ain],
            'above': [p.Ain + 5] * (n // (p.Ain + 5)) + [n % (p.Ain + 5)], 'random': rnd}


def read_ring(state, slot, n_out):
    """the n_out samples a call just produced for `slot`, read before the ring wraps over them"""
    r = state.received(slot)
    return state.ring[slot, (r - n_out + np.arange(n_out, dtype=np.int64)) % state.plan.cap].copy()


def play_stream(p, x, n, pieces, slot=0, S=1):
    """One stream through push_rs_host in the session's protocol: a piece (cut at Ain) is appended, then everything ready is
    produced chunk by chunk; FLUSH rounds at the end.  Returns (the concatenated outputs, the states)."""
    ch = p.channels
    state, rss = st.StreamState(S, SP), srs.ResampleState(S, p)
    got, off, begin = [], 0, st.BEGIN

    def rounds(flag, k, chunk):
        nonlocal begin
        while True:
            limit = SP.C - state.received(slot) % SP.C
            nt, no, status = srs.push_rs_host(state, rss, [slot], [flag | begin], [k], [limit], chunk)
            begin = 0
            assert (int(nt[0]), int(status[0])) == (k, 0), (nt, status, k)     # the protocol never drops a frame
            got.append(read_ring(state, slot, int(no[0])))
            k = 0
            target = p.out_len(rss.in_received(slot)) if flag else p.ready(rss.in_received(slot))
            if target == state.received(slot):
                return

    for piece in pieces:
        while True:                                               # (a piece of 0 frames is a call that only produces)
            k = min(piece, p.Ain)
            rounds(0, k, x[None, off * ch:(off + k) * ch] if k else np.zeros((1, ch), x.dtype))
            off, piece = off + k, piece - k
            if piece == 0:
                break
    assert off == n
    rounds(srs.FLUSH, 0, np.zeros((1, ch), x.dtype))
    return np.concatenate(got + [np.zeros(0, np.float32)]), state, rss


def offline(p, x, n):
    out, ol = rs.resample_host(x[None, :], [n], p.resample_plan, p.channels)
    return out[0, :int(ol[0])]


def schedule(name, dtype, ch, S=4, B=3, seed=0, calls=60):
    """A seeded schedule of qasr_stream_rs_push calls over S slots, B rows each, played on the twin.  Yields per call
    dict(slots, flags, n_in, out_limit, chunk [B][pitch * ch], n_taken, n_out, status, block, ring, rs_block, hist) - the
    twin's outputs and both states AFTER the call - and finally dict(done=True, taken={slot: frames}, outs={slot: samples}).
    Slot 3 is filled without producing until the history clamp cuts an append (status 1); slot 1 is begun again half-way;
    rows with slot -1 or S are skipped; a stream that has ended is flushed, twice."""
    p = splan(name, ch)
    rng = np.random.default_rng(seed)
    state, rss = st.StreamState(S, SP), srs.ResampleState(S, p)
    n_total = p.hcap * 3 + 11
    data = {s: signal(rng, dtype, n_total, ch) for s in range(S)}
    taken = {s: 0 for s in range(S)}
    outs = {s: [] for s in range(S)}
    started, ended = set(), set()
    pitch = p.Ain + 5
    sizes = [0, 1, 7, max(p.W, 1), p.W + 1, p.Ain, p.Ain + 5, 2 ** 30, -3]
    for c in range(calls):
        slots = rng.permutation(S)[:B].tolist()
        if c % 9 == 4:
            slots[int(rng.integers(0, B))] = -1 if c % 2 else S
        flags, n_in, limit = [0] * B, [0] * B, [0] * B
        chunk = np.zeros((B, pitch * ch), dtype=data[0].dtype)
        for b, s in enumerate(slots):
            n_in[b] = int(rng.choice(sizes))
            limit[b] = int(rng.choice([0, 5, SP.C - 1, SP.C, 2 ** 30, -1]))
            if not 0 <= s < S:
                chunk[b] = signal(rng, dtype, pitch, ch)
                continue
            if s == 3 and c < calls // 2:
                n_in[b], limit[b] = p.Ain, 0                      # append only, until the history is full
            if s not in started or (s == 1 and c == calls // 2):
                flags[b] |= st.BEGIN
                if s in started:
                    taken[s], outs[s] = 0, []
                    ended.discard(s)
                started.add(s)
            if s in ended or (s == 2 and c >= calls - 8):
                flags[b] |= srs.FLUSH
                n_in[b] = 0
                ended.add(s)
            if taken[s] == n_total:
                ended.add(s)
                flags[b] |= srs.FLUSH
            if n_in[b] > 0:
                n_in[b] = min(n_in[b], n_total - taken[s])        # (only real frames: the outputs are checked against offline)
            w = min(pitch, n_total - taken[s])
            chunk[b, :w * ch] = data[s][taken[s] * ch:(taken[s] + w) * ch]
        nt, no, status = srs.push_rs_host(state, rss, slots, flags, n_in, limit, chunk)
        for b, s in enumerate(slots):
            if 0 <= s < S:
                taken[s] += int(nt[b])
                outs[s].append(read_ring(state, s, int(no[b])))
        yield dict(slots=slots, flags=flags, n_in=n_in, out_limit=limit, chunk=chunk, n_taken=nt, n_out=no, status=status,
                   block=state.block.copy(), ring=state.ring.copy(), rs_block=rss.block.copy(), hist=rss.hist.copy())
    yield dict(done=True, taken=taken, outs={s: np.concatenate(v + [np.zeros(0, np.float32)]) for s, v in outs.items()}, data=data,
               plan=p, ended=ended)
