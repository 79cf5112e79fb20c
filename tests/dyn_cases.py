"""Cases of the dynamic-quantisation kernels (csrc/qasr_dynamic.hip) and their NumPy reference.

Every entry point is restated here as a plain NumPy function composed of the oracle's scalars (oracle/int_oracle.py, pinned
to the reference's own modules by tests/golden through tests/test_oracle_golden.py): sym_scale, quantize,
requant_multiplier, act_clamp, bias_ints, float_view, float_view_with_residue, mask_time, quantile_f32.  Where the kernel
takes a parameter the oracle's scalar derives itself (a multiplier M given from outside, a clamp (lo, hi)), the
restatement takes it too; tests/test_dyn_cases_cpu.py anchors each restatement to OracleNet(dynamic=True)'s own trace and
counts the edges the case lists claim to hold.  tests/test_gpu_dynamic_ops.py runs the kernels on the same cases.

A case is a dict of NumPy arrays: views (`View`), lengths, flags and `want`, the expected output.  No GPU, no torch.
"""
import numpy as np

from oracle import int_oracle as O

f32, f64 = np.float32, np.float64
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FILL = 0x55                                                   # output buffers are pre-filled with this byte

BS, CS, TS = (1, 3), (1, 5, 257), (1, 63, 65, 257, 600)
ALL_SHAPES = [(B, C, T) for B in BS for C in CS for T in TS]
# every B, C and T at least once: C = 257 crosses the 256-thread block of act_params / conv_params, the T values straddle
# one wave (63 / 65) and the 256-stride row loop (257, 600); T = 1 leaves three waves of a row without an element
COVER_SHAPES = [(1, 1, 1), (3, 5, 63), (1, 5, 65), (3, 1, 257), (1, 257, 65), (3, 5, 600), (3, 257, 1), (1, 1, 600)]
PAD_SHAPE = (3, 5, 65, 512)                                   # Tp well beyond T (the runner's Tp is T rounded up to 64)
KINDS = ('i32c', 'i8t', 'sum', 'res', 'xf')                   # operand combinations of qasr_dyn_range(_percentile)
SIGNS = ('mixed', 'neg', 'pos')


def rup(x, m):
    return (x + m - 1) // m * m


def ord32(v):
    """float32 -> uint32 whose unsigned order is the float order (the form minmax[] is kept in)."""
    u = int(np.asarray(v, f32).reshape(()).view(np.uint32))
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


class View:
    """A float32 tensor given as integers x scale: data int32 / int8 [B, C, Tp], scale f32 [C] (per_channel) or [1],
    residue None or (r_lo, r_hi) int32 [B, C, Tp] in units of 2^-24 (value r_lo + 128 r_hi)."""

    def __init__(self, data, scale, per_channel, residue=None):
        self.data, self.scale, self.per_channel, self.residue = data, np.asarray(scale, f32), bool(per_channel), residue
        assert data.dtype in (np.int32, np.int8) and self.scale.shape == ((data.shape[1],) if per_channel else (1,))

    def scales(self):
        return self.scale if self.per_channel else np.repeat(self.scale, self.data.shape[1])

    def floats(self, T):
        """conv_int.float() * scale (quant_modules.py:305-308) on columns [0, T)."""
        z = self.data[:, :, :T].astype(np.int64)
        if self.residue is None:
            return O.float_view(z, self.scales())
        r = self.residue[0][:, :, :T].astype(f64) + 128.0 * self.residue[1][:, :, :T].astype(f64)
        return O.float_view_with_residue(z, r * 2.0 ** -24, self.scales())


# ----------------------------------------------------------------------------- restatements
def ref_x_act(a, b, xf, lens, relu, T):
    """What QuantAct.forward ranges over (quant_modules.py:108,149-167): identity(b) + x(a), ReLU, MaskedConv1d's zeros;
    with `xf` the float features themselves (first layer; a, b and relu unused).  float32 [B, C, T]."""
    if xf is not None:
        y = np.asarray(xf, f32)[:, :, :T]
    else:
        y = a.floats(T)
        if b is not None:
            y = (b.floats(T) + y).astype(f32)
        if relu:
            y = np.maximum(y, f32(0))
    if lens is not None:
        y = O.mask_time(y, np.minimum(np.asarray(lens, np.int64), T))
    return np.ascontiguousarray(y, f32)


def ref_range(x_act):
    """qasr_dyn_range: (x_act.min(), x_act.max()) in the ordered encoding."""
    return np.array([ord32(x_act.min()), ord32(x_act.max())], np.uint32)


def ref_range_percentile(x_act, p):
    """qasr_dyn_range_percentile: torch.quantile at fl32(1 - p/100) and fl32(p/100) (quant_modules.py:158-167)."""
    return np.array([ord32(O.quantile_f32(x_act, f32(1 - p / 100))), ord32(O.quantile_f32(x_act, f32(p / 100)))], np.uint32)


def multiplier(pre_sf, out_sf):
    """m 2^-e of requant_multiplier as the float64 fixedpoint_mul multiplies with (exact: m <= 2^31)."""
    m, e = O.requant_multiplier(pre_sf, out_sf)
    return m.astype(f64) * np.power(2.0, -e.astype(f64))


def ref_act_params(mn, mx, bits, C, sa, sb):
    """qasr_dyn_act_params: (s_out, Ma [C], Mb [C] or None); sa / sb [C] or [1]."""
    s = O.sym_scale(bits, mn, mx)
    bc = lambda v: np.broadcast_to(np.asarray(v, f32), (C,))
    return f32(s), multiplier(bc(sa), s), (None if sb is None else multiplier(bc(sb), s))


def ref_operand(v, M, relu, T):
    """One operand of fixedpoint_mul.forward (quant_utils.py:187-198) with the multiplier given: z = round(y / pre_sf) in
    float32, round(f64(z) M).  Returns (out, z, z M) as (int64, int64, float64)."""
    y = v.floats(T)
    if relu:
        y = np.maximum(y, f32(0))
    z = np.rint((y / v.scales().reshape(1, -1, 1)).astype(f32))
    prod = z.astype(f64) * np.asarray(M, f64).reshape(1, -1, 1)
    return np.rint(prod).astype(np.int64), z.astype(np.int64), prod


def ref_requant(a, Ma, b, Mb, lens, relu, T, Tp, lo, hi):
    """qasr_dyn_requant: codes [B, C, Tp] as bytes (q & 0xff); columns >= min(len, T) are 0."""
    q = ref_operand(a, Ma, relu, T)[0]
    if b is not None:
        q = ref_operand(b, Mb, False, T)[0] + q
    q = np.clip(q, lo, hi)
    if lens is not None:
        q = O.mask_time(q, np.minimum(np.asarray(lens, np.int64), T))
    out = np.zeros(q.shape[:2] + (Tp,), np.int64)
    out[:, :, :T] = q
    return (out & 0xff).astype(np.uint8)


def ref_quant_in(xf, mn, mx, lens, bits, T, Tp):
    """qasr_dyn_quant_in: the first layer's SymmetricQuantFunction (quant_modules.py:180-184) -> (s_out, codes bytes)."""
    s = O.sym_scale(bits, mn, mx)
    q = O.act_clamp(O.quantize(np.asarray(xf, f32)[:, :, :T], bits, s), bits)     # the clamp that follows: identity here
    q = O.mask_time(q, np.minimum(np.asarray(lens, np.int64), T))
    out = np.zeros(q.shape[:2] + (Tp,), np.int64)
    out[:, :, :T] = q
    return f32(s), (out & 0xff).astype(np.uint8)


def ref_conv_params(s_x, s_w, bprime, wsum128, C_pad):
    """qasr_dyn_conv_params: (sf [C_pad], bias int32 [C_pad], bias_ints int64 [C] before saturation).  The bias is
    bias_ints saturated to int32, + wsum128 modulo 2^32; tail entries are sf = 1, bias = 0."""
    bint, s_b = O.bias_ints(bprime, s_w, s_x)
    C = s_b.shape[0]
    bint = np.zeros(C, np.int64) if bint is None else bint
    b = np.clip(bint, I32_MIN, I32_MAX)
    if wsum128 is not None:
        b = b + np.asarray(wsum128, np.int64)
    b = ((b + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    sf, bias = np.ones(C_pad, f32), np.zeros(C_pad, np.int32)
    sf[:C], bias[:C] = s_b, b
    return sf, bias, bint


# ----------------------------------------------------------------------------- case builders
def _ints(rng, shape, sign, lo=10, hi=50000):
    v = rng.integers(lo, hi, shape)
    if sign == 'neg':
        return -v
    if sign == 'mixed':
        return v * rng.choice([-1, 1], shape)
    return v


def _padded(v, Tp, fill):
    """[B, C, T] -> [B, C, Tp] with `fill` in the padding: a kernel that reads past T shows in its result."""
    out = np.full(v.shape[:2] + (Tp,), fill, v.dtype)
    out[:, :, :v.shape[2]] = v
    return out


def make_view(rng, B, C, T, Tp, kind, sign='mixed', big=0):
    """kind: 'i32c' int32 x per-channel scale, 'i32t' int32 x per-tensor scale, 'i8t' / 'i8c' int8 codes, 'res' int32 x
    per-channel scale with a residue pair.  big: that many elements (at most) are set to |acc| >= 2^24."""
    pc = kind in ('i32c', 'i8c', 'res')
    scale = np.exp(rng.uniform(-12, -4, C if pc else 1)).astype(f32)
    if kind in ('i8t', 'i8c'):
        d = np.clip(_ints(rng, (B, C, T), sign, 1, 128), -128, 127).astype(np.int8)
        return View(_padded(d, Tp, np.int8(-128 if sign == 'pos' else 127)), scale, pc)
    d = _ints(rng, (B, C, T), sign).astype(np.int64)
    for _ in range(big):
        i = tuple(int(rng.integers(0, n)) for n in (B, C, T))
        d[i] = np.sign(d[i]) * int(rng.integers(2 ** 24 + 1, 2 ** 31 - 1))
    d = _padded(d.astype(np.int32), Tp, np.int32(I32_MIN if sign == 'pos' else I32_MAX))
    residue = None
    if kind == 'res':                                         # accumulators of the residue convs: sum(w lo), sum(w hi)
        residue = (_padded(rng.integers(-5000, 5001, (B, C, T)).astype(np.int32), Tp, np.int32(I32_MAX)),
                   _padded(rng.integers(-200, 201, (B, C, T)).astype(np.int32), Tp, np.int32(I32_MAX)))
    return View(d, scale, pc, residue)


def make_lens(B, T, i):
    """Lengths of case number i: 0, 1, T and a value above T all occur over a case list."""
    if B == 1:
        return np.array([[T], [T + 5], [1], [0], [max(T // 2, 1)]][i % 5], np.int32)
    return np.array([[T + 5, 1, 0], [T, max(T // 2, 1), 1], [max(T - 1, 0), T, T + 64]][i % 3][:B], np.int32)


def range_case(kind, shape, i, with_lens, sign):
    """One qasr_dyn_range / _range_percentile case: operands of `kind`, x_act and the min / max encoding."""
    B, C, T = shape[:3]
    Tp = shape[3] if len(shape) > 3 else rup(T, 64)
    rng = np.random.default_rng([11, KINDS.index(kind), B, C, T, i])
    c = dict(kind=kind, B=B, C=C, T=T, Tp=Tp, a=None, b=None, xf=None, Tx=0, relu=0, sign=sign,
             lens=make_lens(B, T, i) if with_lens else None)
    if kind == 'xf':                                          # the float features: Tx > T, junk beyond T
        c['Tx'] = T + 7
        x = rng.standard_normal((B, C, c['Tx'])).astype(f32) * f32(3)
        x = {'mixed': x, 'neg': -np.abs(x) - f32(0.01), 'pos': np.abs(x) + f32(0.01)}[sign]
        x[:, :, T:] = f32(-1e30 if sign == 'pos' else 1e30)
        c['xf'] = x
    elif kind == 'sum':                                       # identity(b) + x(a): mixed data types and scale kinds, ReLU after
        c['a'] = make_view(rng, B, C, T, Tp, 'i32c' if i % 2 else 'i32t', 'mixed', big=2)
        c['b'] = make_view(rng, B, C, T, Tp, 'i8t' if i % 2 else 'i8c', sign)
        if i % 2:                                             # bring the two operands to the same magnitude
            c['b'].scale = (c['b'].scale * f32(300)).astype(f32)
        c['relu'] = int(i % 3 != 0)
    else:
        c['a'] = make_view(rng, B, C, T, Tp, kind, sign, big=2 if kind == 'i32c' else 0)
        c['relu'] = int(kind == 'i32c' and i % 4 == 3)
    c['x_act'] = ref_x_act(c['a'], c['b'], c['xf'], c['lens'], c['relu'], T)
    c['want'] = ref_range(c['x_act'])
    return c


def range_cases(kind, shapes=None):
    shapes = (ALL_SHAPES + [PAD_SHAPE]) if shapes is None else shapes
    out = []
    for i, sh in enumerate(shapes):
        for with_lens in (False, True):
            out.append(range_case(kind, sh, i, with_lens, SIGNS[(i + with_lens) % 3]))
    return out


def negzero_cases():
    """Float features whose only zero is -0.0: as the minimum of a positive-only tensor and as the maximum of a
    negative-only one (no mask: its zeros are +0.0).  ord32(-0.0) = 0x7fffffff, one below ord32(+0.0)."""
    out = []
    for sign in (1, -1):
        rng = np.random.default_rng([12, sign + 1])
        x = (sign * (np.abs(rng.standard_normal((3, 5, 72))) + 0.5)).astype(f32)
        x[1, 2, 40] = f32(-0.0)
        c = dict(kind='xf', B=3, C=5, T=65, Tp=128, a=None, b=None, xf=x, Tx=72, relu=0, lens=None, sign='negzero')
        c['x_act'] = ref_x_act(None, None, x, None, 0, 65)
        c['want'] = ref_range(c['x_act'])
        out.append(c)
    return out


PERCENTILES = (99.9, 99.0, 100.0, 50.0)
# B C T = 1, 2, 3, 5 (no float4 in k_qs_hist: n4 = 0), 4k + 1 (325, 945) and 4k + 3 (63, 771), and the row loops
PCT_SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 5), (1, 5, 65), (1, 1, 63), (3, 1, 257), (3, 5, 63), (1, 257, 65),
              (3, 5, 600), PAD_SHAPE]


def percentile_cases(kind):
    out = []
    for c in range_cases(kind, PCT_SHAPES):
        c['want_p'] = {p: ref_range_percentile(c['x_act'], p) for p in PERCENTILES}
        out.append(c)
    return out


def act_params_cases():
    """minmax hand-encoded; bits 6..9; operand b absent, per channel and per tensor; scales over exp(U(-30, 2)); the floor."""
    out = []
    i = 0
    for C in CS:
        for bits in (6, 7, 8, 9):
            for bmode in (None, 'c', 't'):
                rng = np.random.default_rng([13, C, bits, i])
                a_pc = bool(i % 2) or bmode == 't'
                sa = np.exp(rng.uniform(-30, 2, C if a_pc else 1)).astype(f32)
                sb = None if bmode is None else np.exp(rng.uniform(-30, 2, C if bmode == 'c' else 1)).astype(f32)
                mx = f32(np.exp(rng.uniform(-30, 6)))
                mn, mx = [(f32(-0.3) * mx, mx), (-mx, f32(0.5) * mx), (f32(0), f32(0)), (f32(0), mx)][i % 4]   # i % 4 == 2: floor
                s, Ma, Mb = ref_act_params(mn, mx, bits, C, sa, sb)
                out.append(dict(C=C, bits=bits, mm=np.array([ord32(mn), ord32(mx)], np.uint32), mn=mn, mx=mx, sa=sa, a_pc=a_pc,
                                sb=sb, b_pc=bmode == 'c', s=s, Ma=Ma, Mb=Mb))
                i += 1
    return out


CLAMPS = ((-128, 127), (0, 127), (-32, 31), (0, 255), (-256, -1))
TIE_M = (0.5, 0.25, 1.5)


def requant_cases():
    """Ma / Mb are inputs, so the ties are constructed: channels cycle through M = 0.5, 0.25, 1.5 (z odd, or z = 2 mod 4,
    lands on k + 0.5) and one free multiplier.  Kinds: 'tie' small integers (z = acc exactly, both clamps reached),
    'big' |acc| up to 2^31 - 1 with multipliers near 2^-23, 'res' a view with residue, 'two' x(a) with ReLU + int8
    identity(b) on a per-tensor scale."""
    out = []
    i = 0
    for sh in COVER_SHAPES + [PAD_SHAPE]:
        B, C, T = sh[:3]
        Tp = sh[3] if len(sh) > 3 else rup(T, 64)
        for kind in ('tie', 'big', 'res', 'two'):
            lo, hi = CLAMPS[i % 5]
            rng = np.random.default_rng([14, B, C, T, i])
            free = rng.uniform(0.3, 2.0, C)
            Ma = np.where(np.arange(C) % 4 < 3, np.asarray(TIE_M)[np.arange(C) % 4 % 3], free).astype(f64)
            b = Mb = None
            relu = 0
            if kind == 'big':
                a = make_view(rng, B, C, T, Tp, 'i32c', 'mixed')
                d = rng.integers(I32_MIN, I32_MAX, (B, C, T), dtype=np.int64, endpoint=True)
                d.reshape(-1)[:2] = (I32_MAX, I32_MIN)[:d.size]
                a.data[:, :, :T] = d.astype(np.int32)
                Ma = rng.uniform(0.3, 2.0, C) * 2.0 ** -23
            elif kind == 'res':
                a = make_view(rng, B, C, T, Tp, 'res', 'mixed', big=0)
                a.data[:, :, :T] = _ints(rng, (B, C, T), 'mixed', 0, 400).astype(np.int32)
            else:
                a = make_view(rng, B, C, T, Tp, 'i32c' if i % 2 else 'i32t', 'mixed')
                a.data[:, :, :T] = _ints(rng, (B, C, T), 'mixed', 0, 400).astype(np.int32)
                if kind == 'two':
                    b = make_view(rng, B, C, T, Tp, 'i8t', 'mixed')
                    Mb = np.asarray(TIE_M)[(np.arange(C) + 1) % 3].astype(f64)
                    relu = 1
            lens = make_lens(B, T, i) if i % 3 else None
            c = dict(kind=kind, B=B, C=C, T=T, Tp=Tp, a=a, b=b, Ma=Ma, Mb=Mb, lens=lens, relu=relu, lo=lo, hi=hi)
            c['want'] = ref_requant(a, Ma, b, Mb, lens, relu, T, Tp, lo, hi)
            out.append(c)
            i += 1
    return out


def quant_in_cases():
    """Float features [B, C, Tx], Tx != Tp.  'tie': max |x| = n exactly, so s = 1, fl32(1/s) = 1 and x = k + 0.5 are ties
    of fl32(inv x); +n lands on n - 1 and -n on -n (the asymmetric clamp).  'rand': Gaussian, max element present.
    'zero': all-zero input -> the scale floor, all-zero codes."""
    out = []
    i = 0
    for B, C, T in COVER_SHAPES:
        for bits in (6, 8):
            for kind in ('tie', 'rand', 'zero'):
                n = 2 ** (bits - 1) - 1
                rng = np.random.default_rng([15, B, C, T, bits, i])
                Tx, Tp = T + 3, rup(T, 64)
                lens = make_lens(B, T, i)
                if kind == 'tie':
                    x = (rng.integers(-n - 2, n + 2, (B, C, Tx)) + 0.5).astype(f32)
                    x.reshape(-1)[:2] = (n, -n)[:x.size]
                    mn, mx = f32(-n), f32(n)
                elif kind == 'rand':
                    x = (rng.standard_normal((B, C, Tx)) * np.exp(rng.uniform(-8, 4))).astype(f32)
                    xa = ref_x_act(None, None, x, lens, 0, T)  # what qasr_dyn_range(xf=...) ranges over
                    mn, mx = xa.min(), xa.max()
                else:
                    x = np.zeros((B, C, Tx), f32)
                    mn, mx = f32(0), f32(0)
                s, want = ref_quant_in(x, mn, mx, lens, bits, T, Tp)
                out.append(dict(kind=kind, B=B, C=C, T=T, Tx=Tx, Tp=Tp, bits=bits, x=x, mn=mn, mx=mx, lens=lens, s=s, want=want,
                                from_range=kind == 'rand' and i % 2 == 0))
                i += 1
    return out


def conv_params_cases():
    """s_x over exp(U(-30, 2)) and at the floor (bias integers saturate on both sides there), power-of-two scales with
    bprime = (k + 0.5) s_b (ties of the bias), with / without bprime and wsum128 (both signs, near +-2^22)."""
    out = []
    i = 0
    for C in CS:
        for kind in ('rand', 'floor', 'tie'):
            for has_b in (True, False):
                for has_w in (True, False):
                    rng = np.random.default_rng([16, C, i])
                    s_w = np.exp(rng.uniform(-8, -1, C)).astype(f32)
                    s_x = f32(np.exp(rng.uniform(-30, 2)))
                    bp = (rng.standard_normal(C) * 0.5).astype(f32)
                    if kind == 'floor':
                        s_x = O.sym_scale(8 if i % 2 else 9, 0.0, 0.0)
                        bp[:3] = (0.25, -0.25, 0.0)[:C]       # both signs saturate whatever the draw
                    elif kind == 'tie':
                        s_w = np.exp2(-rng.integers(1, 9, C)).astype(f32)
                        s_x = f32(2.0 ** -4)
                        bp = ((rng.integers(-3000, 3000, C) + 0.5) * s_w.astype(f64) * 2.0 ** -4).astype(f32)
                    wsum = None
                    if has_w:
                        wsum = (rng.integers(-2 ** 22, 2 ** 22, C, endpoint=True)).astype(np.int32)
                        wsum[:2] = (2 ** 22 - 128, -(2 ** 22 - 128))[:C]
                    C_pad = rup(C, 128)
                    sf, bias, bint = ref_conv_params(s_x, s_w, bp if has_b else None, wsum, C_pad)
                    out.append(dict(kind=kind, C=C, C_pad=C_pad, s_x=f32(s_x), s_w=s_w, bprime=bp if has_b else None, wsum128=wsum,
                                    sf=sf, bias=bias, bint=bint))
                    i += 1
    return out
