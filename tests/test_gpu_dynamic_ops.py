"""Operator-level GPU tests of the dynamic path: every qasr_dyn_* entry point and qasr_quantile2 called directly on the
cases of tests/dyn_cases.py and compared with their NumPy restatement of the oracle's scalars - every comparison is
integer or float32 equality.  tests/test_dyn_cases_cpu.py anchors the restatements and counts the edges the cases hold.
Then the silent batch end to end (all-zero features: every scale at its floor, bias integers saturated) against
OracleNet(dynamic=True), the radix select's edges, and the refusals of every entry point."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import dyn_cases as D  # noqa: E402
from oracle import int_oracle as O  # noqa: E402
from qasr import dynamic, engine, synth, topology  # noqa: E402

f32 = np.float32
ERR_ARG = 1


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.set_grad_enabled(False)


def _lib():
    return engine.load_library()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _filled(shape, dtype):
    """An output buffer pre-filled with 0x55 bytes: what a kernel leaves unwritten shows."""
    t = torch.empty(shape, dtype=dtype, device='cuda:0')
    t.view(torch.uint8).fill_(D.FILL)
    return t


def _untouched(*ts):
    return all(bool((t.view(torch.uint8) == D.FILL).all()) for t in ts)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


class _DView:
    """A dyn_cases.View on the device + the qasr_dyn_view that points at it."""

    def __init__(self, v):
        self.keep = [_dev(v.data), _dev(v.scale)] + ([_dev(r) for r in v.residue] if v.residue is not None else [])
        s = dynamic.DynView()
        s.data, s.scale = self.keep[0].data_ptr(), self.keep[1].data_ptr()
        s.is_int8, s.per_channel = int(v.data.dtype == np.int8), int(v.per_channel)
        if v.residue is not None:
            s.residue_lo, s.residue_hi = self.keep[2].data_ptr(), self.keep[3].data_ptr()
        self.s = s

    @staticmethod
    def ref(dv):
        return None if dv is None else C.byref(dv.s)


def _up(v):
    return None if v is None else _DView(v)


def _range_args(c, up):
    a, b, xf, lens = up
    return (_DView.ref(a), _DView.ref(b), engine._ptr(xf), c['Tx'], engine._ptr(lens), c['relu'], c['B'], c['C'], c['T'], c['Tp'])


def _upload_range(c):
    return _up(c['a']), _up(c['b']), _dev(c['xf']), _dev(c['lens'])


def _tag(c):
    return {k: c[k] for k in ('kind', 'B', 'C', 'T', 'Tp', 'relu', 'sign') if k in c}, None if c.get('lens') is None else c['lens'].tolist()


# ----------------------------------------------------------------------------- qasr_dyn_range
@pytest.mark.parametrize('kind', D.KINDS)
def test_range(kind):
    """Both words of minmax against the encoding of the reference's float32 min and max: every shape, with and without
    lens (0, 1, T, above T), negative-only / positive-only / mixed inputs, padding that would show if read."""
    lib = _lib()
    cases = D.range_cases(kind) + (D.negzero_cases() if kind == 'xf' else [])
    for c in cases:
        up = _upload_range(c)
        mm = _filled(2, torch.int32)
        assert lib.qasr_dyn_range(engine._stream_ptr(), *_range_args(c, up), engine._ptr(mm)) == 0
        got = _bits(mm)
        assert np.array_equal(got, c['want']), (_tag(c), [hex(v) for v in got], [hex(v) for v in c['want']])


# ----------------------------------------------------------------------------- qasr_dyn_range_percentile
@pytest.mark.parametrize('kind', D.KINDS)
def test_range_percentile(kind):
    """x_act [B][C][T] on every bit (and nothing written behind it), minmax = the encoding of quantile_f32 at
    fl32(1 - p/100) and fl32(p/100); B C T = 1, 2, 3, 5, 4k + 1, 4k + 3 run k_qs_hist's scalar tail without and with float4s."""
    lib = _lib()
    ws = torch.empty(lib.qasr_quantile_workspace_bytes(), dtype=torch.uint8, device='cuda:0')
    for c in D.percentile_cases(kind):
        up = _upload_range(c)
        n = c['B'] * c['C'] * c['T']
        for p in D.PERCENTILES:
            xa = _filled(n + 16, torch.float32)
            mm = _filled(2, torch.int32)
            rc = lib.qasr_dyn_range_percentile(engine._stream_ptr(), *_range_args(c, up), C.c_float(1 - p / 100), C.c_float(p / 100),
                                               engine._ptr(xa), engine._ptr(ws), ws.numel(), engine._ptr(mm))
            assert rc == 0
            assert np.array_equal(_bits(xa[:n]), c['x_act'].reshape(-1).view(np.uint32)), (_tag(c), p, 'x_act')
            assert _untouched(xa[n:]), (_tag(c), p, 'written past x_act')
            got = _bits(mm)
            assert np.array_equal(got, c['want_p'][p]), (_tag(c), p, [hex(v) for v in got], [hex(v) for v in c['want_p'][p]])


# ----------------------------------------------------------------------------- qasr_dyn_act_params
def test_act_params():
    """s_out, Ma and Mb against sym_scale and m 2^-e of requant_multiplier: bits 6..9, operand b per channel and per
    tensor, scales over exp(U(-30, 2)), the floor (multipliers of 2^30 and more); Mb untouched without operand b."""
    lib = _lib()
    for c in D.act_params_cases():
        mm, sa, sb = _dev(c['mm'].view(np.int32)), _dev(c['sa']), _dev(c['sb'])
        s, Ma, Mb = _filled(1, torch.float32), _filled(c['C'], torch.float64), _filled(c['C'], torch.float64)
        rc = lib.qasr_dyn_act_params(engine._stream_ptr(), engine._ptr(mm), c['bits'], c['C'], engine._ptr(sa), int(c['a_pc']),
                                     engine._ptr(sb), int(c['b_pc']), engine._ptr(s), engine._ptr(Ma), engine._ptr(Mb))
        tag = (c['C'], c['bits'], c['a_pc'], c['b_pc'], float(c['mn']), float(c['mx']))
        assert rc == 0
        assert _bits(s)[0] == np.asarray(c['s']).view(np.uint32), tag
        assert np.array_equal(Ma.cpu().numpy(), c['Ma']), tag
        if c['sb'] is None:
            assert _untouched(Mb), tag
        else:
            assert np.array_equal(Mb.cpu().numpy(), c['Mb']), tag


# ----------------------------------------------------------------------------- qasr_dyn_requant
def test_requant():
    """Codes of one and two operands with the multipliers given (constructed ties), ReLU on operand a only, five clamp
    ranges, |acc| up to 2^31 - 1, residue views, int8 identity on a per-tensor scale, lens; columns [min(len, T), Tp) are 0."""
    lib = _lib()
    for c in D.requant_cases():
        a, b = _up(c['a']), _up(c['b'])
        Ma, Mb, lens = _dev(c['Ma']), _dev(c['Mb']), _dev(c['lens'])
        out = _filled((c['B'], c['C'], c['Tp']), torch.int8)
        rc = lib.qasr_dyn_requant(engine._stream_ptr(), _DView.ref(a), engine._ptr(Ma), _DView.ref(b), engine._ptr(Mb),
                                  engine._ptr(lens), c['relu'], c['B'], c['C'], c['T'], c['Tp'], c['lo'], c['hi'], engine._ptr(out))
        assert rc == 0
        got = out.view(torch.uint8).cpu().numpy()
        tag = (_tag(c), c['lo'], c['hi'])
        assert np.array_equal(got, c['want']), (tag, int((got != c['want']).sum()))
        for bi in range(c['B']):
            end = c['T'] if c['lens'] is None else min(int(c['lens'][bi]), c['T'])
            assert not got[bi, :, end:].any(), (tag, bi)


# ----------------------------------------------------------------------------- qasr_dyn_quant_in
def test_quant_in():
    """Bits 6 and 8; minmax hand-encoded and from qasr_dyn_range(xf=...); +max -> n - 1; ties of fl32(inv x); Tx != Tp;
    lens; s_out; the all-zero input (scale floor, all-zero codes)."""
    lib = _lib()
    for c in D.quant_in_cases():
        x, lens = _dev(c['x']), _dev(c['lens'])
        if c['from_range']:
            mm = _filled(2, torch.int32)
            assert lib.qasr_dyn_range(engine._stream_ptr(), None, None, engine._ptr(x), c['Tx'], engine._ptr(lens), 0, c['B'], c['C'],
                                      c['T'], c['Tp'], engine._ptr(mm)) == 0
        else:
            mm = _dev(np.array([D.ord32(c['mn']), D.ord32(c['mx'])], np.uint32).view(np.int32))
        s, out = _filled(1, torch.float32), _filled((c['B'], c['C'], c['Tp']), torch.int8)
        rc = lib.qasr_dyn_quant_in(engine._stream_ptr(), engine._ptr(x), c['Tx'], engine._ptr(mm), engine._ptr(lens), c['bits'], c['B'],
                                   c['C'], c['T'], c['Tp'], engine._ptr(s), engine._ptr(out))
        tag = (_tag(c), c['bits'], c['from_range'])
        assert rc == 0
        assert _bits(s)[0] == np.asarray(c['s']).view(np.uint32), tag
        assert np.array_equal(out.view(torch.uint8).cpu().numpy(), c['want']), tag


# ----------------------------------------------------------------------------- qasr_dyn_conv_params
def test_conv_params():
    """sf and bias for C = 1, 5, 257 (C_pad to 128; tail sf = 1, bias = 0), with / without bprime and wsum128, s_x over
    exp(U(-30, 2)) and at the floor, ties of the bias.  The bias is bias_ints saturated to [INT32_MIN, INT32_MAX] - the
    positive side to INT32_MAX, whose float is the reference's 2^31 - then + wsum128 modulo 2^32."""
    lib = _lib()
    for c in D.conv_params_cases():
        s_x, s_w, bp, ws = _dev(np.array([c['s_x']], f32)), _dev(c['s_w']), _dev(c['bprime']), _dev(c['wsum128'])
        sf, bias = _filled(c['C_pad'], torch.float32), _filled(c['C_pad'], torch.int32)
        rc = lib.qasr_dyn_conv_params(engine._stream_ptr(), engine._ptr(s_x), engine._ptr(s_w), engine._ptr(bp), engine._ptr(ws),
                                      c['C'], c['C_pad'], engine._ptr(sf), engine._ptr(bias))
        tag = (c['kind'], c['C'], c['bprime'] is not None, c['wsum128'] is not None, float(c['s_x']))
        assert rc == 0
        assert np.array_equal(_bits(sf), c['sf'].view(np.uint32)), tag
        got = bias.cpu().numpy()
        bad = np.flatnonzero(got != c['bias'])
        assert bad.size == 0, (tag, bad[:4], got[bad[:4]], c['bias'][bad[:4]], c['bint'][bad[:4]])


# ----------------------------------------------------------------------------- the silent batch, end to end
_NETS = {}


def _mini():
    if not _NETS:
        cfg = topology.mini_quartznet()
        _NETS['cfg'], _NETS['sd'] = cfg, synth.make_state_dict(cfg, 21)
    return _NETS['cfg'], _NETS['sd']


def _against_oracle(x, lens, percentile, residue):
    cfg, sdn = _mini()
    net = O.OracleNet(topology.conv_plan(cfg), cfg, sdn, None, None, 8, 8, dynamic=True, percentile=percentile,
                      division_residue=residue)
    want = net.forward(x, lens)
    r = dynamic.DynamicRunner(cfg, {k: torch.from_numpy(v) for k, v in sdn.items()}, 8, 8, 'cuda:0', percentile=percentile,
                              division_residue=residue)
    r.trace = []
    out = r.forward(torch.from_numpy(x).cuda(), torch.tensor(lens))
    assert len(r.trace) == len(net.trace)
    saturated = 0
    for i, (t, w) in enumerate(zip(r.trace, net.trace)):
        assert float(t['s_x'][0]) == float(w['s_x']), (i, t['key'], 's_x', float(t['s_x'][0]), float(w['s_x']))
        codes = (t['codes'].view(torch.uint8) if t['unsigned'] else t['codes']).cpu().numpy().astype(np.int64)
        assert np.array_equal(codes, w['xint']), (i, t['key'], 'codes')
        # the oracle's accumulator is an int64: where its float32 bias clamp gave 2^31 it lies one past int32
        acc, sat = t['acc'].cpu().numpy(), np.clip(w['acc'], D.I32_MIN, D.I32_MAX)
        assert np.array_equal(acc, sat), (i, t['key'], 'acc', int(np.abs(w['acc']).max()), int(acc.max()), int(acc.min()))
        saturated += int((w['acc'] != sat).sum())
    assert np.array_equal(out['enc_len'].cpu().numpy(), want['enc_len'])
    assert np.array_equal(out['tokens'].cpu().numpy(), want['tokens'])
    return saturated, max(int(np.abs(w['acc']).max()) for w in net.trace)


@pytest.mark.parametrize('residue', [True, False])
@pytest.mark.parametrize('percentile', [None, 99.9])
@pytest.mark.parametrize('lens', [[96], [96, 40]])
def test_silent_batch_against_oracle(lens, percentile, residue):
    """All-zero features: s_x sits at the 1e-8 / n floor, s_b = s_w s_x is about 1e-13 and the 32-bit bias quantisation
    saturates; the reference clamps in float32 to n - 1, which is 2^31.  Required at every conv: s_x equal, codes equal,
    accumulator equal to the oracle's saturated to int32 (its float view is then the reference's); tokens and lengths."""
    cfg, _ = _mini()
    x = np.zeros((len(lens), cfg.feat_in, 96), f32)
    saturated, top = _against_oracle(x, lens, percentile, residue)
    assert top == 2 ** 31 and saturated > 0                   # the case is what it claims: the oracle leaves int32


@pytest.mark.parametrize('percentile', [None, 99.9])
def test_half_silent_batch_against_oracle(percentile):
    """Row 0 random, row 1 silent: the ranges come from row 0, nothing saturates."""
    cfg, _ = _mini()
    x = synth.make_features(2, cfg.feat_in, 96, 7)
    x[1] = 0
    saturated, _ = _against_oracle(x, [96, 96], percentile, True)
    assert saturated == 0


# ----------------------------------------------------------------------------- qasr_quantile2 edges
def _quantile2(x, q_lo, q_hi):
    lib = _lib()
    ws = torch.empty(lib.qasr_quantile_workspace_bytes(), dtype=torch.uint8, device='cuda:0')
    out = _filled(2, torch.float32)
    assert lib.qasr_quantile2(engine._stream_ptr(), engine._ptr(x), x.numel(), C.c_float(q_lo), C.c_float(q_hi), engine._ptr(out),
                              engine._ptr(ws), ws.numel()) == 0
    return out.cpu().numpy()


_QS = ((0.0, 1.0), (0.001, 0.999), (0.5, 0.5), (0.25, 0.75), (0.33, 0.67))


def _quantile_inputs():
    rng = np.random.default_rng(31)
    ins = {f'n{n}': rng.standard_normal(n).astype(f32) for n in (1, 2, 3, 5, 7)}
    tiny = np.float32(1.4e-45)
    ins['denormal'] = (rng.integers(-4000, 4000, 301).astype(f32) * tiny).astype(f32)
    # keys equal in the top three bytes: only pass 3 of the radix select tells them apart
    ins['low_byte'] = rng.permutation((np.uint32(0x3fc00000) + np.arange(200, dtype=np.uint32))).view(f32)
    ins['low_byte_neg'] = rng.permutation((np.uint32(0xbfc00000) + np.arange(200, dtype=np.uint32))).view(f32)
    # the four order statistics in four top-byte bins (n = 4: ranks 0, 1, 2, 3 for q = 0.33 / 0.67) ...
    ins['four_bins'] = np.array([3e20, -2e-10, -5e15, 7e-3], f32)
    # ... and in one (every key shares the top byte; n = 1001 puts the four ranks in one bin of pass 0)
    ins['one_bin'] = (f32(1.0) + rng.random(1001).astype(f32) * f32(0.5)).astype(f32)
    v = rng.standard_normal(9).astype(f32)
    v[[2, 6]] = (np.inf, -np.inf)
    ins['inf'] = v                                            # +-inf present, ranks 2 and 6 of 9 (q = 0.25 / 0.75) are finite
    return ins


def test_quantile_edges():
    for name, x in _quantile_inputs().items():
        xd = _dev(x)
        for q_lo, q_hi in _QS:
            if name == 'inf' and (q_lo, q_hi) != (0.25, 0.75):
                continue                                      # an infinity selected: inf - inf in the interpolation, not asked
            got = _quantile2(xd, q_lo, q_hi)
            want = np.array([O.quantile_f32(x, f32(q_lo)), O.quantile_f32(x, f32(q_hi))], f32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, q_lo, q_hi, got, want)


def test_quantile_signed_zeros():
    """-0.0 and +0.0 mixed: the radix select orders -0.0 below +0.0, a sort leaves them as they came; equal as floats."""
    x = np.array([0.0, -0.0, -0.0, 0.0, 1.0, -1.0, -0.0, 0.0, 2.0, -3.0, 0.0], f32)
    xd = _dev(x)
    for q_lo, q_hi in _QS:
        got = _quantile2(xd, q_lo, q_hi)
        want = np.array([O.quantile_f32(x, f32(q_lo)), O.quantile_f32(x, f32(q_hi))], f32)
        assert np.array_equal(got, want), (q_lo, q_hi, got, want)
    got = _quantile2(xd, 0.0, 1.0)
    assert got[0] == -3.0 and got[1] == 2.0


def test_quantile_rank_beyond_float24():
    """n = 16777220 > 2^24: fl32(n - 1) rounds up to n, so q = 1 asks for rank n; both ranks clamp to n - 1 and q = 1 is
    the maximum (torch.quantile refuses inputs this large: the clamp is the only sensible value)."""
    n = 16777220
    assert int(f32(n - 1)) == n
    g = torch.Generator(device='cuda:0')
    g.manual_seed(5)
    x = torch.randn(n, device='cuda:0', generator=g)
    got = _quantile2(x, 0.0, 1.0)
    want = np.array([float(x.min()), float(x.max())], f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


# ----------------------------------------------------------------------------- refusals
def _small():
    rng = np.random.default_rng(41)
    B, Cc, T, Tp = 2, 5, 70, 128
    v32 = D.make_view(rng, B, Cc, T, Tp, 'res')
    v8 = D.make_view(rng, B, Cc, T, Tp, 'i8t')
    return B, Cc, T, Tp, v32, v8


def _broken_views(v32, v8):
    """(name, view) the entry points must refuse: a residue pair on an int8 view, only one of the pair."""
    a = _DView(v32)
    both8 = _DView(v8)
    both8.s.residue_lo, both8.s.residue_hi = a.keep[2].data_ptr(), a.keep[3].data_ptr()
    only_lo, only_hi = _DView(v32), _DView(v32)
    only_lo.s.residue_hi = None
    only_hi.s.residue_lo = None
    return a, [('int8 + residue', both8), ('residue_lo only', only_lo), ('residue_hi only', only_hi)]


def test_refusals_range_and_percentile():
    lib = _lib()
    B, Cc, T, Tp, v32, v8 = _small()
    ok, broken = _broken_views(v32, v8)
    good8 = _DView(v8)
    xf = _dev(np.ones((B, Cc, T), f32))
    mm, xa = _filled(2, torch.int32), _filled(B * Cc * Tp, torch.float32)
    ws = torch.empty(lib.qasr_quantile_workspace_bytes(), dtype=torch.uint8, device='cuda:0')
    sp = engine._stream_ptr

    def rng_(a, b, x, Tx, T_, Tp_):
        return lib.qasr_dyn_range(sp(), _DView.ref(a), _DView.ref(b), engine._ptr(x), Tx, None, 0, B, Cc, T_, Tp_, engine._ptr(mm))

    def pct(a, b, x, Tx, T_, Tp_, q_lo=0.01, q_hi=0.99, wsb=None):
        return lib.qasr_dyn_range_percentile(sp(), _DView.ref(a), _DView.ref(b), engine._ptr(x), Tx, None, 0, B, Cc, T_, Tp_,
                                             C.c_float(q_lo), C.c_float(q_hi), engine._ptr(xa), engine._ptr(ws),
                                             ws.numel() if wsb is None else wsb, engine._ptr(mm))

    for f in (rng_, pct):
        assert f(ok, None, None, 0, Tp + 1, Tp) == ERR_ARG, 'T > Tp'
        assert f(None, None, xf, T, T + 1, Tp) == ERR_ARG, 'T > Tx'
        for name, v in broken:
            assert f(v, None, None, 0, T, Tp) == ERR_ARG, name
            assert f(good8, v, None, 0, T, Tp) == ERR_ARG, name + ' (operand b)'
    assert pct(ok, None, None, 0, T, Tp, q_lo=-0.1) == ERR_ARG
    assert pct(ok, None, None, 0, T, Tp, q_hi=1.5) == ERR_ARG
    assert pct(ok, None, None, 0, T, Tp, wsb=ws.numel() - 1) == ERR_ARG
    assert _untouched(mm, xa)
    assert rng_(ok, good8, None, 0, T, Tp) == 0 and pct(ok, good8, None, 0, T, Tp) == 0   # the same calls, unbroken, run


def test_refusals_requant_and_quant_in():
    lib = _lib()
    B, Cc, T, Tp, v32, v8 = _small()
    ok, broken = _broken_views(v32, v8)
    good8 = _DView(v8)
    M = _dev(np.full(Cc, 0.5))
    out, s = _filled((B, Cc, Tp), torch.int8), _filled(1, torch.float32)
    sp = engine._stream_ptr

    def rq(a=ok, b=None, B_=B, C_=Cc, T_=T, Tp_=Tp, lo=-128, hi=127):
        return lib.qasr_dyn_requant(sp(), _DView.ref(a), engine._ptr(M), _DView.ref(b), engine._ptr(M) if b is not None else None,
                                    None, 0, B_, C_, T_, Tp_, lo, hi, engine._ptr(out))

    assert rq(T_=Tp + 1) == ERR_ARG
    for name, v in broken:
        assert rq(a=v) == ERR_ARG, name
        assert rq(b=v) == ERR_ARG, name + ' (operand b)'
    assert rq(lo=5, hi=4) == ERR_ARG and rq(lo=-128, hi=128) == ERR_ARG and rq(lo=-256, hi=0) == ERR_ARG
    assert rq(B_=0) == ERR_ARG and rq(C_=0) == ERR_ARG and rq(T_=-1) == ERR_ARG and rq(B_=-2) == ERR_ARG

    x = _dev(np.ones((B, Cc, T), f32))
    lens = _dev(np.array([T, 3], np.int32))
    mm = _dev(np.array([D.ord32(-1.0), D.ord32(1.0)], np.uint32).view(np.int32))

    def qi(bits=8, B_=B, C_=Cc, T_=T, Tx=T, Tp_=Tp):
        return lib.qasr_dyn_quant_in(sp(), engine._ptr(x), Tx, engine._ptr(mm), engine._ptr(lens), bits, B_, C_, T_, Tp_,
                                     engine._ptr(s), engine._ptr(out))

    assert qi(T_=Tp + 1, Tx=Tp + 1) == ERR_ARG and qi(T_=T, Tx=T - 1) == ERR_ARG
    assert qi(bits=1) == ERR_ARG and qi(bits=9) == ERR_ARG
    assert qi(B_=0) == ERR_ARG and qi(C_=0) == ERR_ARG and qi(T_=-1) == ERR_ARG
    assert _untouched(out, s)
    assert rq(b=good8) == 0 and qi() == 0


def test_refusals_params_residue_codes_and_quantile():
    lib = _lib()
    sp = engine._stream_ptr
    Cc = 5
    mm = _dev(np.array([D.ord32(-1.0), D.ord32(1.0)], np.uint32).view(np.int32))
    sa = _dev(np.ones(Cc, f32))
    s, Ma = _filled(1, torch.float32), _filled(Cc, torch.float64)
    for bits in (1, 17, 0, -3):
        assert lib.qasr_dyn_act_params(sp(), engine._ptr(mm), bits, Cc, engine._ptr(sa), 1, None, 0, engine._ptr(s), engine._ptr(Ma),
                                       None) == ERR_ARG, bits
    assert lib.qasr_dyn_act_params(sp(), engine._ptr(mm), 8, 0, engine._ptr(sa), 1, None, 0, engine._ptr(s), engine._ptr(Ma), None) == ERR_ARG
    sf, bias = _filled(128, torch.float32), _filled(128, torch.int32)
    s_x = _dev(np.ones(1, f32))
    assert lib.qasr_dyn_conv_params(sp(), engine._ptr(s_x), engine._ptr(sa), None, None, Cc, Cc - 1, engine._ptr(sf),
                                    engine._ptr(bias)) == ERR_ARG
    assert lib.qasr_dyn_conv_params(sp(), engine._ptr(s_x), engine._ptr(sa), None, None, 0, 128, engine._ptr(sf), engine._ptr(bias)) == ERR_ARG
    assert _untouched(s, Ma, sf, bias)

    codes = _dev(np.arange(64, dtype=np.int8))
    lo, hi = _filled(64, torch.int8), _filled(64, torch.int8)

    def rc_(n=64, dc=0, dl=0, dh=0):
        return lib.qasr_dyn_residue_codes(sp(), C.c_void_p(codes.data_ptr() + dc), 0, engine._ptr(s_x), n, C.c_void_p(lo.data_ptr() + dl),
                                          C.c_void_p(hi.data_ptr() + dh))

    assert rc_(n=24) == ERR_ARG and rc_(n=0) == ERR_ARG
    assert rc_(n=32, dc=8) == ERR_ARG and rc_(n=32, dl=4) == ERR_ARG and rc_(n=32, dh=1) == ERR_ARG
    assert _untouched(lo, hi)
    assert rc_() == 0

    x = _dev(np.arange(40, dtype=f32))
    out = _filled(2, torch.float32)
    ws = torch.empty(lib.qasr_quantile_workspace_bytes(), dtype=torch.uint8, device='cuda:0')

    def q2(q_lo=0.1, q_hi=0.9, wsb=ws.numel(), n=40):
        return lib.qasr_quantile2(sp(), engine._ptr(x), n, C.c_float(q_lo), C.c_float(q_hi), engine._ptr(out), engine._ptr(ws), wsb)

    assert q2(q_lo=-0.01) == ERR_ARG and q2(q_hi=1.01) == ERR_ARG and q2(q_lo=float('nan')) == ERR_ARG
    assert q2(wsb=ws.numel() - 1) == ERR_ARG and q2(n=0) == ERR_ARG
    assert _untouched(out)
    assert q2() == 0
