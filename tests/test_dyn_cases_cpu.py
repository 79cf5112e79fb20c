"""tests/dyn_cases.py on the CPU: (a) its restatements of the qasr_dyn_* entry points, chained as DynamicRunner chains the
kernels, reproduce OracleNet(dynamic=True)'s own trace exactly; (b) its case lists hold the edges they claim - counted on
the inputs with the reference alone, so a GPU run that passes has met them."""
import numpy as np
import pytest

import dyn_cases as D
from oracle import int_oracle as O
from qasr import synth, topology

f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------- (a) anchoring
def _residue_pair(tr, s):
    """The residue accumulators of conv `tr` as the runner carries them: sum(w residue(q)) in units of 2^-24, lo + 128 hi."""
    r = O.conv1d_f64(O.division_residue(tr['xint'], tr['s_x']), tr['wint'], s.stride, s.padding, s.dilation, s.groups)
    R = np.rint(r * 2.0 ** 24)
    assert np.array_equal(R, r * 2.0 ** 24)                   # a multiple of 2^-24, exactly
    R = R.astype(np.int64)
    hi = R // 128
    return (R - 128 * hi).astype(np.int32), hi.astype(np.int32)


@pytest.mark.parametrize('percentile', [None, 99.9])
@pytest.mark.parametrize('residue', [False, True])
def test_restatements_replay_oracle_trace(percentile, residue):
    cfg = topology.mini_quartznet()
    plan = topology.conv_plan(cfg)
    sd = synth.make_state_dict(cfg, 21)
    B, T0 = 2, 96
    lens0 = np.array([96, 50], np.int64)
    net = O.OracleNet(plan, cfg, sd, None, None, 8, 8, dynamic=True, percentile=percentile, division_residue=residue)
    net.forward(synth.make_features(B, cfg.feat_in, T0, 5), lens0)
    ti, lens, chains = 0, lens0, 0
    for sites in plan:
        msites = [s for s in sites if s.role != 'res']
        cur = lens
        for j, s in enumerate(msites):
            tr = net.trace[ti + j]
            assert tr['key'] == s.key
            # conv_params: s_b and the bias integers from s_x, the weight scales and the folded float bias
            w, b = net._site_weights(s)
            _, s_w = O.weight_ints(w, 8)
            sf, bias, _ = D.ref_conv_params(tr['s_x'], s_w, b, None, D.rup(s.cout, 128))
            assert np.array_equal(sf[:s.cout], tr['s_b']) and np.all(sf[s.cout:] == 1) and not bias[s.cout:].any()
            assert np.array_equal(bias[:s.cout], np.zeros(s.cout) if tr['bint'] is None else tr['bint'])
            cur = (cur + 2 * s.padding - s.dilation * (s.kernel - 1) - 1) // s.stride + 1
            if j + 1 == len(msites):
                break
            # conv j -> QuantAct -> conv j + 1: range -> act_params -> requant on (acc_j, s_b_j) gives xint_{j+1}, s_x_{j+1}
            nxt, ns = net.trace[ti + j + 1], msites[j + 1]
            acc = tr['acc']
            T = acc.shape[2]
            Tp = D.rup(T, 64)
            pad = lambda v: D._padded(v.astype(np.int32), Tp, np.int32(D.I32_MAX))
            a = D.View(pad(acc), tr['s_b'], True, tuple(pad(r) for r in _residue_pair(tr, s)) if residue else None)
            x_act = D.ref_x_act(a, None, None, cur, int(s.relu_after), T)
            if percentile is None:
                mn, mx = x_act.min(), x_act.max()
            else:
                mn, mx = O.quantile_f32(x_act, f32(1 - percentile / 100)), O.quantile_f32(x_act, f32(percentile / 100))
            bits = 8 + int(ns.asymmetric)
            s_out, Ma, _ = D.ref_act_params(mn, mx, bits, s.cout, tr['s_b'], None)
            assert s_out == nxt['s_x'], (ti + j, s.key)
            n = 2 ** (bits - 1) - 1
            codes = D.ref_requant(a, Ma, None, None, cur, int(s.relu_after), T, Tp, 0 if ns.asymmetric else -n - 1, n)
            assert np.array_equal(codes[:, :, :T], (nxt['xint'] & 0xff).astype(np.uint8)), (ti + j, s.key)
            assert not codes[:, :, T:].any()
            # and with the oracle's own (m, e) form of the multiplier
            q, _ = O.fixedpoint_requant(x_act, tr['s_b'], s_out)
            assert np.array_equal(O.mask_time(O.act_clamp(q, bits), cur), nxt['xint'])
            chains += 1
        ti += len(sites)
        lens = cur
    assert chains >= 9                                        # dw -> pw and pw -> dw of every block


def test_first_layer_restatement_replays_oracle_trace():
    cfg = topology.mini_quartznet()
    sd = synth.make_state_dict(cfg, 21)
    x = synth.make_features(2, cfg.feat_in, 96, 5)
    lens = np.array([96, 50])
    net = O.OracleNet(topology.conv_plan(cfg), cfg, sd, None, None, 8, 8, dynamic=True)
    net.forward(x, lens)
    xa = D.ref_x_act(None, None, x, lens, 0, 96)
    s, codes = D.ref_quant_in(x, xa.min(), xa.max(), lens, 8, 96, 128)
    assert s == net.trace[0]['s_x']
    assert np.array_equal(codes[:, :, :96], (net.trace[0]['xint'] & 0xff).astype(np.uint8))


# ----------------------------------------------------------------------------- (b) the edges are there
@pytest.fixture(scope='module')
def requant():
    return D.requant_cases()


def _sum_before_clamp(c):
    ops = [D.ref_operand(c['a'], c['Ma'], c['relu'], c['T'])]
    if c['b'] is not None:
        ops.append(D.ref_operand(c['b'], c['Mb'], False, c['T']))
    keep = np.ones((c['B'], 1, c['T']), bool)
    if c['lens'] is not None:
        keep = (np.arange(c['T'])[None, :] < np.minimum(c['lens'], c['T'])[:, None])[:, None, :]
    return ops, sum(o[0] for o in ops), keep


def test_requant_cases_hold_ties_and_both_clamps(requant):
    down = up = 0
    at_lo, at_hi = {k: 0 for k in D.CLAMPS}, {k: 0 for k in D.CLAMPS}
    for c in requant:
        ops, q, keep = _sum_before_clamp(c)
        for out, _, prod in ops:
            tie = (prod - np.floor(prod) == 0.5) & keep
            down += int((tie & (out == np.floor(prod))).sum())   # half to even went down: half-up / half-away fail here
            up += int((tie & (out == np.ceil(prod))).sum())      # ... went up: truncation / half-down fail here
        at_lo[(c['lo'], c['hi'])] += int(((q < c['lo']) & keep).sum())
        at_hi[(c['lo'], c['hi'])] += int(((q > c['hi']) & keep).sum())
    assert down >= 1000 and up >= 1000, (down, up)
    assert all(v >= 100 for v in at_lo.values()) and all(v >= 100 for v in at_hi.values()), (at_lo, at_hi)
    assert {(c['lo'], c['hi']) for c in requant} == set(D.CLAMPS)
    assert {c['kind'] for c in requant} == {'tie', 'big', 'res', 'two'}


def test_requant_cases_hold_rounding_accumulators_and_residues(requant):
    rounds = extreme = nonzero = 0
    for c in requant:
        a, T = c['a'], c['T']
        z = a.data[:, :, :T].astype(np.int64)
        if c['kind'] == 'big':
            rounds += int((z.astype(f32).astype(f64) != z).sum())       # (float)acc is not acc: |acc| >= 2^24
            extreme += int((z == D.I32_MAX).sum()) + int((z == D.I32_MIN).sum())
        if a.residue is not None:
            nonzero += int((a.floats(T) != O.float_view(z, a.scales())).sum())   # the residue moves the float view
    assert rounds >= 10000 and extreme >= 2 and nonzero >= 1000, (rounds, extreme, nonzero)


def test_range_cases_hold_fma_mask_and_sign_edges():
    fma = mask_min = rounds = nonzero = 0
    lens_seen, signs = set(), set()
    for kind in D.KINDS:
        for c in D.range_cases(kind):
            T = c['T']
            signs.add((kind, c['sign']))
            if c['lens'] is not None:
                for v in c['lens']:
                    lens_seen.add('0' if v == 0 else '1' if v == 1 else 'T' if v == T else '>T' if v > T else 'mid')
                raw = D.ref_x_act(c['a'], c['b'], c['xf'], None, c['relu'], T)
                mask_min += int(raw.min() > 0 and c['want'][0] == D.ord32(0.0))   # the minimum is a mask zero only
            if kind == 'sum':                                 # fma(z, s, identity) against fl32(fl32(z s) + identity)
                a, b = c['a'], c['b']
                zf = a.data[:, :, :T].astype(f32).astype(f64)
                fused = (zf * a.scales().astype(f64).reshape(1, -1, 1) + b.floats(T).astype(f64)).astype(f32)
                fma += int((fused != (b.floats(T) + a.floats(T)).astype(f32)).sum())
            if kind == 'i32c':
                z = c['a'].data[:, :, :T].astype(np.int64)
                rounds += int((z.astype(f32).astype(f64) != z).sum())
            if kind == 'res':
                z = c['a'].data[:, :, :T].astype(np.int64)
                nonzero += int((c['a'].floats(T) != O.float_view(z, c['a'].scales())).sum())
    assert lens_seen >= {'0', '1', 'T', '>T'}
    assert signs == {(k, s) for k in D.KINDS for s in D.SIGNS}
    assert fma >= 10000 and mask_min >= 10 and rounds >= 30 and nonzero >= 10000, (fma, mask_min, rounds, nonzero)
    for c in D.negzero_cases():
        x = c['x_act']
        assert (x == 0).sum() == 1 and np.signbit(x[x == 0]).all() and 0x7fffffff in c['want']


def test_percentile_cases_cover_the_scalar_tail():
    ns = {c['B'] * c['C'] * c['T'] for c in D.percentile_cases('i32c')}
    assert {1, 2, 3, 5} <= ns
    assert any(n > 4 and n % 4 == 1 for n in ns) and any(n > 4 and n % 4 == 3 for n in ns)


def test_quant_in_cases_hold_ties_and_the_asymmetric_clamp():
    ties = top = bottom = zero = 0
    for c in D.quant_in_cases():
        n = 2 ** (c['bits'] - 1) - 1
        T = c['T']
        keep = (np.arange(T)[None, :] < np.minimum(c['lens'], T)[:, None])[:, None, :] & np.ones((1, c['C'], 1), bool)
        x = c['x'][:, :, :T]
        v = ((f32(1) / c['s']).astype(f32) * x).astype(f32)
        ties += int(((v - np.floor(v) == 0.5) & (np.abs(v) < n - 1) & keep).sum())
        is_max = (x == max(abs(c['mn']), abs(c['mx']))) & keep & (c['mx'] > 0)
        top += int(is_max.sum())
        assert (c['want'][:, :, :T][is_max] == n - 1).all()   # +max -> n - 1, not n
        bottom += int((c['want'][:, :, :T].astype(np.int8)[keep] == -n).sum())
        if c['kind'] == 'zero':
            zero += 1
            assert c['s'] == f32(1e-8) / f32(n) and not c['want'].any()
        assert c['Tx'] != c['Tp']
    assert ties >= 1000 and top >= 5 and bottom >= 100 and zero >= 4, (ties, top, bottom, zero)


def test_conv_params_cases_hold_saturation_ties_and_wide_sums():
    pos = neg = ties = near = 0
    for c in D.conv_params_cases():
        pos += int((c['bint'] == 2 ** 31).sum())              # the float32 clamp to n - 1 rounds to 2^31: outside int32
        neg += int((c['bint'] == -2 ** 31).sum())
        if c['bprime'] is not None:
            s_b = (c['s_w'] * c['s_x']).astype(f32)
            v = ((f32(1) / s_b).astype(f32) * c['bprime']).astype(f32)
            ties += int(((v - np.floor(v) == 0.5) & (np.abs(v) < 2 ** 23)).sum())
        if c['wsum128'] is not None:
            w = c['wsum128'].astype(np.int64)
            near += int((w > 2 ** 22 - 1000).any()) + int((w < -2 ** 22 + 1000).any())
    assert pos >= 6 and neg >= 6 and ties >= 500 and near >= 20, (pos, neg, ties, near)
    assert {c['C'] for c in D.conv_params_cases()} == {1, 5, 257}


def test_act_params_cases_cover_bits_operands_and_the_floor():
    cs = D.act_params_cases()
    assert {c['bits'] for c in cs} == {6, 7, 8, 9} and {c['C'] for c in cs} == {1, 5, 257}
    assert {(c['sb'] is not None, c['b_pc']) for c in cs} == {(False, False), (True, True), (True, False)}
    floor = [c for c in cs if c['mn'] == 0 and c['mx'] == 0]
    assert len(floor) >= 6 and all(c['s'] == f32(1e-8) / f32(2 ** (c['bits'] - 1) - 1) for c in floor)
    assert max(c['Ma'].max() for c in floor) >= 2.0 ** 30     # multipliers of 2^30 and more at the floor
