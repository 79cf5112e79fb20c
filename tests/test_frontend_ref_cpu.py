"""The front-end's float64 reference (tests/frontend_ref.py) checked on the CPU before tests/test_gpu_frontend.py relies on
it: it agrees with the committed fixture of the reference's own module, the float32 restatement of the kernel sits within
BOUND / 4 of it over every case the GPU tests run, the faults a front-end kernel can have push a named case above BOUND,
and the NumPy packing of the plan workspace is the dense projection term for term."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frontend_ref as fr  # noqa: E402


def _case_errors(case, fault=None):
    """(max raw log-mel error, max scaled normalised error) of emu32 against ref64 over the rows of a case"""
    fb, w = fr.bank(case.fb_name), fr.window(case.win_name)
    raw = nrm = 0.0
    for b, ref in enumerate(fr.case_refs(case)):
        e = fr.emu32(case.audio[b], case.lens[b], case.preemph, w, fb, fault)
        assert e.n == ref.n
        raw = max(raw, fr.err_raw(e.lm, ref))
        if ref.n >= 2:
            nrm = max(nrm, fr.err_norm(e.norm, ref))
            if fault is None:
                fr.check_row(e.norm, ref.n, ref, ref.lm.shape[1])      # zeros behind n, exact zeros on silent rows
    return raw, nrm


def test_ref64_agrees_with_the_reference_fixture(golden_dir):
    """frontend.npz holds FilterbankFeatures.forward of the reference in float32.  An exact spectrum followed by its float32
    steps is 5.5e-5 max / 4e-7 mean from it (the figure in the header of qasr_frontend.hip: the fixture's own float32 FFT
    noise), so ref64 must be within 6e-5 max and 1e-6 mean; measured 5.46e-5 and 6.0e-7 (worst row)."""
    d = np.load(os.path.join(golden_dir, 'frontend.npz'))
    B, M, T_pad = d['feats'].shape
    for b in range(B):
        ref = fr.ref64(d['audio'][b], d['lens'][b], 0.97, d['window'], d['fb'])
        assert ref.n == d['seq_len'][b]
        T = ref.norm.shape[1]
        err = np.abs(ref.norm - d['feats'][b, :, :T])
        print(f'row {b}: max {err.max():.3e} mean {err.mean():.3e}')
        assert err.max() <= 6e-5 and err.mean() <= 1e-6, (b, err.max(), err.mean())
        assert np.all(ref.norm[:, ref.n:] == 0) and np.all(d['feats'][b, :, ref.n:] == 0)
        assert T_pad == fr.frames_pad(d['audio'].shape[1], 16)


def test_noise_floor():
    """emu32 against ref64 over every case of (a) - (f): the distance a correct float32 front-end keeps from float64, in
    log-mel units.  Measured 2.36e-6 (e_long_S163679, normalised; raw log-mel at most 1.12e-6): FLOOR, and BOUND = 1e-5
    is four times that rounded up to one digit."""
    worst = (0.0, None)
    for case in fr.all_cases():
        raw, nrm = _case_errors(case)
        print(f'{case.name:28s} raw {raw:.3e} normalised {nrm:.3e}')
        worst = max(worst, (raw, case.name), (nrm, case.name))
    print('floor', worst)
    assert worst[0] <= fr.BOUND / 4, worst
    assert worst[0] <= fr.FLOOR * 1.05, ('frontend_ref.FLOOR is out of date', worst)
    assert 4 * fr.FLOOR <= fr.BOUND <= 2e-5


# fault -> the case that catches it (figure measured with emu32, log-mel units)
CATCHERS = {
    'fft32':           'b_bank_slaney128_8000',        # 6.0e-4 (narrow filters on a wide dynamic range; broad ones average it out)
    'window_reversed': 'c_random_window',              # 4.2; a symmetric window cannot see it
    'reflect_lo':      'd_lengths_S2560',              # 5.0
    'reflect_hi':      'a_signals_len4005',            # 7.6
    'run_lo':          'b_bank_slaney64_300_3400',     # 3.9
    'run_hi':          'b_bank_slaney65_8000',         # 0.79
    'twiddle':         'c_hamming',                    # 1.7e-5: see the docstring
}


@pytest.mark.parametrize('fault', fr.FAULTS)
def test_fault_is_caught(fault):
    """Each fault switched on in emu32 pushes the named case above BOUND.  The wrong twiddle - bin 64 off by 1e-7 relative,
    the last three bits of a float32 - is the resolution limit: it reaches 1.7e-5 on c_hamming, where X[64] is small against
    its odd half so that the relative error is amplified, and stays at or below 6.8e-6, under BOUND, on every other case;
    BOUND was not tuned to catch it."""
    case = {c.name: c for c in fr.all_cases()}[CATCHERS[fault]]
    raw, nrm = _case_errors(case, fault)
    print(f'{fault}: {case.name} raw {raw:.3e} normalised {nrm:.3e}')
    assert max(raw, nrm) > fr.BOUND, (fault, case.name, raw, nrm)


@pytest.mark.parametrize('name', list(fr.BANKS))
def test_plan_packing(name):
    """The packed table is the dense product term for term: the float32 fma chain over each run, read through offs, equals
    the chain over all 257 bins (skipped terms are fma(0, P, acc) = acc); runs are padded with zeros to a multiple of four
    and lie back to back; the table length and the LDS / global-memory path are the ones the issue's table states."""
    fb = fr.bank(name)
    length, path, passes = fr.BANKS[name]
    p = fr.pack_plan(fb)
    M = fb.shape[0]
    assert p.hdr.tolist() == [fr.MEL_MAGIC, M, p.total if p.fits else fr.MEL_FBMAX + 1, 0]
    assert p.fits == (path == 'lds') and (length is None or p.total == length), (p.fits, p.total)
    assert passes == -(-M // 64) and (M <= 64 or name.startswith('slaney'))
    assert np.all(p.offs % 4 == 0) and np.all(p.ranges[:, 0] <= p.ranges[:, 1]) and p.ranges.max() <= fr.NBIN
    if not p.fits:
        assert M > fr.MEL_MAXM or p.total > fr.MEL_FBMAX
        assert not p.table.any()
        return
    P = np.random.default_rng(5).uniform(0.0, 3.0, (fr.NBIN, 6)).astype(np.float32)
    dense = np.zeros((M, P.shape[1]), np.float32)
    for k in range(fr.NBIN):
        dense = fr._fma32(fb[:, k:k + 1], P[None, k], dense)
    used = np.zeros(fr.MEL_FBMAX, bool)
    for m, (lo, hi) in enumerate(p.ranges):
        acc = np.zeros(P.shape[1], np.float32)
        for k in range(lo, hi):
            acc = fr._fma32(p.table[p.offs[m] + k - lo], P[k], acc)
        assert acc.tobytes() == dense[m].tobytes(), m
        n4 = (hi - lo + 3) & ~3
        assert not used[p.offs[m]:p.offs[m] + n4].any() and not p.table[p.offs[m] + hi - lo:p.offs[m] + n4].any()
        used[p.offs[m]:p.offs[m] + n4] = True
    assert used[:p.total].all() and not used[p.total:].any() and not p.table[p.total:].any()


def test_twiddle_reference_and_plan_split():
    """twiddles_exact against numpy's float64 cos / sin (a plausibility check of the octant symmetry: numpy's own argument
    is rounded), exact on the axes, on the unit circle; and split_plan against a workspace laid out by hand"""
    tw = fr.twiddles_exact()
    k = np.arange(fr.NFFT)
    want = np.stack([np.cos(2 * np.pi * k / fr.NFFT), -np.sin(2 * np.pi * k / fr.NFFT)], 1)
    assert np.abs(tw - want).max() <= 2e-15                    # (the rounded angle 2 pi k / 512 alone costs numpy 7e-16)
    assert np.all(np.abs(tw[:, 0] ** 2 + tw[:, 1] ** 2 - 1) <= 4.5e-16)
    assert tw[0].tolist() == [1, 0] and tw[128].tolist() == [0, -1] and tw[256].tolist() == [-1, 0] and tw[384].tolist() == [0, 1]
    p = fr.pack_plan(fr.bank('hand3_edges'))
    M = 5
    head = np.concatenate([p.hdr, p.ranges.ravel(), p.offs]).astype(np.int32).tobytes()
    head += b'\0' * (-len(head) % 16)
    ws = np.frombuffer(head + p.table.tobytes() + tw.tobytes(), np.uint8)
    hdr, ranges, offs, table, tw2 = fr.split_plan(ws, M)
    assert (hdr.tolist(), ranges.tolist(), offs.tolist()) == (p.hdr.tolist(), p.ranges.tolist(), p.offs.tolist())
    assert table.tobytes() == p.table.tobytes() and tw2.tobytes() == tw.tobytes()
