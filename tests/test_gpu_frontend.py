"""The mel front-end on an MI355X (k_melrange, k_melpack, k_twiddle, k_mel, k_norm in csrc/qasr_frontend.hip) against the float64
reference of tests/frontend_ref.py: signals other than white noise, filterbanks on every path of the projection (one and
several m0 passes, the LDS table exactly full and one run past it, the global-memory projection), windows that are not
symmetric, sample counts from the 257-sample minimum, pad_to 0 / 5 / 16, lengths from 0, both paths of k_norm, and k_mel's raw
log-mel through the engine.  Every case: the metric of frontend_ref (log-mel units) <= BOUND on the valid frames, exact zeros
behind them and in the padding, the reference's feature lengths, the padded shape.  Each test prints the maximum it reached."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frontend_ref as fr  # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _mel(case, pad_to, plan=None):
    from qasr import engine
    fb = torch.from_numpy(fr.bank(case.fb_name)).cuda().contiguous()
    y, flen = engine.frontend_mel(torch.from_numpy(case.audio).cuda(), torch.tensor(case.lens, dtype=torch.int32).cuda(), fb,
                                  torch.from_numpy(fr.window(case.win_name)).cuda(), case.preemph, pad_to,
                                  plan=engine.frontend_plan(fb) if plan is None else plan)
    torch.cuda.synchronize()
    return y.cpu().numpy(), flen.cpu().numpy()


def _check(case, pad_to=16, plan=None):
    """One call of the front-end on a case, every assertion of the module docstring on every row; -> the maximum metric"""
    from qasr import engine
    y, flen = _mel(case, pad_to, plan)
    refs = fr.case_refs(case)
    B, S = case.audio.shape
    T_pad = engine.load_library().qasr_frontend_frames(S, pad_to)
    assert T_pad == fr.frames_pad(S, pad_to)
    assert y.shape == (B, refs[0].lm.shape[0], T_pad) and y.dtype == np.float32
    assert flen.tolist() == [r.n for r in refs]
    errs = [fr.err_norm(y[b], r) if r.n >= 2 else 0.0 for b, r in enumerate(refs)]
    print(f'{case.name} pad_to {pad_to}: max {max(errs):.3e} per row ' + ' '.join(f'{e:.2e}' for e in errs))
    for b, r in enumerate(refs):
        fr.check_row(y[b], flen[b], r, T_pad)
    return max(errs)


@pytest.mark.parametrize('case', fr.cases_signals(), ids=lambda c: c.name)
def test_signals(case):
    """(a) noise, a tone on a bin and one between bins, 1e-4 and PCM-scale noise, noise that stops, an impulse, DC, a chirp
    and silence in one batch; all lengths S, then all 2500."""
    assert fr.window('hann').tobytes() == torch.hann_window(320, periodic=False).numpy().tobytes()
    assert case.audio.shape == (len(fr.SIGNAL_NAMES), fr.S0) and fr.n_frames(fr.S0) == 26
    _check(case)


@pytest.mark.parametrize('case', fr.cases_banks(), ids=lambda c: c.name)
def test_banks(case):
    """(b) the plan of each bank says which projection k_mel takes - read it back: header, runs, and where the table fits the
    offsets and the packed weights, byte for byte the NumPy packing - and the features follow the reference on that path."""
    from qasr import engine
    fb = fr.bank(case.fb_name)
    length, path, _ = fr.BANKS[case.fb_name]
    plan = engine.frontend_plan(torch.from_numpy(fb).cuda().contiguous())
    torch.cuda.synchronize()
    hdr, ranges, offs, table, _ = fr.split_plan(plan.cpu().numpy(), fb.shape[0])
    want = fr.pack_plan(fb)
    assert hdr.tolist() == want.hdr.tolist(), (hdr, want.hdr)
    assert (hdr[2] <= fr.MEL_FBMAX) == (path == 'lds') and (length is None or want.total == length)
    assert ranges.tobytes() == want.ranges.tobytes()
    if want.fits:
        assert offs.tobytes() == want.offs.tobytes() and table.tobytes() == want.table.tobytes()
    _check(case, plan=plan)


def test_twiddles():
    """k_twiddle: tw[k] within 2 ulp of (cos, sin)(-2 pi k / 512) evaluated in higher precision, exact on the axes"""
    from qasr import engine
    plan = engine.frontend_plan(torch.from_numpy(fr.bank('slaney64_8000')).cuda().contiguous())
    torch.cuda.synchronize()
    tw = fr.split_plan(plan.cpu().numpy(), 64)[4]
    want = fr.twiddles_exact()
    ulps = np.abs(tw - want) / np.where(want == 0, 1.0, np.spacing(np.abs(want)))
    print(f'twiddles: max {ulps[want != 0].max():.2f} ulp')
    assert np.all(tw[want == 0] == 0) and ulps.max() <= 2, ulps.max()


@pytest.mark.parametrize('case', fr.cases_window(), ids=lambda c: c.name)
def test_window_and_preemphasis(case):
    """(c) a hamming window, a random positive window without symmetry (a reversed or shifted window index shows only
    there), pre-emphasis 0 and 1."""
    _check(case)


@pytest.mark.parametrize('pad_to', fr.PAD_TOS)
@pytest.mark.parametrize('S', fr.LENGTH_S)
def test_lengths(S, pad_to):
    """(d) one row per length 0, 1, 160, 161, 320, S - 1, S (those <= S), non-zero noise behind every length.  Length 0: all
    zeros, feature length 0.  Lengths 1 - 160: one valid frame, whose unbiased std is NaN in the reference: frame 0 is NaN and
    everything else zero (check_row).  S = 2560 at full length computes 17 frames of which 16 are valid."""
    case = fr.case_lengths(S)
    assert {0, 1, S - 1, S} <= set(case.lens) and (S < 320 or {160, 161, 320} <= set(case.lens))
    _check(case, pad_to)


def test_fewer_samples_than_the_reflect_padding_are_refused():
    from qasr import engine
    a = torch.from_numpy(fr.noise(256, 1, 0.1)[None]).cuda()
    fb = torch.from_numpy(fr.bank('slaney64_8000')).cuda()
    with pytest.raises(engine.QasrError):
        engine.frontend_mel(a, torch.tensor([256], dtype=torch.int32).cuda(), fb, torch.from_numpy(fr.window('hann')).cuda())


@pytest.mark.parametrize('S', fr.LONG_S)
def test_long_rows(S):
    """(e) T_pad = 1024, the last row k_norm keeps in registers, and 1040, the first it walks in a loop; lengths S and
    S - 20000."""
    assert fr.frames_pad(S, 16) == {163679: 1024, 164003: 1040}[S]
    _check(fr.case_long(S))


def test_raw_log_mel_of_the_fused_engine(golden_dir):
    """(f) forward_audio of a QuartzNet15x5 engine with fuse_norm leaves k_mel's un-normalised log-mel in the caller's `feats`
    (k_norm is not launched; k_stem normalises): |lm - lm_ref| <= BOUND on every computed frame, whatever the row's length,
    and nothing written behind them - the buffer is zeroed before the call and the padding must still be zero.  A k_mel fault
    shows here and in (a) - (e), a k_norm fault only there."""
    from qasr import engine, melbank, pack, synth, topology
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    sd = synth.make_state_dict(cfg, meta['seed'])
    blob, _ = pack.pack_model(cfg, sd, d['act_min'], d['act_max'], 8, 8)
    fb = torch.from_numpy(melbank.mel_filterbank(16000, 512, 64, 0.0, 8000.0).astype(np.float32)).cuda().contiguous()
    win = torch.hann_window(320, periodic=False).cuda()
    case = fr.case_raw()
    assert fb.cpu().numpy().tobytes() == fr.bank(case.fb_name).tobytes() and win.cpu().numpy().tobytes() == fr.window('hann').tobytes()
    B, S = case.audio.shape
    eng = engine.Engine(blob, 0, graph=False, fuse_norm=True)
    assert eng.opts.fuse_norm == 1
    T_pad, T = eng.lib.qasr_frontend_frames(S, 16), fr.n_frames(S)
    fbuf = torch.zeros(B, 64, T_pad, device='cuda')
    lbuf = torch.empty(B, dtype=torch.int32, device='cuda')
    eng.forward_audio(torch.from_numpy(case.audio).cuda(), torch.tensor(case.lens, dtype=torch.int32).cuda(), fb, win,
                      engine.frontend_plan(fb), 0.97, 16, feats=fbuf, feat_lens=lbuf)
    torch.cuda.synchronize()
    lm = fbuf.cpu().numpy()
    eng.close()
    refs = fr.case_refs(case)
    assert lbuf.cpu().tolist() == [r.n for r in refs]
    errs = [fr.err_raw(lm[b], r, T) for b, r in enumerate(refs)]
    print(f'{case.name}: raw log-mel max {max(errs):.3e} per row ' + ' '.join(f'{e:.2e}' for e in errs))
    assert np.all(lm[:, :, T:] == 0)
    assert max(errs) <= fr.BOUND, errs
