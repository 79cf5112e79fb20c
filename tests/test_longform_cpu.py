"""qasr.longform without a GPU: the plan's arithmetic and refusals, cut_host against slicing, the slice property of
stitch_host, the seam rule on hand-made overlaps, structure on windows that disagree everywhere, decode_long on the host
modules and the argument refusals of the two entry points through the binding (nothing is launched)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import longform_cases as lc  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import ctc, longform as lf, synth  # noqa: E402


def test_plan_arithmetic_at_every_edge():
    Wf, Of = 8, 3
    Wl, Ov, H = Wf * lc.SPF, Of * lc.SPF, (Wf - Of) * lc.SPF
    cases = {1: 1, Wl - 1: 1, Wl: 1, Wl + 1: 2, Wl + H: 2, Wl + H + 1: 3, Wl + 7 * H - 5: 8}
    p = lc.plan_frames(list(cases), Wf, Of, 1)
    assert (p.Wl, p.Ov, p.H, p.guard, p.hop_frames) == (Wl, Ov, H, 1, Wf - Of)
    assert p.count.tolist() == list(cases.values()) and p.Wn == sum(cases.values())
    assert p.first.tolist() == np.concatenate([[0], np.cumsum(p.count)[:-1]]).tolist()
    assert p.table.dtype == np.int32 and p.table.shape == (p.Wn, 4)
    for r, S in enumerate(cases):
        rows = p.table[p.first[r]:p.first[r] + p.count[r]]
        n = len(rows)
        assert n == (1 if S <= Wl else 1 + -(-(S - Wl) // H))
        covered = np.zeros(S, dtype=bool)
        for k, (rec, start, ns, f0) in enumerate(rows.tolist()):
            assert rec == r and start == k * H and ns == min(Wl, S - k * H) and f0 * lc.SPF == start
            covered[start:start + ns] = True
        assert covered.all()
        if n > 1:
            assert rows[-1, 2] > Ov and (rows[:-1, 2] == Wl).all()
    last = p.table[p.first + p.count - 1]
    assert p.Tmax == max(int(f) + int(n) // lc.SPF + 1 for _, _, n, f in last)
    assert lc.plan_frames([Wl], Wf, Of, 1, frames_of=lambda n: 100).Tmax == 100
    # seconds round to whole frames
    q = lf.WindowPlan([10], 30.0, 4.0, 1.0, 16000, 320)
    assert (q.Wl, q.Ov, q.guard) == (480000, 64000, 50)
    assert lf.WindowPlan([10], 0.031, 0.011, 0.0, 16000, 320).Wl == 640


@pytest.mark.parametrize('kw,name', [(dict(window_s=2.0, overlap_s=2.0), 'overlap_s'), (dict(window_s=2.0, overlap_s=3.0), 'overlap_s'),
                                     (dict(window_s=2.0, overlap_s=0.0), 'overlap_s'), (dict(window_s=2.0, overlap_s=-1.0), 'overlap_s'),
                                     (dict(window_s=2.0, overlap_s=0.5, guard_s=0.26), 'guard_s'),
                                     (dict(window_s=2.0, overlap_s=0.5, guard_s=-0.1), 'guard_s'),
                                     (dict(window_s=2.0, overlap_s=1.2, guard_s=0.1), 'window_s')])
def test_plan_refusals_name_the_argument(kw, name):
    with pytest.raises(ValueError, match=name):
        lf.WindowPlan([16000], **{'guard_s': 0.1, **kw})


def test_cut_host_is_slicing():
    args = dict(window_f=4, overlap_f=1)
    lens = lc.rec_lens(args, [1, 2, 5])
    p = lc.plan_frames(lens, 4, 1, 0)
    assert p.count.tolist() == [1, 2, 5]
    rng = np.random.default_rng(0)
    audio = rng.standard_normal((3, max(lens) + 99)).astype(np.float32)          # garbage behind each length
    win, wl = lf.cut_host(audio, lens, p)
    assert win.shape == (8, 1280) and win.dtype == np.float32 and wl.dtype == np.int32
    for w, (r, s, n, _) in enumerate(p.table.tolist()):
        assert wl[w] == n == min(1280, lens[r] - s)
        assert np.array_equal(win[w, :n], audio[r, s:s + n]) and not win[w, n:].any()
    shorter = [lens[0], lens[1] - 400, 1000]                                     # lens below the plan's: windows shrink, never below 0
    win, wl = lf.cut_host(audio, shorter, p)
    for w, (r, s, n, _) in enumerate(p.table.tolist()):
        m = max(0, min(n, shorter[r] - s))
        assert wl[w] == m and np.array_equal(win[w, :m], audio[r, s:s + m]) and not win[w, m:].any()


@pytest.mark.parametrize('seam', ['blank', 'middle'])
@pytest.mark.parametrize('with_scores', [True, False])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_slice_property(seed, with_scores, seam):
    """windows cut from one global row stitch back to that row on every byte, whatever seams are picked, and so does the
    collapse"""
    args = dict(window_f=24, overlap_f=8)
    p = lc.plan_frames(lc.rec_lens(args, [1, 4, 2, 1, 7]), 24, 8, 2)
    Tw = 26
    c = lc.slice_case(p, Tw, seed, bpfs=(4, 20, 160), ties=seed == 2)
    fs = c['frame_score'] if with_scores else None
    out, total, seams = lf.stitch_host(p, c['enc'], c['tokens'], fs, c['planes'], lc.BLANK, seam)
    want = c['want'] if with_scores else [c['want'][0]] + c['want'][2:]
    assert np.array_equal(total, c['total']) and total.dtype == seams.dtype == np.int32
    assert len(out) == len(want)
    for o, w in zip(out, want):
        assert o.dtype == w.dtype and o.shape == w.shape and o.tobytes() == w.tobytes()
    for r in range(p.R):                                                         # seams lie inside the overlaps, past the guards
        for w in range(p.first[r] + 1, p.first[r] + p.count[r]):
            lo, hi = p.table[w, 3], p.table[w - 1, 3] + c['enc'][w - 1]
            assert lo <= seams[w] <= hi
            if min(hi - p.guard, lo + c['enc'][w]) > lo + p.guard:
                assert lo + p.guard <= seams[w] < hi - p.guard
    got = ctc.collapse_host(out[0], out[1] if with_scores else None, total, blank=lc.BLANK)
    ref = ctc.collapse_host(c['want'][0], c['want'][1] if with_scores else None, c['total'], blank=lc.BLANK)
    for f in ('labels', 'n_labels', 'start', 'nframes', 'score', 'utt_score'):
        a, b = getattr(got, f), getattr(ref, f)
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), f


def _pair(encA=20, encB=20, guard=1):
    """two windows of 20 frames that overlap on the global frames [10, 10 + encA): candidates 11 .. 18, mid 15"""
    p = lc.plan_frames([30 * lc.SPF], 20, 10, guard)
    assert p.count.tolist() == [2] and p.table[1, 3] == 10
    tok = np.stack([np.full(21, 1), np.full(21, 2)]).astype(np.int32)           # they disagree everywhere
    fs = np.full((2, 21), -1.0, dtype=np.float32)
    return p, tok, fs, np.array([encA, encB], dtype=np.int32)


def _agree(tok, g, value):
    tok[0, g], tok[1, g - 10] = value, value


def _seam(p, tok, fs, enc, seam='blank'):
    out, total, seams = lf.stitch_host(p, enc, tok, fs, (), lc.BLANK, seam)
    s = int(seams[1])
    assert seams[0] == 0 and total[0] == 10 + min(enc[1], 20)
    assert np.array_equal(out[0][0, :s], tok[0, :s]) and np.array_equal(out[0][0, s:total[0]], tok[1, s - 10:total[0] - 10])
    return s


def test_seam_rule_on_hand_made_overlaps():
    p, tok, fs, enc = _pair()
    assert _seam(p, tok, fs, enc) == 15                                          # nothing agrees: the middle
    _agree(tok, 15, 7)
    _agree(tok, 12, lc.BLANK)
    assert _seam(p, tok, fs, enc) == 12                                          # both blank beats a closer agreeing label
    assert _seam(p, tok, fs, enc, 'middle') == 15                                # 'middle' ignores the tokens
    _agree(tok, 17, lc.BLANK)
    assert _seam(p, tok, fs, enc) == 17                                          # same class, same sum: closer to the middle
    fs[0, 12] = -0.25
    assert _seam(p, tok, fs, enc) == 12                                          # the higher score sum wins inside a class
    fs[1, 7] = -0.25                                                             # frame 17: -1 - 0.25 = frame 12's sum
    assert _seam(p, tok, fs, enc) == 17
    assert _seam(p, tok, None, enc) == 17                                        # no scores: class, then distance
    _agree(tok, 13, lc.BLANK)
    fs[0, 13], fs[1, 3] = -0.5, -0.75                                            # three equal sums: 13 and 17 tie on distance
    assert _seam(p, tok, fs, enc) == 13                                          # ... the left one
    # -0 < +0 in the order of the keys: (+0) + (-0) = +0 beats (-0) + (-0) = -0
    p, tok, fs, enc = _pair()
    fs[...] = -0.0
    for g in (14, 18):
        _agree(tok, g, lc.BLANK)
    assert _seam(p, tok, fs, enc) == 14
    fs[1, 8] = 0.0
    assert _seam(p, tok, fs, enc) == 18
    # a label two windows agree on beats disagreement; the guard keeps the edges out
    p, tok, fs, enc = _pair()
    _agree(tok, 10, lc.BLANK)
    _agree(tok, 19, lc.BLANK)
    _agree(tok, 18, 3)
    assert _seam(p, tok, fs, enc) == 18
    # frames B does not hold are no candidates
    p, tok, fs, enc = _pair(encB=5)
    _agree(tok, 16, lc.BLANK)
    assert _seam(p, tok, fs, enc) == 14                                          # candidates 11 .. 14, mid 15: the closest


def test_seam_without_a_candidate_is_the_clamped_middle():
    for encA, want in ((11, 10), (12, 11), (10, 10), (3, 10)):                   # [lo + 1, hi - 1) is empty; hi < lo: lo
        p, tok, fs, enc = _pair(encA=encA)
        lo, hi = 10, encA
        out, total, seams = lf.stitch_host(p, enc, tok, fs, (), lc.BLANK)
        assert seams[1] == want
        if hi >= lo:
            assert want == min(hi, max(lo, (lo + hi) // 2))
        assert (out[0][0, :min(encA, want)] == 1).all() and (out[0][0, min(encA, want):want] == lc.BLANK).all()
        assert (out[0][0, want:30] == 2).all() and total[0] == 30


@pytest.mark.parametrize('seam', ['blank', 'middle'])
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_garbage_windows_keep_the_structure(seed, seam):
    args = dict(window_f=12, overlap_f=6)                                        # Wl = 2 Ov: the tightest plan
    p = lc.plan_frames(lc.rec_lens(args, [3, 1, 6, 2]), 12, 6, 1 + seed % 2)
    Tw = 14
    c = lc.garbage_case(p, Tw, seed)
    out, total, seams = lf.stitch_host(p, c['enc'], c['tokens'], c['frame_score'], c['planes'], lc.BLANK, seam)
    lc.check_structure(p, Tw, c, out, total, seams)


def test_stitch_refusals():
    p, tok, fs, enc = _pair()
    with pytest.raises(ValueError, match='blank'):
        lf.stitch_host(p, enc, tok, fs)
    with pytest.raises(ValueError, match='seam'):
        lf.stitch_host(p, enc, tok, fs, (), lc.BLANK, 'left')
    with pytest.raises(ValueError, match='multiple of 4'):
        lf.stitch_host(p, enc, tok, fs, [np.zeros((2, 21, 3), dtype=np.int16)], lc.BLANK)
    with pytest.raises(ValueError, match='at most 6'):
        lf.stitch_host(p, enc, tok, fs, [tok[:, :, None]] * 5, lc.BLANK)
    assert 'class' in lf.SEAM_RULES and '_order_key' in lf.SEAM_RULES


# ---- the facade on the host modules
@pytest.fixture(scope='module')
def host_model():
    torch.set_grad_enabled(False)
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_mode('none')
    return m


def test_decode_long_of_a_short_recording_is_decode(host_model):
    m = host_model
    audio = torch.from_numpy(synth.make_audio(2, 30000, seed=5))
    lens = torch.tensor([30000, 21111])
    got = m.decode_long(audio, lens, window_s=2.0, overlap_s=0.5, guard_s=0.1)
    want = m.decode(input_signal=audio, input_signal_length=lens)
    for b in range(2):
        assert got[b] == want[b] and got[b].seams_s is None and len(want[b].text) > 0
    wide = torch.cat([audio, torch.zeros(2, 5000)], dim=1)              # a batch padded past the window: still decode()'s
    assert m.decode_long(wide, lens, window_s=2.0, overlap_s=0.5, guard_s=0.1) == m.decode(input_signal=wide, input_signal_length=lens)


@pytest.mark.parametrize('seam', ['blank', 'middle'])
def test_decode_long_of_three_windows_is_the_composition(host_model, seam):
    m = host_model
    S = 32000 + 2 * 24000 - 5000                         # three windows of 2 s that overlap by 0.5 s; the last is ragged
    audio = torch.from_numpy(synth.make_audio(1, S, seed=6))
    lens = torch.tensor([S])
    plan, want, _ = lc.compose_on_host(m, audio, lens, 2.0, 0.5, 0.1, batch_size=2, seam=seam)
    assert plan.count.tolist() == [3]
    got = m.decode_long(audio, lens, window_s=2.0, overlap_s=0.5, guard_s=0.1, batch_size=2, seam=seam)
    assert [dataclasses.astuple(h) for h in got] == [dataclasses.astuple(h) for h in want]
    h = got[0]
    assert len(h.seams_s) == 2 and 1.5 < h.seams_s[0] < 2.0 and 3.0 < h.seams_s[1] < 3.5
    assert h.end_s[-1] > 2.0 and max(h.start_s) > 2.0 and h.end_s[-1] <= S / 16000 + 0.04      # times of the recording
    assert all(a <= b for a, b in zip(h.start_s, h.start_s[1:]))


def test_decode_long_refusals(host_model):
    m = host_model
    audio, lens = torch.zeros(1, 40000), torch.tensor([40000])
    for kw, word in ((dict(overlap_s=2.5), 'overlap_s'), (dict(guard_s=0.3), 'guard_s'), (dict(seam='left'), 'seam'),
                     (dict(batch_size=0), 'batch_size'), (dict(lm='x.arpa'), 'beam_width'), (dict(boost=['a']), 'beam_width')):
        with pytest.raises(ValueError, match=word):
            m.decode_long(audio, lens, **{'window_s': 2.0, 'overlap_s': 0.5, 'guard_s': 0.1, **kw})
    with pytest.raises(ValueError, match='window_s'):
        m.transcribe(['x.wav'], logprobs=True, window_s=2.0)


def test_hypothesis_gains_a_defaulted_field():
    h = ctc.Hypothesis('a', [0], [0.0], [0.02], None, None)
    assert h.seams_s is None and [f.name for f in dataclasses.fields(ctc.Hypothesis)][-1] == 'seams_s'


# ---- the entry points' argument checks (host code: nothing is launched, no GPU is touched)
def test_abi_argument_refusals():
    from qasr import engine
    lib = engine.load_library()
    err = lambda: lib.qasr_last_error().decode()
    buf = np.zeros(64, dtype=np.int32)                   # stands for every pointer: a refused call reads none of them
    ptr = buf.ctypes.data

    def cut(**kw):
        a = engine.LongformCutArgs()
        a.struct_size = C.sizeof(engine.LongformCutArgs)
        a.R, a.Wn, a.Wl, a.pitch = 1, 1, 1280, 4000
        a.audio = a.lens = a.table = a.windows = a.window_lens = ptr
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.qasr_longform_cut(None, C.byref(a))

    def stitch(planes=((ptr, ptr, 4),), **kw):
        a = engine.LongformStitchArgs()
        a.struct_size = C.sizeof(engine.LongformStitchArgs)
        a.R, a.Wn, a.Tw, a.Tmax, a.guard, a.hop_frames, a.blank, a.seam_mode = 1, 1, 64, 64, 2, 48, 28, 0
        a.table = a.enc_lens = a.tokens = a.frame_score = a.total_frames = a.seams = ptr
        a.n_planes = len(planes)
        for i, (s, d, b) in enumerate(planes[:6]):
            a.planes[i].src, a.planes[i].dst, a.planes[i].bytes_per_frame = s, d, b
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.qasr_longform_stitch(None, C.byref(a))

    assert C.sizeof(engine.LongformCutArgs) == 64 and C.sizeof(engine.LongformPlane) == 32
    assert C.sizeof(engine.LongformStitchArgs) == 40 + 48 + 6 * 32
    assert lib.qasr_longform_cut(None, None) == 1 and 'NULL' in err()
    assert cut(struct_size=60) == 1 and 'struct_size' in err()
    for name in ('audio', 'lens', 'table', 'windows', 'window_lens'):
        assert cut(**{name: None}) == 1 and 'required' in err(), name
    assert cut(Wn=0) == 1 and 'Wn' in err()
    assert cut(Wl=0) == 1 and 'Wl' in err()
    assert cut(pitch=-1) == 1 and 'pitch' in err()
    assert lib.qasr_longform_stitch(None, None) == 1 and 'NULL' in err()
    assert stitch(struct_size=C.sizeof(engine.LongformStitchArgs) + 8) == 1 and 'struct_size' in err()
    for name in ('table', 'enc_lens', 'tokens', 'total_frames', 'seams'):
        assert stitch(**{name: None}) == 1 and 'required' in err(), name
    assert stitch(Wn=0) == 1 and 'Wn' in err()
    assert stitch(guard=-1) == 1 and 'guard' in err()
    assert stitch(seam_mode=2) == 1 and 'seam_mode' in err()
    assert stitch(n_planes=7) == 1 and 'planes' in err()
    for b in (0, 2, 6, 18, -4):
        assert stitch(planes=((ptr, ptr, b),)) == 1 and 'multiple of 4' in err(), b
    assert stitch(planes=((ptr, None, 4),)) == 1 and 'NULL' in err()
    assert stitch(planes=((ptr, ptr, 4), (None, ptr, 4))) == 1 and 'plane 1' in err()
    assert stitch(planes=((ptr + 2, ptr, 4),)) == 1 and 'aligned' in err()
