"""k_cut and k_stitch on an MI355X against their NumPy twins (qasr.longform), every byte: ragged recordings behind a wide
pitch, aligned and unaligned rows; planes of every width, with and without frame scores, both seam modes, ties, windows that
disagree everywhere, a search longer than one pass of the work-group, and one captured launch of both replayed on new data."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import longform_cases as lc  # noqa: E402
from qasr import longform as lf  # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _cut_plan():
    lens = lc.rec_lens(dict(window_f=4, overlap_f=1), [1, 2, 5])
    p = lc.plan_frames(lens, 4, 1, 0)
    assert p.count.tolist() == [1, 2, 5] and (p.Wl, p.Ov) == (1280, 320)
    return p, lens


def test_cut_equals_the_twin():
    from qasr import engine
    p, lens = _cut_plan()
    rng = np.random.default_rng(0)
    pitch = max(lens) + 131                                                      # wider than the longest recording, garbage behind
    audio = rng.standard_normal((3, pitch)).astype(np.float32)
    for ln in (lens, [lens[0] - 3, lens[1] - 401, 1000], [0, 1, lens[2]]):       # the plan's lengths, shorter ones, empty windows
        want, want_len = lf.cut_host(audio, ln, p)
        pitch4 = pitch + (-pitch) % 4
        for off in (0, 4, 1, 3):                                                 # every row 16-byte aligned, or none, or some
            for pt in (pitch4, pitch4 + 1):
                base = torch.full((off + 3 * pt,), 9.0, device='cuda')
                x = base[off:off + 3 * pt].view(3, pt)[:, :pitch]
                x.copy_(_cuda(audio))
                win, wl = engine.longform_cut(x, torch.tensor(ln), p)
                torch.cuda.synchronize()
                assert win.cpu().numpy().tobytes() == want.tobytes(), (ln, off, pt)
                assert wl.cpu().numpy().tobytes() == want_len.tobytes(), (ln, off, pt)
    out = (torch.full((p.Wn, p.Wl), 7.0, device='cuda'), torch.full((p.Wn,), -1, dtype=torch.int32, device='cuda'))
    got = engine.longform_cut(_cuda(audio), torch.tensor(lens).cuda(), p, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and out[0].cpu().numpy().tobytes() == lf.cut_host(audio, lens, p)[0].tobytes()


def _stitch_both(p, c, with_scores, seam):
    from qasr import engine
    fs = c['frame_score'] if with_scores else None
    want = lf.stitch_host(p, c['enc'], c['tokens'], fs, c['planes'], lc.BLANK, seam)
    got = engine.longform_stitch(p, _cuda(c['enc']), _cuda(c['tokens']), None if fs is None else _cuda(fs),
                                 [_cuda(x) for x in c['planes']], lc.BLANK, seam)
    torch.cuda.synchronize()
    assert len(got[0]) == len(want[0])
    for i, (g, w) in enumerate(zip(got[0], want[0])):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f'plane {i}'
    assert got[1].cpu().numpy().tobytes() == want[1].tobytes(), 'total_frames'
    assert got[2].cpu().numpy().tobytes() == want[2].tobytes(), 'seams'
    return want


def _small_plan(guard=2):
    args = dict(window_f=63, overlap_f=16)                                       # Tw = 64 frames, overlaps of 16
    return lc.plan_frames(lc.rec_lens(args, [1, 3, 1, 4, 2]), 63, 16, guard), 64


@pytest.mark.parametrize('seam', ['blank', 'middle'])
@pytest.mark.parametrize('with_scores', [True, False])
def test_stitch_equals_the_twin_on_sliced_rows(with_scores, seam):
    """planes of 4, 20 (not 16-byte aligned), 160 and 20 828 bytes per frame; the stitched rows are the global rows"""
    p, Tw = _small_plan()
    for seed, ties in ((0, False), (1, True)):
        c = lc.slice_case(p, Tw, seed, bpfs=(4, 20, 160, 20828), ties=ties)
        want = _stitch_both(p, c, with_scores, seam)
        ref = c['want'] if with_scores else [c['want'][0]] + c['want'][2:]
        for o, w in zip(want[0], ref):
            assert o.tobytes() == w.tobytes()


@pytest.mark.parametrize('seam', ['blank', 'middle'])
def test_stitch_equals_the_twin_on_windows_that_disagree(seam):
    """lengths of every kind, equal score sums and both zeros (the tie order), the tightest plan (Wl = 2 Ov)"""
    for seed in range(4):
        p, Tw = _small_plan(guard=seed)
        c = lc.garbage_case(p, Tw, seed)
        want = _stitch_both(p, c, seed % 2 == 0, seam)
        if seed % 2 == 0:
            lc.check_structure(p, Tw, c, *want)
    p = lc.plan_frames(lc.rec_lens(dict(window_f=12, overlap_f=6), [3, 1, 6, 2]), 12, 6, 1)
    c = lc.garbage_case(p, 14, 9)
    lc.check_structure(p, 14, c, *_stitch_both(p, c, True, seam))


def test_stitch_with_a_search_longer_than_the_work_group():
    """an overlap of 600 frames: every lane folds several candidates before the reduction"""
    p = lc.plan_frames(lc.rec_lens(dict(window_f=1300, overlap_f=600), [2, 3, 1]), 1300, 600, 10)
    for seed, ties, p_blank in ((0, False, 0.5), (1, True, 0.9), (2, True, 0.0)):
        c = lc.slice_case(p, 1301, seed, bpfs=(20,), ties=ties, p_blank=p_blank)
        _stitch_both(p, c, True, 'blank')
    _stitch_both(p, lc.garbage_case(p, 1301, 3), True, 'blank')
    _stitch_both(p, c, False, 'middle')


def test_cut_and_stitch_in_one_captured_graph():
    """nothing is read back and the plan's table is uploaded beforehand: both launches are captured once and replayed on new
    audio, lengths and window outputs of the same plan"""
    from qasr import engine
    pc, lens = _cut_plan()
    p, Tw = _small_plan()
    engine.longform_table(pc, 'cuda'), engine.longform_table(p, 'cuda')          # the uploads happen outside the capture
    pitch = max(lens) + 4
    xd, ld = torch.zeros(3, pitch, device='cuda'), torch.zeros(3, dtype=torch.int32, device='cuda')
    cut_out = (torch.empty(pc.Wn, pc.Wl, device='cuda'), torch.empty(pc.Wn, dtype=torch.int32, device='cuda'))
    c = lc.slice_case(p, Tw, 0, bpfs=(20, 160))
    src = dict(enc=_cuda(c['enc']), tok=_cuda(c['tokens']), fs=_cuda(c['frame_score']), pl=[_cuda(x) for x in c['planes']])
    st_out = ([torch.empty((p.R, p.Tmax) + tuple(t.shape[2:]), dtype=t.dtype, device='cuda') for t in [src['tok'], src['fs']] + src['pl']],
              torch.empty(p.R, dtype=torch.int32, device='cuda'), torch.empty(p.Wn, dtype=torch.int32, device='cuda'))
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.longform_cut(xd, ld, pc, out=cut_out)
            engine.longform_stitch(p, src['enc'], src['tok'], src['fs'], src['pl'], lc.BLANK, 'blank', out=st_out)
    rng = np.random.default_rng(5)
    for k, ln in enumerate((lens, [lens[0] - 9, 700, lens[2] - 1000])):
        audio = rng.standard_normal((3, pitch)).astype(np.float32)
        c = lc.slice_case(p, Tw, 10 + k, bpfs=(20, 160), ties=k == 1) if k == 0 else {**lc.garbage_case(p, Tw, 10 + k), 'planes': [
            lc.plane_rows(rng, (p.Wn, Tw), 20), lc.plane_rows(rng, (p.Wn, Tw), 160)]}
        xd.copy_(_cuda(audio)), ld.copy_(torch.tensor(ln, dtype=torch.int32))
        src['enc'].copy_(_cuda(c['enc'])), src['tok'].copy_(_cuda(c['tokens'])), src['fs'].copy_(_cuda(c['frame_score']))
        for d, x in zip(src['pl'], c['planes']):
            d.copy_(_cuda(x))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_cut = lf.cut_host(audio, ln, pc)
        assert cut_out[0].cpu().numpy().tobytes() == want_cut[0].tobytes() and cut_out[1].cpu().numpy().tobytes() == want_cut[1].tobytes()
        want = lf.stitch_host(p, c['enc'], c['tokens'], c['frame_score'], c['planes'], lc.BLANK, 'blank')
        for i, (d, w) in enumerate(zip(st_out[0], want[0])):
            assert d.cpu().numpy().tobytes() == w.tobytes(), f'replay {k} plane {i}'
        assert st_out[1].cpu().numpy().tobytes() == want[1].tobytes() and st_out[2].cpu().numpy().tobytes() == want[2].tobytes()


def test_binding_refusals_on_the_device():
    from qasr import engine
    p, Tw = _small_plan()
    c = lc.slice_case(p, Tw, 0)
    enc, tok, fs = _cuda(c['enc']), _cuda(c['tokens']), _cuda(c['frame_score'])
    with pytest.raises(ValueError, match='at most 6'):
        engine.longform_stitch(p, enc, tok, fs, [tok[:, :, None]] * 5, lc.BLANK)
    with pytest.raises(ValueError, match='multiple of 4'):
        engine.longform_stitch(p, enc, tok, fs, [torch.zeros(p.Wn, Tw, 3, dtype=torch.int16, device='cuda')], lc.BLANK)
    with pytest.raises(ValueError, match='seam'):
        engine.longform_stitch(p, enc, tok, fs, (), lc.BLANK, 'left')
    with pytest.raises(ValueError, match='blank'):
        engine.longform_stitch(p, enc, tok, fs)
