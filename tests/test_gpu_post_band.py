"""CTC posteriors inside the band on an MI355X: k_post_band (csrc/qasr_post_band.hip) against its NumPy statement
qasr.align.post_band_host, every byte of every output, no tolerance and no case left out - the smallest shapes at which each
instantiation's band moves, a band that holds every state, a wildcard plane, pitches, lengths, invalid rows; refused arguments
launch nothing; the chain k_align_band -> k_post_band replays from a graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_band_cases as abc  # noqa: E402
import align_cases  # noqa: E402
import post_band_cases as pbc  # noqa: E402
import post_cases as pc  # noqa: E402
import star_cases as sc  # noqa: E402
from qasr import align, beam  # noqa: E402
from test_gpu_align import FILL32, FILL64  # noqa: E402

NEG = beam.NEG


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _filled_out(P, T, ML, pitch=None, total=True):
    """caller-owned outputs pre-filled with 0x5a..., so that an unwritten tail shows; frame_post rows of `pitch` >= T"""
    i32 = dict(dtype=torch.int32, device='cuda')
    fp = torch.full((P, pitch or T), FILL32, **i32)
    out = align.PostResult(fp[:, :T], torch.full((P, ML), FILL32, **i32),
                           torch.full((P,), FILL64, dtype=torch.int64, device='cuda') if total else None, torch.full((P,), FILL32, **i32))
    out._whole = fp
    return out


def _dev(res, start=None, nframes=None, ok=None, band_base=None):
    """a BandResult of NumPy arrays as ctc_post_band's band_result, any of its four arrays replaced"""
    def d(x, y):
        return torch.from_numpy(np.ascontiguousarray(x if y is None else y)).cuda()
    return align.BandResult(None, None, d(res.start, start), d(res.nframes, nframes), ok=d(res.ok, ok), band_base=d(res.band_base, band_base),
                            band_states=res.band_states)


def _run(eng, lp_d, lens_d, tg, tl, blank, bres, want, what, star=None, pitch=None, total=True):
    P, ML = tg.shape
    T = lp_d.shape[1]
    out = _filled_out(P, T, ML, pitch, total)
    ws = torch.full((eng.ctc_post_band_workspace_bytes(P, T) + 8,), 0x5a, dtype=torch.uint8, device='cuda')
    eng.ctc_post_band(lp_d, lens_d, torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), blank, bres, star=star, workspace=ws, out=out)
    torch.cuda.synchronize()
    if not total:
        out.total = torch.from_numpy(want.total).cuda()
    pc.same_bytes(out, want, what)
    assert (out._whole[:, T:] == FILL32).all()                   # the columns behind T are the caller's
    assert (ws[-8:] == 0x5a).all()                               # and so is what lies behind the workspace
    return out


def _wide(lp):
    """the same log-probabilities with a recording pitch and a frame pitch of their own"""
    P, T, C_ = lp.shape
    wide = torch.full((P, T + 3, C_ + 7), 7.0, device='cuda')
    wide[:, :T, :C_] = torch.from_numpy(lp).cuda()
    return wide, wide[:, :T, :C_]


@pytest.mark.parametrize('name', [d[0] for d in abc.DEVICE])
def test_k_post_band_equals_the_twin_where_the_band_moves(eng, name):
    bw, lp, tg, tl = abc.device_case(name)
    T = lp.shape[1]
    wide, view = _wide(lp)
    for lens in (None, np.array([T - 45], dtype=np.int32)):
        res, want = pbc.band_and_post(lp, lens, tg, tl, abc.BLANK, bw)
        assert res.ok[0] == 1 and want.ok[0] == 1 and pbc.n_bases(res) >= 5 and want.frame_post.min() < 0
        lens_d = None if lens is None else torch.from_numpy(lens).cuda()
        _run(eng, torch.from_numpy(lp).cuda(), lens_d, tg, tl, abc.BLANK, _dev(res), want, (name, lens))
        _run(eng, view, lens_d, tg, tl, abc.BLANK, _dev(res), want, (name, lens, 'pitches'), pitch=T + 5, total=False)
    assert (wide[:, T:, :] == 7.0).all() and (wide[:, :, abc.C:] == 7.0).all()


@pytest.mark.parametrize('bw', align.BAND_STATES)
def test_k_post_band_with_a_band_that_holds_every_state(eng, bw):
    """S <= 256 in every instantiation: the twin (and through it post_host); shortened, zero and oversized lens; no labels"""
    lp1, y = abc.synth(5, 60, a=3.0, per_label=(1, 3), gap=(0, 2), tail=2)
    T = lp1.shape[0]
    rng = np.random.Generator(np.random.PCG64(bw))
    rows = [y, [], y[:17], sc.labels_without_blank(rng, 127, abc.C, abc.BLANK, repeats=0.3), y[:5], []]
    tg, tl = align_cases.pad_targets(rows, abc.BLANK)
    lp = np.stack([lp1, lp1, lp1[::-1], lp1, lp1, lp1])
    wide, view = _wide(lp)
    for lens in (None, np.array([T, T - 9, 40, T, 0, 0], dtype=np.int32), np.array([T + 5, 1, T, 254, 4, -3], dtype=np.int32)):
        res, want = pbc.band_and_post(lp, lens, tg, tl, abc.BLANK, bw)
        full, same = pc.align_and_post(lp, lens, tg, tl, abc.BLANK)
        pc.same_bytes(want, same, 'the twin is post_host here')
        assert want.ok.sum() >= 4
        lens_d = None if lens is None else torch.from_numpy(lens).cuda()
        _run(eng, torch.from_numpy(lp).cuda(), lens_d, tg, tl, abc.BLANK, _dev(res), want, (bw, lens))
        _run(eng, view, lens_d, tg, tl, abc.BLANK, _dev(res), want, (bw, lens, 'pitches'), pitch=T + 1, total=False)


@pytest.mark.parametrize('bw', align.BAND_STATES)
def test_k_post_band_with_a_plane(eng, bw):
    """STAR = true: at 256 states the band moves under the wildcards, at 1024 and 4352 it holds every state; a plane whose pitch
    is greater than T; without the plane the wildcard's id is a label outside [0, C) and the row is refused"""
    lp, tg, tl, blank, _ = sc.moving_band_case()
    T = lp.shape[1]
    lens = np.array([T - 100], dtype=np.int32)
    star = align.star_host(lp, lens, 1.5)
    res, want = pbc.band_and_post(lp, lens, tg, tl, blank, bw, star=star)
    assert res.ok[0] == 1 and want.ok[0] == 1 and (pbc.n_bases(res) > 3) == (bw == 256) and want.frame_post.min() < 0
    plane = torch.full((1, T + 9), 3.0, device='cuda')
    plane[:, :T] = torch.from_numpy(star).cuda()
    lp_d, lens_d = torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda()
    _run(eng, lp_d, lens_d, tg, tl, blank, _dev(res), want, bw, star=plane[:, :T])
    assert (plane[:, T:] == 3.0).all()
    bare = pbc.post_band(lp, lens, tg, tl, blank, res)
    assert not bare.ok.any()
    _run(eng, lp_d, lens_d, tg, tl, blank, _dev(res), bare, (bw, 'bare'))


def test_k_post_band_invalid_rows_are_zero_and_leave_the_others_alone(eng):
    """three recordings in one launch, the middle one invalid in every way POST_BAND_RULES and POST_RULES name"""
    lp2, lens2, tg2, tl2, res2, _ = pbc.pair_case()
    lp, lens, tg, tl = (np.concatenate([x, x[1:]]) for x in (lp2, lens2, tg2, tl2))
    res = align.align_band_host(lp, lens, tg, tl, abc.BLANK, band_states=256)
    good = pbc.post_band(lp, lens, tg, tl, abc.BLANK, res)
    assert good.ok.tolist() == [1, 1, 1]
    lim = int(lens[1])
    variants = pbc.invalid_bands(res, tg, tl, 1, lim)
    for name, (st, nf, ok) in pc.invalid_paths(res, tg, tl, 1, lim).items():
        variants[name] = (st, nf, ok, res.band_base)
    assert len(variants) == 18
    lp_d, lens_d = torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda()
    for name, (st, nf, ok, bb) in variants.items():
        want = pbc.post_band(lp, lens, tg, tl, abc.BLANK, res, start=st, nframes=nf, ok=ok, band_base=bb)
        assert want.ok.tolist() == [1, int(name.startswith('control')), 1], name
        _run(eng, lp_d, lens_d, tg, tl, abc.BLANK, _dev(res, st, nf, ok, bb), want, name)
    # targets k_align_band refuses, with a path that would otherwise do
    for bad_tl in (None, -1, tg.shape[1] + 1):
        tg_b, tl_b = tg.copy(), tl.copy()
        if bad_tl is None:
            tg_b[1, 3], tg_b[2, 0] = abc.BLANK, abc.C
        else:
            tl_b[1] = bad_tl
        want = pbc.post_band(lp, lens, tg_b, tl_b, abc.BLANK, res)
        assert want.ok.tolist() == [1, 0, int(bad_tl is not None)]
        _run(eng, lp_d, lens_d, tg_b, tl_b, abc.BLANK, _dev(res), want, ('bad target', bad_tl))


def test_k_post_band_refuses_bad_arguments_and_writes_nothing(eng):
    lib = eng.load_library()
    B, T, C_, ML, blank, BW = 2, 40, 29, 6, 28, 256
    NB = (T + 31) // 32
    lp = torch.zeros(B, T, C_, device='cuda')
    tg = torch.zeros(B, ML, dtype=torch.int32, device='cuda')
    tl = torch.full((B,), 2, dtype=torch.int32, device='cuda')
    st = torch.zeros(B, ML, dtype=torch.int32, device='cuda')
    st[:, 1] = 2
    nf = torch.ones(B, ML, dtype=torch.int32, device='cuda')
    ok_in = torch.ones(B, dtype=torch.int32, device='cuda')
    bb = torch.zeros(B, NB, dtype=torch.int32, device='cuda')
    out = _filled_out(B, T, ML)
    need = eng.ctc_post_band_workspace_bytes(B, T)
    assert need == B * T * 8 and eng.ctc_post_band_workspace_bytes(0, T) == 0 and eng.ctc_post_band_workspace_bytes(B, 0) == 0
    assert eng.ctc_post_band_workspace_bytes(B, align.BAND_MAX_FRAMES + 1) == 0
    assert eng.ctc_post_band_workspace_bytes(1024, align.BAND_MAX_FRAMES) == 1024 * align.BAND_MAX_FRAMES * 8 == 2 ** 35    # size_t
    ws = torch.full((need + 8,), 0x5a, dtype=torch.uint8, device='cuda')
    tab = eng.lae_table_device('cuda')
    star = torch.zeros(B, T, device='cuda')

    def args(**kw):
        a = eng.PostBandArgs()
        a.struct_size = C.sizeof(eng.PostBandArgs)
        a.B, a.T, a.C, a.blank, a.max_labels, a.band_states = B, T, C_, blank, ML, BW
        a.pitch_utt, a.pitch_frame = T * C_, C_
        a.log_probs, a.targets, a.target_lens = lp.data_ptr(), tg.data_ptr(), tl.data_ptr()
        a.lae_entries, a.lae_table, a.workspace, a.workspace_bytes = beam.TAB_ENTRIES, tab.data_ptr(), ws.data_ptr(), need
        a.start, a.nframes, a.ok_in, a.band_base = st.data_ptr(), nf.data_ptr(), ok_in.data_ptr(), bb.data_ptr()
        a.frame_post, a.post_pitch, a.label_post = out.frame_post.data_ptr(), T, out.label_post.data_ptr()
        a.total, a.ok = out.total.data_ptr(), out.ok.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=C.sizeof(eng.PostBandArgs) - 16), dict(B=0), dict(T=0), dict(T=align.BAND_MAX_FRAMES + 1),
           dict(C=0), dict(max_labels=0), dict(max_labels=align.BAND_MAX_LABELS + 1), dict(band_states=0), dict(band_states=512),
           dict(band_states=4096), dict(blank=-1), dict(blank=C_), dict(pitch_frame=C_ - 1), dict(pitch_utt=T * C_ - 1),
           dict(lae_table=None), dict(lae_entries=4096), dict(lae_entries=0), dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
           dict(workspace=ws.data_ptr() + 4), dict(post_pitch=T - 1), dict(post_pitch=0), dict(star_logp=star.data_ptr(), star_pitch=T - 1)]
    bad += [{k: None} for k in ('log_probs', 'targets', 'target_lens', 'workspace', 'ok', 'start', 'nframes', 'band_base', 'frame_post',
                                'label_post')]
    for kw in bad:
        assert lib.qasr_ctc_post_band(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_post_band(s, None) == 1
    with pytest.raises(ValueError, match='band_states'):     # and a width that is none is refused on the host side of the binding
        eng.ctc_post_band(lp, None, tg, tl, blank, align.BandResult(None, None, st, nf, ok=ok_in, band_base=bb, band_states=512))
    torch.cuda.synchronize()
    assert (out._whole == FILL32).all() and (out.label_post == FILL32).all() and (out.ok == FILL32).all() and (out.total == FILL64).all()
    assert (ws == 0x5a).all()
    assert lib.qasr_ctc_post_band(s, C.byref(args())) == 0                     # and the same block unchanged is accepted,
    assert lib.qasr_ctc_post_band(s, C.byref(args(total=None, ok_in=None))) == 0   # as is one without total and without ok_in
    assert lib.qasr_ctc_post_band(s, C.byref(args(star_logp=star.data_ptr(), star_pitch=T))) == 0
    assert lib.qasr_ctc_post_band(s, C.byref(args(band_states=4352))) == 0
    torch.cuda.synchronize()
    assert (out.ok.cpu().numpy() == 1).all() and (ws[need:] == 0x5a).all()


def test_the_chain_k_align_band_k_post_band_is_capturable(eng):
    """nothing is allocated and no length is read on the host: k_post_band reads k_align_band's outputs on the device, and both
    replay from one graph on new inputs; the replay equals the eager run and the twin"""
    (lp0, lens0, tg0, tl0, _, _) = pbc.pair_case()
    blank, BW = abc.BLANK, 256
    B, T, _ = lp0.shape
    ML = tg0.shape[1]
    NB = (T + 31) // 32
    inputs = [(lp0, lens0, tg0, tl0), (lp0[::-1].copy(), lens0[::-1].copy(), tg0[::-1].copy(), tl0[::-1].copy())]
    lp_d, lens_d = torch.from_numpy(lp0).cuda(), torch.from_numpy(lens0).cuda()
    tg_d, tl_d = torch.from_numpy(tg0).cuda(), torch.from_numpy(tl0).cuda()
    i32 = dict(dtype=torch.int32, device='cuda')
    aout = align.BandResult(tg_d, tl_d, torch.full((B, ML), FILL32, **i32), torch.full((B, ML), FILL32, **i32), None, None, None,
                            torch.full((B,), FILL32, **i32), blank, 1, None, torch.full((B, NB), FILL32, **i32), BW)
    out = _filled_out(B, T, ML)
    ws_a = torch.empty(eng.ctc_align_band_workspace_bytes(B, T, BW), dtype=torch.uint8, device='cuda')
    ws_p = torch.empty(eng.ctc_post_band_workspace_bytes(B, T), dtype=torch.uint8, device='cuda')
    eng.lae_table_device('cuda')                         # uploaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, blank, band_states=BW, workspace=ws_a, out=aout)
            eng.ctc_post_band(lp_d, lens_d, tg_d, tl_d, blank, aout, workspace=ws_p, out=out)
    for lp, lens, tg, tl in inputs:
        lp_d.copy_(torch.from_numpy(lp)), lens_d.copy_(torch.from_numpy(lens))
        tg_d.copy_(torch.from_numpy(tg)), tl_d.copy_(torch.from_numpy(tl))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        res, want = pbc.band_and_post(lp, lens, tg, tl, blank, BW)
        assert want.ok.all() and np.array_equal(aout.start.cpu().numpy(), res.start)
        assert np.array_equal(aout.band_base.cpu().numpy(), res.band_base)
        pc.same_bytes(out, want, 'replay')
        eager_a = eng.ctc_align_band(lp_d, lens_d, tg_d, tl_d, blank, band_states=BW)
        eager = eng.ctc_post_band(lp_d, lens_d, tg_d, tl_d, blank, eager_a)
        torch.cuda.synchronize()
        for f in pc.POST_FIELDS:
            assert torch.equal(getattr(eager, f), getattr(out, f)), f
