"""CTC posteriors on an MI355X: k_post (csrc/qasr_post.hip) against its NumPy statement qasr.align.post_host, every byte of
every output, no tolerance and no case left out; refused arguments launch nothing; the chain k_align -> k_post replays from a
graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases  # noqa: E402
import beam_cases  # noqa: E402
import post_cases as pc  # noqa: E402
import star_cases as sc  # noqa: E402
from qasr import align, beam  # noqa: E402
from test_gpu_align import FILL32, FILL64, LS, _lens, _targets  # noqa: E402

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


def _dev(res):
    """an AlignResult of NumPy arrays as ctc_post's align_result"""
    return align.AlignResult(None, None, torch.from_numpy(res.start).cuda(), torch.from_numpy(res.nframes).cuda(), None, None, None,
                             torch.from_numpy(res.ok).cuda(), res.blank, res.problems_per_utt)


def _run(eng, lp_d, lens_d, tg, tl, blank, ares, want, what, K=1, star=None, ws=None, pitch=None, total=True):
    P, ML = tg.shape
    T = lp_d.shape[1]
    out = _filled_out(P, T, ML, pitch, total)
    eng.ctc_post(lp_d, lens_d, torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), blank, ares, problems_per_utt=K, star=star,
                 workspace=ws, out=out)
    torch.cuda.synchronize()
    if not total:
        out.total = torch.from_numpy(want.total).cuda()
    pc.same_bytes(out, want, what)
    assert (out._whole[:, T:] == FILL32).all()                   # the columns behind T are the caller's
    return out


@pytest.mark.parametrize('T', [1, 37, 300])
@pytest.mark.parametrize('C_', [2, 29, 5207])
def test_k_post_equals_post_host_every_byte(eng, C_, T):
    B, blank, ML = 3, C_ - 1, 130
    rng = np.random.Generator(np.random.PCG64(1000 * T + C_))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C_, blank, blend=(i % 2 == 1)) for i in range(B)])
    lens = _lens(rng, B, T)
    lp_d, lens_d = torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda()
    wide = torch.full((B, T + 3, C_ + 7), 7.0, device='cuda')             # both pitches differ from T * C and C
    wide[:, :T, :C_] = lp_d
    n_ok = n_cases = 0
    # K = 1: five launches rotate the five lengths over the three utterances (full, empty, clamped); K = 3: all at once,
    # with the utterance's greedy string among them
    plans = [(1, [LS[(p + r) % 5] for p in range(B)]) for r in range(5)] + [(3, [LS[(2 * p) % 5] for p in range(3 * B)])]
    for K, lens_of in plans:
        tg, tl = _targets(rng, lens_of, C_, blank, ML)
        if K == 3:
            g = list(beam_cases.greedy(lp[0], blank))[:ML]
            tg[2, :] = blank
            tg[2, :len(g)], tl[2] = g, len(g)
        P = B * K
        ws = torch.empty(eng.ctc_post_workspace_bytes(P, T), dtype=torch.uint8, device='cuda')
        for use_lens in (True, False):
            res, want = pc.align_and_post(lp, lens if use_lens else None, tg, tl, blank, K)
            assert want.total.tobytes() == res.total.tobytes() and want.ok.tobytes() == res.ok.tobytes()
            n_ok += int(want.ok.sum())
            ares = _dev(res)
            for src, pitch, total in ((lp_d, None, True), (wide[:, :T, :C_], T + 5, False)):
                _run(eng, src, lens_d if use_lens else None, tg, tl, blank, ares, want, (K, lens_of, use_lens, pitch), K, ws=ws,
                     pitch=pitch, total=total)
                n_cases += 1
    assert (wide[:, T:, :] == 7.0).all() and (wide[:, :, C_:] == 7.0).all()
    assert n_cases == 24 and n_ok >= 10 and (T < 300 or n_ok >= 30)


@pytest.mark.parametrize('T', [2 * align.MAX_LABELS + 1, 2 * align.MAX_LABELS - 1, 2 * align.MAX_LABELS - 2])
def test_k_post_at_the_label_cap_with_every_label_repeated(eng, T):
    """4097 states, 17 per thread; 2048 equal labels on 4095 frames have a single path, so every posterior is exactly 0; on
    4097 frames the twin decides; one frame fewer than 4095 is not alignable"""
    ML, C_, blank = align.MAX_LABELS, 2, 1
    rng = np.random.Generator(np.random.PCG64(T))
    lp = np.log(rng.dirichlet(np.ones(C_), size=(1, T))).astype(np.float32)
    tg, tl = np.zeros((1, ML), dtype=np.int32), np.array([ML], dtype=np.int32)
    res, want = pc.align_and_post(lp, None, tg, tl, blank)
    assert want.ok[0] == (T >= 2 * ML - 1)
    if T == 2 * ML - 1:
        assert not want.frame_post.any() and not want.label_post.any()
    if T == 2 * ML - 2:
        # k_align says ok = 0 here; k_post also refuses a made-up path of the right shape that ends behind lim
        res.start[0], res.nframes[0], res.ok[0] = 2 * np.arange(ML), 1, 1
        want = align.post_host(lp, None, tg, tl, blank, res.start, res.nframes, res.ok)
        assert want.ok[0] == 0
    _run(eng, torch.from_numpy(lp).cuda(), None, tg, tl, blank, _dev(res), want, T)


def test_k_post_long_utterance_mid_size_target(eng):
    """the 4- and 8-state instantiations: T = 1000, targets of 300 and 600 labels"""
    C_, T, blank = 29, 1000, 28
    rng = np.random.Generator(np.random.PCG64(5))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C_, blank, blend=True)])
    g = list(beam_cases.greedy(lp[0], blank))
    for ML in (300, 600):
        tg, tl = _targets(rng, [ML, 0], C_, blank, ML)
        tg[1, :len(g)], tl[1] = g, len(g)
        res, want = pc.align_and_post(lp, None, tg, tl, blank, 2)
        assert want.ok.all() and want.frame_post.min() < 0
        _run(eng, torch.from_numpy(lp).cuda(), None, tg, tl, blank, _dev(res), want, ML, 2)


def test_k_post_special_values(eng):
    C_, T, B, ML, blank = 6, 40, 3, 9, 5
    rng = np.random.Generator(np.random.PCG64(3))
    lp = np.log(rng.dirichlet(np.ones(C_), size=(B, T))).astype(np.float32)
    lp[0, 0, :2] = [np.nan, -np.inf]
    lp[0, 1, 0] = np.inf
    lp[1, 3, :] = -np.inf
    lp[1, 4, :] = np.nan
    lp[2, 5, :] = -200.0
    lp[2, 6, :] = 0.0
    lp[2, 7, :] = -0.0
    tg, tl = _targets(rng, [9, 4, 7], C_, blank, ML)
    res, want = pc.align_and_post(lp, None, tg, tl, blank)
    assert want.ok.all()
    _run(eng, torch.from_numpy(lp).cuda(), None, tg, tl, blank, _dev(res), want, 'special values')


@pytest.mark.parametrize('L', [127, 128])
def test_k_post_with_a_plane(eng, L):
    """STAR = true at 255 and 257 states, a plane whose pitch is greater than T"""
    C_, T, B, K, blank = 29, 300, 2, 2, 28
    rng = np.random.Generator(np.random.PCG64(L))
    lp = sc.logp(rng, B, T, C_, blank)
    lens = np.array([T, 281], dtype=np.int32)
    star = align.star_host(lp, lens, 1.0)
    rows = [sc.with_wildcards(sc.labels_without_blank(rng, L - 2, C_, blank), C_, 'two_with_a_label_between'),
            sc.with_wildcards(sc.labels_without_blank(rng, L - 1, C_, blank), C_, 'first'),
            sc.with_wildcards(sc.labels_without_blank(rng, 5, C_, blank), C_, 'next_to_a_repeat'), [C_]]
    assert len(rows[0]) == len(rows[1]) == L
    tg, tl = align_cases.pad_targets(rows, blank, L)
    res, want = pc.align_and_post(lp, lens, tg, tl, blank, K, star=star)
    assert want.ok.all() and want.frame_post.min() < 0
    plane = torch.full((B, T + 9), 3.0, device='cuda')
    plane[:, :T] = torch.from_numpy(star).cuda()
    _run(eng, torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), tg, tl, blank, _dev(res), want, L, K, star=plane[:, :T])
    assert (plane[:, T:] == 3.0).all()
    # without the plane the wildcard's id is a label outside [0, C): rows refused, nothing read through it
    bare = align.post_host(lp, lens, tg, tl, blank, res.start, res.nframes, res.ok, problems_per_utt=K)
    assert not bare.ok.any()
    _run(eng, torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), tg, tl, blank, _dev(res), bare, (L, 'bare'), K)


def test_k_post_invalid_rows_are_zero_and_leave_the_others_alone(eng):
    C_, T, blank, K = 29, 50, 28, 2
    rng = np.random.Generator(np.random.PCG64(11))
    lp = sc.logp(rng, 2, T, C_, blank)
    lens = np.array([T, 44], dtype=np.int32)
    rows = [sc.labels_without_blank(rng, n, C_, blank) for n in (12, 9, 20, 5)]
    rows[2][1] = rows[2][2]
    tg, tl = align_cases.pad_targets(rows, blank)
    res, good = pc.align_and_post(lp, lens, tg, tl, blank, K)
    assert good.ok.all()
    lp_d, lens_d = torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda()
    for name, (st, nf, ok) in pc.invalid_paths(res, tg, tl, 2, 44).items():
        want = align.post_host(lp, lens, tg, tl, blank, st, nf, ok, problems_per_utt=K)
        assert want.ok.tolist() == [1, 1, 0, 1], name
        ares = align.AlignResult(None, None, torch.from_numpy(st).cuda(), torch.from_numpy(nf).cuda(), ok=torch.from_numpy(ok).cuda())
        _run(eng, lp_d, lens_d, tg, tl, blank, ares, want, name, K)
    # targets k_align refuses, with a path that would otherwise do
    tg2, tl2 = np.concatenate([tg, tg]), np.concatenate([tl, tl])
    tg2[1, 3] = blank
    tg2[2, 0] = C_
    tg2[3, 1] = -1
    tl2[5], tl2[6] = -1, tg.shape[1] + 1
    lp4, lens4 = np.concatenate([lp, lp]), np.concatenate([lens, lens])
    st, nf, ok = (np.concatenate([x, x]) for x in (res.start, res.nframes, res.ok))
    want = align.post_host(lp4, lens4, tg2, tl2, blank, st, nf, ok, problems_per_utt=K)
    assert want.ok.tolist() == [1, 0, 0, 0, 1, 0, 0, 1]
    ares = align.AlignResult(None, None, torch.from_numpy(st).cuda(), torch.from_numpy(nf).cuda(), ok=torch.from_numpy(ok).cuda())
    _run(eng, torch.from_numpy(lp4).cuda(), torch.from_numpy(lens4).cuda(), tg2, tl2, blank, ares, want, 'bad targets', K)


def test_k_post_refuses_bad_arguments_and_writes_nothing(eng):
    lib = eng.load_library()
    B, T, C_, K, ML, blank = 2, 8, 29, 2, 6, 28
    P = B * K
    lp = torch.zeros(B, T, C_, device='cuda')
    tg = torch.zeros(P, ML, dtype=torch.int32, device='cuda')
    tl = torch.full((P,), 2, dtype=torch.int32, device='cuda')
    st = torch.zeros(P, ML, dtype=torch.int32, device='cuda')
    st[:, 1] = 2
    nf = torch.ones(P, ML, dtype=torch.int32, device='cuda')
    ok_in = torch.ones(P, dtype=torch.int32, device='cuda')
    out = _filled_out(P, T, ML)
    need = eng.ctc_post_workspace_bytes(P, T)
    assert need == P * T * 8 and eng.ctc_post_workspace_bytes(0, T) == 0 and eng.ctc_post_workspace_bytes(P, 0) == 0
    assert eng.ctc_post_workspace_bytes(P, 65537) == 0
    assert eng.ctc_post_workspace_bytes(64, 65536) == 64 * 65536 * 8
    assert eng.ctc_post_workspace_bytes(16384, 65536) == 16384 * 65536 * 8 == 2 ** 33        # size_t: no 32-bit overflow
    ws = torch.full((need + 8,), 0x5a, dtype=torch.uint8, device='cuda')
    tab = eng.lae_table_device('cuda')
    star = torch.zeros(B, T, device='cuda')

    def args(**kw):
        a = eng.PostArgs()
        a.struct_size = C.sizeof(eng.PostArgs)
        a.B, a.T, a.C, a.P, a.K, a.blank, a.max_labels = B, T, C_, P, K, blank, ML
        a.pitch_utt, a.pitch_frame = T * C_, C_
        a.log_probs, a.targets, a.target_lens = lp.data_ptr(), tg.data_ptr(), tl.data_ptr()
        a.lae_entries, a.lae_table, a.workspace, a.workspace_bytes = beam.TAB_ENTRIES, tab.data_ptr(), ws.data_ptr(), need
        a.start, a.nframes, a.ok_in = st.data_ptr(), nf.data_ptr(), ok_in.data_ptr()
        a.frame_post, a.post_pitch, a.label_post = out.frame_post.data_ptr(), T, out.label_post.data_ptr()
        a.total, a.ok = out.total.data_ptr(), out.ok.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=C.sizeof(eng.PostArgs) - 16), dict(B=0), dict(T=0), dict(T=65537), dict(C=0), dict(K=0),
           dict(P=P + 1), dict(P=B), dict(max_labels=0), dict(max_labels=align.MAX_LABELS + 1), dict(blank=-1), dict(blank=C_),
           dict(pitch_frame=C_ - 1), dict(pitch_utt=T * C_ - 1), dict(lae_table=None), dict(lae_entries=4096), dict(lae_entries=0),
           dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=ws.data_ptr() + 4), dict(post_pitch=T - 1),
           dict(post_pitch=0), dict(star_logp=star.data_ptr(), star_pitch=T - 1)]
    bad += [{k: None} for k in ('log_probs', 'targets', 'target_lens', 'workspace', 'ok', 'start', 'nframes', 'frame_post', 'label_post')]
    for kw in bad:
        assert lib.qasr_ctc_post(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_post(s, None) == 1
    with pytest.raises(ValueError):                      # and a pitch above the cap is refused on the host side of the binding
        eng.ctc_post(lp, None, torch.zeros(P, align.MAX_LABELS + 1, dtype=torch.int32, device='cuda'), tl, blank,
                     align.AlignResult(None, None, st, nf, ok=ok_in), problems_per_utt=K)
    torch.cuda.synchronize()
    assert (out._whole == FILL32).all() and (out.label_post == FILL32).all() and (out.ok == FILL32).all() and (out.total == FILL64).all()
    assert (ws == 0x5a).all()
    assert lib.qasr_ctc_post(s, C.byref(args())) == 0                      # and the same block unchanged is accepted,
    assert lib.qasr_ctc_post(s, C.byref(args(total=None, ok_in=None))) == 0    # as is one without total and without ok_in
    assert lib.qasr_ctc_post(s, C.byref(args(star_logp=star.data_ptr(), star_pitch=T))) == 0
    torch.cuda.synchronize()
    assert (out.ok.cpu().numpy() == 1).all() and (ws[need:] == 0x5a).all()


def test_the_chain_k_align_k_post_is_capturable(eng):
    """nothing is allocated and no length is read on the host: k_post reads k_align's outputs on the device, and both replay from
    one graph on new inputs"""
    C_, T, B, ML, blank = 29, 64, 2, 20, 28
    rng = np.random.Generator(np.random.PCG64(13))
    lps = [np.stack([beam_cases.peaky_logp(rng, T, C_, blank) for _ in range(B)]) for _ in range(2)]
    tgs = [_targets(rng, [15, 20], C_, blank, ML), _targets(rng, [3, 0], C_, blank, ML)]
    lp_d = torch.from_numpy(lps[0]).cuda()
    tg_d, tl_d = torch.from_numpy(tgs[0][0]).cuda(), torch.from_numpy(tgs[0][1]).cuda()
    i32 = dict(dtype=torch.int32, device='cuda')
    aout = align.AlignResult(None, None, torch.full((B, ML), FILL32, **i32), torch.full((B, ML), FILL32, **i32), None, None, None,
                             torch.full((B,), FILL32, **i32), blank, 1)
    out = _filled_out(B, T, ML)
    ws_a = torch.empty(eng.ctc_align_workspace_bytes(B, T, ML), dtype=torch.uint8, device='cuda')
    ws_p = torch.empty(eng.ctc_post_workspace_bytes(B, T), dtype=torch.uint8, device='cuda')
    eng.lae_table_device('cuda')                         # uploaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_align(lp_d, None, tg_d, tl_d, blank, workspace=ws_a, out=aout)
            eng.ctc_post(lp_d, None, tg_d, tl_d, blank, aout, workspace=ws_p, out=out)
    for lp, (tg, tl) in zip(lps, tgs):
        lp_d.copy_(torch.from_numpy(lp)), tg_d.copy_(torch.from_numpy(tg)), tl_d.copy_(torch.from_numpy(tl))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        res, want = pc.align_and_post(lp, None, tg, tl, blank)
        assert want.ok.all() and np.array_equal(aout.start.cpu().numpy(), res.start)
        pc.same_bytes(out, want, 'replay')
