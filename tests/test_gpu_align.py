"""CTC forced alignment on an MI355X: k_align (csrc/qasr_align.hip) against its NumPy statement qasr.align.align_host, every
byte of every output, no tolerance and no case left out; refused arguments launch nothing."""
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
from qasr import align, beam  # noqa: E402

FILL32, FILL64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
FIELDS = ('start', 'nframes', 'score', 'path_score', 'total', 'ok')


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _lens(rng, B, T):
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = T + 5                                  # beyond the row: clamps
    return lens


def _filled_out(P, ML, blank, K, drop=()):
    """caller-owned outputs pre-filled with 0x5a..., so that an unwritten tail shows; `drop`: the optional ones left out"""
    i32 = dict(dtype=torch.int32, device='cuda')
    out = align.AlignResult(None, None, torch.full((P, ML), FILL32, **i32), torch.full((P, ML), FILL32, **i32),
                            torch.full((P, ML), FILL32, **i32).view(torch.float32),
                            torch.full((P,), FILL64, dtype=torch.int64, device='cuda'),
                            torch.full((P,), FILL64, dtype=torch.int64, device='cuda'), torch.full((P,), FILL32, **i32), blank, K)
    for f in drop:
        setattr(out, f, None)
    return out


def _assert_equal(got, want, what, drop=()):
    for f in FIELDS:
        if f in drop:
            continue
        g, w = getattr(got, f).cpu().numpy(), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        if f == 'score':
            g, w = g.view(np.int32), w.view(np.int32)
        assert np.array_equal(g, w), (what, f, np.argwhere(g != w)[:4].tolist())


def _targets(rng, lens_of, C_, blank, pitch):
    """one target per requested length: random non-blank labels with adjacent repeats"""
    rows = []
    for L in lens_of:
        y = rng.integers(0, C_ - 1, size=L)
        rep = rng.random(L) < 0.2
        for i in range(1, L):
            if rep[i]:
                y[i] = y[i - 1]
        rows.append([int(c) for c in y])
    return align_cases.pad_targets(rows, blank, pitch)


LS = (0, 1, 127, 128, 129)                               # 255, 257 and 259 states straddle the 256-thread stride


@pytest.mark.parametrize('T', [1, 37, 300])
@pytest.mark.parametrize('C_', [2, 29, 5207])
def test_k_align_equals_align_host_every_byte(eng, C_, T):
    B, blank, ML = 3, C_ - 1, 130
    rng = np.random.Generator(np.random.PCG64(1000 * T + C_))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C_, blank, blend=(i % 2 == 1)) for i in range(B)])
    lens = _lens(rng, B, T)
    lp_d, lens_d = torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda()
    wide = torch.full((B, T + 3, C_ + 7), 7.0, device='cuda')             # both pitches differ from T * C and C
    wide[:, :T, :C_] = lp_d
    n_ok = 0
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
        tg_d, tl_d = torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda()
        ws = torch.empty(eng.ctc_align_workspace_bytes(P, T, ML), dtype=torch.uint8, device='cuda')
        for use_lens in (True, False):
            want = align.align_host(lp, lens if use_lens else None, tg, tl, blank, problems_per_utt=K)
            n_ok += int(want.ok.sum())
            for src in (lp_d, wide[:, :T, :C_]):
                for drop in ((), ('total',)):
                    out = _filled_out(P, ML, blank, K, drop)
                    eng.ctc_align(src, lens_d if use_lens else None, tg_d, tl_d, blank, problems_per_utt=K, workspace=ws, out=out)
                    torch.cuda.synchronize()
                    _assert_equal(out, want, (K, lens_of, use_lens, drop), drop)
    assert (wide[:, T:, :] == 7.0).all() and (wide[:, :, C_:] == 7.0).all()
    assert n_ok >= 10 and (T < 300 or n_ok >= 30)


def test_k_align_every_optional_output_absent_in_turn(eng):
    C_, T, B, K, ML, blank = 29, 120, 2, 2, 40, 28
    rng = np.random.Generator(np.random.PCG64(77))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C_, blank) for _ in range(B)])
    tg, tl = _targets(rng, [30, 0, 12, 40], C_, blank, ML)
    want = align.align_host(lp, None, tg, tl, blank, problems_per_utt=K)
    assert want.ok.all()
    lp_d, tg_d, tl_d = torch.from_numpy(lp).cuda(), torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda()
    for drop in [(f,) for f in FIELDS[:-1]] + [FIELDS[:-1]]:
        out = _filled_out(B * K, ML, blank, K, drop)
        eng.ctc_align(lp_d, None, tg_d, tl_d, blank, problems_per_utt=K, out=out)
        torch.cuda.synchronize()
        _assert_equal(out, want, drop, drop)
    got = eng.ctc_align(lp_d, None, tg_d, tl_d, blank, problems_per_utt=K)      # buffers of its own
    torch.cuda.synchronize()
    _assert_equal(got, want, 'own buffers')
    got = eng.ctc_align(lp_d, None, tg_d, tl_d, blank, problems_per_utt=K, want_total=False)
    assert got.total is None
    _assert_equal(got, want, 'own buffers, no total', ('total',))


@pytest.mark.parametrize('T', [2 * align.MAX_LABELS + 1, 2 * align.MAX_LABELS - 1, 2 * align.MAX_LABELS - 2])
def test_k_align_at_the_label_cap_with_every_label_repeated(eng, T):
    """4097 states, 17 per thread; 2048 equal labels need 2 * 2048 - 1 frames: one frame fewer is not alignable"""
    ML, C_, blank = align.MAX_LABELS, 2, 1
    rng = np.random.Generator(np.random.PCG64(T))
    lp = np.log(rng.dirichlet(np.ones(C_), size=(1, T))).astype(np.float32)
    tg, tl = np.zeros((1, ML), dtype=np.int32), np.array([ML], dtype=np.int32)
    want = align.align_host(lp, None, tg, tl, blank)
    assert want.ok[0] == (T >= 2 * ML - 1)
    out = _filled_out(1, ML, blank, 1)
    eng.ctc_align(torch.from_numpy(lp).cuda(), None, torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), blank, out=out)
    torch.cuda.synchronize()
    _assert_equal(out, want, T)


def test_k_align_long_utterance_mid_size_target(eng):
    """more than one back-walk window and the 4- and 8-state instantiations: T = 1000, targets of 300 and 600 labels"""
    C_, T, blank = 29, 1000, 28
    rng = np.random.Generator(np.random.PCG64(5))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C_, blank, blend=True)])
    g = list(beam_cases.greedy(lp[0], blank))
    for ML in (300, 600):
        tg, tl = _targets(rng, [ML, 0], C_, blank, ML)
        tg[1, :len(g)], tl[1] = g, len(g)
        want = align.align_host(lp, None, tg, tl, blank, problems_per_utt=2)
        assert want.ok.all()
        out = _filled_out(2, ML, blank, 2)
        eng.ctc_align(torch.from_numpy(lp).cuda(), None, torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), blank,
                      problems_per_utt=2, out=out)
        torch.cuda.synchronize()
        _assert_equal(out, want, ML)


def test_k_align_values_no_decoder_writes(eng):
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
    want = align.align_host(lp, None, tg, tl, blank)
    assert want.ok.all()
    out = _filled_out(B, ML, blank, 1)
    eng.ctc_align(torch.from_numpy(lp).cuda(), None, torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), blank, out=out)
    torch.cuda.synchronize()
    _assert_equal(out, want, 'special values')


def test_k_align_rows_that_are_not_alignable_leave_the_others_alone(eng):
    C_, T, B, K, ML, blank = 29, 50, 2, 4, 60, 28
    rng = np.random.Generator(np.random.PCG64(11))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C_, blank) for _ in range(B)])
    tg, tl = _targets(rng, [20, 20, 55, 20, 20, 20, 20, 3], C_, blank, ML)
    tg[1, 7] = blank                                     # a blank inside the target
    tg[3, 0] = C_                                        # past the classes: nothing may be read through it
    tg[4, 19] = -1
    tg[5, 5] = 2 ** 31 - 1
    tl[6] = -1                                           # negative length
    tl[7] = ML + 1                                       # above the row pitch
    want = align.align_host(lp, None, tg, tl, blank, problems_per_utt=K)
    assert want.ok.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]  # (row 2: 55 labels in 50 frames)
    tg[2, :], tl[2] = tg[0], 20
    want2 = align.align_host(lp, None, tg, tl, blank, problems_per_utt=K)
    assert want2.ok.tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    for w in (want, want2):
        out = _filled_out(B * K, ML, blank, K)
        eng.ctc_align(torch.from_numpy(lp).cuda(), None, torch.from_numpy(w.labels).cuda(), torch.from_numpy(w.n_labels).cuda(),
                      blank, problems_per_utt=K, out=out)
        torch.cuda.synchronize()
        _assert_equal(out, w, 'bad rows')
    # the good row is what it is alone
    alone = align.align_host(lp[:1], None, want.labels[:1], want.n_labels[:1], blank)
    assert alone.path_score[0] == want.path_score[0] and np.array_equal(alone.start[0], want.start[0])


def test_k_align_refuses_bad_arguments_and_writes_nothing(eng):
    lib = eng.load_library()
    B, T, C_, K, ML, blank = 2, 8, 29, 2, 6, 28
    P = B * K
    lp = torch.zeros(B, T, C_, device='cuda')
    tg = torch.zeros(P, ML, dtype=torch.int32, device='cuda')
    tl = torch.full((P,), 2, dtype=torch.int32, device='cuda')
    out = _filled_out(P, ML, blank, K)
    need = eng.ctc_align_workspace_bytes(P, T, ML)
    assert need > 0 and eng.ctc_align_workspace_bytes(P, T, align.MAX_LABELS + 1) == 0 and eng.ctc_align_workspace_bytes(0, T, ML) == 0
    assert eng.ctc_align_workspace_bytes(1, 65536, align.MAX_LABELS) == 16384 * 4100       # size_t: no 32-bit overflow in sight
    assert eng.ctc_align_workspace_bytes(64, 65536, align.MAX_LABELS) == 64 * 16384 * 4100 > 2 ** 32
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device='cuda')
    tab = eng.lae_table_device('cuda')

    def args(**kw):
        a = eng.AlignArgs()
        a.struct_size = C.sizeof(eng.AlignArgs)
        a.B, a.T, a.C, a.P, a.K, a.blank, a.max_labels = B, T, C_, P, K, blank, ML
        a.pitch_utt, a.pitch_frame = T * C_, C_
        a.log_probs, a.targets, a.target_lens = lp.data_ptr(), tg.data_ptr(), tl.data_ptr()
        a.lae_entries, a.lae_table, a.workspace, a.workspace_bytes = beam.TAB_ENTRIES, tab.data_ptr(), ws.data_ptr(), need
        for f in FIELDS:
            setattr(a, f, getattr(out, f).data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(B=0), dict(T=0), dict(T=65537), dict(C=0), dict(K=0), dict(P=P + 1), dict(P=B), dict(max_labels=0),
           dict(max_labels=align.MAX_LABELS + 1), dict(blank=-1), dict(blank=C_), dict(pitch_frame=C_ - 1), dict(pitch_utt=T * C_ - 1),
           dict(lae_table=None), dict(lae_entries=4096), dict(workspace_bytes=need - 1), dict(workspace_bytes=0)]
    bad += [{k: None} for k in ('log_probs', 'targets', 'target_lens', 'workspace', 'ok')]
    for kw in bad:
        assert lib.qasr_ctc_align(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_align(s, None) == 1
    with pytest.raises(ValueError):                      # and a pitch above the cap is refused on the host side of the binding
        eng.ctc_align(lp, None, torch.zeros(P, align.MAX_LABELS + 1, dtype=torch.int32, device='cuda'), tl, blank, problems_per_utt=K)
    torch.cuda.synchronize()
    for f in ('start', 'nframes', 'ok'):
        assert (getattr(out, f) == FILL32).all(), f
    assert (out.score.view(torch.int32) == FILL32).all() and (out.path_score == FILL64).all() and (out.total == FILL64).all()
    assert (ws == 0x5a).all()
    assert lib.qasr_ctc_align(s, C.byref(args())) == 0                     # and the same block unchanged is accepted,
    assert lib.qasr_ctc_align(s, C.byref(args(total=None, lae_table=None, lae_entries=0))) == 0      # as is one without total
    torch.cuda.synchronize()
    assert (out.ok.cpu().numpy() == 1).all()


def test_k_align_is_capturable(eng):
    """nothing is allocated and no length is read on the host: the launch replays from a graph on new inputs"""
    C_, T, B, ML, blank = 29, 64, 2, 20, 28
    rng = np.random.Generator(np.random.PCG64(13))
    lps = [np.stack([beam_cases.peaky_logp(rng, T, C_, blank) for _ in range(B)]) for _ in range(2)]
    tgs = [_targets(rng, [15, 20], C_, blank, ML), _targets(rng, [3, 0], C_, blank, ML)]
    lp_d = torch.from_numpy(lps[0]).cuda()
    tg_d, tl_d = torch.from_numpy(tgs[0][0]).cuda(), torch.from_numpy(tgs[0][1]).cuda()
    out = _filled_out(B, ML, blank, 1)
    ws = torch.empty(eng.ctc_align_workspace_bytes(B, T, ML), dtype=torch.uint8, device='cuda')
    eng.lae_table_device('cuda')                         # uploaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_align(lp_d, None, tg_d, tl_d, blank, workspace=ws, out=out)
    for lp, (tg, tl) in zip(lps, tgs):
        lp_d.copy_(torch.from_numpy(lp)), tg_d.copy_(torch.from_numpy(tg)), tl_d.copy_(torch.from_numpy(tl))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(out, align.align_host(lp, None, tg, tl, blank), 'replay')
