"""MBR re-ranking on an MI355X: k_edit_cut / k_mbr_pair / k_mbr_pick (csrc/qasr_mbr.hip) against qasr.mbr.mbr_host - every byte of
dist, weight, wsum, risk, order and ok, outputs pre-filled with 0x5a, no tolerance; refused arguments launch nothing; the chain
k_topn -> k_beam -> qasr_ctc_mbr replays from a graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_cases  # noqa: E402
import mbr_cases as mc  # noqa: E402
from qasr import beam, mbr  # noqa: E402

FILL32, FILL64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
NAMES = ('dist', 'weight', 'wsum', 'risk', 'order', 'ok')


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(B, K, dist=True):
    f32 = lambda *s: torch.full(s, FILL32, dtype=torch.int32, device='cuda')
    f64 = lambda *s: torch.full(s, FILL64, dtype=torch.int64, device='cuda')
    return mbr.MbrResult(f32(B, K, K) if dist else None, f32(B, K), f64(B), f64(B, K), f32(B, K), f32(B, K))


def _equal(got, want, what, dist=True):
    for n in NAMES[0 if dist else 1:]:
        g, w = getattr(got, n).cpu().numpy(), getattr(want, n)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            at = np.argwhere(g != w)[:6]
            raise AssertionError(f'{what}: {n} differs at {at.tolist()}: got {[g[tuple(i)].item() for i in at]} want {[w[tuple(i)].item() for i in at]}')


def _run(eng, case, mode, scale=1.0, wide=False, dist=True, what=''):
    """one call against the twin on every byte"""
    want = mbr.mbr_host(case['labels'], case['n_labels'], case['score'], case['n_hyps'], case['C'], mode=mode, is_space=case['is_space'],
                        scale=scale)
    B, K, L = case['labels'].shape
    labels = _cuda(case['labels'])
    if wide:                                                        # rows of a larger pitch, the pad filled with refused ids
        big = torch.full((B, K, L + 5), case['C'] + 9, dtype=torch.int32, device='cuda')
        big[:, :, :L] = labels
        labels = big[:, :, :L]
    out = _filled(B, K, dist)
    got = eng.mbr_rerank(labels, _cuda(case['n_labels']), _cuda(case['score']), _cuda(case['n_hyps']), case['C'], mode=mode,
                         is_space=_cuda(case['is_space']), scale=scale, out=out)
    torch.cuda.synchronize()
    _equal(got, want, f'{what} {mode}', dist)
    return want


def _lengths(m):
    """K = 3 and K = 2 rows of 0 / 1 / fewer / more / as many units than their partner; twelve and five pairs: more than one
    work-group, different lengths inside one"""
    f, s = max(m - 5, 0), max(m - 3, 0)
    return [[m, m, s], [0, 1, m], [m, f, m], [m, 1, 0], [f, m, m]], [[m, m], [0, m], [m, 1], [f, m], [m, s]]


# units at which k_mbr_pair<NC> changes: 64 NC - 1, 64 NC, 64 NC + 1 for NC = 1, 4, 16 (the width picks NC), then two and three strips
UNITS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize('m', UNITS)
def test_pairs_equal_mbr_host_every_byte_char(eng, m):
    for lens in _lengths(m):
        case = mc.nbest(100 + m, 29, B=5, K=len(lens[0]), L=max(m, 1), lengths=lens)
        want = _run(eng, case, 'char', what=f'm={m} K={len(lens[0])}')
        assert (want.ok == 1).all() and want.dist[0, 0, 1] > 0 or m < 2
        assert want.dist[1, 0, -1] == m


@pytest.mark.parametrize('n_words', UNITS)
def test_pairs_equal_mbr_host_every_byte_word(eng, n_words):
    for counts in _lengths(n_words):
        case = mc.words_case(200 + n_words, counts)
        assert (case['labels'].shape[2] + 1) // 2 == max(n_words, 1)     # the width makes n_words the unit bound, which picks NC
        want = _run(eng, case, 'word', what=f'words={n_words} K={len(counts[0])}')
        assert (want.ok == 1).all() and want.dist[1, 0, -1] == n_words


@pytest.mark.parametrize('n_words', [65, 700, 1025])
def test_longer_words(eng, n_words):
    f = n_words - 5
    case = mc.words_case(300 + n_words, [[n_words, f, n_words], [f, n_words, 1]], max_len=3)
    want = _run(eng, case, 'word', what=f'long words={n_words}')
    assert want.dist[0, 0, 2] > 0
    _run(eng, case, 'char', what=f'long words={n_words}')


def test_words_and_chunk_boundaries(eng):
    """a word across the 64-id chunk boundary, a word of more than 64 ids, whitespace at ids 63 and 64, words of equal length
    with a common prefix that differ in the last id"""
    sp, a, b, c = 0, 1, 2, 3
    long_word = [a, b] * 50
    rows = [[[a] * 3 + [sp] + [b] * 58 + [sp] + [c] * 10 + [sp, a],              # ids 61 .. 71 are one word
             [a] * 3 + [sp] + [b] * 58 + [sp] + [c] * 9 + [b, sp, a],
             [a] * 3 + [sp, sp] + [b] * 58 + [sp] + [c] * 10 + [sp, a, sp]],
            [long_word + [sp] + long_word[:-1] + [c] + [sp, b],                 # two 100-id words that differ in the last id
             long_word[:-1] + [c] + [sp] + long_word[:-1] + [c] + [sp, sp, b],
             long_word + [sp] + long_word + [sp, b]],
            [[a] * 63 + [sp, sp] + [b] * 5 + [sp], [a] * 63 + [sp] + [a] + [b] * 5, [a] * 64],
            [[sp] * 64 + [a] + [sp] * 63 + [b], [a, sp, b], [a] * 128 + [sp] + [b]]]
    case = mc.from_lists(rows, [[-70000, -90000, -95000]] * 4)
    want = _run(eng, case, 'word', what='boundaries')
    assert want.dist[:, 0, 1].tolist() == [1, 1, 1, 0] and want.dist[:, 0, 2].tolist() == [0, 1, 2, 1]
    _run(eng, case, 'char', what='boundaries')
    _run(eng, case, 'word', wide=True, dist=False, what='boundaries, wide rows, no dist')


@pytest.mark.parametrize('K,B', [(16, 1), (16, 5), (128, 1), (128, 5), (1, 1), (1, 5)])
@pytest.mark.parametrize('mode', ['char', 'word'])
def test_larger_lists(eng, K, B, mode):
    case = mc.nbest(50 + K + B, 29, B=B, K=K, L=40, min_len=10, sort=False)
    want = _run(eng, case, mode, what=f'K={K} B={B}')
    if K == 1:
        assert (want.order == 0).all() and (want.risk == 0).all() and (want.dist == 0).all() and (want.wsum == 1 << 24).all()
    else:
        assert (want.order[:, 0] != 0).any() or B == 1


@pytest.mark.parametrize('C_', mc.CLASSES)
@pytest.mark.parametrize('mode', ['char', 'word'])
@pytest.mark.parametrize('scale', [0.0, 1.0, 16.0])
def test_classes_pitches_scales_and_no_dist(eng, C_, mode, scale):
    case = mc.nbest(40 + C_, C_, B=7, K=6, L=150, min_len=20, spread=2.0 if C_ != 2 else 0.3, edit_p=0.2 if C_ != 2 else 0.5)
    want = _run(eng, case, mode, scale, wide=True, what=f'C={C_} wide scale={scale}')
    _run(eng, case, mode, scale, dist=False, what=f'C={C_} no dist scale={scale}')
    assert (want.ok == 1).all() and (want.weight[:, 0] == 1 << 24).all()
    if scale == 0.0:
        assert (want.weight == 1 << 24).all()


@pytest.mark.parametrize('mode', ['char', 'word'])
def test_absent_and_invalid_rows_between_valid_ones(eng, mode):
    case = mc.nbest(77, 29, B=7, K=4, L=90, min_len=30, sort=False)
    case['n_hyps'] = np.array([4, 1, 0, 4, 3, 4, 4], dtype=np.int32)
    case['labels'][1, 2, 0] = 29                                    # absent: its bad id is not looked at
    case['labels'][3, 1, 0] = -1                                    # invalid between valid rows
    case['n_labels'][3, 1] = max(case['n_labels'][3, 1], 1)
    case['n_labels'][4, 0] = 91                                     # a length outside the row
    case['score'][5, 2] = -(1 << 62)                                # the beam's empty slot inside n_hyps
    case['score'][5, 3] = -(1 << 61)
    case['score'][6, :] = -(1 << 62)                                # no present row
    want = _run(eng, case, mode, what='present rows')
    assert want.ok.tolist() == [[1] * 4, [1, 2, 2, 2], [2] * 4, [1, 0, 1, 1], [0, 1, 1, 2], [1, 1, 0, 0], [0] * 4]
    assert want.pick.tolist()[1:3] == [0, -1] and want.pick[6] == -1
    _run(eng, dict(case, n_hyps=None), mode, dist=False, what='present rows, no n_hyps')


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_launch_nothing(eng):
    lib = eng.load_library()
    B, K, C_, L = 2, 3, 29, 12
    labels = torch.ones(B * K, L, dtype=torch.int32, device='cuda')
    n_labels = torch.full((B * K,), 5, dtype=torch.int32, device='cuda')
    score = torch.arange(B * K, dtype=torch.int64, device='cuda') * -40000
    sp = torch.zeros(C_, dtype=torch.uint8, device='cuda')
    tab = eng.mbr_table_device('cuda')
    out = _filled(B, K)
    need = eng.mbr_workspace_bytes(B, K, L, 'word')
    assert need > 0 and eng.mbr_workspace_bytes(B, K, L, 'char') > 0
    ws = torch.full((need + 16,), 0x5a, dtype=torch.uint8, device='cuda')
    size = C.sizeof(eng.MbrArgs)

    def args(**kw):
        a = eng.MbrArgs()
        a.struct_size, a.mode, a.B, a.K, a.C, a.max_ids, a.scale_q, a.wtab_entries, a.label_pitch = size, 1, B, K, C_, L, 1 << 16, 16384, L
        a.labels, a.n_labels, a.score, a.is_space, a.wtab = labels.data_ptr(), n_labels.data_ptr(), score.data_ptr(), sp.data_ptr(), tab.data_ptr()
        for n in NAMES:
            setattr(a, n, getattr(out, n).data_ptr())
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(struct_size=size + 8), dict(struct_size=size - 8)]
    bad += [{f: None} for f in ('labels', 'n_labels', 'score', 'wtab', 'weight', 'wsum', 'risk', 'order', 'ok', 'workspace', 'is_space')]
    bad += [dict(mode=2), dict(mode=-1), dict(B=0), dict(K=0), dict(K=129), dict(C=0), dict(max_ids=0), dict(max_ids=65537, label_pitch=1 << 17),
            dict(B=1 << 12, K=128), dict(scale_q=-1), dict(scale_q=(16 << 16) + 1), dict(wtab_entries=16383), dict(wtab_entries=0),
            dict(label_pitch=L - 1), dict(workspace_bytes=need - 1), dict(workspace=ws.data_ptr() + 8), dict(wsum=out.wsum.data_ptr() + 4),
            dict(risk=out.risk.data_ptr() + 4), dict(dist=out.dist.data_ptr() + 2), dict(weight=out.weight.data_ptr() + 2),
            dict(order=out.order.data_ptr() + 1), dict(ok=out.ok.data_ptr() + 2)]
    for kw in bad:
        assert lib.qasr_ctc_mbr(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_mbr(s, None) == 1
    for shape in ((0, K, L, 1), (B, 0, L, 0), (B, 129, L, 0), (B, K, 0, 0), (B, K, 65537, 0), (B, K, L, 2), (1 << 12, 128, L, 0)):
        assert lib.qasr_mbr_workspace_bytes(*shape) == 0, shape
    lab3 = labels.view(B, K, L)
    with pytest.raises(ValueError, match='mode'):
        eng.mbr_rerank(lab3, n_labels.view(B, K), score.view(B, K), None, C_, mode='phone')
    with pytest.raises(ValueError, match='word mode needs is_space'):
        eng.mbr_rerank(lab3, n_labels.view(B, K), score.view(B, K), None, C_, mode='word')
    with pytest.raises(ValueError, match='mbr_scale'):
        eng.mbr_rerank(lab3, n_labels.view(B, K), score.view(B, K), None, C_, mode='char', scale=16.5)
    with pytest.raises(ValueError, match='score must be'):
        eng.mbr_rerank(lab3, n_labels.view(B, K), score, None, C_, mode='char')
    torch.cuda.synchronize()
    for n in NAMES:
        t = getattr(out, n)
        assert (t == (FILL64 if t.dtype == torch.int64 else FILL32)).all(), n
    assert (ws == 0x5a).all()
    # the same arguments, unbroken, are taken; char mode needs no mask; without dist the matrix lives in the workspace
    for kw in (dict(), dict(dist=None), dict(mode=0, is_space=None)):
        assert lib.qasr_ctc_mbr(s, C.byref(args(**kw))) == 0, kw
        torch.cuda.synchronize()
        want = mbr.mbr_host(lab3.cpu().numpy(), n_labels.view(B, K).cpu().numpy(), score.view(B, K).cpu().numpy(), None, C_,
                            mode='char' if 'mode' in kw else 'word', is_space=np.zeros(C_, dtype=np.uint8))
        _equal(out, want, str(kw))


# ---------------------------------------------------------------------------------------------------------------- graph
def test_topn_beam_mbr_chain_is_capturable(eng):
    """nothing is allocated and nothing is read on the host: qasr_ctc_topn -> qasr_ctc_beam -> qasr_ctc_mbr replays from a graph on
    new log-probabilities in the same buffer, and equals the twin over the twin's beam on every byte"""
    T, B, W, NB, N, blank = 60, 3, 8, 4, 20, 28
    rng = np.random.Generator(np.random.PCG64(95))
    lps = [np.stack([beam_cases.peaky_logp(rng, T, 29, blank, blend=True) for _ in range(B)]) for _ in range(3)]
    mask = mc.space_mask(blank)
    lp_d = _cuda(lps[0])
    cand = (torch.empty(B, T, N, dtype=torch.int32, device='cuda'), torch.empty(B, T, N, dtype=torch.int32, device='cuda'))
    first = eng.ctc_beam_search(lp_d, None, blank, W, NB, N)         # the tables are uploaded and the result's layout is taken
    res = beam.BeamResult(torch.full_like(first.labels, FILL32), torch.full_like(first.n_labels, FILL32),
                          torch.full_like(first.score, FILL64), torch.full_like(first.n_hyps, FILL32), blank)
    bws = torch.empty(eng.ctc_beam_workspace_bytes(B, T, W), dtype=torch.uint8, device='cuda')
    mws = torch.empty(eng.mbr_workspace_bytes(B, NB, T, 'word'), dtype=torch.uint8, device='cuda')
    out = _filled(B, NB)
    sp_d = _cuda(mask)
    eng.lae_table_device('cuda'), eng.mbr_table_device('cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.ctc_topn(lp_d, None, N, out=cand)
            eng.ctc_beam(cand[0], cand[1], None, blank, W, NB, workspace=bws, out=res)
            eng.mbr_rerank(res.labels, res.n_labels, res.score, res.n_hyps, blank, mode='word', is_space=sp_d, workspace=mws, out=out)
    for lp in (lps[1], lps[0], lps[2]):
        lp_d.copy_(torch.from_numpy(lp))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = beam.search_host(lp, None, blank, W, NB, N)
        want = mbr.mbr_host(host.labels, host.n_labels, host.score, host.n_hyps, blank, mode='word', is_space=mask)
        assert (want.ok == 1).sum() >= 2 * B
        _equal(out, want, 'replay')
