"""CTC prefix beam search on an MI355X: k_topn and k_beam (csrc/qasr_beam.hip) against their NumPy statements
qasr.beam.topn_host / beam_search_host, every byte, no tolerance and no case left out; refused arguments launch nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_cases  # noqa: E402
from qasr import beam  # noqa: E402


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


# ------------------------------------------------------------------------------------------------------------ k_topn
@pytest.mark.parametrize('C_', [2, 29, 64, 65, 5207, 8192])
def test_k_topn_equals_topn_host_every_byte(eng, C_):
    B, T = 3, 37
    rng = np.random.default_rng(C_)
    blocks = [beam_cases.tie_rows(C_ + 1, B * T, C_).reshape(B, T, C_),
              np.stack([beam_cases.peaky_logp(rng, T, C_, C_ - 1) for _ in range(B)])]
    special = blocks[1].copy()                           # the values a real decoder never writes still have an order
    special[0, 0, :2] = [np.nan, -np.inf]
    special[0, 1, 0] = np.inf
    special[1, 3, :] = -np.inf
    special[2, 5, :] = -200.0
    blocks.append(special)
    for k, lp in enumerate(blocks):
        lens = _lens(rng, B, T)
        lp_d, lens_d = torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda()
        # the same values inside a larger allocation: utterance and frame pitches that are not T * C and C
        wide = torch.full((B, T + 3, C_ + 7), 7.0, device='cuda')
        wide[:, :T, :C_] = lp_d
        for N in (1, 20, 40, 64):
            for use_lens in (False, True):
                want_id, want_q = beam.topn_host(lp, N, lens if use_lens else None)
                for src in (lp_d, wide[:, :T, :C_]):
                    cid = torch.full((B, T, N), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
                    cq = torch.full((B, T, N), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
                    eng.ctc_topn(src, lens_d if use_lens else None, N, out=(cid, cq))
                    torch.cuda.synchronize()
                    assert np.array_equal(cid.cpu().numpy(), want_id), (k, N, use_lens, 'ids')
                    assert np.array_equal(cq.cpu().numpy(), want_q), (k, N, use_lens, 'q')
        assert (wide[:, T:, :] == 7.0).all() and (wide[:, :, C_:] == 7.0).all()


def test_k_topn_refuses_bad_arguments_and_writes_nothing(eng):
    lib = eng.load_library()
    lp = torch.zeros(2, 8, 29, device='cuda')
    cid = torch.full((2, 8, 20), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    cq = cid.clone()

    def args(**kw):
        a = eng.TopnArgs()
        a.struct_size = C.sizeof(eng.TopnArgs)
        a.B, a.T, a.C, a.N, a.pitch_utt, a.pitch_frame = 2, 8, 29, 20, 8 * 29, 29
        a.log_probs, a.cand_id, a.cand_q = lp.data_ptr(), cid.data_ptr(), cq.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    assert lib.qasr_ctc_topn(s, C.byref(args())) == 0
    torch.cuda.synchronize()
    cid.fill_(0x5a5a5a5a), cq.fill_(0x5a5a5a5a)
    for kw in (dict(struct_size=8), dict(B=0), dict(T=0), dict(T=65537), dict(C=0), dict(N=0), dict(N=65), dict(pitch_frame=28),
               dict(pitch_utt=8 * 29 - 1), dict(log_probs=None), dict(cand_id=None), dict(cand_q=None)):
        assert lib.qasr_ctc_topn(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_topn(s, None) == 1
    torch.cuda.synchronize()
    assert (cid == 0x5a5a5a5a).all() and (cq == 0x5a5a5a5a).all()


# ------------------------------------------------------------------------------------------------------------ k_beam
def _assert_beam_equal(got, want, what):
    for name in ('labels', 'n_labels', 'score', 'n_hyps'):
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


def _filled_out(eng, B, nb, T, blank):
    i32 = dict(dtype=torch.int32, device='cuda')
    return beam.BeamResult(labels=torch.full((B, nb, T), 0x5a5a5a5a, **i32), n_labels=torch.full((B, nb), 0x5a5a5a5a, **i32),
                           score=torch.full((B, nb), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device='cuda'),
                           n_hyps=torch.full((B,), 0x5a5a5a5a, **i32), blank=blank)


def _slice(want, nb):
    return beam.BeamResult(want.labels[:, :nb], want.n_labels[:, :nb], want.score[:, :nb], np.minimum(want.n_hyps, nb).astype(np.int32),
                           want.blank)


@pytest.mark.parametrize('T', [1, 63, 64, 65, 250, 1000])
@pytest.mark.parametrize('W', [1, 2, 16, 128])
def test_k_beam_equals_beam_search_host_every_byte(eng, W, T):
    for C_, N in ((29, 20), (29, 40), (5207, 40), (5207, 64)):
        B = 4 if C_ == 29 else 3
        rng = np.random.Generator(np.random.PCG64(1000 * T + W + C_))
        lp = np.stack([beam_cases.peaky_logp(rng, T, C_, C_ - 1, blend=(i % 2 == 1)) for i in range(B)])
        lens = _lens(rng, B, T)
        cid, cq = beam.topn_host(lp, N, None)            # candidates on every frame, so that lens decides where to stop
        cid_d, cq_d, lens_d = torch.from_numpy(cid).cuda(), torch.from_numpy(cq).cuda(), torch.from_numpy(lens).cuda()
        ws = torch.empty(eng.ctc_beam_workspace_bytes(B, T, W), dtype=torch.uint8, device='cuda')
        for use_lens in (True, False):
            want = beam.beam_search_host(cid, cq, lens if use_lens else None, C_ - 1, W)
            assert want.n_hyps.max() >= 1 and (use_lens is False or want.n_hyps[1] == 1)
            for nb in range(1, W + 1):                  # every n_best, at every length
                out = _filled_out(eng, B, nb, T, C_ - 1)
                eng.ctc_beam(cid_d, cq_d, lens_d if use_lens else None, C_ - 1, W, nb, workspace=ws, out=out)
                torch.cuda.synchronize()
                _assert_beam_equal(out, _slice(want, nb), (C_, N, use_lens, nb))
            again = _filled_out(eng, B, W, T, C_ - 1)
            eng.ctc_beam(cid_d, cq_d, lens_d if use_lens else None, C_ - 1, W, W, workspace=ws, out=again)
            torch.cuda.synchronize()
            _assert_beam_equal(again, want, (C_, N, use_lens, 'second call'))


def test_k_beam_on_candidates_no_top_n_would_write(eng):
    """duplicate, negative and out-of-vocabulary ids, several blanks, arbitrary q: the kernel follows the stated rules (first
    match counts, empty slots are skipped) and stays inside its buffers"""
    B, T, N, W, blank = 3, 40, 12, 16, 7
    rng = np.random.default_rng(5)
    cid = rng.integers(-2, 10, size=(B, T, N)).astype(np.int32)
    cq = rng.integers(-(1 << 22), 1, size=(B, T, N)).astype(np.int32)
    cq[0, 5] = beam.EMPTY_Q
    cid[1, 7] = -1                                        # a frame without candidates: the beam dies there
    want = beam.beam_search_host(cid, cq, None, blank, W)
    assert want.n_hyps[1] == 0
    out = _filled_out(eng, B, W, T, blank)
    eng.ctc_beam(torch.from_numpy(cid).cuda(), torch.from_numpy(cq).cuda(), None, blank, W, W, out=out)
    torch.cuda.synchronize()
    _assert_beam_equal(out, want, 'garbage')


def test_k_beam_ties_at_the_cut(eng):
    """few distinct q values: many candidates share the score at the W-th place, and the candidate index decides"""
    B, T, N, blank = 4, 30, 8, 11
    rng = np.random.default_rng(21)
    cid = np.stack([np.stack([rng.permutation(12)[:N] for _ in range(T)]) for _ in range(B)]).astype(np.int32)
    cq = (-65536 * rng.integers(0, 3, size=(B, T, N))).astype(np.int32)
    cq[0] = 0                                             # every candidate of every frame ties
    cid_d, cq_d = torch.from_numpy(cid).cuda(), torch.from_numpy(cq).cuda()
    for W in (1, 2, 16, 128):
        want = beam.beam_search_host(cid, cq, None, blank, W)
        out = _filled_out(eng, B, W, T, blank)
        eng.ctc_beam(cid_d, cq_d, None, blank, W, W, out=out)
        torch.cuda.synchronize()
        _assert_beam_equal(out, want, ('ties', W))


def test_k_topn_then_k_beam_equal_the_host_search(eng):
    rng = np.random.default_rng(9)
    lp = np.stack([beam_cases.peaky_logp(rng, 120, 5207, 5206, blend=True) for _ in range(2)])
    lens = np.array([120, 77], dtype=np.int32)
    got = eng.ctc_beam_search(torch.from_numpy(lp).cuda(), torch.from_numpy(lens).cuda(), None, 16, 5, 40)
    torch.cuda.synchronize()
    _assert_beam_equal(got, beam.search_host(lp, lens, None, 16, 5, 40), 'chain')


def test_k_beam_refuses_bad_arguments_and_writes_nothing(eng):
    lib = eng.load_library()
    B, T, N, W, nb, blank = 2, 8, 20, 16, 4, 28
    cid = torch.zeros(B, T, N, dtype=torch.int32, device='cuda')
    cq = torch.zeros(B, T, N, dtype=torch.int32, device='cuda')
    out = _filled_out(eng, B, nb, T, blank)
    need = eng.ctc_beam_workspace_bytes(B, T, W)
    assert need > 0 and eng.ctc_beam_workspace_bytes(B, T, 129) == 0 and eng.ctc_beam_workspace_bytes(0, T, W) == 0
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device='cuda')
    tab = eng.lae_table_device('cuda')
    assert tab is eng.lae_table_device('cuda:%d' % torch.cuda.current_device()) is eng.lae_table_device(torch.device('cuda'))

    def args(**kw):
        a = eng.BeamArgs()
        a.struct_size = C.sizeof(eng.BeamArgs)
        a.B, a.T, a.N, a.beam_width, a.n_best, a.blank, a.lae_entries = B, T, N, W, nb, blank, beam.TAB_ENTRIES
        a.cand_id, a.cand_q, a.lae_table, a.workspace, a.workspace_bytes = cid.data_ptr(), cq.data_ptr(), tab.data_ptr(), ws.data_ptr(), need
        a.labels, a.n_labels, a.score, a.n_hyps = out.labels.data_ptr(), out.n_labels.data_ptr(), out.score.data_ptr(), out.n_hyps.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    s = eng._stream_ptr()
    bad = [dict(struct_size=8), dict(B=0), dict(T=0), dict(T=65537), dict(N=0), dict(N=65), dict(beam_width=0), dict(beam_width=129),
           dict(n_best=0), dict(n_best=W + 1), dict(blank=-1), dict(lae_entries=4096), dict(workspace_bytes=need - 1),
           dict(workspace_bytes=0)]
    bad += [{k: None} for k in ('cand_id', 'cand_q', 'lae_table', 'workspace', 'labels', 'n_labels', 'score', 'n_hyps')]
    for kw in bad:
        assert lib.qasr_ctc_beam(s, C.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error()
    assert lib.qasr_ctc_beam(s, None) == 1
    torch.cuda.synchronize()
    for t in (out.labels, out.n_labels, out.n_hyps):
        assert (t == 0x5a5a5a5a).all()
    assert (out.score == 0x5a5a5a5a5a5a5a5a).all() and (ws == 0x5a).all()
    assert lib.qasr_ctc_beam(s, C.byref(args())) == 0                      # and the same block unchanged is accepted
    torch.cuda.synchronize()
    assert (out.n_hyps.cpu().numpy() == nb).all()
