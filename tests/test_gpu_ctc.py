"""Greedy CTC decoding on an MI355X: k_ctc (csrc/qasr_ctc.hip) against qasr.ctc.collapse_host bit for bit, the per-frame
best-path score of the three decoder kernels against the log-probabilities of the same run, and the engine attachment
(eager, graph replay, re-capture, detach) on mini nets and on full-size QuartzNet15x5 En / Zh."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctc_cases  # noqa: E402
from qasr import ctc, pack, synth, topology  # noqa: E402


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_result_equal(got, want, what=''):
    for name in ('labels', 'n_labels', 'start', 'nframes', 'score', 'utt_score'):
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        assert w is not None, name
        assert np.array_equal(_bits(g), _bits(w)), (what, name)


# ------------------------------------------------------------------------------------------------ k_ctc stand-alone
def _matrices(B, T, n_labels, seed):
    """Token matrices of B rows that together hold every adversarial row (all blank / one run over every chunk / every
    frame emits / first and last frame emit) and realistic rows"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = ctc_cases.adversarial_rows(rng, T, n_labels)
    while len(rows) < max(B, 6) or len(rows) % B:
        rows.append(ctc_cases.realistic_row(rng, T, n_labels, first_emits=len(rows) % 2 == 0))
    rows = np.stack(rows)
    return [rows[i:i + B] for i in range(0, len(rows), B)]


@pytest.mark.parametrize('T', [1, 63, 64, 65, 250, 1000, 4097])
@pytest.mark.parametrize('B', [1, 3, 32])
def test_k_ctc_equals_collapse_host_bit_for_bit(eng, B, T):
    for n_labels in (28, 5206):
        for rep, tok in enumerate(_matrices(B, T, n_labels, 100 * T + B)):
            fs = ctc_cases.frame_scores(T + B + rep, tok.shape)
            rng = np.random.default_rng(T * 31 + B + rep)
            lens = rng.integers(0, T + 1, size=B).astype(np.int32)
            if B > 1:
                lens[0], lens[-1] = 0, T + 3                 # nothing; beyond the row: clamps
            elif rep == 0:
                lens[0] = T
            tok_d, fs_d, lens_d = torch.from_numpy(tok).cuda(), torch.from_numpy(fs).cuda(), torch.from_numpy(lens).cuda()
            for use_lens in (False, True):
                for use_fs in (False, True):
                    got = eng.ctc_collapse(tok_d, fs_d if use_fs else None, lens_d if use_lens else None, blank=n_labels)
                    torch.cuda.synchronize()
                    want = ctc.collapse_host(tok, fs if use_fs else None, lens if use_lens else None, blank=n_labels)
                    _assert_result_equal(got, want, (n_labels, rep, use_lens, use_fs))
                    assert (got.score is None) == (not use_fs)
            # optional outputs null: only labels / n_labels are written; and the scores without the times
            out = eng.ctc_buffers(B, T, 'cuda', scores=False, blank=n_labels)
            out.start = out.nframes = None
            got = eng.ctc_collapse(tok_d, fs_d, lens_d, blank=n_labels, out=out)
            only_score = eng.ctc_buffers(B, T, 'cuda', scores=True, blank=n_labels)
            only_score.start = only_score.nframes = only_score.utt_score = None
            got2 = eng.ctc_collapse(tok_d, fs_d, lens_d, blank=n_labels, out=only_score)
            torch.cuda.synchronize()
            _assert_result_equal(got, want)
            _assert_result_equal(got2, want)


def test_k_ctc_on_the_reference_fixture(eng, golden_dir):
    d = np.load(os.path.join(golden_dir, 'ctc_decode.npz'))
    for c in json.loads(str(d['meta']))['cases']:
        tok = d['tokens_' + c['name']]
        got = eng.ctc_collapse(torch.from_numpy(tok).cuda(), blank=c['n_labels'])
        torch.cuda.synchronize()
        _assert_result_equal(got, ctc.collapse_host(tok, blank=c['n_labels']), c['name'])
        texts = [h.text for h in ctc.to_hypotheses(got, ctc_cases.vocabulary(c['n_labels']), 0.02)]
        assert texts == json.loads(str(d['hyps_' + c['name']])), c['name']


def test_argument_errors_launch_nothing(eng):
    tok = torch.zeros(2, 8, dtype=torch.int32, device='cuda')
    out = eng.ctc_buffers(2, 8, 'cuda', scores=True, blank=3)
    with pytest.raises(eng.QasrError, match='frame_score'):
        eng.ctc_collapse(tok, None, None, blank=3, out=out)              # score / utt_score without frame_score
    lib = eng.load_library()
    import ctypes as C
    o = eng._ctc_out_struct(eng.ctc_buffers(2, 8, 'cuda', scores=False, blank=3))
    s = eng._stream_ptr()
    assert lib.qasr_ctc_collapse(s, C.c_void_p(tok.data_ptr()), None, None, 2, 0, 3, C.byref(o)) == 1      # T < 1
    assert lib.qasr_ctc_collapse(s, C.c_void_p(tok.data_ptr()), None, None, 0, 8, 3, C.byref(o)) == 1      # B < 1
    assert lib.qasr_ctc_collapse(s, None, None, None, 2, 8, 3, C.byref(o)) == 1
    assert lib.qasr_ctc_collapse(s, C.c_void_p(tok.data_ptr()), None, None, 2, 8, 3, None) == 1
    o.struct_size += 8
    assert lib.qasr_ctc_collapse(s, C.c_void_p(tok.data_ptr()), None, None, 2, 8, 3, C.byref(o)) == 1
    assert b'struct_size' in lib.qasr_last_error()
    o.struct_size -= 8
    o.labels = None
    assert lib.qasr_ctc_collapse(s, C.c_void_p(tok.data_ptr()), None, None, 2, 8, 3, C.byref(o)) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ decoder frame scores
def _ranges(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name + '.npz'))
    return d['act_min'], d['act_max'], json.loads(str(d['meta']))


def _mini_wide(width):
    n = width - 1
    return dataclasses.replace(topology.mini_quartznet(), num_classes=n, vocabulary=topology.zh_placeholder_vocabulary(n))


MINI_LENS = [256, 128, 66, 1]


def _mini_k_dec():
    """MiniQuartzNet with a 256-channel last block: k_dec takes decoder inputs of a multiple of 256 channels (the stock
    mini net's 64 go to the generic path).  The fixture's ranges stay valid quantiser settings for it."""
    cfg = topology.mini_quartznet()
    return dataclasses.replace(cfg, blocks=cfg.blocks[:-1] + [dataclasses.replace(cfg.blocks[-1], filters=256)])


@pytest.mark.parametrize('case', ['k_dec', 'k_logsoftmax', 'k_decw_5207', 'k_decw_1000', 'k_logsoftmax_1000'])
def test_frame_score_is_the_logp_of_the_token_bit_for_bit(eng, golden_dir, case):
    width = {'k_dec': 29, 'k_logsoftmax': 29, 'k_decw_5207': 5207, 'k_decw_1000': 1000, 'k_logsoftmax_1000': 1000}[case]
    amin, amax, meta = _ranges(golden_dir, 'net_miniq_wide_w8a8' if width == 5207 else 'net_miniq_w8a8')
    cfg = _mini_k_dec() if width == 29 else _mini_wide(width)
    blob, _ = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), amin, amax, 8, 8)
    kw = dict(fuse_decoder=False) if 'logsoftmax' in case else {}
    x = torch.from_numpy(synth.make_features(len(MINI_LENS), cfg.feat_in, max(MINI_LENS), 5)).cuda()
    lens = torch.tensor(MINI_LENS)
    plain = eng.Engine(blob, 0, **kw)                        # never has anything attached
    lp0, tk0, el0 = plain.forward(x, lens)
    _, tk0n, el0n = plain.forward(x, lens, want_logp=False)
    torch.cuda.synchronize()
    n0 = plain.num_launches()
    kernel = case.split('_')[0] + '_' + case.split('_')[1]
    assert kernel in plain.op_labels(), plain.op_labels()[-3:]
    e = eng.Engine(blob, 0, **kw)
    To = e.out_frames(x.shape[2])
    fs = torch.full((len(MINI_LENS), To), 7.0, device='cuda')
    e.attach_ctc(frame_score=fs)
    for want_logp in (True, False):                          # k_decw: its tokens-only form returns before the GEMM
        fs.fill_(7.0)
        lp, tk, el = e.forward(x, lens, want_logp=want_logp)
        torch.cuda.synchronize()
        assert e.num_launches() == n0                        # frame_score alone: no launch more
        assert torch.equal(tk, tk0) and torch.equal(el, el0)
        if want_logp:
            assert torch.equal(lp.view(torch.int32), lp0.view(torch.int32))
        want = lp0.gather(2, tk0.long().unsqueeze(-1)).squeeze(-1)
        assert torch.equal(fs.view(torch.int32), want.view(torch.int32)), (case, want_logp)
        assert float(fs.max()) <= 0.0
    e.detach_ctc()
    fs.fill_(7.0)
    lp, tk, el = e.forward(x, lens)
    torch.cuda.synchronize()
    assert float(fs.min()) == 7.0                            # detached: the buffer is the caller's again
    assert torch.equal(lp.view(torch.int32), lp0.view(torch.int32)) and torch.equal(tk, tk0) and torch.equal(tk0n, tk0)
    assert torch.equal(el0n, el0)
    plain.close()
    e.close()


# ------------------------------------------------------------------------------------------------ engine attachment
def _host_of(tokens, fs, enc_len, blank):
    return ctc.collapse_host(tokens.cpu().numpy(), fs.cpu().numpy(), enc_len.cpu().numpy(), blank=blank)


def _attachment_roundtrip(eng, blob, x, lens, ncls, tokens_only):
    """eager decode=, graph replay with caller-owned buffers, re-capture after a pointer change, detach"""
    blank = ncls - 1
    plain = eng.Engine(blob, 0)
    lp0, tk0, el0 = plain.forward(x, lens)
    torch.cuda.synchronize()
    n0 = plain.num_launches()
    want_fs = lp0.gather(2, tk0.long().unsqueeze(-1)).squeeze(-1)
    e = eng.Engine(blob, 0)
    lp, tk, el, res = e.forward(x, lens, want_logp=not tokens_only, decode=True)
    torch.cuda.synchronize()
    assert e.num_launches() == n0 + 1
    assert torch.equal(tk, tk0) and torch.equal(el, el0)
    assert torch.equal(res.frame_score.view(torch.int32), want_fs.view(torch.int32))
    want = _host_of(tk, res.frame_score, el, blank)
    _assert_result_equal(res, want, 'eager')
    assert int(want.n_labels.sum()) > 0
    if tokens_only:
        assert lp is None
    # ragged lengths matter: some row stops before the padded row's last emission
    full = ctc.collapse_host(tk.cpu().numpy(), None, None, blank=blank)
    assert (full.n_labels >= want.n_labels).all()
    lp1, tk1, el1 = e.forward(x, lens)                       # decode= dropped again: the default call is what it was
    torch.cuda.synchronize()
    assert e.num_launches() == n0 and torch.equal(tk1, tk0) and torch.equal(lp1.view(torch.int32), lp0.view(torch.int32))
    e.close()

    g = eng.Engine(blob, 0, graph=True)
    B, To = x.shape[0], g.out_frames(x.shape[2])
    out = (None if tokens_only else torch.empty(B, To, ncls, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))
    bufs = eng.ctc_buffers(B, To, 'cuda', scores=True, blank=blank)
    side = torch.cuda.Stream()
    lens_d = lens.to(device='cuda', dtype=torch.int32)
    g.attach_ctc(bufs.frame_score, bufs, use_lens=True)
    for it in range(7):                                      # direct, capture, replay, replay | new score buffer: direct, capture, replay
        if it == 4:
            bufs.score = torch.empty_like(bufs.score)        # one attached pointer changes: the graph is dropped
            g.attach_ctc(bufs.frame_score, bufs, use_lens=True)
        for t in (bufs.labels, bufs.n_labels, bufs.start, bufs.nframes, bufs.score, bufs.utt_score, bufs.frame_score, out[1]):
            t.fill_(-3)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            _, tkg, elg = g.forward(x, lens_d, want_logp=not tokens_only, out=out)
        torch.cuda.synchronize()
        assert g.num_launches() == n0 + 1
        assert torch.equal(tkg, tk0) and torch.equal(elg, el0), it
        assert torch.equal(bufs.frame_score.view(torch.int32), want_fs.view(torch.int32)), it
        _assert_result_equal(bufs, want, f'graph call {it}')
    g.detach_ctc()
    for t in (bufs.labels, bufs.frame_score):
        t.fill_(-3)
    with torch.cuda.stream(side):
        _, tkg, elg = g.forward(x, lens_d, want_logp=not tokens_only, out=out)
    torch.cuda.synchronize()
    assert g.num_launches() == n0 and torch.equal(tkg, tk0)
    assert int((bufs.labels != -3).sum()) == 0 and float(bufs.frame_score.max()) == -3.0
    # a qasr_ctc_out is attached: tokens are required
    g.attach_ctc(bufs.frame_score, bufs)
    with pytest.raises(eng.QasrError, match='tokens'):
        g.forward(x, lens_d, out=(out[0], None, out[2]))
    g.close()
    plain.close()
    return want


@pytest.mark.parametrize('width', [29, 1000])
def test_attachment_on_mini_nets(eng, golden_dir, width):
    amin, amax, meta = _ranges(golden_dir, 'net_miniq_w8a8')
    cfg = _mini_k_dec() if width == 29 else _mini_wide(width)
    blob, _ = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), amin, amax, 8, 8)
    x = torch.from_numpy(synth.make_features(len(MINI_LENS), cfg.feat_in, max(MINI_LENS), 5)).cuda()
    _attachment_roundtrip(eng, blob, x, torch.tensor(MINI_LENS), width, tokens_only=False)


@pytest.mark.parametrize('model', ['En', 'Zh'])
def test_attachment_full_size_bs32_x_500(eng, golden_dir, model):
    amin, amax, meta = _ranges(golden_dir, 'net_quartznet_w8a8')
    cfg = topology.quartznet15x5() if model == 'En' else topology.quartznet15x5_zh()
    ncls = cfg.num_classes + 1
    blob, pm = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), amin, amax, 8, 8)
    B, T = 32, 500
    x = torch.from_numpy(synth.make_features(B, 64, T, 23)).cuda()
    rng = np.random.default_rng(9)
    lens = rng.integers(1, T + 1, size=B)
    lens[:4] = [500, 129, 1, 64]
    lens = torch.tensor(lens, dtype=torch.int32)
    want = _attachment_roundtrip(eng, blob, x, lens, ncls, tokens_only=False)
    if model == 'Zh':
        # tokens-only with frame_score + decode: what a log-prob run gives, and still no float-logits / log-prob buffer
        want2 = _attachment_roundtrip(eng, blob, x, lens, ncls, tokens_only=True)
        _assert_result_equal(want2, want)
        e = eng.Engine(blob, 0)
        _, tk, el, res = e.forward(x, lens, want_logp=False, decode=True)
        torch.cuda.synchronize()
        _assert_result_equal(res, want, 'tokens-only')
        assert 'k_decw' in e.op_labels()
        with pytest.raises(Exception, match='never materialised'):
            e.read_tensor(pm['n_tensors'] - 1, ncls, dtype=np.float32)
        e.close()


def test_attach_refuses_what_it_cannot_serve(eng, golden_dir):
    amin, amax, meta = _ranges(golden_dir, 'net_miniq_w8a8')
    cfg = topology.mini_quartznet()
    blob, _ = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), amin, amax, 8, 8)
    e = eng.Engine(blob, 0)
    bufs = eng.ctc_buffers(4, 128, 'cuda', scores=True, blank=28)
    with pytest.raises(eng.QasrError, match='frame_score'):
        e.attach_ctc(None, bufs)                             # score / utt_score without frame_score
    bufs.score = bufs.utt_score = None
    e.attach_ctc(None, bufs)                                 # labels and times alone are fine
    x = torch.from_numpy(synth.make_features(4, cfg.feat_in, 256, 5)).cuda()
    _, tk, el = e.forward(x, torch.tensor(MINI_LENS))
    torch.cuda.synchronize()
    _assert_result_equal(bufs, ctc.collapse_host(tk.cpu().numpy(), None, el.cpu().numpy(), blank=28))
    e.attach_ctc(None, bufs, use_lens=False)                 # the padded row, like the reference
    _, tk, el = e.forward(x, torch.tensor(MINI_LENS))
    torch.cuda.synchronize()
    _assert_result_equal(bufs, ctc.collapse_host(tk.cpu().numpy(), None, None, blank=28))
    e.close()
