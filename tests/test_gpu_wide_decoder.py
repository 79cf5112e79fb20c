"""k_decw, the fused decoder for vocabularies wider than k_dec's 32 classes (csrc/qasr_decoder_wide.hip), on an MI355X:
mini nets with widened decoders and QuartzNet15x5Base-Zh (5206 labels + blank) against the CPU oracles and against the
generic two-launch path (k_sep logits + k_logsoftmax).  The calibrated ranges of the En / mini fixtures apply unchanged:
synth draws the decoder's weights last, so the encoders are the fixtures' own."""
import dataclasses
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import int_oracle as O  # noqa: E402
from qasr import pack, synth, topology  # noqa: E402


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()          # raises if the extension was not built: no silent fallback
    return engine


def _ranges(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name + '.npz'))
    return d['act_min'], d['act_max'], json.loads(str(d['meta']))


def _mini_wide(width):
    n = width - 1
    return dataclasses.replace(topology.mini_quartznet(), num_classes=n, vocabulary=topology.zh_placeholder_vocabulary(n))


def _check_valid_frames(logp, tokens, enc_len, want):
    wl = np.asarray(want['enc_len'])
    assert np.array_equal(np.asarray(enc_len), wl)
    for b in range(len(wl)):
        n = int(wl[b])
        assert np.array_equal(np.asarray(tokens)[b, :n], np.asarray(want['tokens'])[b, :n]), b
        np.testing.assert_allclose(np.asarray(logp)[b, :n], np.asarray(want['log_probs'])[b, :n], rtol=1e-4, atol=5e-5)


MINI_LENS = [256, 128, 66, 1]          # 128 / 64 / 33 / 1 encoder frames: the last valid frame on a tile edge, one past it


@pytest.mark.parametrize('width', [33, 129, 1000, 5207, 8171])
@pytest.mark.parametrize('fixture,bits', [('net_miniq_w8a8', 8), ('net_miniq_w6a6', 6)], ids=['w8a8', 'w6a6'])
def test_mini_net_widths_against_oracle(eng, golden_dir, width, fixture, bits):
    amin, amax, meta = _ranges(golden_dir, fixture)
    cfg = _mini_wide(width)
    sd = synth.make_state_dict(cfg, meta['seed'])
    blob, _ = pack.pack_model(cfg, sd, amin, amax, bits, bits)
    x = synth.make_features(len(MINI_LENS), cfg.feat_in, max(MINI_LENS), 5)
    want = O.OracleNet(topology.conv_plan(cfg), cfg, sd, amin, amax, bits, bits).forward(x, MINI_LENS)
    e = eng.Engine(blob, 0)
    logp, tokens, enc_len = e.forward(torch.from_numpy(x).cuda(), torch.tensor(MINI_LENS))
    torch.cuda.synchronize()
    labels = e.op_labels()
    assert 'k_decw' in labels and 'k_logsoftmax' not in labels and 'k_dec' not in labels, labels[-3:]
    assert logp.shape[2] == width
    _check_valid_frames(logp.cpu().numpy(), tokens.cpu().numpy(), enc_len.cpu().numpy(), want)
    e.close()


def test_debug_engine_decoder_accumulators_5207(eng, golden_dir):
    """Debug engine on the wide path: every decoder accumulator (read_acc) equals the oracle's integers, and the float
    logits tensor is materialised (read_tensor) as fl32(fl32(acc) * s_b)."""
    amin, amax, meta = _ranges(golden_dir, 'net_miniq_w8a8')
    cfg = _mini_wide(5207)
    sd = synth.make_state_dict(cfg, meta['seed'])
    blob, pm = pack.pack_model(cfg, sd, amin, amax, 8, 8)
    x = synth.make_features(len(MINI_LENS), cfg.feat_in, max(MINI_LENS), 6)
    net = O.OracleNet(topology.conv_plan(cfg), cfg, sd, amin, amax, 8, 8)
    want = net.forward(x, MINI_LENS)
    e = eng.Engine(blob, 0, debug=True)
    logp, tokens, enc_len = e.forward(torch.from_numpy(x).cuda(), torch.tensor(MINI_LENS))
    torch.cuda.synchronize()
    assert 'k_decw' in e.op_labels()
    op, pane = pm['sites'][-1]
    acc_want = net.trace[-1]['acc']
    got = e.read_acc(op, pane, 5207, acc_want.shape[2])
    wl = want['enc_len']
    T = int(enc_len.max())
    assert T == 128                              # T == Tp: read_tensor's [B][channels][Tp] buffer is the [B][T][C] logits
    logits = e.read_tensor(pm['n_tensors'] - 1, 5207, dtype=np.float32).reshape(len(wl), T, 5207)
    s_b = np.asarray(net.trace[-1]['s_b'], dtype=np.float32).reshape(-1)[:5207]
    for b in range(len(wl)):
        n = int(wl[b])
        assert np.array_equal(got[b, :, :n], acc_want[b, :, :n]), b
        # fl32(fl32(acc) * s_b) of the oracle's integers, bit for bit
        assert np.array_equal(logits[b, :n], (acc_want[b, :, :n].astype(np.float32) * s_b[:, None]).T), b
    _check_valid_frames(logp.cpu().numpy(), tokens.cpu().numpy(), enc_len.cpu().numpy(), want)
    e.close()


def test_equal_maxima_give_the_lower_class(eng, golden_dir):
    """torch.argmax's first maximum across lanes, waves and class groups: the decoder row of a class that wins frames is
    copied (weights and bias) to classes 32 (another wave), 128 (the same lane of the same wave) and far above it (the last
    class group), and once far below it.  Duplicates above never win; the duplicate below takes every frame its
    original won."""
    amin, amax, meta = _ranges(golden_dir, 'net_miniq_w8a8')
    cfg = _mini_wide(5207)
    sd = synth.make_state_dict(cfg, meta['seed'])
    x = synth.make_features(len(MINI_LENS), cfg.feat_in, max(MINI_LENS), 8)
    base = O.OracleNet(topology.conv_plan(cfg), cfg, sd, amin, amax, 8, 8).forward(x, MINI_LENS)
    valid = np.arange(base['tokens'].shape[1])[None, :] < np.asarray(base['enc_len'])[:, None]
    vals, counts = np.unique(base['tokens'][valid], return_counts=True)
    c0 = int(vals[np.argmax(np.where((vals >= 600) & (vals < 5000), counts, -1))])   # room below and above
    wk, bk = 'decoder.decoder_layers.0.weight', 'decoder.decoder_layers.0.bias'
    for dups, expect in (([c0 + 32, c0 + 128, 5205], c0), ([c0 - 517], c0 - 517)):
        sd2 = dict(sd)
        sd2[wk], sd2[bk] = sd[wk].copy(), sd[bk].copy()
        for c in dups:
            sd2[wk][c], sd2[bk][c] = sd[wk][c0], sd[bk][c0]
        want = O.OracleNet(topology.conv_plan(cfg), cfg, sd2, amin, amax, 8, 8).forward(x, MINI_LENS)
        wt = np.asarray(want['tokens'])
        assert np.array_equal(wt == expect, base['tokens'] == c0)                # the oracle's own first-maximum rule
        blob, _ = pack.pack_model(cfg, sd2, amin, amax, 8, 8)
        e = eng.Engine(blob, 0)
        logp, tokens, enc_len = e.forward(torch.from_numpy(x).cuda(), torch.tensor(MINI_LENS))
        torch.cuda.synchronize()
        assert 'k_decw' in e.op_labels()
        tk = tokens.cpu().numpy()
        assert (tk[valid] == expect).sum() == (base['tokens'][valid] == c0).sum() > 0, (dups, expect)
        _check_valid_frames(logp.cpu().numpy(), tk, enc_len.cpu().numpy(), want)
        e.close()


@pytest.fixture(scope='module')
def zh_full(golden_dir):
    """FakeQuantNet on QuartzNet15x5Base-Zh w8a8 at 8 utterances x 500 frames, ragged lengths."""
    from oracle.fakequant_torch import FakeQuantNet
    amin, amax, meta = _ranges(golden_dir, 'net_quartznet_w8a8')
    cfg = topology.quartznet15x5_zh()
    sd = synth.make_state_dict(cfg, meta['seed'])
    B, T = 8, 500
    x = synth.make_features(B, 64, T, 23)
    lens = [500, 129, 256, 255, 383, 64, 437, 1]
    want = FakeQuantNet(topology.conv_plan(cfg), cfg, sd, amin, amax, 8, 8).forward(x, lens)
    want = {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in want.items()}
    blob, pm = pack.pack_model(cfg, sd, amin, amax, 8, 8)
    return dict(x=x, lens=lens, want=want, blob=blob, pm=pm)


@pytest.mark.parametrize('tile', [32, 128])
def test_zh_full_size_against_oracle_and_generic_path(eng, zh_full, tile):
    o = zh_full
    x, lens = torch.from_numpy(o['x']).cuda(), torch.tensor(o['lens'])
    e = eng.Engine(o['blob'], 0, tile=tile)
    logp, tokens, enc_len = e.forward(x, lens)
    torch.cuda.synchronize()
    labels = e.op_labels()
    assert 'k_decw' in labels and 'k_logsoftmax' not in labels
    n_launch = e.num_launches()                   # QuartzNet15x5's 78 .. 82, plus k_decw's second launch
    assert 79 <= n_launch <= 83, n_launch
    lp, tk, el = logp.cpu().numpy(), tokens.cpu().numpy(), enc_len.cpu().numpy()
    _check_valid_frames(lp, tk, el, o['want'])
    with pytest.raises(Exception, match='never materialised'):     # no arena slot for the unstored float logits
        e.read_tensor(o['pm']['n_tensors'] - 1, 5207, dtype=np.float32)
    # the generic path (k_sep logits + k_logsoftmax) at 5207 classes: the same tokens, log-probs within the same bound
    g = eng.Engine(o['blob'], 0, tile=tile, fuse_decoder=False)
    glp, gtk, gel = g.forward(x, lens)
    torch.cuda.synchronize()
    assert 'k_logsoftmax' in g.op_labels() and 'k_decw' not in g.op_labels()
    assert np.array_equal(gel.cpu().numpy(), el)
    for b in range(len(el)):
        n = int(el[b])
        assert np.array_equal(gtk.cpu().numpy()[b, :n], tk[b, :n]), b
        np.testing.assert_allclose(glp.cpu().numpy()[b, :n], lp[b, :n], rtol=1e-4, atol=5e-5)
    e.close()
    g.close()


def test_zh_graph_replay_and_tokens_only(eng, zh_full):
    """graph=True: capture on the second call, replays equal direct launches bit for bit; want_logp=False (the
    tokens-only k_decw_out, no GEMM recompute) returns the same tokens and lengths."""
    o = zh_full
    x, lens = torch.from_numpy(o['x']).cuda(), torch.tensor(o['lens'], dtype=torch.int32).cuda()
    ref = eng.Engine(o['blob'], 0)
    lp0, tk0, el0 = ref.forward(x, lens)
    _, tk1, el1 = ref.forward(x, lens, want_logp=False)
    torch.cuda.synchronize()
    assert torch.equal(tk1, tk0) and torch.equal(el1, el0)
    g = eng.Engine(o['blob'], 0, graph=True)
    B, To = x.shape[0], g.out_frames(x.shape[2])
    out = (torch.empty(B, To, 5207, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for it in range(4):                                  # direct, capture, replay, replay
        out[0].zero_()
        out[1].zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            lp, tk, el = g.forward(x, lens, out=out)
        torch.cuda.synchronize()
        assert torch.equal(tk, tk0) and torch.equal(lp, lp0) and torch.equal(el, el0), it
    ref.close()
    g.close()
