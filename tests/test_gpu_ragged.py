"""Reserved engines on the GPU (qasr_engine_reserve / qasr_engine_forward_ragged[_audio]): a ragged sequence of batches
through ONE reserved engine against a second, unreserved engine of the same blob run at every batch's exact shape - the
path the oracle and the reference fixtures pin.  Bit-exact: torch.equal on every output."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from qasr import melbank, pack, ragged, synth, topology  # noqa: E402


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    return engine


def _ranges(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name + '.npz'))
    return d['act_min'], d['act_max'], json.loads(str(d['meta']))


def _blob(golden_dir, case):
    """(blob, cfg) of a test net; the fixtures' calibrated ranges are the quantiser settings"""
    if case == 'miniq_w8a8':
        cfg, fx, w, a = topology.mini_quartznet(), 'net_miniq_w8a8', 8, 8
    elif case == 'miniq_w6a6':
        cfg, fx, w, a = topology.mini_quartznet(), 'net_miniq_w6a6', 6, 6
    elif case == 'minij_w8a8':
        cfg, fx, w, a = topology.mini_jasper(), 'net_minij_w8a8', 8, 8
    elif case == 'mini_wide':                                  # 1000 classes: k_decw
        cfg = topology.mini_quartznet()
        cfg = dataclasses.replace(cfg, num_classes=999, vocabulary=topology.zh_placeholder_vocabulary(999))
        fx, w, a = 'net_miniq_w8a8', 8, 8
    elif case == 'mini_k_dec':                                 # 256 decoder input channels: k_dec
        cfg = topology.mini_quartznet()
        cfg = dataclasses.replace(cfg, blocks=cfg.blocks[:-1] + [dataclasses.replace(cfg.blocks[-1], filters=256)])
        fx, w, a = 'net_miniq_w8a8', 8, 8
    else:
        cfg, fx, w, a = topology.quartznet15x5(), 'net_quartznet_w8a8', 8, 8
    amin, amax, meta = _ranges(golden_dir, fx)
    blob, _ = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), amin, amax, w, a)
    return blob, cfg


def _edge_lens(T, B, rng):
    """lengths on every edge of the mask logic, then random ones: full; one frame into the second 128-frame tile; inside the
    last 32-frame tile; one frame; under half the frames (whole tiles behind the length)"""
    edges = [T, min(T, 129), max(1, T - 5), 1, max(1, T // 2 - 40), max(1, min(T, 128)), max(1, T - 32)]
    lens = [int(rng.integers(1, T + 1)) for _ in range(B)]
    order = rng.permutation(B)
    for i, e in zip(order, edges):
        lens[int(i)] = int(e)
    return lens                                                # (order[0] holds T: one utterance always fills the batch)


def _feature_sequence(max_batch, max_frames, n, seed):
    """n batches (B, T) with different B and T; includes B = 1, the envelope's maximum and a one-tile batch"""
    rng = np.random.default_rng(seed)
    shapes = [(max_batch, max_frames), (1, 200), (2, 127), (max_batch, 64), (3, 129)]
    while len(shapes) < n:
        shapes.append((int(rng.integers(1, max_batch + 1)), int(rng.integers(40, max_frames + 1))))
    return shapes, rng


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _equal(got, want, what):
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    g, w = _bits(got.contiguous()), _bits(want.contiguous())
    assert torch.equal(g, w), (what, int((g != w).sum()))


def _compare(got, want, decode, what):
    _equal(got[1], want[1], what + ' tokens')
    _equal(got[2], want[2], what + ' encoded lengths')
    _equal(got[0], want[0], what + ' log-probs')
    if decode:
        g, w = got[3], want[3]
        for f in ('labels', 'n_labels', 'start', 'nframes', 'score', 'utt_score', 'frame_score'):
            _equal(getattr(g, f), getattr(w, f), f'{what} ctc.{f}')


def _check_stats(st0, st, calls):
    """no allocation or free after reserve(); at most one graph per bucket; every visit of a bucket after its first is a
    graph launch"""
    assert st['device_allocs'] == st0['device_allocs'] and st['device_frees'] == st0['device_frees'], (st0, st)
    assert sum(st['buckets'].values()) == calls
    assert 1 <= st['graphs_captured'] <= len(st['buckets'])
    assert st['eager_runs'] == len(st['buckets'])
    assert st['graph_replays'] == calls - len(st['buckets'])
    assert st['graphs_captured'] == sum(1 for c in st['buckets'].values() if c >= 2)


def _run_feature_sequence(eng, blob, cfg, max_batch, max_frames, n, seed, decode, max_graphs=None):
    ref = eng.Engine(blob, 0)
    res = eng.Engine(blob, 0).reserve(max_batch, max_frames=max_frames, want_logp=True, decode=decode, max_graphs=max_graphs)
    st0 = res.ragged_stats()
    assert st0['graphs_captured'] == 0 and st0['buckets'] == {}
    stream = torch.cuda.Stream()
    shapes, rng = _feature_sequence(max_batch, max_frames, n, seed)
    assert len(set(shapes)) >= 12
    M = ragged.envelope_frames(0, max_frames, 16)
    for i, (B, T) in enumerate(shapes):
        x = torch.from_numpy(synth.make_features(B, cfg.feat_in, T, seed + i)).cuda()
        lens = torch.tensor(_edge_lens(T, B, rng), dtype=torch.int32)
        want = ref.forward(x, lens, decode=True if decode else None)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            got = res.forward_ragged(x, lens, stream=stream)
        torch.cuda.synchronize()
        assert res.last_ragged.bucket_frames == ragged.bucket_frames(M, max_graphs or 16, T)
        _compare(got, want, decode, f'batch {i} ({B} x {T})')
    st = res.ragged_stats()
    _check_stats(st0, st, len(shapes))
    assert set(st['buckets']) <= set(ragged.bucket_edges(M, max_graphs or 16))
    ref.close()
    res.close()


@pytest.mark.parametrize('case', ['miniq_w8a8', 'miniq_w6a6', 'minij_w8a8', 'mini_wide', 'mini_k_dec'])
def test_feature_entry_mini_nets(eng, golden_dir, case):
    blob, cfg = _blob(golden_dir, case)
    _run_feature_sequence(eng, blob, cfg, max_batch=5, max_frames=600, n=14, seed=31, decode=True, max_graphs=4)


def test_feature_entry_full_size_quartznet(eng, golden_dir):
    blob, cfg = _blob(golden_dir, 'quartznet')
    x = torch.from_numpy(synth.make_features(2, cfg.feat_in, 256, 1)).cuda()
    for reserve, kernel in ((False, 'k_sep2<'), (True, 'k_sep2s<')):      # the mask-skip kernels are the reserved engine's
        e = eng.Engine(blob, 0)
        if reserve:
            e.reserve(2, max_frames=256)
            e.forward_ragged(x, torch.tensor([256, 3]))
        else:
            e.forward(x, torch.tensor([256, 3]))
        torch.cuda.synchronize()
        assert sum(l.startswith(kernel) for l in e.op_labels()) >= 70, e.op_labels()
        e.close()
    _run_feature_sequence(eng, blob, cfg, max_batch=8, max_frames=700, n=12, seed=5, decode=True, max_graphs=3)


def _front(n_mels):
    fb = torch.from_numpy(melbank.mel_filterbank(16000, 512, n_mels, 0.0, 8000.0).astype(np.float32)).cuda().contiguous()
    return fb, torch.hann_window(320, periodic=False).cuda()


def _run_audio_sequence(eng, blob, cfg, max_batch, max_samples, n, seed, decode, fuse_norm=None, max_graphs=None):
    fb, win = _front(cfg.feat_in)
    plan = eng.frontend_plan(fb)
    ref = eng.Engine(blob, 0, fuse_norm=fuse_norm)
    res = eng.Engine(blob, 0, fuse_norm=fuse_norm).reserve(max_batch, max_samples=max_samples, want_logp=True, decode=decode,
                                                           max_graphs=max_graphs)
    st0 = res.ragged_stats()
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(seed)
    shapes = [(max_batch, max_samples), (1, 16000), (2, 20319), (max_batch, 9000), (3, 20480)]
    while len(shapes) < n:
        shapes.append((int(rng.integers(1, max_batch + 1)), int(rng.integers(3000, max_samples + 1))))
    assert len(set(shapes)) >= 12
    for i, (B, S) in enumerate(shapes):
        audio = torch.from_numpy(synth.make_audio(B, S, seed=seed + i)).cuda()
        # sample counts on the edges: the full row (reflect padding at the batch's own S), one frame past a 128-frame
        # tile, near the end of the row, a few hundred samples, under half the row
        pool = [min(S, 160 * 128 + 1), max(400, S - 700), 400, max(400, S // 2 - 3000)] + [int(rng.integers(400, S + 1)) for _ in range(B)]
        al = [S] + [int(v) for v in rng.permutation(pool)[:B - 1]]
        alen = torch.tensor(al, dtype=torch.int32).cuda()
        want = ref.forward_audio(audio, alen, fb, win, plan, 0.97, 16, decode=True if decode else None)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            got = res.forward_ragged_audio(audio, alen, fb, win, plan, 0.97, 16, stream=stream)
        torch.cuda.synchronize()
        _compare(got, want, decode, f'batch {i} ({B} x {S} samples)')
    _check_stats(st0, res.ragged_stats(), len(shapes))
    ref.close()
    res.close()


@pytest.mark.parametrize('case', ['miniq_w8a8', 'minij_w8a8'])
def test_audio_entry_mini_nets(eng, golden_dir, case):
    blob, cfg = _blob(golden_dir, case)
    _run_audio_sequence(eng, blob, cfg, max_batch=4, max_samples=60000, n=13, seed=77, decode=True, max_graphs=3)


@pytest.mark.parametrize('fuse_norm', [None, False], ids=['norm_in_stem', 'k_norm'])
def test_audio_entry_full_size_quartznet(eng, golden_dir, fuse_norm):
    """both front-end forms: per-tile statistics folded into k_stem (the default) and the k_norm launch"""
    blob, cfg = _blob(golden_dir, 'quartznet')
    _run_audio_sequence(eng, blob, cfg, max_batch=6, max_samples=100000, n=12, seed=3, decode=True, fuse_norm=fuse_norm, max_graphs=3)


def test_padded_row_decode_walks_the_batchs_own_frames(eng, golden_dir):
    """decode='padded' (use_lens = 0, the reference's walk over the padded row): the row ends at the batch's T', not at the
    bucket's"""
    blob, cfg = _blob(golden_dir, 'mini_k_dec')
    ref = eng.Engine(blob, 0)
    res = eng.Engine(blob, 0).reserve(4, max_frames=512, decode='padded', max_graphs=2)
    for i, (B, T) in enumerate([(3, 200), (4, 300), (2, 200), (3, 257)]):
        x = torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 90 + i)).cuda()
        lens = torch.tensor([T, 77, 1, 150][:B], dtype=torch.int32)
        To = ref.out_frames(T)
        buf = eng.ctc_buffers(B, To, x.device, scores=True, blank=ref.n_classes - 1)
        ref.attach_ctc(buf.frame_score, buf, use_lens=False)
        want = ref.forward(x, lens) + (buf,)
        torch.cuda.synchronize()
        got = res.forward_ragged(x, lens)
        torch.cuda.synchronize()
        _compare(got, want, True, f'batch {i}')
    ref.close()
    res.close()


def test_same_batch_twice_with_a_loud_batch_in_between(eng, golden_dir):
    """Stale data in skipped tiles and in the staging buffers must not leak: a short batch, then a full-length batch of
    large values over the whole envelope, then the short batch again - same bytes, all equal to the exact-shape run."""
    blob, cfg = _blob(golden_dir, 'quartznet')
    ref = eng.Engine(blob, 0)
    res = eng.Engine(blob, 0).reserve(6, max_frames=640, decode=True, max_graphs=1)
    B, T = 3, 210
    x = torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 4)).cuda()
    lens = torch.tensor([210, 130, 3], dtype=torch.int32)
    loud = torch.from_numpy(synth.make_features(6, cfg.feat_in, 640, 8)).cuda() * 50.0
    loud_lens = torch.full((6,), 640, dtype=torch.int32)
    want = ref.forward(x, lens, decode=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    kept = []
    for rnd in range(3):                                       # direct launches, capture, replay
        with torch.cuda.stream(stream):
            got = res.forward_ragged(x, lens, stream=stream)
        torch.cuda.synchronize()
        _compare(got, want, True, f'round {rnd}')
        kept.append([t.clone() for t in got[:3]])
        with torch.cuda.stream(stream):
            res.forward_ragged(loud, loud_lens, stream=stream)
        torch.cuda.synchronize()
    for k in kept[1:]:
        for a, b_ in zip(k, kept[0]):
            _equal(a, b_, 'repeat')
    ref.close()
    res.close()


def test_outside_the_envelope_is_refused_and_the_engine_lives_on(eng, golden_dir):
    blob, cfg = _blob(golden_dir, 'miniq_w8a8')
    ref = eng.Engine(blob, 0)
    res = eng.Engine(blob, 0).reserve(3, max_frames=300, max_samples=32000)
    st0 = res.ragged_stats()
    x = torch.from_numpy(synth.make_features(4, cfg.feat_in, 200, 1)).cuda()
    with pytest.raises(eng.QasrError, match=r'\(1\).*max_batch 3'):
        res.forward_ragged(x, torch.tensor([200, 100, 50, 1]))
    x2 = torch.from_numpy(synth.make_features(2, cfg.feat_in, 385, 1)).cuda()
    with pytest.raises(eng.QasrError, match=r'\(1\).*max_frames 384'):
        res.forward_ragged(x2, torch.tensor([385, 100]))
    fb, win = _front(cfg.feat_in)
    plan = eng.frontend_plan(fb)
    audio = torch.from_numpy(synth.make_audio(2, 32001, seed=1)).cuda()
    with pytest.raises(eng.QasrError, match=r'\(1\).*max_samples 32000'):
        res.forward_ragged_audio(audio, torch.tensor([32001, 400], dtype=torch.int32).cuda(), fb, win, plan)
    with pytest.raises(eng.QasrError, match='reserved'):       # the plain entry would rebuild the plan
        res.forward(x[:2].contiguous(), torch.tensor([200, 100]))
    with pytest.raises(eng.QasrError, match='reserved already'):
        res.reserve(3, max_frames=300)
    lens = torch.tensor([200, 100, 1])
    got = res.forward_ragged(x[:3].contiguous(), lens)
    want = ref.forward(x[:3].contiguous(), lens)
    torch.cuda.synchronize()
    _compare(got, want, False, 'after the refusals')
    st = res.ragged_stats()
    assert st['device_allocs'] == st0['device_allocs'] and st['device_frees'] == st0['device_frees']
    # before reserve(), and on engines that cannot be reserved
    with pytest.raises(eng.QasrError, match='qasr_engine_reserve first'):
        ref.forward_ragged(x[:3].contiguous(), lens)
    dbg = eng.Engine(blob, 0, debug=True)
    with pytest.raises(eng.QasrError, match='debug'):
        dbg.reserve(3, max_frames=300)
    dbg.close()
    ref.close()
    res.close()


SKIP_SHAPES = [(33, 256, 256, 0), (51, 512, 512, 512), (75, 512, 512, 0), (75, 512, 512, 512)]


@pytest.mark.parametrize('gen,tile', [(2, 32), (2, 64), (2, 128), (1, 32), (1, 64)],
                         ids=['k_sep2_32', 'k_sep2_64', 'k_sep2_128', 'k_sep_32', 'k_sep_64'])
@pytest.mark.parametrize('K,cin,cout,rcin', SKIP_SHAPES)
def test_mask_skip_writes_what_the_full_path_writes(eng, gen, tile, K, cin, cout, rcin):
    """The mask-skip rule at operator level (qasr_sep_layer, production kernels without hooks; gen = 3 routes k_sep2's shapes
    to the k_sep2s instantiations a reserved engine launches, k_sep carries the rule in every build): lengths that leave
    whole tiles behind them, output buffers pre-filled with a non-zero pattern - every byte equals the oracle's, for u8
    (hi = 255) and signed (hi = 127) consumers, with and without the residual branch; the row padding up to Tp holds
    the zero code as well."""
    import test_gpu_parity as P
    from oracle import int_oracle as O
    from qasr.pack import F_MASK_OUT, F_RELU
    T = 380
    rng = np.random.default_rng(K + cin + rcin + tile)
    lens = np.array([380, 257, 256, 130, 128, 33, 1, 200])
    for signed_first in (False, True):
        c = P._sep_case(rng, len(lens), T, cin, cout, K, True, rcin or None, 2 if (rcin or gen == 1) else 1)
        if signed_first and not rcin:
            c['outs'][0] = dict(c['outs'][0], hi=127)
        c['lens'] = lens
        c['x'] = np.where(np.arange(T)[None, None, :] < lens[:, None, None], c['x'], 0)
        if c['res'] is not None:
            c['res']['x'] = np.where(np.arange(T)[None, None, :] < lens[:, None, None], c['res']['x'], 0)
        want = O.sep_layer_ref(c['x'], c['lens'], c['wdw'], c['m_dw'], (-128, 127), c['wpw'], c['bias'], c['outs'], relu=True,
                               mask_out=True, sb=c['sb'], res=c['res'])
        res = None
        if c['res'] is not None:
            res = dict(c['res'], x=torch.from_numpy(c['res']['x'].astype(np.uint8)).cuda())
        got = eng.sep_layer(torch.from_numpy(c['x'].astype(np.uint8)).cuda(), c['lens'], c['wpw'], c['bias'], c['outs'],
                            wdw=c['wdw'], m_dw=c['m_dw'], x_unsigned=True, flags=F_RELU | F_MASK_OUT, sb=c['sb'], res=res,
                            tile=tile, gen=3 if gen == 2 else gen, hooks=False, out_fill=0x5a)
        assert got['label'].startswith('k_sep2s<' if gen == 2 else 'k_sep<') and 'true' not in got['label'], got['label']
        for j, o in enumerate(c['outs']):
            g = got['outs'][j].cpu().numpy()
            g = g.view(np.uint8).astype(np.int64) if o['hi'] > 127 else g.astype(np.int64)
            assert np.array_equal(g, want['outs'][j]), (got['label'], f'consumer {j}', int((g != want['outs'][j]).sum()))
            full = got['outs_padded'][j].cpu().numpy()
            for b_, n_ in enumerate(lens):
                assert not full[b_, :, n_:].any(), (got['label'], 'bytes behind the length are not the zero code', b_)
