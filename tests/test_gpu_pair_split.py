"""The paired form of the plain 512 -> 512 separable layers (k_sep2p): a 128-frame tile on two work-groups that
exchange their halves of the depthwise output inside the launch.  The bytes are those of the unpaired kernels and of the numpy
oracle at operator level, through replays that reuse the exchange buffer and the flag words, on concurrent streams, and through
the whole network (direct launches, capture, graph replays); the rule that switches it on follows the hardware-queue hint."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import int_oracle as O  # noqa: E402
from qasr import pack, synth, topology  # noqa: E402

EDGE_LENS = [250, 249, 224, 208, 131, 100, 17, 1]      # every edge of the mask logic, and a tile wholly behind the length


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    return engine


@pytest.fixture(scope='module')
def blob(golden_dir):
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    b, _ = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), d['act_min'], d['act_max'], 8, 8)
    return b, cfg


@pytest.fixture
def hint(monkeypatch):
    for name in ('QASR_RES_TILE', 'QASR_RES_TILE128', 'QASR_TILE128', 'QASR_WIDE_TILES', 'QASR_SEP_GEN', 'QASR_PAIR_SPLIT'):
        monkeypatch.delenv(name, raising=False)

    def set_hint(value):
        if value is None:
            monkeypatch.delenv('GPU_MAX_HW_QUEUES', raising=False)
        else:
            monkeypatch.setenv('GPU_MAX_HW_QUEUES', value)
    return set_hint


def _sep_case(rng, B, T, K, lens=None, big=False):
    """operands of a plain 512 -> 512 layer in the manner of test_gpu_parity._sep_case (u8 input, one consumer)"""
    cin = cout = 512
    lens = np.array([T] + list(rng.integers(1, T + 1, B - 1))) if lens is None else np.array(lens)
    x = rng.integers(0, 256, (B, cin, T))
    x = np.where(np.arange(T)[None, None, :] < lens[:, None, None], x, 0)
    wdw = rng.integers(-127, 127, (cin, K))
    m_dw = 127.0 / (np.abs(wdw).sum(1) * 255 * rng.uniform(0.2, 0.6, cin))
    wpw = rng.integers(-127, 127, (cout, cin))
    bias = rng.integers(-20000, 20000, cout)
    sb = rng.uniform(1e-6, 3e-6, cout).astype(np.float32)
    if big:                                                    # same-sign rows + a large bias: |acc| well past 2^22
        wpw[:8] = np.abs(wpw[:8])
        wpw[8:16] = -np.abs(wpw[8:16])
        wpw[256:264] = np.abs(wpw[256:264])                    # (in the second member's pass too)
        wdw[:] = np.abs(wdw)
        m_dw = m_dw * 4
        bias[:8] += 3_000_000
        bias[8:16] -= 3_000_000
        bias[256:264] += 3_000_000
    outs = [dict(mode=1, lo=0, hi=255, M=rng.uniform(2e-4, 2e-3, cout))]
    return dict(x=x, lens=lens, wdw=wdw, m_dw=m_dw, wpw=wpw, bias=bias, sb=sb, outs=outs)


def _launch(eng, c, x, big, pair, **kw):
    from qasr.pack import F_EXACT_Z, F_MASK_OUT, F_RELU
    return eng.sep_layer(x, c['lens'], c['wpw'], c['bias'], c['outs'], wdw=c['wdw'], m_dw=c['m_dw'], x_unsigned=True,
                         flags=F_RELU | F_MASK_OUT | (F_EXACT_Z if big else 0), sb=c['sb'], tile=128, gen=2, hooks=False,
                         pair=pair, row_pad=kw.pop('row_pad', 128), **kw)


@pytest.mark.parametrize('B,T,lens', [(3, 301, None), (8, 250, EDGE_LENS)], ids=['B3_T301', 'B8_T250_edges'])
@pytest.mark.parametrize('K', [51, 63, 75])
def test_paired_layer_against_oracle_and_unpaired(eng, K, B, T, lens):
    """three tiles with an odd pair count and B no multiple of 8 / every mask edge: bit-exact against the oracle and the
    unpaired kernel, with and without accumulators beyond 2^22 (QASR_F_EXACT_Z), frames behind the length zero"""
    rng = np.random.default_rng(K * 131 + T + B)
    for big in (False, True):
        c = _sep_case(rng, B, T, K, lens, big)
        want = O.sep_layer_ref(c['x'], c['lens'], c['wdw'], c['m_dw'], (-128, 127), c['wpw'], c['bias'], c['outs'], relu=True,
                               mask_out=True, sb=c['sb'], exact_z=big, res=None)
        if big:
            assert np.abs(want['acc']).max() >= 1 << 22
        x = torch.from_numpy(c['x'].astype(np.uint8)).cuda()
        got = _launch(eng, c, x, big, True)
        ref = _launch(eng, c, x, big, False)
        assert got['label'] == ref['label'] == f'k_sep2<{K}, 4, 0, 2, false, 128, 1>'
        assert eng.sep_pair_timeouts(got['pair_ws'], B, got['outs_padded'][0].shape[2]) == 0
        g = got['outs'][0].cpu().numpy().view(np.uint8).astype(np.int64)
        bad = int((g != want['outs'][0]).sum())
        print(f'k{K} B{B} T{T} big={big}: {bad} bytes differ from the oracle')
        assert bad == 0, (K, B, T, big, bad)
        assert torch.equal(got['outs_padded'][0], ref['outs_padded'][0]), (K, B, T, big)
        for b_, n_ in enumerate(c['lens']):
            assert not g[b_, :, n_:].any(), ('frames behind the length are not zero', b_)


def test_paired_layer_needs_a_128_frame_pitch(eng):
    """rows of 192 frames, which 128 does not divide: the unpaired layer falls back to 64-frame tiles there, and the paired
    form is refused"""
    rng = np.random.default_rng(5)
    c = _sep_case(rng, 2, 190, 51)
    x = torch.from_numpy(c['x'].astype(np.uint8)).cuda()
    assert _launch(eng, c, x, False, False, row_pad=64)['label'] == 'k_sep2<51, 4, 0, 2, false, 64, 1>'
    with pytest.raises(eng.QasrError, match='no paired form'):
        _launch(eng, c, x, False, True, row_pad=64)


def test_replays_reuse_exchange_buffer_and_flags(eng):
    """20 launches back to back on one stream with one workspace and different inputs, then two streams at once with a
    workspace each: every result equals its unpaired counterpart, no spin gave up"""
    K, B, T = 75, 3, 384
    rng = np.random.default_rng(77)
    c = _sep_case(rng, B, T, K)
    xs = [torch.from_numpy(np.where(np.arange(T)[None, None, :] < c['lens'][:, None, None], rng.integers(0, 256, (B, 512, T)), 0)
                           .astype(np.uint8)).cuda() for _ in range(20)]
    want = [_launch(eng, c, x, False, False)['outs_padded'][0] for x in xs]
    assert not torch.equal(want[0], want[1])
    ws = eng.sep_pair_workspace(B, T, 'cuda')
    got = [_launch(eng, c, x, False, True, pair_ws=ws, sync=False) for x in xs]
    assert eng.sep_pair_timeouts(ws, B, T) == 0
    for i in range(20):
        assert torch.equal(got[i]['outs_padded'][0], want[i]), i
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    wss = [eng.sep_pair_workspace(B, T, 'cuda') for _ in streams]
    torch.cuda.synchronize()
    got2 = []
    for i in range(20):
        with torch.cuda.stream(streams[i % 2]):
            got2.append(_launch(eng, c, xs[i], False, True, pair_ws=wss[i % 2], sync=False))
    assert eng.sep_pair_timeouts(wss[0], B, T) == 0 and eng.sep_pair_timeouts(wss[1], B, T) == 0
    for i in range(20):
        assert torch.equal(got2[i]['outs_padded'][0], want[i]), i


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    for g, w, name in zip(got, want, ('log-probs', 'tokens', 'encoded lengths')):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), f'{what}: {name} differ'


@pytest.mark.parametrize('T', [500, 260])
def test_engine_paired_equals_unpaired(eng, blob, hint, T):
    """full QuartzNet15x5, B = 3, ragged lengths: direct launches, capture and three replays on changing inputs; same bits,
    labels and launch count as the unpaired plan.  T = 500: rows of 256 frames, two tiles, 35 paired ops; its second utterance
    (260 features = 130 frames) leaves the second tile nearly empty, the third the first.  T = 260: 130 frames in rows of 192,
    where the plain layers of a 128-frame engine run on 64-frame tiles (sep2_tile) and nothing is paired."""
    hint('4')
    b, cfg = blob
    B = 3
    lens = torch.tensor([T, 260, 17], dtype=torch.int32).cuda()
    n_want = 35 if T == 500 else 0
    e0 = eng.Engine(b, 0, tile=128, pair_split=0)
    e1 = eng.Engine(b, 0, tile=128, pair_split=1, graph=True)
    xbuf = torch.empty(B, cfg.feat_in, T, device='cuda')
    To = e1.out_frames(T)
    out = (torch.empty(B, To, e1.n_classes, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))
    st = torch.cuda.Stream()
    for call in range(5):                                       # direct, capture, replay x 3
        xbuf.copy_(torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 30 + call)))
        want = [t.clone() for t in e0.forward(xbuf, lens)]
        for t in out:
            t.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            e1.forward(xbuf, lens, stream=st, out=out)
        torch.cuda.synchronize()
        _same(out, want, f'T={T} call {call}')
    assert e1.pair_timeouts() == 0
    assert e1.op_labels() == e0.op_labels() and e1.num_launches() == e0.num_launches()
    paired = e1.op_paired()
    assert sum(paired) == n_want and not any(e0.op_paired())
    for l, p in zip(e1.op_labels(), paired):
        assert p == (l in ('k_sep2<51, 4, 0, 2, false, 128, 1>', 'k_sep2<63, 4, 0, 2, false, 128, 1>', 'k_sep2<75, 4, 0, 2, false, 128, 1>')), l
    # run_op launches the same form: rerunning a paired op on the last forward's activations leaves the result as it is
    if n_want:
        for _ in range(3):
            e1.run_op(paired.index(True))
        assert e1.pair_timeouts() == 0
    e0.close()
    e1.close()


def test_four_engines_on_four_streams(eng, blob, hint):
    """the benchmark's loop shape at B = 8: four engines, a stream each, steps in flight together; every stream's result
    equals its own serial result"""
    hint('4')
    b, cfg = blob
    B, T, n = 8, 500, 4
    lens = torch.tensor([T, T - 3, 400, 385, 384, 129, 128, 1], dtype=torch.int32).cuda()
    xs = [torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 60 + i)).cuda() for i in range(n)]
    engs = [eng.Engine(b, 0, tile=128, pair_split=1) for _ in range(n)]
    want = []
    for e, x in zip(engs, xs):
        want.append([t.clone() for t in e.forward(x, lens)])
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(n)]
    got = [None] * n
    for rep in range(3):
        for i in range(n):
            with torch.cuda.stream(streams[i]):
                got[i] = engs[i].forward(xs[i], lens, stream=streams[i])
    torch.cuda.synchronize()
    for i in range(n):
        _same(got[i], want[i], f'stream {i}')
        assert sum(engs[i].op_paired()) == 35 and engs[i].pair_timeouts() == 0
        engs[i].close()


def test_graph_replays_back_to_back_at_batch_32(eng, blob, hint):
    """the benchmark's own shape: four engines with a captured graph each, 32 utterances (128 work-groups per paired launch, so
    that four chains overfill the chip and members wait for their partners), replays enqueued back to back without a
    synchronise between them: every stream's last result equals its serial result.  (Zeroing the flag words with a memset node
    instead of a kernel node failed exactly this: flags of the previous replay were still seen set.)"""
    hint('4')
    b, cfg = blob
    B, T, n = 32, 500, 4
    lens = torch.tensor([T - 11 * (i % 13) - (i % 3) for i in range(B)], dtype=torch.int32).cuda()
    xs = [torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 40 + i)).cuda() for i in range(n)]
    engs = [eng.Engine(b, 0, tile=128, pair_split=1, graph=True) for _ in range(n)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    To = engs[0].out_frames(T)
    outs = [(None, torch.empty(B, To, dtype=torch.int32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda')) for _ in range(n)]

    def step(i):
        with torch.cuda.stream(streams[i]):
            engs[i].forward(xs[i], lens, want_logp=False, stream=streams[i], out=outs[i])
    want = []
    for rep in range(3):                                        # direct launches, capture, one replay - one step at a time
        want = []
        for i in range(n):
            step(i)
            torch.cuda.synchronize()
            want.append(outs[i][1].clone())
    for steps in (2, 8):
        for rep in range(steps):
            for i in range(n):
                step(i)
        torch.cuda.synchronize()
        for i in range(n):
            assert torch.equal(outs[i][1], want[i]), (steps, i, int((outs[i][1] != want[i]).sum()))
    for e in engs:
        assert sum(e.op_paired()) == 35 and e.pair_timeouts() == 0
        e.close()


def test_rule(eng, blob, hint, monkeypatch):
    """default: by the hardware-queue hint (paired below 8 queues); explicit 0 / 1 win over the hint, QASR_PAIR_SPLIT over both;
    never for 32- / 64-frame tiles, debug, timing or reserved engines"""
    b, cfg = blob
    B, T = 2, 256
    x = torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 3)).cuda()
    lens = torch.tensor([T, 100], dtype=torch.int32).cuda()

    def n_paired(reserve=False, **kw):
        e = eng.Engine(b, 0, **kw)
        if reserve:
            e.reserve(B, max_frames=T, want_logp=True)
            e.forward_ragged(x, lens)
        else:
            e.forward(x, lens)
        torch.cuda.synchronize()
        n = sum(e.op_paired())
        assert e.pair_timeouts() == 0
        e.close()
        return n

    for queues, want in (('4', 35), (None, 35), ('many', 35), ('8', 0), ('16', 0)):
        hint(queues)
        assert n_paired(tile=128) == want, queues
        assert n_paired(tile=128, pair_split=0) == 0 and n_paired(tile=128, pair_split=1) == 35, queues
    hint('4')
    for kw in (dict(tile=32), dict(tile=64), dict(tile=128, debug=True), dict(tile=128, timing=True)):
        assert n_paired(pair_split=1, **kw) == 0, kw
    assert n_paired(reserve=True, tile=128, pair_split=1) == 0
    monkeypatch.setenv('QASR_PAIR_SPLIT', '0')
    assert n_paired(tile=128) == 0 and n_paired(tile=128, pair_split=1) == 0
    monkeypatch.setenv('QASR_PAIR_SPLIT', '1')
    hint('8')
    assert n_paired(tile=128) == 35 and n_paired(tile=128, pair_split=0) == 35
    assert n_paired(tile=64) == 0
