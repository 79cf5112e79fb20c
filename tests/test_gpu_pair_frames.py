"""k_sep2p splits a pair's 128-frame tile by frames: member hm serves frames [64 hm, 64 hm + 64) of the tile over
all 512 input and output channels with the 64-frame body, the members exchange nothing, and each counts itself once in its
completion word.  Everything goes through the public bindings and is compared bit for bit: at operator level on the boundary
between the members (one member wholly masked, a tile almost empty, halos that cross into the other member's half and into the
neighbouring pair's tile), through the whole network (direct call, capture, replays back to back), and once at the benchmark's
shape on four streams."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from qasr import pack, synth, topology  # noqa: E402

N_PAIRED = 35


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
    for name in ('QASR_RES_TILE', 'QASR_RES_TILE128', 'QASR_TILE128', 'QASR_WIDE_TILES', 'QASR_SEP_GEN', 'QASR_PAIR_SPLIT',
                 'QASR_NO_FUSE_STEM'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '4')


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    for g, w, name in zip(got, want, ('log-probs', 'tokens', 'encoded lengths')):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), f'{what}: {name} differ'


# (B, T, lengths): one pair on one tile with the length on, next to and far from the boundary between the members; two
# utterances on two tiles, where a member's halo reaches into the other member's half and into the neighbouring pair's tile
OP_CASES = [(1, 128, (128,)), (1, 128, (65,)), (1, 128, (64,)), (1, 128, (63,)), (1, 128, (1,)),
            (2, 256, (256, 129)), (2, 256, (192, 1))]


@pytest.mark.parametrize('B,T,lens', OP_CASES, ids=['_'.join(['B%d' % c[0], 'T%d' % c[1]] + ['%d' % n for n in c[2]]) for c in OP_CASES])
@pytest.mark.parametrize('K', [51, 63, 75])
def test_member_halves_against_unpaired_and_k_sep(eng, K, B, T, lens):
    """the paired kernel's bytes equal those of the unpaired 128-frame kernel and of k_sep (sep_gen = 1), with and without
    accumulators beyond 2^22; both members have written something other than zero"""
    from qasr.pack import F_EXACT_Z, F_MASK_OUT, F_RELU
    from test_gpu_pair_split import _launch, _sep_case
    rng = np.random.default_rng(1000 * K + 10 * T + sum(lens))
    for big in (False, True):
        c = _sep_case(rng, B, T, K, list(lens), big)
        x = torch.from_numpy(c['x'].astype(np.uint8)).cuda()
        got = _launch(eng, c, x, big, True)
        ref = _launch(eng, c, x, big, False)
        old = eng.sep_layer(x, c['lens'], c['wpw'], c['bias'], c['outs'], wdw=c['wdw'], m_dw=c['m_dw'], x_unsigned=True,
                            flags=F_RELU | F_MASK_OUT | (F_EXACT_Z if big else 0), sb=c['sb'], tile=128, gen=1, hooks=False,
                            row_pad=128)
        assert got['label'] == ref['label'] == f'k_sep2<{K}, 4, 0, 2, false, 128, 1>'
        assert old['label'].startswith('k_sep<'), old['label']
        g = got['outs_padded'][0]
        assert g.shape == (B, 512, T)
        assert eng.sep_pair_timeouts(got['pair_ws'], B, T) == 0
        assert torch.equal(g, ref['outs_padded'][0]), (K, B, T, lens, big, 'unpaired 128-frame kernel')
        assert torch.equal(g, old['outs_padded'][0]), (K, B, T, lens, big, 'k_sep')
        # a masked frame is code 0, so with a length of at most 64 the second member's half is zero by definition; what it
        # must have written is looked for in the bytes the mask leaves
        assert g[:, :, :64].any(), 'nothing but zeros below frame 64'
        if max(lens) > 64:
            assert g[:, :, 64:].any(), 'nothing but zeros from frame 64 on'
        for b_, n_ in enumerate(lens):
            assert not g[b_, :, n_:].any(), ('frames behind the length are not zero', b_)
        # every member has counted itself exactly once; the rest of the 256-byte block of words stays zero
        words = got['pair_ws'][:eng.load_library().qasr_sep_pair_timeout_offset(B, T)].view(torch.int32).cpu().numpy()
        n = 2 * B * (T // 128)
        assert (words[:n] == 1).all() and not words[n:].any(), words[:n + 2]


def test_engine_direct_capture_replays(eng, blob, hint):
    """full QuartzNet15x5, B = 3, T = 500, lengths [500, 257, 1], a 128-frame engine with pair_split = 1 and a graph on a stream
    of its own: the direct call, the capture, then four replays back to back without a host synchronise, on changing inputs.
    Log-probs, tokens and lengths are the pair_split = 0 engine's bytes, no time-out is reported, and the completion words
    after the last forward equal those after the first (each forward zeroes them, each member adds 1)."""
    b, cfg = blob
    B, T = 3, 500
    lens = torch.tensor([500, 257, 1], dtype=torch.int32).cuda()
    xs = [torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 70 + i)).cuda() for i in range(3)]
    e0 = eng.Engine(b, 0, tile=128, pair_split=0)
    want = [[t.clone() for t in e0.forward(x, lens)] for x in xs]
    torch.cuda.synchronize()
    assert not torch.equal(want[0][1], want[1][1]) and not torch.equal(want[1][1], want[2][1])
    e1 = eng.Engine(b, 0, tile=128, pair_split=1, graph=True)
    st = torch.cuda.Stream()
    To = e1.out_frames(T)
    xbuf = torch.empty(B, cfg.feat_in, T, device='cuda')
    out = (torch.empty(B, To, e1.n_classes, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))

    def step(i):                                                # the input changes on the engine's own stream: no host sync
        with torch.cuda.stream(st):
            xbuf.copy_(xs[i], non_blocking=True)
            e1.forward(xbuf, lens, stream=st, out=out)

    torch.cuda.synchronize()
    step(0)                                                     # direct launches
    torch.cuda.synchronize()
    _same(out, want[0], 'direct call')
    first = e1.pair_flag_words()
    assert first.size > 0 and set(np.unique(first).tolist()) == {0, 1} and int(first.sum()) == N_PAIRED * 2 * B * 2
    step(1)                                                     # the capture
    torch.cuda.synchronize()
    _same(out, want[1], 'capture')
    for rep in range(4):                                        # replays
        step((rep + 2) % 3)
    torch.cuda.synchronize()
    _same(out, want[(3 + 2) % 3], 'last replay')
    assert e1.pair_timeouts() == 0
    assert np.array_equal(e1.pair_flag_words(), first)
    assert sum(e1.op_paired()) == N_PAIRED and not any(e0.op_paired())
    assert e1.op_labels() == e0.op_labels() and e1.num_launches() == e0.num_launches()
    e0.close()
    e1.close()


def test_benchmark_shape_on_four_streams(eng, blob, hint):
    """B = 32, T = 500 - the benchmark's shape, the only case at that size: four engines on four streams, three replays each,
    enqueued round-robin; every engine's tokens equal its own serial result"""
    b, cfg = blob
    B, T, n = 32, 500, 4
    lens = torch.tensor([T - 11 * (i % 13) - (i % 3) for i in range(B)], dtype=torch.int32).cuda()
    xs = [torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 80 + i)).cuda() for i in range(n)]
    engs = [eng.Engine(b, 0, tile=128, pair_split=1, graph=True) for _ in range(n)]
    streams = [torch.cuda.Stream() for _ in range(n)]
    To = engs[0].out_frames(T)
    outs = [(None, torch.empty(B, To, dtype=torch.int32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda')) for _ in range(n)]

    def step(i):
        with torch.cuda.stream(streams[i]):
            engs[i].forward(xs[i], lens, want_logp=False, stream=streams[i], out=outs[i])
    want = []
    for rep in range(2):                                        # direct launches, then the capture - one step at a time
        want = []
        for i in range(n):
            step(i)
            torch.cuda.synchronize()
            want.append(outs[i][1].clone())
    assert not torch.equal(want[0], want[1])
    for t in outs:
        t[1].zero_()
    torch.cuda.synchronize()
    for rep in range(3):                                        # replays, round-robin, all in flight together
        for i in range(n):
            step(i)
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(outs[i][1], want[i]), (i, int((outs[i][1] != want[i]).sum()))
        assert sum(engs[i].op_paired()) == N_PAIRED and engs[i].pair_timeouts() == 0
        engs[i].close()
