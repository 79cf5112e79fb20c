"""Halved ops: with two launch chains at a time (fewer than 8 hardware queues) a tile_frames == 128 engine
launches its unpaired plain k_sep2 layers - K = 33 and 39 at 256 channels, the 256 -> 512 layer, block 16 - as the 64-frame
instantiations of the same kernels on grid (B, Tp / 64).  Labels, launch count and the paired ops stay what they were, and so
does every byte: the plan rule, the bytes on the boundaries between the halves (against the unhalved engine, the generic
k_sep path and the numpy oracle), and graph replay with two engines in flight."""
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

HALVED = ('k_sep2<33, 2, 0, 1, false, 128, 1>', 'k_sep2<39, 2, 0, 1, false, 128, 1>', 'k_sep2<51, 2, 0, 2, false, 128, 1>',
          'k_sep2<87, 4, 0, 2, false, 128, 2>')
PLAIN512 = tuple(f'k_sep2<{k}, 4, 0, 2, false, 128, 1>' for k in (51, 63, 75))
N_HALVED, N_PAIRED = 26, 35


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    return engine


@pytest.fixture(scope='module')
def net(golden_dir):
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    sd = synth.make_state_dict(cfg, meta['seed'])
    blob, _ = pack.pack_model(cfg, sd, d['act_min'], d['act_max'], 8, 8)
    oracle = O.OracleNet(topology.conv_plan(cfg), cfg, sd, d['act_min'], d['act_max'], 8, 8)
    return dict(blob=blob, cfg=cfg, oracle=oracle)


@pytest.fixture
def hint(monkeypatch):
    for name in ('QASR_RES_TILE', 'QASR_RES_TILE128', 'QASR_TILE128', 'QASR_WIDE_TILES', 'QASR_SEP_GEN', 'QASR_PAIR_SPLIT',
                 'QASR_NO_FUSE_STEM', 'QASR_HALF_TILES'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '4')
    return lambda value: monkeypatch.setenv('GPU_MAX_HW_QUEUES', value)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    for g, w, name in zip(got, want, ('log-probs', 'tokens', 'encoded lengths')):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), f'{what}: {name} differ'


def _forward(e, x, lens):
    out = [t.clone() for t in e.forward(x, lens)]
    torch.cuda.synchronize()
    return out


def test_plan(eng, net, hint, monkeypatch):
    """which ops are halved, and that nothing else about the plan moves"""
    B, T = 3, 500
    cfg = net['cfg']
    x = torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 11)).cuda()
    lens = torch.tensor([T, 258, 2], dtype=torch.int32).cuda()

    def plan(T_=T, reserve=False, **kw):
        e = eng.Engine(net['blob'], 0, **kw)
        xx = x[:, :, :T_].contiguous()
        ll = torch.clamp(lens, max=T_)
        if reserve:
            e.reserve(4, max_frames=640, want_logp=True)
            e.forward_ragged(xx, ll)
        else:
            e.forward(xx, ll)
        torch.cuda.synchronize()
        got = dict(labels=e.op_labels(), halved=e.op_halved(), paired=e.op_paired(), launches=e.num_launches())
        e.close()
        return got

    p = plan(tile=128)
    assert sum(p['halved']) == N_HALVED
    assert all(h == (l in HALVED) for l, h in zip(p['labels'], p['halved'])), [l for l, h in zip(p['labels'], p['halved']) if h]
    assert [sum(l == name for l in p['labels']) for name in HALVED] == [12, 12, 1, 1]
    assert sum(p['paired']) == N_PAIRED and not any(h and q for h, q in zip(p['halved'], p['paired']))
    assert all(q == (l in PLAIN512) for l, q in zip(p['labels'], p['paired']))
    monkeypatch.setenv('QASR_HALF_TILES', '0')
    off = plan(tile=128)
    monkeypatch.delenv('QASR_HALF_TILES')
    assert not any(off['halved']) and off['paired'] == p['paired']
    assert off['labels'] == p['labels'] and off['launches'] == p['launches']
    # zero halved ops: enough queues for four chains side by side, smaller tiles, rows 128 does not divide, reserved / debug /
    # timing engines
    for q in ('8', '16'):
        hint(q)
        assert not any(plan(tile=128)['halved']), f'hint {q}'
    hint('4')
    for what, kw in (('tile 64', dict(tile=64)), ('tile 32', dict(tile=32)), ('rows of 192', dict(tile=128, T_=260)),
                     ('reserved', dict(tile=128, reserve=True)), ('debug', dict(tile=128, debug=True)),
                     ('timing', dict(tile=128, timing=True))):
        assert not any(plan(**kw)['halved']), what
    # pairing off: the 35 plain 512 -> 512 layers are halved as well
    monkeypatch.setenv('QASR_PAIR_SPLIT', '0')
    np_ = plan(tile=128)
    assert sum(np_['halved']) == N_HALVED + N_PAIRED == 61 and not any(np_['paired'])
    assert all(h == (l in HALVED + PLAIN512) for l, h in zip(np_['labels'], np_['halved']))
    assert np_['labels'] == p['labels'] and np_['launches'] == p['launches']


# (T, mel lengths): encoded lengths 250, 64, 65, 63, 128, 193 - on, one past and one short of a half boundary, on a tile boundary,
# inside the fourth half; and rows of 128 frames, one tile, whose second half has 61 valid frames
BOUNDARY_CASES = [(500, [500, 128, 130, 126, 256, 386], [250, 64, 65, 63, 128, 193]), (250, [250, 2, 128], [125, 1, 64])]


@pytest.mark.parametrize('T,lens,enc', BOUNDARY_CASES, ids=['T500', 'T250'])
def test_bytes_on_the_half_boundaries(eng, net, hint, monkeypatch, T, lens, enc):
    """the halved engine's log-probs (as bits), tokens and encoded lengths equal the unhalved engine's and the generic k_sep
    path's; tokens and lengths equal the numpy oracle's on the valid frames"""
    B = len(lens)
    x = synth.make_features(B, net['cfg'].feat_in, T, 23 + T)
    xg = torch.from_numpy(x).cuda()
    lg = torch.tensor(lens, dtype=torch.int32).cuda()
    e = eng.Engine(net['blob'], 0, tile=128)
    got = _forward(e, xg, lg)
    assert sum(e.op_halved()) == N_HALVED and sum(e.op_paired()) == N_PAIRED
    e.close()
    monkeypatch.setenv('QASR_HALF_TILES', '0')
    e = eng.Engine(net['blob'], 0, tile=128)
    ref = _forward(e, xg, lg)
    assert not any(e.op_halved()) and sum(e.op_paired()) == N_PAIRED
    e.close()
    monkeypatch.delenv('QASR_HALF_TILES')
    e = eng.Engine(net['blob'], 0, sep_gen=1)
    gen1 = _forward(e, xg, lg)
    assert not any(l.startswith('k_sep2') for l in e.op_labels()) and not any(e.op_halved())
    e.close()
    _same(got, ref, 'against QASR_HALF_TILES=0')
    _same(got, gen1, 'against sep_gen=1')
    want = net['oracle'].forward(x, lens)
    assert list(want['enc_len']) == enc
    assert np.array_equal(got[2].cpu().numpy(), want['enc_len'])
    tokens = got[1].cpu().numpy()
    for b in range(B):
        n = enc[b]
        assert np.array_equal(tokens[b, :n], want['tokens'][b, :n]), ('oracle tokens', b)


def test_replay_and_two_engines_in_flight(eng, net, hint):
    """eager, captured and replayed forwards on the same buffers give the same bytes; two halved engines on two streams,
    enqueued back to back without a synchronise in between, reproduce their serial results"""
    B, T = 3, 500
    cfg = net['cfg']
    lens = torch.tensor([500, 257, 130], dtype=torch.int32).cuda()
    xs = [torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 90 + i)).cuda() for i in range(2)]
    engs = [eng.Engine(net['blob'], 0, tile=128, graph=True) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    To = engs[0].out_frames(T)
    outs = [(torch.empty(B, To, engs[0].n_classes, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
             torch.empty(B, dtype=torch.int32, device='cuda')) for _ in range(2)]

    def step(i):
        with torch.cuda.stream(streams[i]):
            engs[i].forward(xs[i], lens, stream=streams[i], out=outs[i])

    torch.cuda.synchronize()
    want = []
    for i in range(2):
        runs = []
        for what in ('eager', 'captured', 'replayed'):
            for t in outs[i]:
                t.zero_()
            torch.cuda.synchronize()
            step(i)
            torch.cuda.synchronize()
            runs.append([t.clone() for t in outs[i]])
            _same(runs[-1], runs[0], what)
        assert sum(engs[i].op_halved()) == N_HALVED and sum(engs[i].op_paired()) == N_PAIRED
        want.append(runs[0])
    assert not torch.equal(want[0][1], want[1][1])
    for o in outs:
        for t in o:
            t.zero_()
    torch.cuda.synchronize()
    for rep in range(3):                                        # replays of both engines, all in flight together
        for i in range(2):
            step(i)
    torch.cuda.synchronize()
    for i in range(2):
        _same(outs[i], want[i], f'engine {i} in flight')
        engs[i].close()
