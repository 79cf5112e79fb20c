"""The work-group prologue of k_sep2 / k_sep2p / k_sep2s: group 0's requests leave before the masks, the
LDS addresses and lens[b] are looked at, and every kernel argument arrives in one round of scalar loads (k_sep2s keeps the
order before).
Nothing the prologue computes depends on the activations, so every byte must be what the generic k_sep path (sep_gen = 1)
and the numpy oracle give - through the whole network at every tile size and queue hint, on a reserved engine, and at
operator level for every kernel family with signed and unsigned depthwise input."""
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
from test_gpu_parity import _sep_case  # noqa: E402

B = 3
PLAIN512 = tuple(f'k_sep2<{k}, 4, 0, 2, false, 128, 1>' for k in (51, 63, 75))


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    return engine


@pytest.fixture
def hint(monkeypatch):
    for name in ('QASR_RES_TILE', 'QASR_RES_TILE128', 'QASR_TILE128', 'QASR_WIDE_TILES', 'QASR_SEP_GEN', 'QASR_PAIR_SPLIT'):
        monkeypatch.delenv(name, raising=False)
    return lambda value: monkeypatch.setenv('GPU_MAX_HW_QUEUES', value)


@pytest.fixture(scope='module')
def net(golden_dir):
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    sd = synth.make_state_dict(cfg, meta['seed'])
    blob, _ = pack.pack_model(cfg, sd, d['act_min'], d['act_max'], 8, 8)
    oracle = O.OracleNet(topology.conv_plan(cfg), cfg, sd, d['act_min'], d['act_max'], 8, 8)
    return dict(blob=blob, cfg=cfg, oracle=oracle, cases={})


@pytest.fixture(scope='module')
def plan(golden_dir):
    """op labels, paired ops and launch counts of the commit before this change, recorded from its engines on these shapes"""
    return json.load(open(os.path.join(golden_dir, 'sep2_prologue_plan.json')))


def _case(eng, net, T):
    """input, lengths {T', 129, 1} in encoded frames, the oracle's result and the generic k_sep path's - computed once per T"""
    if T not in net['cases']:
        x = synth.make_features(B, net['cfg'].feat_in, T, 7 + T)
        lens = [T, 258, 2]
        want = net['oracle'].forward(x, lens)
        assert list(want['enc_len']) == [T // 2, 129, 1]
        xg = torch.from_numpy(x).cuda()
        lg = torch.tensor(lens, dtype=torch.int32).cuda()
        e = eng.Engine(net['blob'], 0, sep_gen=1)
        gen1 = [t.clone() for t in e.forward(xg, lg)]
        torch.cuda.synchronize()
        assert not any(l.startswith('k_sep2') for l in e.op_labels())
        e.close()
        net['cases'][T] = dict(x=xg, lens=lg, want=want, gen1=gen1)
    return net['cases'][T]


def _check_net(got, c, what):
    logp, tokens, enc_len = got
    g1 = c['gen1']
    assert torch.equal(enc_len, g1[2]) and torch.equal(tokens, g1[1]), f'{what}: tokens / lengths differ from the k_sep path'
    assert torch.equal(logp.view(torch.int32), g1[0].view(torch.int32)), f'{what}: log-probs differ from the k_sep path'
    want = c['want']
    assert np.array_equal(enc_len.cpu().numpy(), want['enc_len'])
    for b in range(B):
        n = int(want['enc_len'][b])
        assert np.array_equal(tokens.cpu().numpy()[b, :n], want['tokens'][b, :n]), (what, b)
        np.testing.assert_allclose(logp.cpu().numpy()[b, :n], want['log_probs'][b, :n], rtol=1e-4, atol=5e-5)


# (tile, queue hint) -> what the launch plan must look like at T = 500 (rows of 256 frames) / T = 260 (rows of 192)
PLANS = [(128, '4'), (128, '8'), (32, '4')]


@pytest.mark.parametrize('tile,queues', PLANS, ids=['tile128_q4', 'tile128_q8', 'tile32'])
@pytest.mark.parametrize('T', [500, 260])
def test_network_equals_k_sep_path_and_oracle(eng, net, plan, hint, T, tile, queues):
    """full QuartzNet15x5: 256 and 512 plain layers paired (q4) and unpaired (q8), block-end layers at 64 (q4) and 128 (q8)
    frames, block 16's dilation, the bare 1x1; T = 260 puts the 128-frame engine on its 64-frame fallback.  The plan - every label,
    the paired ops, the launch count - equals the recorded plan of the parent commit (tests/golden/sep2_prologue_plan.json)."""
    hint(queues)
    c = _case(eng, net, T)
    e = eng.Engine(net['blob'], 0, tile=tile)
    got = e.forward(c['x'], c['lens'])
    torch.cuda.synchronize()
    _check_net(got, c, f'T={T} tile={tile} q={queues}')
    labels, paired = e.op_labels(), e.op_paired()
    assert e.pair_timeouts() == 0
    want = plan[f'T{T}_tile{tile}_q{queues}']                   # the plan of the commit before the prologue was reordered
    assert e.num_launches() == want['launches'] and 78 <= want['launches'] <= 82
    assert labels == want['labels'], [(i, a, b) for i, (a, b) in enumerate(zip(labels, want['labels'])) if a != b]
    assert [int(p) for p in paired] == want['paired']
    assert sum(paired) == (35 if (tile, queues, T) == (128, '4', 500) else 0)
    assert all(p == (l in PLAIN512) for l, p in zip(labels, paired)) or not any(paired)
    if tile == 128 and T == 500:
        res_tt = '64, 1>' if queues == '4' else '128, 1>'
        assert any(l.startswith('k_sep2<75, 4, 4, 2, false, ') and l.endswith(res_tt) for l in labels), labels
        assert 'k_sep2<33, 2, 0, 1, false, 128, 1>' in labels and 'k_sep2<87, 4, 0, 2, false, 128, 2>' in labels
        assert any(l.startswith('k_sep2<0, 4, 0, 4, false, 64') for l in labels), labels
    if tile == 128 and T == 260:
        assert not any(l.endswith('128, 1>') for l in labels), labels
    e.close()


def test_reserved_engine_on_a_ragged_batch(eng, net, plan, hint):
    """k_sep2s (the mask-skip instantiations, which keep the prologue order before): one ragged batch inside a larger
    envelope, and the reserved engine's plan is the recorded one - 77 k_sep2s launches"""
    hint('4')
    c = _case(eng, net, 500)
    e = eng.Engine(net['blob'], 0, tile=128).reserve(4, max_frames=640, want_logp=True)
    got = [t.clone() for t in e.forward_ragged(c['x'], c['lens'])[:3]]
    torch.cuda.synchronize()
    _check_net(got, c, 'reserved')
    want = plan['reserved_T500_tile128_q4']
    labels = e.op_labels()
    assert labels == want['labels'] and e.num_launches() == want['launches'] and not any(e.op_paired())
    assert sum(l.startswith('k_sep2s<') for l in labels) == 77, labels
    e.close()


# family -> (K, cin, cout, residual cin, dilation, tile, paired)
FAMILIES = {
    'plain256': (33, 256, 256, 0, 1, 128, False),
    'plain512': (51, 512, 512, 0, 1, 128, False),
    'plain512_paired': (75, 512, 512, 0, 1, 128, True),
    'block_end_64': (75, 512, 512, 512, 1, 64, False),
    'block_end_128': (39, 256, 256, 256, 1, 128, False),
    'dilation2': (87, 512, 512, 0, 2, 128, False),
    'bare_1x1': (0, 512, 1024, 0, 1, 64, False),
    'plain256_tile32': (39, 256, 256, 0, 1, 32, False),
}


@pytest.mark.parametrize('x_unsigned', [True, False], ids=['u8', 's8'])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_sep_layer_families(eng, family, x_unsigned):
    """one production launch per kernel family through qasr_sep_layer, T = 301 (three 128-frame tiles, a partial last one),
    lengths {301, 129, 1}: bit-exact against the numpy oracle and against k_sep"""
    from qasr.pack import F_MASK_OUT, F_RELU
    K, cin, cout, rcin, dil, tile, pair = FAMILIES[family]
    T = 301
    rng = np.random.default_rng(K * 31 + cin + rcin + tile + x_unsigned)
    c = _sep_case(rng, B, T, cin, cout, K or 33, x_unsigned, rcin or None, 2 if rcin else 1)
    lens = np.array([T, 129, 1])
    c['lens'] = lens
    c['x'] = np.where(np.arange(T)[None, None, :] < lens[:, None, None], c['x'], 0)
    res = None
    if c['res'] is not None:
        c['res']['x'] = np.where(np.arange(T)[None, None, :] < lens[:, None, None], c['res']['x'], 0)
        res = dict(c['res'], x=torch.from_numpy(c['res']['x'].astype(np.uint8)).cuda())
    wdw, m_dw = (c['wdw'], c['m_dw']) if K else (None, None)
    want = O.sep_layer_ref(c['x'], lens, wdw, m_dw, (-128, 127) if K else None, c['wpw'], c['bias'], c['outs'], dilation=dil,
                           relu=True, mask_out=True, res=c['res'])
    x = torch.from_numpy(c['x'].astype(np.uint8 if x_unsigned else np.int8)).cuda()
    kw = dict(wdw=wdw, m_dw=m_dw, x_unsigned=x_unsigned, dilation=dil, flags=F_RELU | F_MASK_OUT, res=res)
    extra = dict(row_pad=128 if tile == 128 else 64, **(dict(pair=True) if pair else {}))
    got = eng.sep_layer(x, lens, c['wpw'], c['bias'], c['outs'], tile=tile, gen=2, hooks=False, **kw, **extra)
    ref = eng.sep_layer(x, lens, c['wpw'], c['bias'], c['outs'], tile=64, gen=1, hooks=False, **kw)
    assert got['label'].startswith(f'k_sep2<{K}, ') and got['label'].endswith(f'false, {tile}, {dil}>'), got['label']
    assert not ref['label'].startswith('k_sep2'), ref['label']
    if pair:
        assert eng.sep_pair_timeouts(got['pair_ws'], B, got['outs_padded'][0].shape[2]) == 0
    for j, o in enumerate(c['outs']):
        g = got['outs'][j].cpu().numpy()
        g = g.view(np.uint8).astype(np.int64) if o['hi'] > 127 else g.astype(np.int64)
        assert np.array_equal(g, want['outs'][j]), (got['label'], f'consumer {j}', int((g != want['outs'][j]).sum()))
        assert torch.equal(got['outs'][j], ref['outs'][j]), (got['label'], f'consumer {j} differs from k_sep')
        for b_, n_ in enumerate(lens):
            assert not g[b_, :, n_:].any(), (got['label'], 'frames behind the length are not zero', b_)
