"""The pair hand-off of k_sep2p as DESIGN.md 5.9 leaves it: the partner's half image goes straight into LDS, and in a forward
with the fused stem the flag words are zeroed by k_stem instead of a k_pair_zero node.  Neither changes a byte, a label or a
launch count: checked through the whole network (direct launches, capture, replays back to back) with the fused stem and
without it (the k_pair_zero path), by reading the flag words themselves, and at operator level on a single pair."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from qasr import pack, synth, topology  # noqa: E402

B, T = 3, 500                       # rows of 256 frames: two 128-frame tiles, 6 pairs per paired op
LENS = [500, 257, 1]                # full; 129 frames, just inside the second tile; one frame, a tile wholly behind it
N_PAIRED = 35
PAIRED_LABELS = tuple(f'k_sep2<{K}, 4, 0, 2, false, 128, 1>' for K in (51, 63, 75))


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

    def set_hint(value):
        monkeypatch.setenv('GPU_MAX_HW_QUEUES', value)
    return set_hint


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    for g, w, name in zip(got, want, ('log-probs', 'tokens', 'encoded lengths')):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), f'{what}: {name} differ'


def _words_of_one_forward(w):
    """every member of every pair has added 1 to its own word exactly once since the words were zeroed: 35 ops x 6 pairs x 2
    words hold 1, the padding of each op's 256-byte block holds 0"""
    return w.size > 0 and set(np.unique(w).tolist()) == {0, 1} and int(w.sum()) == N_PAIRED * 2 * B * 2


def test_engine_handoff_and_flag_words(eng, blob, hint):
    """Full QuartzNet15x5, B = 3, lengths [500, 257, 1].  A paired engine with the fused stem (k_stem zeroes the flag words) and
    one without (k_pair_zero does): direct launches, capture, then 6 graph replays back to back without a host synchronise,
    each engine on a stream of its own, on changing inputs.  Log-probs, tokens and encoded lengths equal the unpaired engine's
    bytes after the direct call, after the capture and after the last replay; no spin gave up.

    Labels and launch counts: fuse_stem = 0 names ops 0..2 by their own kernels and adds k_lens (three launches more,
    qasr_engine_num_launches), whatever pair_split is, so the three engines cannot be equal in them as a whole.  Compared are:
    each paired engine with an unpaired engine of the same fuse_stem (all labels, the count), the labels from op 3 on across all
    engines, and the difference of exactly 3 launches between the two stem settings.

    Flag words (needs no race to fail): a forward that did not zero them leaves 2, 3, ... where one that did leaves 1.  Read
    after the first forward and after the last replay on both paired engines, and after two run_op calls of a paired op."""
    hint('4')
    b, cfg = blob
    lens = torch.tensor(LENS, dtype=torch.int32).cuda()
    xs = [torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 90 + i)).cuda() for i in range(3)]
    ref = eng.Engine(b, 0, tile=128, pair_split=0)
    ref_nostem = eng.Engine(b, 0, tile=128, pair_split=0, fuse_stem=0)
    want = [[t.clone() for t in ref.forward(x, lens)] for x in xs]
    _same(ref_nostem.forward(xs[0], lens), want[0], 'unpaired engines, fused stem against fuse_stem = 0')
    torch.cuda.synchronize()
    assert not torch.equal(want[0][1], want[1][1]) and not torch.equal(want[1][1], want[2][1])

    engs = {'fused stem': eng.Engine(b, 0, tile=128, pair_split=1, graph=True),
            'fuse_stem=0': eng.Engine(b, 0, tile=128, pair_split=1, graph=True, fuse_stem=0)}
    To = ref.out_frames(T)
    st, xbuf, out, first = {}, {}, {}, {}
    for name, e in engs.items():
        st[name] = torch.cuda.Stream()
        xbuf[name] = torch.empty(B, cfg.feat_in, T, device='cuda')
        out[name] = (torch.empty(B, To, e.n_classes, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
                     torch.empty(B, dtype=torch.int32, device='cuda'))

    def step(name, i):                                          # the input changes on the engine's own stream: no host sync
        with torch.cuda.stream(st[name]):
            xbuf[name].copy_(xs[i], non_blocking=True)
            engs[name].forward(xbuf[name], lens, stream=st[name], out=out[name])

    torch.cuda.synchronize()
    for call in range(2):                                       # direct launches, then the capture
        for name, e in engs.items():
            step(name, call)
            torch.cuda.synchronize()
            _same(out[name], want[call], f'{name}, call {call}')
            if call == 0:
                first[name] = e.pair_flag_words()
                print(f'{name}: {first[name].size} flag words, sum {int(first[name].sum())}, max {int(first[name].max())} after the first forward')
                assert _words_of_one_forward(first[name]), name
    for rep in range(6):                                        # replays, both engines in flight together
        for name in engs:
            step(name, rep % 3)
    torch.cuda.synchronize()
    for name, e in engs.items():
        _same(out[name], want[2], f'{name}, last replay')
        assert e.pair_timeouts() == 0, name
        last = e.pair_flag_words()
        print(f'{name}: sum {int(last.sum())}, max {int(last.max())} after the last replay')
        assert np.array_equal(last, first[name]), f'{name}: flag words after 8 forwards differ from those after one'
        paired = e.op_paired()
        assert sum(paired) == N_PAIRED
        for l, p in zip(e.op_labels(), paired):
            assert p == (l in PAIRED_LABELS), l
        for _ in range(2):                                      # outside a forward: the op zeroes its own words (k_pair_zero)
            e.run_op(paired.index(True))
        assert e.pair_timeouts() == 0, name
        assert np.array_equal(e.pair_flag_words(), first[name]), f'{name}: flag words after run_op'

    fused, nostem = engs['fused stem'], engs['fuse_stem=0']
    assert fused.op_labels() == ref.op_labels() and fused.num_launches() == ref.num_launches()
    assert nostem.op_labels() == ref_nostem.op_labels() and nostem.num_launches() == ref_nostem.num_launches()
    assert fused.op_labels()[0] == 'k_stem' and nostem.op_labels()[0] == 'k_quant_in'
    assert fused.op_labels()[3:] == nostem.op_labels()[3:] == ref.op_labels()[3:]
    assert nostem.num_launches() == fused.num_launches() + 3
    assert ref.pair_flag_words().size == 0 and not any(ref.op_paired())
    for e in (ref, ref_nostem, fused, nostem):
        e.close()


@pytest.mark.parametrize('K', [51, 63, 75])
def test_one_pair_one_tile(eng, K):
    """B = 1, T = 128: a single pair, a single tile - the smallest launch of the paired form (16 work-groups, 14 of which leave
    at once); bit-equal to the unpaired kernel, with and without accumulators beyond 2^22"""
    from test_gpu_pair_split import _launch, _sep_case
    rng = np.random.default_rng(K * 7 + 1)
    for big in (False, True):
        c = _sep_case(rng, 1, 128, K, None, big)
        x = torch.from_numpy(c['x'].astype(np.uint8)).cuda()
        got = _launch(eng, c, x, big, True)
        ref = _launch(eng, c, x, big, False)
        assert got['label'] == ref['label'] == f'k_sep2<{K}, 4, 0, 2, false, 128, 1>'
        assert eng.sep_pair_timeouts(got['pair_ws'], 1, got['outs_padded'][0].shape[2]) == 0
        assert got['outs_padded'][0].any()
        assert torch.equal(got['outs_padded'][0], ref['outs_padded'][0]), (K, big)
