"""The block-end tile of a `tile_frames == 128` engine (csrc/qasr_engine.hip, res_tile_default): with
qasr_engine_opts.res_tile128 at its default the engine goes by GPU_MAX_HW_QUEUES, read at create time as a hint of how many
launch chains the process runs side by side; explicit 0 / 1 keep meaning 64 / 128 frames.  Whatever the tile, the outputs
are the same bytes; the plain layers never move; engines built for 32- or 64-frame tiles are not touched by the rule."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from qasr import pack, synth, topology  # noqa: E402

SIDE_BY_SIDE_QUEUES = 8        # smallest tested queue count at which four chains ran side by side
FEW_CHAINS_TILE = 64           # block-end tile below it
B, T = 32, 500
# (res_tile128, GPU_MAX_HW_QUEUES at create time or None = unset) -> block-end tile
CASES = [(None, '4', FEW_CHAINS_TILE), (None, '8', 128), (None, None, FEW_CHAINS_TILE), (None, '16', 128), (None, 'many', FEW_CHAINS_TILE),
         (0, '4', 64), (0, '8', 64), (1, '4', 128), (1, '8', 128)]


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    return engine


@pytest.fixture(scope='module')
def net(golden_dir):
    """full-size QuartzNet15x5 w8a8, 32 utterances x 500 frames, ragged lengths on the edges of the 128-frame tiles"""
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    blob, _ = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), d['act_min'], d['act_max'], 8, 8)
    x = synth.make_features(B, cfg.feat_in, T, 21)
    lens = [T - 11 * (i % 13) - (i % 3) for i in range(B)]
    lens[3], lens[17], lens[29] = 500, 129, 1
    return dict(blob=blob, x=torch.from_numpy(x), lens=torch.tensor(lens, dtype=torch.int32))


@pytest.fixture
def hint(monkeypatch):
    """sets / unsets the hint for the create calls of one test; the A/B overrides never leak in from the caller's shell"""
    for name in ('QASR_RES_TILE', 'QASR_RES_TILE128', 'QASR_TILE128', 'QASR_WIDE_TILES', 'QASR_SEP_GEN'):
        monkeypatch.delenv(name, raising=False)

    def set_hint(value):
        if value is None:
            monkeypatch.delenv('GPU_MAX_HW_QUEUES', raising=False)
        else:
            monkeypatch.setenv('GPU_MAX_HW_QUEUES', value)
    return set_hint


def _sep2_tiles(labels, kernel):
    """(block-end tiles, plain tiles) of the k_sep2 / k_sep2s ops: k_sep2<K, NG, NGP, NP, DBG, TT, DIL>, k_sep2s<K, NG, NGP, NP, TT, DIL>.
    Plain = the separable layers without a residual (K > 0).  The one bare 1x1 layer (K = 0, block 17) is no part of either list: it
    has no 128-frame instantiation (qasr_sep2_impl.h: it spills there) and must sit on 64 frames in every wide-tile plan."""
    res, plain, bare = [], [], []
    for l in labels:
        if not l.startswith(kernel):
            continue
        a = l[len(kernel):-1].split(', ')
        (res if int(a[2]) != 0 else plain if int(a[0]) > 0 else bare).append(int(a[-2]))
    assert len(bare) == 1 and bare[0] in (32, 64), labels
    return res, plain


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    for g, w, name in zip(got, want, ('log-probs', 'tokens', 'encoded lengths')):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), f'{what}: {name} differ'


def _run(e, net, reserved):
    if reserved:
        e.reserve(B, max_frames=T, want_logp=True)
        out = e.forward_ragged(net['x'].cuda(), net['lens'])
    else:
        out = e.forward(net['x'].cuda(), net['lens'])
    torch.cuda.synchronize()
    return [t.clone() for t in out[:3]], e.op_labels()


@pytest.mark.parametrize('reserved', [False, True], ids=['plain', 'reserved'])
def test_block_end_tile_follows_the_rule_and_results_do_not(eng, net, hint, reserved):
    kernel = 'k_sep2s<' if reserved else 'k_sep2<'
    first = None
    for res_tile128, queues, want_tile in CASES:
        hint(queues)
        e = eng.Engine(net['blob'], 0, tile=128, res_tile128=res_tile128)
        out, labels = _run(e, net, reserved)
        e.close()
        what = f'res_tile128={res_tile128} GPU_MAX_HW_QUEUES={queues}'
        res, plain = _sep2_tiles(labels, kernel)
        assert len(res) == 15 and set(res) == {want_tile}, (what, labels)      # the 15 block-end layers of blocks 1 .. 15
        assert len(plain) == 61 and set(plain) == {128}, (what, labels)        # no plain layer moves (60 + block 16's dilation-2 form)
        assert not any('true' in l for l in labels), labels
        if first is None:
            first = out
        else:
            _same(out, first, what)


@pytest.mark.parametrize('tile', [32, 64])
def test_narrow_tile_engines_ignore_the_hint(eng, net, hint, tile):
    """tile_frames 32 / 64: every k_sep2 op on that tile (block 16's dilation-2 form has 64 as its smallest), whatever the hint
    and whatever res_tile128 says"""
    seen = []
    for res_tile128, queues in ((None, '4'), (None, '8'), (0, '4'), (1, '8')):
        hint(queues)
        e = eng.Engine(net['blob'], 0, tile=tile, res_tile128=res_tile128)
        out, labels = _run(e, net, False)
        e.close()
        res, plain = _sep2_tiles(labels, 'k_sep2<')
        assert len(res) == 15 and set(res) == {tile}, labels
        assert len(plain) == 61 and set(plain) <= {tile, 64} and sum(t == tile for t in plain) >= 60, labels   # (64: block 16 in a 32-frame engine)
        seen.append((out, labels))
    for out, labels in seen[1:]:
        assert labels == seen[0][1]
        _same(out, seen[0][0], f'tile={tile}')


def test_override_reaches_every_block_end_tile(eng, net, hint, monkeypatch):
    """QASR_RES_TILE=32|64|128 (A/B runs of an unmodified caller, include/qasr.h) wins over the option and the hint; anything
    else is ignored"""
    hint('4')
    want = None
    for value, want_tile in (('32', 32), ('64', 64), ('128', 128), ('48', FEW_CHAINS_TILE)):
        monkeypatch.setenv('QASR_RES_TILE', value)
        e = eng.Engine(net['blob'], 0, tile=128)
        out, labels = _run(e, net, False)
        e.close()
        res, plain = _sep2_tiles(labels, 'k_sep2<')
        assert len(res) == 15 and set(res) == {want_tile} and len(plain) == 61 and set(plain) == {128}, (value, labels)
        if want is None:
            want = out
        else:
            _same(out, want, f'QASR_RES_TILE={value}')
