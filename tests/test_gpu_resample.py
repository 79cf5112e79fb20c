"""k_resample on an MI355X against its NumPy twin (qasr.resample.resample_host): every byte of `out` - the whole pitch, zeros
behind each row's length included - and of `out_lens` is equal, for int16 and float32 input, 1 - 3 channels, ragged batches with
full-scale fill behind the lengths, output lengths around the tile edges, a 14 M sample utterance whose positions pass 2^31, a
captured launch replayed on new data, and the steep-ratio instantiation that reads global memory per tap."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_cases as rc  # noqa: E402
from qasr import resample as rs  # noqa: E402

TILE = rc.TILE              # 256 outputs per work-group (RS_TILE)
_plans = {}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()


def plan(sr, quality='best'):
    if (sr, quality) not in _plans:
        _plans[sr, quality] = rs.ResamplePlan(sr, 16000, quality)
    return _plans[sr, quality]


def _run(x, lens, p, ch=1, pitch=None):
    from qasr import engine
    xd = torch.from_numpy(x).cuda()
    ld = torch.tensor(list(lens), dtype=torch.int32).cuda()
    out = None if pitch is None else torch.full((x.shape[0], pitch), 7.0, device='cuda')
    out, out_lens = engine.resample(xd, ld, p, channels=ch, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_lens.cpu().numpy()


def _assert_equal(got, want, what):
    (go, gl), (wo, wl) = got, want
    assert gl.dtype == wl.dtype == np.int32 and gl.tobytes() == wl.tobytes(), (what, gl, wl)
    assert go.dtype == wo.dtype == np.float32 and go.shape == wo.shape, (what, go.shape, wo.shape)
    if go.tobytes() != wo.tobytes():
        bad = np.argwhere(go.view(np.uint32) != wo.view(np.uint32))
        raise AssertionError(f'{what}: {len(bad)} of {go.size} outputs differ, first at {bad[0].tolist()}: '
                             f'{go[tuple(bad[0])]!r} != {wo[tuple(bad[0])]!r}')


@pytest.mark.parametrize('sr,quality', [(8000, 'best'), (11025, 'best'), (32000, 'best'), (44100, 'best'), (48000, 'best'),
                                        (44100, 'fast'), (8000, 'fast'), (96000, 'best'), (12000, 'fast')])
@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_rates_ragged_batch(sr, quality, dtype):
    """B = 4 with lengths 0, 1, W - 1 and full, 32767 / -32768 behind each length; more than one tile per row"""
    p = plan(sr, quality)
    S = max(rc.frames_for(p, 2 * TILE + 77), p.W + 3)
    lens = [0, 1, p.W - 1, S]
    x = rc.fill_behind(rc.pcm(4, S, 1, seed=sr), lens)
    if dtype == 'float32':
        x = rc.to_float(x)
    want = rs.resample_host(x, lens, p)
    assert want[0].shape[1] > 2 * TILE and want[1][3] == want[0].shape[1]
    _assert_equal(_run(x, lens, p), want, f'{sr} {quality} {dtype}')


@pytest.mark.parametrize('sr', [8000, 32000, 44100, 48000])
def test_tile_edges(sr):
    """output lengths of TILE - 1, TILE, TILE + 1 and 2 TILE + 1 (TILE = 256 outputs per work-group), in rows of a longer pitch
    (8 kHz doubles every length: 256, 256, 258 and 514 there)"""
    p = plan(sr, 'fast')
    targets = [TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    lens = [rc.frames_for(p, t) for t in targets]
    if sr == 8000:
        targets = [TILE, TILE, TILE + 2, 2 * TILE + 2]
    S = max(lens) + 40
    x = rc.fill_behind(rc.pcm(len(lens), S, 1, seed=sr + 1), lens)
    want = rs.resample_host(x, lens, p)
    assert want[1].tolist() == targets
    _assert_equal(_run(x, lens, p), want, f'{sr} tile edges')
    # a caller's pitch that is no multiple of the tile, longer than every row: zeros to the pitch; and one that cuts the longest row
    pitch = 3 * TILE + 5
    got = _run(x, lens, p, pitch=pitch)
    wide = np.zeros((len(lens), pitch), np.float32)
    wide[:, :want[0].shape[1]] = want[0]
    _assert_equal(got, (wide, want[1]), f'{sr} wide pitch')
    got = _run(x, lens, p, pitch=TILE + 1)
    _assert_equal(got, (want[0][:, :TILE + 1].copy(), np.minimum(want[1], TILE + 1).astype(np.int32)), f'{sr} cut pitch')


@pytest.mark.parametrize('dtype', ['int16', 'float32'])
@pytest.mark.parametrize('ch', [1, 2, 3])
def test_channels(ch, dtype):
    for sr, quality in ((44100, 'best'), (8000, 'fast'), (16000, 'best')):          # 16000: the equal-rate bypass
        p = plan(sr, quality)
        S = rc.frames_for(p, TILE + 9) if not p.equal else TILE + 9
        lens = [S, S // 2, 0]
        x = rc.pcm(3, S, ch, seed=sr + ch)
        x[:, ::ch] |= 1                                              # odd channel sums: the division by ch is exercised
        x = rc.fill_behind(x, lens, ch)
        if dtype == 'float32':
            x = rc.to_float(x)
        _assert_equal(_run(x, lens, p, ch), rs.resample_host(x, lens, p, channels=ch), f'{sr} {quality} {ch} channels {dtype}')


def test_steep_ratio_takes_the_direct_instantiation():
    """above about 14 : 1 (fast; 10 : 1 with best) the tile's input stretch no longer fits the LDS stage (4096 frames): the same bytes from global memory"""
    p = rs.ResamplePlan(400000, 16000, 'fast')                       # 25 : 1, W = 471: 255 * 25 + 1 + 942 > 4096
    assert (p.L, p.M) == (1, 25) and 255 * p.M + 1 + 2 * p.W > 4096
    S = rc.frames_for(p, TILE + 3)
    lens = [S, p.W - 1, 1]
    for ch, dtype in ((1, 'int16'), (2, 'float32')):
        x = rc.fill_behind(rc.pcm(3, S, ch, seed=4), lens, ch)
        if dtype == 'float32':
            x = rc.to_float(x)
        _assert_equal(_run(x, lens, p, ch), rs.resample_host(x, lens, p, channels=ch), f'400 kHz {dtype}')


def test_long_utterance_positions_pass_2_31():
    """one 44.1 kHz utterance of 14 000 000 samples: 5.08 M outputs, i * M passes 2^31 after 4.87 M; the first and the last 4096
    outputs against the twin's out_range"""
    from qasr import engine
    p = plan(44100)
    n = 14_000_000
    rng = np.random.default_rng(0)
    x = rng.integers(-32768, 32768, (1, n), dtype=np.int16)
    P = p.out_len(n)
    assert (P - 1) * p.M > 2 ** 31 and P > 5_000_000
    out, out_lens = engine.resample(torch.from_numpy(x).cuda(), torch.tensor([n], dtype=torch.int32).cuda(), p)
    torch.cuda.synchronize()
    assert out.shape == (1, P) and out_lens.tolist() == [P]
    head, tail = out[:, :4096].cpu().numpy(), out[:, P - 4096:].cpu().numpy()
    assert head.tobytes() == rs.resample_host(x, [n], p, out_range=(0, 4096))[0].tobytes()
    assert tail.tobytes() == rs.resample_host(x, [n], p, out_range=(P - 4096, P))[0].tobytes()
    mid = 4_870_000                                                   # where the 32-bit product would wrap
    assert out[:, mid:mid + 512].cpu().numpy().tobytes() == rs.resample_host(x, [n], p, out_range=(mid, mid + 512))[0].tobytes()


def test_graph_capture_and_replay():
    """lengths are device data and nothing is read back: a captured launch replayed on new samples and new lengths"""
    from qasr import engine
    p = plan(44100)
    S = rc.frames_for(p, 2 * TILE + 30)
    engine.resample_plan(p, 'cuda')                                  # the upload happens outside the capture
    xd = torch.zeros(3, S, dtype=torch.int16, device='cuda')
    ld = torch.zeros(3, dtype=torch.int32, device='cuda')
    out = torch.empty(3, p.out_len(S), device='cuda')
    out_lens = torch.empty(3, dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.resample(xd, ld, p, out=out, out_lens=out_lens)
    for k, lens in enumerate(([S, 100, 0], [5, S - 1, S // 2])):
        x = rc.fill_behind(rc.pcm(3, S, 1, seed=20 + k), lens)
        xd.copy_(torch.from_numpy(x)), ld.copy_(torch.tensor(lens, dtype=torch.int32))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _assert_equal((out.cpu().numpy(), out_lens.cpu().numpy()), rs.resample_host(x, lens, p), f'replay {k}')


def test_bad_arguments_return_err_arg_without_launching():
    from qasr import engine
    lib = engine.load_library()
    p = plan(8000)
    blob = engine.resample_plan(p, 'cuda')
    x = torch.zeros(2, 64, dtype=torch.int16, device='cuda')
    ln = torch.full((2,), 64, dtype=torch.int32, device='cuda')
    out = torch.full((2, 128), 7.0, device='cuda')
    ol = torch.full((2,), -5, dtype=torch.int32, device='cuda')

    def args(**kw):
        a = engine.ResampleArgs()
        a.struct_size = ctypes.sizeof(engine.ResampleArgs)
        a.B, a.channels, a.dtype, a.L, a.M, a.W = 2, 1, engine.PCM_S16, p.L, p.M, p.W
        a.blob, a.blob_bytes = blob.data_ptr(), blob.numel()
        a.in_, a.in_lens, a.in_pitch = x.data_ptr(), ln.data_ptr(), 64
        a.out, a.out_pitch, a.out_lens = out.data_ptr(), 128, ol.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    stream = engine._stream_ptr()
    assert lib.qasr_resample(stream, None) == 1
    for kw in (dict(struct_size=8), dict(blob=0), dict(in_=0), dict(in_lens=0), dict(out=0), dict(out_lens=0), dict(B=0), dict(B=65536),
               dict(channels=0), dict(channels=9), dict(dtype=2), dict(L=0), dict(M=0), dict(W=0), dict(W=4097), dict(L=4, M=2),
               dict(blob=blob.data_ptr() + 4), dict(blob_bytes=blob.numel() - 4), dict(W=p.W + 1), dict(in_pitch=-1),
               dict(in_pitch=2 ** 38 + 1), dict(out_pitch=-1), dict(out_pitch=2 ** 38 + 1)):
        assert lib.qasr_resample(stream, ctypes.byref(args(**kw))) == 1, kw
        assert lib.qasr_last_error().decode().startswith('resample:')
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(ol == -5)             # nothing was launched
    assert lib.qasr_resample(stream, ctypes.byref(args())) == 0
    torch.cuda.synchronize()
    assert ol.tolist() == [128, 128]
    with pytest.raises(ValueError, match='channels'):
        engine.resample(x, ln, p, channels=3)
    with pytest.raises(ValueError, match='int16 or float32'):
        engine.resample(x.double(), ln, p)
