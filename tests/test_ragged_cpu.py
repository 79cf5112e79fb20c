"""Reserved engines (qasr_engine_reserve), the parts that need no GPU: the bucket policy in Python and in C, the ABI's
argument checks, and the invariance premise the feature rests on."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import nemo.quantization.utils.quantize_model as qm
from nemo.collections.asr.models import EncDecCTCModel
from qasr import configs, ragged, synth, topology

torch.set_grad_enabled(False)


@pytest.fixture(scope='module')
def lib():
    from qasr import build, engine
    build.build_native()
    return engine.load_library()


ENVELOPES = [1, 100, 128, 129, 500, 1000, 1664, 2048, 2049, 128 * 64, 128 * 65, 128 * 1000 + 1]
GRAPHS = [1, 2, 3, 7, 16, 64]


@pytest.mark.parametrize('max_graphs', GRAPHS)
@pytest.mark.parametrize('frames', ENVELOPES)
def test_bucket_policy_properties(frames, max_graphs):
    """Every shape of an envelope maps to a bucket >= it; edges are multiples of 128 frames (hence of every pad_to that
    divides 128); there are at most max_graphs of them; envelopes of one frame and of the maximum work."""
    M = ragged.envelope_frames(0, frames, 16)
    assert M >= frames and M % ragged.TILE == 0 and M - frames < ragged.TILE
    edges = ragged.bucket_edges(M, max_graphs)
    assert 1 <= len(edges) <= max_graphs and edges[-1] == M
    seen = set()
    ts = range(1, M + 1) if M <= 4096 else list(range(1, M + 1, 61)) + [M - 1, M]
    for T in ts:
        b = ragged.bucket_frames(M, max_graphs, T)
        assert T <= b <= M and b % ragged.TILE == 0, (T, b)
        for pad_to in (1, 2, 16, 64, 128):
            assert b % pad_to == 0
        assert b in edges
        seen.add(b)
    if M <= 4096:
        assert seen == set(edges)                              # every edge is reachable, none beyond them
    assert ragged.bucket_frames(M, max_graphs, 1) == edges[0] and ragged.bucket_frames(M, max_graphs, M) == M
    assert ragged.bucket_frames(M, max_graphs, M + 1) == -1 and ragged.bucket_frames(M, max_graphs, 0) == -1
    # monotone: a longer batch never lands in a smaller bucket
    bs = [ragged.bucket_frames(M, max_graphs, T) for T in ts]
    assert bs == sorted(bs)


def test_envelope_from_samples_and_bad_arguments():
    assert ragged.envelope_frames(16 * 16000, 0, 16) == 1664       # 16 s: 1601 STFT frames -> 1616 (pad_to 16) -> 13 tiles
    assert ragged.envelope_frames(16 * 16000, 2000, 16) == 2048    # the larger of the two entries
    assert ragged.envelope_frames(0, 0, 16) == -1 and ragged.envelope_frames(1000, 0, 48) == -1
    assert ragged.envelope_frames(-1, 10, 16) == -1
    assert ragged.bucket_frames(1000, 16, 10) == -1                # not a multiple of the tile


def test_c_policy_agrees_with_python(lib):
    """csrc/qasr_ragged.hip states the policy once, qasr/ragged.py restates it: held together over a sweep of shapes."""
    rng = np.random.default_rng(17)
    for frames in ENVELOPES:
        for pad_to in (0, 1, 16, 128, 48):
            for samples in (0, 257, 16000, 16 * 16000 + 3):
                assert lib.qasr_ragged_envelope_frames(samples, frames, pad_to) == ragged.envelope_frames(samples, frames, pad_to)
        M = ragged.envelope_frames(0, frames, 16)
        for g in GRAPHS:
            ts = [0, 1, 2, 127, 128, 129, M - 1, M, M + 1] + [int(t) for t in rng.integers(1, M + 1, 200)]
            for T in ts:
                assert lib.qasr_ragged_bucket_frames(M, g, T) == ragged.bucket_frames(M, g, T), (M, g, T)
    assert lib.qasr_ragged_bucket_frames(1000, 16, 10) == -1 and lib.qasr_ragged_bucket_frames(1024, 0, 10) == -1
    for s in (1, 159, 160, 80000, 256001):
        for p in (0, 1, 16):
            assert lib.qasr_frontend_frames(s, p) == ragged.frontend_frames(s, p)


def test_abi_is_declared_exported_and_sized(lib, tmp_path):
    from qasr import engine
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'qasr.h')).read()
    for sym in ('qasr_engine_reserve', 'qasr_engine_forward_ragged', 'qasr_engine_forward_ragged_audio', 'qasr_engine_ragged_stats',
                'qasr_ragged_bucket_frames', 'qasr_ragged_envelope_frames'):
        assert sym + '(' in hdr and sym in engine.SYMBOLS and hasattr(lib, sym), sym
    import subprocess
    probe = tmp_path / 'probe.c'
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qasr.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                     'sizeof(qasr_reserve_opts),sizeof(qasr_ragged_out),sizeof(qasr_ragged_stats),offsetof(qasr_ragged_out, ctc),'
                     'offsetof(qasr_ragged_out, feats),offsetof(qasr_ragged_stats, bucket_calls));return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include'), str(probe),
                    '-o', str(exe)], check=True)
    sizes = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert sizes[0] == C.sizeof(engine.ReserveOpts) and sizes[1] == C.sizeof(engine.RaggedOut)
    assert sizes[2] == C.sizeof(engine.RaggedStats) and sizes[3] == engine.RaggedOut.ctc.offset
    assert sizes[4] == engine.RaggedOut.feats.offset and sizes[5] == engine.RaggedStats.bucket_calls.offset


def test_bad_arguments_are_refused_without_a_gpu(lib):
    """struct sizes, zero maxima, a missing engine: QASR_ERR_ARG with a message, before any HIP call."""
    from qasr import engine
    err = lambda: lib.qasr_last_error().decode()
    o = engine.ReserveOpts()
    o.struct_size, o.max_batch, o.max_frames = C.sizeof(o) - 4, 4, 512
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and 'struct_size' in err()
    o.struct_size = C.sizeof(o) + 8
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and 'struct_size' in err()
    o.struct_size, o.max_batch = C.sizeof(o), 0
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and 'max_batch' in err()
    o.max_batch, o.max_frames, o.max_samples = 4, 0, 0
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and 'max_samples and max_frames' in err()
    o.max_samples = 200
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and '256' in err()
    o.max_samples, o.pad_to = 16000, 48
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and 'pad_to' in err()
    o.pad_to, o.max_graphs = 16, 65
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and 'max_graphs' in err()
    o.max_graphs = 0
    assert lib.qasr_engine_reserve(None, C.byref(o)) == 1 and 'engine is NULL' in err()
    assert lib.qasr_engine_reserve(None, None) == 1
    ro = engine.RaggedOut()
    ro.struct_size = C.sizeof(ro)
    x = (C.c_float * 16)()
    n = (C.c_int32 * 4)()
    assert lib.qasr_engine_forward_ragged(None, None, x, n, 1, 16, C.byref(ro)) == 1
    assert lib.qasr_engine_forward_ragged_audio(None, None, x, n, 1, 16, x, x, 64, C.c_float(0.97), 16, x, 64, C.byref(ro)) == 1
    st = engine.RaggedStats()
    st.struct_size = C.sizeof(st)
    assert lib.qasr_engine_ragged_stats(None, C.byref(st)) == 1


def _calibrated_mini(golden_dir):
    d = np.load(os.path.join(golden_dir, 'net_miniq_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.mini_quartznet()
    m = EncDecCTCModel(configs.model_config(cfg))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(cfg, meta['seed']).items()}
    m.load_state_dict(sd, strict=False)
    m.eval()
    m.set_quant_bit(meta['wbit'], mode='weight')
    m.set_quant_bit(meta['abit'], mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([meta['frames']] * meta['cal_batch'])
    for c in synth.make_calibration(meta['ncal'], meta['cal_batch'], cfg.feat_in, meta['frames'], meta['seed']):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    return cfg, m


def test_invariance_premise_on_the_host_modules(golden_dir):
    """The premise of bucketed execution, as a standing test on the calibrated fake-quant modules: a static-mode model's
    outputs on rows < B and frames < T' - padded frames of short utterances included - do not change when the batch is
    embedded in a larger [B2][T2] tensor whose added rows have length 0.  (It holds without the feature; it guards the
    premise the engine's bit-exactness tests build on.)"""
    cfg, m = _calibrated_mini(golden_dir)
    B, T, lens = 3, 176, [176, 97, 1]
    x = torch.from_numpy(synth.make_features(B, cfg.feat_in, T, 11))
    e, l, sf = m.encoder(audio_signal=x, length=torch.tensor(lens))
    lp = m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    for B2, T2 in ((5, 320), (3, 256), (4, 176)):
        big = torch.from_numpy(synth.make_features(B2, cfg.feat_in, T2, 12)) * 3.0      # the added frames / rows hold data, not zeros
        big[:B, :, :T] = x
        e2, l2, sf2 = m.encoder(audio_signal=big, length=torch.tensor(lens + [0] * (B2 - B)))
        lp2 = m.decoder(encoder_output=e2, encoder_output_scaling_factor=sf2)
        To = lp.shape[1]
        assert torch.equal(lp2[:B, :To], lp), (B2, T2)
        assert torch.equal(lp2[:B, :To].argmax(-1), lp.argmax(-1))
        assert torch.equal(l2[:B], l)
