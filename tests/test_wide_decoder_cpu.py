"""QuartzNet15x5Base-Zh on the host side (no GPU): the topology registers with the 5206-label placeholder vocabulary, the
model list names it, its packed blob passes qasr_blob_check, and its encoder is QuartzNet15x5's, weights included."""
import json
import os

import numpy as np
import pytest

from qasr import pack, synth, topology


def test_zh_topology_registered():
    cfg = topology.MODELS['QuartzNet15x5Base-Zh']()
    en = topology.quartznet15x5()
    assert cfg.name == 'QuartzNet15x5Base-Zh' and cfg.num_classes == 5206
    assert cfg.blocks == en.blocks and cfg.feat_in == en.feat_in
    v = cfg.vocabulary
    assert len(v) == 5206 and len(set(v)) == 5206 and all(len(c) == 1 for c in v)
    assert v[:3] == [' ', "'", 'A'] and v[28] == '一'


def test_zh_in_available_models():
    torch = pytest.importorskip('torch')  # noqa: F841
    from nemo.collections.asr.models.ctc_models import EncDecCTCModel
    assert 'QuartzNet15x5Base-Zh' in EncDecCTCModel.list_available_models()
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-Zh')
    assert len(m.decoder.vocabulary) == 5206


def test_zh_encoder_weights_equal_en(golden_dir):
    """synth draws the decoder last: one seed gives the En net's encoder bit for bit (so the En fixtures' calibrated
    ranges apply to the Zh net unchanged)."""
    zh = synth.make_state_dict(topology.quartznet15x5_zh(), 0)
    en = synth.make_state_dict(topology.quartznet15x5(), 0)
    enc = [k for k in en if k.startswith('encoder.')]
    assert enc and all(np.array_equal(zh[k], en[k]) for k in enc)
    assert zh['decoder.decoder_layers.0.weight'].shape == (5207, 1024, 1)


def test_zh_blob_passes_check(golden_dir):
    from qasr import engine
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5_zh()
    blob, pm = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), d['act_min'], d['act_max'], 8, 8)
    hdr = np.frombuffer(blob[:40], dtype=np.uint32)
    assert int(hdr[5]) == 5207
    engine.blob_check(blob)                                   # host-only validation, no GPU


def test_oracle_matches_reference_wide_fixture(golden_dir):
    """tests/golden/net_miniq_wide_w8a8.npz (gen_golden_wide.py: MiniQuartzNet with 5206 labels + blank, calibrated and
    run by the reference's own modules): OracleNet - what the GPU tests hold the wide decoder to - reproduces every conv
    checksum, the encoded lengths and tokens exactly, and the log-probs of the stored class columns, the per-frame max
    logit and log-sum-exp within the existing bound."""
    from oracle import int_oracle as O
    import dataclasses
    d = np.load(os.path.join(golden_dir, 'net_miniq_wide_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    n = meta['num_classes']
    cfg = dataclasses.replace(topology.mini_quartznet(), num_classes=n, vocabulary=topology.zh_placeholder_vocabulary(n))
    sd = synth.make_state_dict(cfg, meta['seed'])
    net = O.OracleNet(topology.conv_plan(cfg), cfg, sd, d['act_min'], d['act_max'], meta['wbit'], meta['abit'])
    out = net.forward(synth.make_features(meta['batch'], cfg.feat_in, meta['frames'], meta['seed']), meta['lengths'])
    assert len(net.trace) == meta['nconv']
    for i, t in enumerate(net.trace):
        got = np.concatenate([O.checksum(t['acc']), O.checksum(t['xint']), O.checksum(t['wint'])])
        assert np.array_equal(got, d['conv_checksums'][i]), (i, t['key'])
    assert np.array_equal(out['enc_len'], d['enc_len'])
    assert np.array_equal(out['tokens'], d['tokens'])
    lp = np.asarray(out['log_probs'])
    assert lp.shape[2] == n + 1
    np.testing.assert_allclose(lp[:, :, d['cols']], d['log_probs_cols'], rtol=1e-4, atol=5e-5)
    lg = np.asarray(out['logits'])
    lg = lg if lg.shape[-1] == n + 1 else lg.transpose(0, 2, 1)     # [B][T][C]
    np.testing.assert_allclose(lg.max(-1), d['max_logit'], rtol=1e-5, atol=1e-5)
    lse = lg.max(-1) + np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1))
    np.testing.assert_allclose(lse, d['logsumexp'], rtol=1e-4, atol=5e-5)
