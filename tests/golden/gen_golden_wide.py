#!/usr/bin/env python3
"""Golden fixture of a WIDE decoder: MiniQuartzNet with a 5206-label (+ blank) decoder, calibrated and run by the
reference's own modules on the CPU (gen_golden.py's recipe and helpers, imported, not edited).  Runs only where the
reference tree is available.

    python tests/golden/gen_golden_wide.py      # -> net_miniq_wide_w8a8.npz

The full [B][5207][T] tensors would be ~1 MB per array, so the fixture keeps: the calibrated ranges, encoded lengths,
greedy tokens, per-frame max logit and log-sum-exp, the log-probs of a fixed seeded subset of 256 class columns, and
every conv's checksums (accumulator, input codes, weight codes).
"""
import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402  (sets up the reference import recipe)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qasr import synth, topology  # noqa: E402

NAME = 'net_miniq_wide_w8a8'
SEED, WBIT, ABIT = 1, 8, 8
BATCH, FRAMES, LENGTHS = 2, 96, (96, 57)
NCAL, CAL_BATCH = 3, 4
N_COLS = 256


def wide_cfg():
    n = 5206
    return dataclasses.replace(topology.mini_quartznet(), num_classes=n, vocabulary=topology.zh_placeholder_vocabulary(n))


def class_subset(ncls, n=N_COLS, seed=5206):
    """The fixed, sorted set of class columns whose log-probs the fixture stores (blank and class 0 always included)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cols = rng.choice(np.arange(1, ncls - 1), n - 2, replace=False)
    return np.sort(np.concatenate([[0, ncls - 1], cols])).astype(np.int64)


def main():
    cfg = wide_cfg()
    sd = synth.make_state_dict(cfg, SEED)
    model, blocks = G.build_reference_model(cfg, sd, WBIT, ABIT, None)
    G.qm.calibrate(model)
    clen = torch.tensor([FRAMES] * CAL_BATCH)
    for c in synth.make_calibration(NCAL, CAL_BATCH, cfg.feat_in, FRAMES, SEED):
        o, _, sf = G.encoder_forward(blocks, torch.from_numpy(c), clen)
        G.decoder_forward(model.decoder, o, sf)
    G.qm.evaluate(model)
    G.qm.set_dynamic(model, False)
    x = synth.make_features(BATCH, cfg.feat_in, FRAMES, SEED)
    with G.ConvTap() as tap:
        tap.enabled = True
        enc, enc_len, enc_sf = G.encoder_forward(blocks, torch.from_numpy(x), torch.tensor(LENGTHS))
        logits, logp = G.decoder_forward(model.decoder, enc, enc_sf)
    lt = logits.transpose(1, 2).numpy().astype(np.float32)          # [B][T][C]
    acts = G.quant_acts_in_order(model, blocks)
    cols = class_subset(cfg.num_classes + 1)
    sums = []
    for c in tap.calls:
        sums.append(np.concatenate([G.checksum(np.rint(c['y'].numpy())), G.checksum(np.rint(c['x'].numpy())),
                                    G.checksum(c['w'].numpy())]))
    out = dict(
        meta=np.array(json.dumps(dict(model=NAME, seed=SEED, wbit=WBIT, abit=ABIT, percentile=None, batch=BATCH,
                                      frames=FRAMES, lengths=list(LENGTHS), ncal=NCAL, cal_batch=CAL_BATCH,
                                      nconv=len(tap.calls), num_classes=cfg.num_classes))),
        act_min=np.array([float(a.x_min) for a in acts], dtype=np.float32),
        act_max=np.array([float(a.x_max) for a in acts], dtype=np.float32),
        enc_len=enc_len.numpy().astype(np.int64),
        tokens=logp.argmax(-1).numpy().astype(np.int64),
        max_logit=lt.max(-1),
        logsumexp=torch.logsumexp(torch.from_numpy(lt), dim=-1).numpy().astype(np.float32),
        cols=cols,
        log_probs_cols=logp.numpy()[:, :, cols].astype(np.float32),
        conv_checksums=np.stack(sums),
    )
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print(f'{NAME}: {len(tap.calls)} convs, {os.path.getsize(path)} bytes, tokens[0][:12]={out["tokens"][0][:12].tolist()}')


if __name__ == '__main__':
    main()
