"""Wide-vocabulary decoder timing on one GPU: QuartzNet15x5Base-Zh (5207 classes) at BASELINE config 2's shape
(32 utterances x 500 frames -> 250 encoder frames), calibrated with the En w8a8 fixture's ranges (the encoders are
identical), the En engine alongside as context.

Variants, interleaved in one process: k_decw with log-probs, k_decw tokens-only, and the generic path
(fuse_decoder=False: k_sep logits + k_logsoftmax).  Per variant: whole-step time between device events (mean of
`--steps` forwards, `--rounds` interleaved rounds, median round reported) and the decoder op's time from Engine.time_ops
(tokens-only launches: time_ops replays with logp = NULL).  Rates are computed from shapes.

    python profiles/wide_decoder.py --out profiles/wide_decoder_zh.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]

from qasr import engine, pack, synth, topology  # noqa: E402

INT8_PEAK_OPS = 5.0e15          # MI355X dense int8 MFMA peak
HBM_BYTES_S = 8.0e12


def build(cfg, d):
    sd = synth.make_state_dict(cfg, 0)
    return pack.pack_model(cfg, sd, d['act_min'], d['act_max'], 8, 8)[0]


def step_ms(e, x, lens, want_logp, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        e.forward(x, lens, want_logp=want_logp)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50, help='time_ops replays per op')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('wide_decoder.py measures on the GPU; no GPU found')
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_quartznet_w8a8.npz'))
    zh, en = topology.quartznet15x5_zh(), topology.quartznet15x5()
    bzh, ben = build(zh, d), build(en, d)
    B, T = a.batch, a.frames
    x = torch.from_numpy(synth.make_features(B, 64, T, 2)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    engines = {'zh_fused': engine.Engine(bzh, 0), 'zh_generic': engine.Engine(bzh, 0, fuse_decoder=False),
               'en_fused': engine.Engine(ben, 0)}
    variants = [('zh_fused', True), ('zh_fused', False), ('zh_generic', True), ('zh_generic', False), ('en_fused', True),
                ('en_fused', False)]
    outs = {}
    for name, e in engines.items():                      # warm every shape; keep the outputs for the agreement check
        lp, tk, el = e.forward(x, lens)
        e.forward(x, lens, want_logp=False)
        torch.cuda.synchronize()
        outs[name] = (lp, tk, el)
    To = int(outs['zh_fused'][2][0])
    agree = dict(tokens_equal=bool(torch.equal(outs['zh_fused'][1], outs['zh_generic'][1])),
                 logp_max_abs_diff=float((outs['zh_fused'][0] - outs['zh_generic'][0]).abs().max()))
    samples = {f'{n}/{"logp" if w else "tokens"}': [] for n, w in variants}
    for _ in range(a.rounds):
        for n, w in variants:
            samples[f'{n}/{"logp" if w else "tokens"}'].append(step_ms(engines[n], x, lens, w, a.steps))
    step = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v))) for k, v in samples.items()}
    ops = {}
    for name, e in engines.items():
        e.forward(x, lens, want_logp=False)
        ms = e.time_ops(reps=a.reps)
        labels = e.op_labels()
        dec = [i for i, l in enumerate(labels) if l in ('k_dec', 'k_decw')]
        tail = list(range(len(labels) - 2, len(labels)))
        ops[name] = {f'{i}:{labels[i]}': float(ms[i]) for i in (dec or tail)}
        ops[name]['launches'] = e.num_launches()
    ncls, cin = zh.num_classes + 1, 1024
    gop = 2.0 * B * To * ncls * cin / 1e9
    logp_mb = B * To * ncls * 4 / 1e6
    dec_tok_ms = sum(v for k, v in ops['zh_fused'].items() if 'k_decw' in k)
    gen_ms = sum(v for k, v in ops['zh_generic'].items() if k != 'launches')
    dlogp = step['zh_fused/logp']['median_ms'] - step['zh_fused/tokens']['median_ms']
    res = dict(
        shape=dict(batch=B, frames=T, enc_frames=To, classes=ncls, cin=cin),
        work=dict(decoder_gop=gop, logp_mb=logp_mb, floor_us_int8_peak=gop * 1e9 / INT8_PEAK_OPS * 1e6,
                  floor_us_logp_hbm=logp_mb * 1e6 / HBM_BYTES_S * 1e6),
        step=step, time_ops_ms=ops, agreement_fused_vs_generic=agree,
        decoder=dict(
            k_decw_tokens_only_us=dec_tok_ms * 1e3,
            k_decw_tokens_only_gops=gop / dec_tok_ms / 1e3 if dec_tok_ms else None,
            k_decw_tokens_only_share_int8_peak=(gop * 1e9 / INT8_PEAK_OPS) / (dec_tok_ms * 1e-3) if dec_tok_ms else None,
            k_decw_logp_est_us=(dec_tok_ms + dlogp) * 1e3,
            k_decw_logp_est_logp_gb_s=logp_mb / 1e3 / ((dec_tok_ms + dlogp) * 1e-3) if dec_tok_ms + dlogp > 0 else None,
            generic_tokens_only_us=gen_ms * 1e3,
            zh_over_en_step_logp=step['zh_fused/logp']['median_ms'] / step['en_fused/logp']['median_ms'],
            zh_over_en_step_tokens=step['zh_fused/tokens']['median_ms'] / step['en_fused/tokens']['median_ms']),
        note='k_decw_logp_est = time_ops tokens-only decoder time + (step with log-probs - tokens-only step); kernel times '
             'of both launches are in the rocprofv3 --kernel-trace --stats run of this script')
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    for e in engines.values():
        e.close()


if __name__ == '__main__':
    main()
