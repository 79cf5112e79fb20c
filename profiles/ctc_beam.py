#!/usr/bin/env python3
"""CTC prefix beam search on the device, measured on one GPU: QuartzNet15x5 En (29 classes) and Zh (5207 classes) at
32 utterances x 500 frames (250 encoder frames), N = 40 candidates per frame, beam widths 16 and 128.

  kernels  k_topn and k_beam per launch on the engine's own log-probabilities: device events around --steps launches on one
           stream, --rounds samples, median / min / max; k_beam also per frame, k_topn next to the time its one read of the
           log-probabilities takes at 8 TB/s (166.6 MB -> 21 us for Zh).  The per-kernel table of rocprofv3 comes from a run
           of its own:
             rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o beam -- python profiles/ctc_beam.py --child Zh
  engine   host milliseconds per batch on the engine directly, every buffer (candidates, workspace, results) allocated
           beforehand: forward with log-probabilities + k_topn + k_beam + copy of the best row + to_hypotheses, next to the
           greedy path (forward with the collapse attached + copy + to_hypotheses); synchronise and Python included
  decode   the public entry: a calibrated EncDecCTCModel.from_synthetic of the same architecture on the static engine,
           decode(processed_signal=...) next to decode(..., beam_width=W) per batch, synchronise included (allocations of
           candidates, workspace and outputs, argument checks and to_hypotheses are inside)
  bench    `bench.py --gpus 1` on this build and on a build of the parent commit (QASR_LIB), fresh processes alternating this /
           parent, --bench-runs each, each under its own time limit, stopping at the first one that fails

    python profiles/ctc_beam.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_beam.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]


def child(a):
    import numpy as np
    import torch

    from qasr import beam, ctc, engine, pack, synth, topology
    if not torch.cuda.is_available():
        sys.exit('ctc_beam.py measures on the GPU; no GPU found')
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_quartznet_w8a8.npz'))
    cfg = topology.quartznet15x5() if a.child == 'En' else topology.quartznet15x5_zh()
    blob = pack.pack_model(cfg, synth.make_state_dict(cfg, 0), d['act_min'], d['act_max'], 8, 8)[0]
    B, T, ncls, N = a.batch, a.frames, cfg.num_classes + 1, a.top_n
    x = torch.from_numpy(synth.make_features(B, 64, T, 2)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    e = engine.Engine(blob, 0, graph=True)
    To = e.out_frames(T)
    out = (torch.empty(B, To, ncls, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))
    logp, _, enc_len = e.forward(x, lens, want_logp=True, out=out)[:3]
    torch.cuda.synchronize()
    cand = (torch.empty(B, To, N, dtype=torch.int32, device='cuda'), torch.empty(B, To, N, dtype=torch.int32, device='cuda'))
    widths = [int(w) for w in a.widths.split(',')]
    ws = {W: torch.empty(engine.ctc_beam_workspace_bytes(B, To, W), dtype=torch.uint8, device='cuda') for W in widths}
    res_buf = {}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        samples = []
        for _ in range(a.rounds):
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.steps):
                fn()
            t.record()
            t.synchronize()
            samples.append(s.elapsed_time(t) / a.steps * 1e3)
        return samples

    def run_beam(W):
        res_buf[W] = engine.ctc_beam(cand[0], cand[1], enc_len, ncls - 1, W, W, workspace=ws[W], out=res_buf.get(W))

    kern = dict(k_topn_us=timed(lambda: engine.ctc_topn(logp, enc_len, N, out=cand)))
    for W in widths:
        kern[f'k_beam_w{W}_us'] = timed(lambda: run_beam(W))
    # the device results are the twin's (first two utterances; the test suite holds every byte of many more)
    twin = beam.search_host(logp[:2].cpu().numpy(), enc_len[:2].cpu().numpy(), ncls - 1, widths[0], widths[0], N)
    same = all(np.array_equal(getattr(res_buf[widths[0]], f)[:2].cpu().numpy(), getattr(twin, f)) for f in ('labels', 'n_labels', 'score', 'n_hyps'))
    res = dict(model=a.child, classes=ncls, enc_frames=int(To), top_n=N, kernels_us=kern, equals_twin=bool(same),
               logp_bytes=int(logp.numel() * 4), topn_floor_us=logp.numel() * 4 / 8e12 * 1e6)
    if a.e2e:
        eg = engine.Engine(blob, 0, graph=True)
        spf = ctc.seconds_per_frame(cfg, 0.01)
        t_greedy, t_beam = [], {W: [] for W in widths}
        for k in range(a.e2e + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = eg.forward(x, lens, want_logp=False, decode=True)[3]
            torch.cuda.synchronize()
            hy = ctc.to_hypotheses(r, cfg.vocabulary, spf)
            t1 = time.perf_counter()
            if k >= 2:
                t_greedy.append((t1 - t0) * 1e3)
            for W in widths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lp, _, el = e.forward(x, lens, want_logp=True, out=out)[:3]
                engine.ctc_topn(lp, el, N, out=cand)
                run_beam(W)
                torch.cuda.synchronize()
                hb = beam.to_hypotheses(beam.BeamResult(res_buf[W].labels[:, :1], res_buf[W].n_labels[:, :1], res_buf[W].score[:, :1],
                                                        res_buf[W].n_hyps.clamp(max=1), ncls - 1), cfg.vocabulary)
                t1 = time.perf_counter()
                if k >= 2:
                    t_beam[W].append((t1 - t0) * 1e3)
        res['e2e_host_ms'] = dict(greedy=t_greedy, **{f'beam_w{W}': v for W, v in t_beam.items()},
                                  beam_differs_from_greedy=sum(g.text != b[0].text for g, b in zip(hy, hb)), utterances=B)
        eg.close()
    e.close()
    if a.e2e:
        res['decode_host_ms'] = facade(a, widths, N)
    print('CTC_BEAM_CHILD ' + json.dumps(res), flush=True)


def facade(a, widths, N):
    """EncDecCTCModel.decode per batch: greedy and with a beam, on a calibrated synthetic model (static engine)"""
    import torch

    import nemo.quantization.utils.quantize_model as qm
    from nemo.collections.asr.models import EncDecCTCModel
    from qasr import synth
    torch.set_grad_enabled(False)
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-' + a.child).cuda()
    m.eval()
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([a.frames] * 4).cuda()
    for c in synth.make_calibration(2, 4, 64, a.frames):
        enc, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=enc, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    x = torch.from_numpy(synth.make_features(a.batch, 64, a.frames, 2)).cuda()
    lens = torch.full((a.batch,), a.frames).cuda()
    out = dict(greedy=[], **{f'beam_w{W}': [] for W in widths})
    for k in range(a.e2e + 2):
        for name, kw in [('greedy', {})] + [(f'beam_w{W}', dict(beam_width=W, cutoff_top_n=N)) for W in widths]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.decode(processed_signal=x, processed_signal_length=lens, **kw)
            torch.cuda.synchronize()
            if k >= 2:
                out[name].append((time.perf_counter() - t0) * 1e3)
    assert type(m._engine).__name__ == 'Engine'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['En', 'Zh'], default=None)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--top-n', type=int, default=40)
    ap.add_argument('--widths', default='16,128')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--e2e', type=int, default=5, help='batches of the end-to-end host timing (0: skip)')
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (bench.py A/B)')
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np

    def stat(v):
        return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))

    summary, runs = {}, []
    for model in ('En', 'Zh'):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', model, '--batch', str(a.batch), '--frames', str(a.frames),
               '--top-n', str(a.top_n), '--widths', a.widths, '--steps', str(a.steps), '--rounds', str(a.rounds), '--e2e', str(a.e2e)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f'child {model} ran past {a.child_timeout} s: stopping')
        line = [l for l in p.stdout.splitlines() if l.startswith('CTC_BEAM_CHILD ')]
        if p.returncode or not line:
            sys.exit(f'child {model} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
        r = json.loads(line[0][len('CTC_BEAM_CHILD '):])
        runs.append(r)
        s = {k: stat(v) for k, v in r['kernels_us'].items()}
        for k in list(s):
            if k.startswith('k_beam'):
                s[k + '_per_frame'] = s[k]['median'] / r['enc_frames']
        s['k_topn_floor_us'] = r['topn_floor_us']
        s['equals_twin'] = r['equals_twin']
        for key in ('e2e_host_ms', 'decode_host_ms'):
            if key in r:
                s[key] = {k: (stat(v) if isinstance(v, list) else v) for k, v in r[key].items()}
        summary[model] = s
        print(model, json.dumps(s), flush=True)
    bench = {}
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        bench = dict(this=[], parent=[])
        for r in range(a.bench_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib)):
                cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1']
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.bench_timeout,
                                       env=dict(os.environ, QASR_LIB=os.path.abspath(lib)))
                except subprocess.TimeoutExpired:
                    sys.exit(f'bench.py ({tag}) ran past {a.bench_timeout} s: stopping')
                line = [l for l in p.stdout.splitlines() if l.startswith('{')]
                if p.returncode or not line:
                    sys.exit(f'bench.py ({tag}) failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
                rec = json.loads(line[-1])
                bench[tag].append(dict(ms_per_step=rec['ms_per_step'], value=rec['value'], steps=rec['steps'], warmup=rec['warmup']))
                print(f'bench {tag} run {r}: ' + json.dumps(bench[tag][-1]), flush=True)
    res = dict(shape=dict(batch=a.batch, frames=a.frames, top_n=a.top_n), steps=a.steps, rounds=a.rounds,
               note='kernel times: device events around `steps` launches on one stream (microseconds per launch); synthetic random '
                    'weights, so the distributions are flatter than a trained model\'s', summary=summary, bench=bench, runs=runs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
