#!/usr/bin/env python3
"""What streaming costs, measured on one GPU: full-size QuartzNet15x5Base-En (synthetic weights, calibrated), 1 / 8 / 32 live
streams of synthetic 16 kHz audio, the defaults of EncDecCTCModel.stream (chunks of 0.96 s, 4.0 s of context, 0.96 s of
look-ahead).

  steps    host wall time per session step, read-back included (device synchronised before and after every push of one chunk
           per stream), over the steps whose windows are full; against the bare `_forward(windows, lens, decode='frames')` of
           the identical window batch on the same reserved engine in the same run (the session's own windows, taken from the
           device after the step).  The difference is what streaming costs: push + window + emit, their launches, the small
           uploads and the read-back.  No limit is fixed in advance; when the difference exceeds a tenth of the forward the
           record says so and `kernels` says where the device time goes.  The reserved engine's counters before and after.
  kernels  the three kernels' device times need a rocprofv3 run of its own:
             rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o stream -- python profiles/stream.py --child steps --streams 32
           then --stats-csv <the kernel_stats.csv it wrote> picks k_stream_push / _window / _emit out of the table.
  bench    `bench.py --gpus 1` on this build and on a build of the parent commit (QASR_LIB), fresh processes alternating this /
           parent, --bench-runs each, each under its own time limit, stopping at the first one that fails.

    python profiles/stream.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/stream.json
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
KERNELS = ('k_stream_push', 'k_stream_window', 'k_stream_emit')


def _model():
    import torch

    import nemo.quantization.utils.quantize_model as qm
    from nemo.collections.asr.models import EncDecCTCModel
    from qasr import synth
    torch.set_grad_enabled(False)
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En').cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    length = torch.tensor([500] * 4).cuda()
    for c in synth.make_calibration(2, 4, 64, 500):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=length)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    return m


def child_steps(a):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('stream.py measures on the GPU; no GPU found')
    m = _model()
    B = a.streams
    rng = np.random.default_rng(0)
    with m.stream(max_streams=B) as sess:
        plan = sess.plan
        fill = -(-plan.Wl // plan.C)                            # steps until the windows are full
        n_chunks = fill + a.warm + a.steps
        audio = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, n_chunks * plan.C)).astype(np.float32)).cuda()
        slots = [sess.open() for _ in range(B)]
        step_s, fwd_s, labels = [], [], 0
        s0 = None
        for k in range(n_chunks):
            chunk = audio[:, k * plan.C:(k + 1) * plan.C]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ups = sess.push(slots, chunk)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            labels += sum(len(u.labels) for u in ups)
            if k == fill + a.warm - 1:
                s0 = m._ragged_engine.ragged_stats()
            if k >= fill + a.warm:
                step_s.append(dt)
                win, wl = sess._win[0][:B].clone(), sess._win[1][:B].long()      # the identical window batch, bare
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tok, fs, enc = m._forward(win, wl, decode='frames')
                enc.cpu()                                                        # (a read-back, as the step has one)
                torch.cuda.synchronize()
                fwd_s.append(time.perf_counter() - t0)
        s1 = m._ragged_engine.ragged_stats()
        for s in slots:
            sess.close(s)
    med = lambda x: float(np.median(x))
    rec = dict(streams=B, chunk_samples=plan.C, window_samples=plan.Wl, window_frames=plan.Tw, emit_pitch=plan.emit_pitch,
               steps_measured=len(step_s), labels=labels, step_ms=[1e3 * x for x in step_s], forward_ms=[1e3 * x for x in fwd_s],
               step_median_ms=1e3 * med(step_s), forward_median_ms=1e3 * med(fwd_s),
               streaming_cost_ms=1e3 * (med(step_s) - med(fwd_s)),
               cost_over_a_tenth_of_forward=bool(med(step_s) - med(fwd_s) > 0.1 * med(fwd_s)),
               ragged_stats_delta={k: s1[k] - s0[k] for k in ('device_allocs', 'device_frees', 'graphs_captured', 'graph_replays', 'eager_runs')},
               note='the bare forwards between the steps count in the delta: one replay each')
    print('STREAM_CHILD ' + json.dumps(rec), flush=True)


def pick_kernels(path):
    """k_stream_* out of the kernel table of rocprofv3 --stats (nanoseconds, calls), and the rest as `forward`"""
    out = {k: dict(ns=0, calls=0) for k in KERNELS + ('everything_else',)}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name']
            k = next((k for k in KERNELS if k in name), 'everything_else')     # (with or without namespace and argument list)
            out[k]['ns'] += int(row['TotalDurationNs'])
            out[k]['calls'] += int(row['Calls'])
    missing = [k for k in KERNELS if not out[k]['calls']]
    if missing:
        sys.exit(f'{path}: no calls of {missing} in the kernel table - not a trace of `--child steps`, or the names are printed in a form this does not know')
    for v in out.values():
        v['us_per_call'] = v['ns'] / 1e3 / v['calls']
    return out


def _child(args, timeout, env=None):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        return None, f'ran past {timeout} s'
    line = [l for l in p.stdout.splitlines() if l.startswith('STREAM_CHILD ')]
    if p.returncode or not line:
        return None, f'rc {p.returncode}: {p.stderr[-800:]}'
    return json.loads(line[0][len('STREAM_CHILD '):]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['steps'], default=None)
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--stats-csv', default=None, help='kernel_stats.csv of a rocprofv3 run of `--child steps`')
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (bench.py A/B)')
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_steps(a)
    import numpy as np
    res = dict(note='QuartzNet15x5Base-En, synthetic weights and audio, EncDecCTCModel.stream at its defaults (0.96 / 4.0 / 0.96 s); '
                    'host wall milliseconds per step with the device synchronised before and after', steps={})
    for B in (1, 8, 32):
        rec, why = _child(['--child', 'steps', '--streams', str(B), '--steps', str(a.steps), '--warm', str(a.warm)], a.child_timeout)
        if rec is None:
            sys.exit(f'the child for {B} streams failed ({why}): stopping')
        print(json.dumps({k: v for k, v in rec.items() if not k.endswith('_ms') or 'median' in k or 'cost' in k}), flush=True)
        res['steps'][str(B)] = rec
    if a.stats_csv:
        res['kernels'] = dict(note='rocprofv3 --kernel-trace --stats of `--child steps --streams 32` in a run of its own', **pick_kernels(a.stats_csv))
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        bench = dict(note='`bench.py --gpus 1` in the same session, fresh processes alternating this build / the parent '
                          'commit\'s library (QASR_LIB)', this=[], parent=[])
        for k in range(a.bench_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib)):
                try:
                    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'], capture_output=True, text=True,
                                       timeout=a.bench_timeout, env=dict(os.environ, QASR_LIB=os.path.abspath(lib)))
                except subprocess.TimeoutExpired:
                    sys.exit(f'bench.py ({tag}) ran past {a.bench_timeout} s: stopping')
                line = [l for l in p.stdout.splitlines() if l.startswith('{')]
                if p.returncode or not line:
                    sys.exit(f'bench.py ({tag}) failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
                rec = json.loads(line[-1])
                bench[tag].append(dict(ms_per_step=rec['ms_per_step'], value=rec['value'], steps=rec['steps'], warmup=rec['warmup']))
                print(f'bench {tag} run {k}: ' + json.dumps(bench[tag][-1]), flush=True)
        bench['this_median_ms'] = float(np.median([b['ms_per_step'] for b in bench['this']]))
        bench['parent_median_ms'] = float(np.median([b['ms_per_step'] for b in bench['parent']]))
        bench['parent_slowest_ms'] = float(np.max([b['ms_per_step'] for b in bench['parent']]))
        bench['not_slower'] = bool(bench['this_median_ms'] <= bench['parent_slowest_ms'])
        res['bench'] = bench
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
