#!/usr/bin/env python3
"""What streaming at another sample rate costs, measured on one GPU.

  kernels  32 streams, one chunk of 0.96 s (the default plan): k_stream_rs_append and k_stream_rs_fir per push, for 8 / 44.1 /
           48 kHz x best / fast, int16 mono; in the same process the two references: k_resample producing the same number of
           outputs per row (15 360) from the same audio, and k_stream_push of one chunk at the model's rate.  Device times need
           a rocprofv3 run of its own, one per (rate, preset):
             rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o rs_<rate>_<preset> -- \\
                 python profiles/stream_rs.py --child kernels --rate <rate> --quality <preset>
           then --stats-dir <dir> picks the four kernels out of every *kernel_stats.csv found there.
           EXPECTATION, written down before any number: the FIR launch costs about what k_resample costs for the same outputs
           (same tap loop, same staging; the history is read instead of the PCM), the append about what k_stream_push costs.
  steps    host wall time per session step (device synchronised before and after every push of one chunk per stream), at
           1 / 8 / 32 streams, for a session with input_rate=8000 against the same session at the model's rate fed the same
           seconds of audio; full QuartzNet15x5Base-En, synthetic weights, calibrated.
  bench    `bench.py --gpus 1` on this build and on a build of the parent commit (QASR_LIB), fresh processes alternating this /
           parent, --bench-runs each, medians.  No existing kernel's text changed, so the headline should not move.

No threshold is fixed: nobody has measured any of this yet.

    python profiles/stream_rs.py --stats-dir <dir> --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/stream_rs.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT, os.path.join(ROOT, 'profiles')]
KERNELS = ('k_stream_rs_append', 'k_stream_rs_fir', 'k_resample', 'k_stream_push')
RATES, QUALITIES = (8000, 44100, 48000), ('best', 'fast')


def child_kernels(a):
    """`reps` pushes of one chunk for 32 streams (append + fir), `reps` k_resample launches for the same outputs, `reps`
    k_stream_push launches of one chunk at the model's rate"""
    import numpy as np
    import torch
    from qasr import engine, resample as rs, stream as st, stream_rs as srs
    if not torch.cuda.is_available():
        sys.exit('stream_rs.py measures on the GPU; no GPU found')
    S = a.streams
    sp = st.StreamPlan()
    p = srs.StreamResamplePlan(sp, rs.ResamplePlan(a.rate, sp.sample_rate, a.quality), 1)
    rng = np.random.default_rng(0)
    pcm = torch.from_numpy(rng.integers(-20000, 20000, size=(S, p.Ain), dtype=np.int16)).cuda()
    f32 = torch.from_numpy(rng.uniform(-0.5, 0.5, (S, sp.C)).astype(np.float32)).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    slots, zero = i32(list(range(S))), i32([0] * S)
    n_in, limit, n_new = i32([p.Ain] * S), i32([sp.C] * S), i32([sp.C] * S)
    state, rs_state, work = engine.stream_state(S, sp, 'cuda'), engine.stream_rs_state(S, p, 'cuda'), engine.stream_rs_work(S, 'cuda')
    out = tuple(torch.empty(S, dtype=torch.int32, device='cuda') for _ in range(3))
    lens = i32([p.Ain] * S)
    y, yl = torch.empty(S, sp.C, device='cuda'), torch.empty(S, dtype=torch.int32, device='cuda')
    engine.resample_plan(p.resample_plan, 'cuda')
    produced = []
    for k in range(a.reps + 1):                                  # (the first push produces W L / M outputs fewer: not counted)
        engine.stream_rs_push(state, rs_state, S, p, slots, i32([st.BEGIN if k == 0 else 0] * S), n_in, limit, pcm, work=work, out=out)
        produced.append(int(out[1][0]))
    for k in range(a.reps):
        engine.resample(pcm, lens, p.resample_plan, out=y, out_lens=yl)
    state2 = engine.stream_state(S, sp, 'cuda')
    for k in range(a.reps):
        engine.stream_push(state2, S, sp, slots, zero, n_new, f32)
    torch.cuda.synchronize()
    print('STREAM_RS_CHILD ' + json.dumps(dict(rate=a.rate, quality=a.quality, streams=S, L=p.L, M=p.M, W=p.W, Ain=p.Ain, hcap=p.hcap,
                                               outputs_per_push=produced, resample_outputs=int(yl[0]), reps=a.reps)), flush=True)


def child_steps(a):
    import numpy as np
    import torch
    import stream as plain                                       # profiles/stream.py: the same model
    if not torch.cuda.is_available():
        sys.exit('stream_rs.py measures on the GPU; no GPU found')
    m = plain._model()
    B, rate = a.streams, a.rate
    rng = np.random.default_rng(0)
    kw = dict(input_rate=rate) if rate != 16000 else {}
    with m.stream(max_streams=B, **kw) as sess:
        plan = sess.plan
        piece = plan.C if sess.rs_plan is None else sess.rs_plan.Ain
        fill = -(-plan.Wl // plan.C)
        n_chunks = fill + a.warm + a.steps
        if sess.rs_plan is None:
            audio = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, n_chunks * piece)).astype(np.float32)).cuda()
        else:
            audio = torch.from_numpy(rng.integers(-16000, 16000, size=(B, n_chunks * piece), dtype=np.int16)).cuda()
        slots = [sess.open() for _ in range(B)]
        step_s, labels, s0 = [], 0, None
        for k in range(n_chunks):
            chunk = audio[:, k * piece:(k + 1) * piece]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ups = sess.push(slots, chunk)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            labels += sum(len(u.labels) for u in ups)
            if k == fill + a.warm - 1:
                s0 = m._ragged_engine.ragged_stats()
            if k >= fill + a.warm and ups:
                step_s.append(dt)
        s1 = m._ragged_engine.ragged_stats()
        for s in slots:
            sess.close(s)
    rec = dict(streams=B, input_rate=rate, piece_frames=piece, steps_measured=len(step_s), labels=labels,
               step_ms=[1e3 * x for x in step_s], step_median_ms=1e3 * float(np.median(step_s)),
               ragged_stats_delta={k: s1[k] - s0[k] for k in ('device_allocs', 'device_frees', 'graphs_captured', 'graph_replays', 'eager_runs')})
    print('STREAM_RS_CHILD ' + json.dumps(rec), flush=True)


def pick_kernels(path):
    """the four kernels out of one kernel table of rocprofv3 --stats (nanoseconds, calls); k_resample_copy is not k_resample"""
    out = {k: dict(ns=0, calls=0) for k in KERNELS}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name']
            if 'k_resample_copy' in name:
                continue
            k = next((k for k in KERNELS if k in name), None)
            if k is not None:
                out[k]['ns'] += int(row['TotalDurationNs'])
                out[k]['calls'] += int(row['Calls'])
    missing = [k for k in KERNELS if not out[k]['calls']]
    if missing:
        sys.exit(f'{path}: no calls of {missing} in the kernel table - not a trace of `--child kernels`')
    for v in out.values():
        v['us_per_call'] = v['ns'] / 1e3 / v['calls']
    out['fir_over_k_resample'] = out['k_stream_rs_fir']['us_per_call'] / out['k_resample']['us_per_call']
    out['append_over_k_stream_push'] = out['k_stream_rs_append']['us_per_call'] / out['k_stream_push']['us_per_call']
    return out


def _child(args, timeout, env=None):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        return None, f'ran past {timeout} s'
    line = [l for l in p.stdout.splitlines() if l.startswith('STREAM_RS_CHILD ')]
    if p.returncode or not line:
        return None, f'rc {p.returncode}: {p.stderr[-800:]}'
    return json.loads(line[0][len('STREAM_RS_CHILD '):]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['kernels', 'steps'], default=None)
    ap.add_argument('--rate', type=int, default=8000)
    ap.add_argument('--quality', choices=QUALITIES, default='best')
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--skip-steps', action='store_true')
    ap.add_argument('--stats-dir', default=None, help='directory with the *kernel_stats.csv of the rocprofv3 runs of `--child kernels`')
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (bench.py A/B)')
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child == 'kernels':
        return child_kernels(a)
    if a.child == 'steps':
        return child_steps(a)
    import numpy as np
    res = dict(note='32 streams x one chunk of 0.96 s per launch; QuartzNet15x5Base-En (synthetic weights and audio) for the steps',
               expectation='k_stream_rs_fir costs about what k_resample costs for the same outputs; bench.py does not move')
    if not a.skip_steps:
        res['steps'] = {}
        for B in (1, 8, 32):
            for rate in (16000, 8000):
                rec, why = _child(['--child', 'steps', '--streams', str(B), '--rate', str(rate), '--steps', str(a.steps), '--warm', str(a.warm)],
                                  a.child_timeout)
                if rec is None:
                    sys.exit(f'the child for {B} streams at {rate} Hz failed ({why}): stopping')
                print(json.dumps({k: v for k, v in rec.items() if k != 'step_ms'}), flush=True)
                res['steps'][f'{B}@{rate}'] = rec
            res['steps'][f'{B}_added_ms'] = res['steps'][f'{B}@8000']['step_median_ms'] - res['steps'][f'{B}@16000']['step_median_ms']
    if a.stats_dir:
        res['kernels'] = dict(note='rocprofv3 --kernel-trace --stats of `--child kernels`, one run per (rate, preset)')
        for path in sorted(glob.glob(os.path.join(a.stats_dir, '**', '*kernel_stats.csv'), recursive=True)):
            res['kernels'][os.path.basename(path).replace('_kernel_stats.csv', '')] = pick_kernels(path)
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        bench = dict(note='`bench.py --gpus 1`, fresh processes alternating this build / the parent commit\'s library (QASR_LIB)', this=[], parent=[])
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
        res['bench'] = bench
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
