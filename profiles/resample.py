#!/usr/bin/env python3
"""The device resampler, measured on one GPU: 32 utterances x 5 s of int16 PCM at 8 / 22.05 / 44.1 / 48 kHz, both filter presets.

  kernels  k_resample per launch: device events around --steps launches on one stream, --rounds samples, median / min /
           max, the multiply-adds per launch and the rate they imply; float32 input at 44.1 kHz; and, in the same run, the
           front-end's k_mel + k_norm on the 32 x 5 s of 16 kHz audio that comes out (qasr_frontend_mel_planned) for scale.
           Every timed configuration is compared with the NumPy twin first (equals_twin).  The per-kernel table of rocprofv3
           comes from a run of its own:
             rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o resample -- python profiles/resample.py --child
  twin     qasr.resample.resample_host on one of the 32 utterances, host seconds per 5 s utterance: context, not a bar
  bench    `bench.py --gpus 1` on this build and on a build of the parent commit (QASR_LIB), fresh processes alternating this /
           parent, --bench-runs each, each under its own time limit, stopping at the first one that fails.  No existing
           kernel's text changed, so the two should read alike.

    python profiles/resample.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/resample.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
RATES = (8000, 22050, 44100, 48000)


def child(a):
    import numpy as np
    import torch

    from nemo.collections.asr.models import EncDecCTCModel
    from qasr import engine, resample
    if not torch.cuda.is_available():
        sys.exit('resample.py measures on the GPU; no GPU found')

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

    B = a.batch
    rng = np.random.default_rng(0)
    rows = []
    for sr in RATES:
        S = int(a.seconds * sr)
        x = rng.integers(-20000, 20001, (B, S), dtype=np.int16)
        lens = np.full(B, S, dtype=np.int32)
        xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
        for quality in ('best', 'fast'):
            for dtype in ('int16', 'float32') if sr == 44100 else ('int16',):
                p = resample.ResamplePlan(sr, 16000, quality)
                xin = xd if dtype == 'int16' else (xd.float() / 32768)
                out, out_lens = engine.resample(xin, ld, p)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                want, want_lens = resample.resample_host(xin[:1].cpu().numpy(), lens[:1], p)
                twin_s = time.perf_counter() - t0
                equal = bool(out[:1].cpu().numpy().tobytes() == want.tobytes() and int(out_lens[0]) == int(want_lens[0]))
                us = timed(lambda: engine.resample(xin, ld, p, out=out, out_lens=out_lens))
                macs = B * p.out_len(S) * 2 * p.W
                rows.append(dict(rate=sr, quality=quality, dtype=dtype, L=p.L, M=p.M, W=p.W, table_entries=p.L * 2 * p.W,
                                 out_samples=p.out_len(S), macs_per_launch=macs, k_resample_us=us,
                                 gmacs_per_s=macs / (float(np.median(us)) * 1e-6) / 1e9, twin_host_s_per_utterance=twin_s,
                                 equals_twin=equal))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    # the front-end on the same amount of 16 kHz audio
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En')
    f = m.preprocessor.featurizer
    fb, window = f.fb[0].detach().float().contiguous().cuda(), f.window.detach().float().contiguous().cuda()
    plan = engine.frontend_plan(fb)
    S16 = int(a.seconds * 16000)
    audio = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, S16)).astype(np.float32)).cuda()
    alen = torch.full((B,), S16, dtype=torch.int32).cuda()
    fe = engine.frontend_mel(audio, alen, fb, window, 0.97, 16, plan=plan)
    fe_out = (fe[0], fe[1], None)
    mel_us = timed(lambda: engine.frontend_mel(audio, alen, fb, window, 0.97, 16, out=fe_out, plan=plan))
    print('RESAMPLE_CHILD ' + json.dumps(dict(rows=rows, frontend_mel_us=mel_us)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=5.0)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
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

    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--batch', str(a.batch), '--seconds', str(a.seconds), '--steps',
           str(a.steps), '--rounds', str(a.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f'the kernel child ran past {a.child_timeout} s: stopping')
    line = [l for l in p.stdout.splitlines() if l.startswith('RESAMPLE_CHILD ')]
    if p.returncode or not line:
        sys.exit(f'the kernel child failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
    r = json.loads(line[0][len('RESAMPLE_CHILD '):])
    kernels = []
    for row in r['rows']:
        row = dict(row, k_resample_us=stat(row['k_resample_us']))
        kernels.append(row)
        print(json.dumps(row), flush=True)
    mel = stat(r['frontend_mel_us'])
    print('frontend_mel_us', json.dumps(mel), flush=True)
    bench = {}
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        bench = dict(note='`bench.py --gpus 1` in the same session, fresh processes alternating this build / the parent '
                          'commit\'s library (QASR_LIB)', this=[], parent=[])
        for k in range(a.bench_runs):
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
                print(f'bench {tag} run {k}: ' + json.dumps(bench[tag][-1]), flush=True)
        bench['this_median_ms'] = float(np.median([b['ms_per_step'] for b in bench['this']]))
        bench['parent_slowest_ms'] = float(np.max([b['ms_per_step'] for b in bench['parent']]))
        bench['not_slower'] = bool(bench['this_median_ms'] <= bench['parent_slowest_ms'])
    res = dict(shape=dict(batch=a.batch, seconds=a.seconds), steps=a.steps, rounds=a.rounds,
               note='kernel times: device events around `steps` launches on one stream (microseconds per launch); int16 noise of '
                    'amplitude 20000, full-length rows; frontend_mel_us: k_mel + k_norm on the same batch at 16 kHz',
               kernels=kernels, frontend_mel_us=mel, bench=bench)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
