#!/usr/bin/env python3
"""Headline runs of several builds / launch plans in ONE session, interleaved (A B C A B C ...), each a fresh process:
    python profiles/launch_plan.py out.json [--rounds 3] [--steps 50] [--extra "--gather logits"] RUN [RUN ...]
    RUN = label,lib,queues[,NAME=VALUE ...]
      lib     name of a build: q-asr_amd/qasr/libqasr_<lib>.so (QASR_BUILD_TAG=<lib> builds one; `hip` is the tree's own)
      queues  `inherit` leaves GPU_MAX_HW_QUEUES as this process found it (bench.py then only fills in its own default when the
              variable is unset); a number exports that value
      NAME=VALUE  further environment of the run (the engine's A/B overrides: QASR_RES_TILE=32 ...)
Appends one record per run to out.json: ms/step, RTFx, the environment, the build, and bench.py's `streams finished at` line
(how many launch chains overlapped).  Stops at the first run that fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('runs', nargs='+')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--extra', default='')
    ap.add_argument('--dump', metavar='DIR', help='also --dump-outputs DIR/<label>_r<round> (build-to-build comparison of the outputs)')
    ap.add_argument('--note', default='')
    a = ap.parse_args()
    records = json.load(open(a.out))['runs'] if os.path.exists(a.out) else []
    inherited = os.environ.get('GPU_MAX_HW_QUEUES')
    for r in range(a.rounds):
        for spec in a.runs:
            label, lib, queues, *kv = spec.split(',')
            env = dict(os.environ, QASR_LIB=os.path.join(ROOT, 'q-asr_amd', 'qasr', f'libqasr_{lib}.so'))
            if queues != 'inherit':
                env['GPU_MAX_HW_QUEUES'] = queues
            over = dict(x.split('=', 1) for x in kv)
            env.update(over)
            cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(a.steps), '--warmup', str(a.warmup)] + a.extra.split()
            if a.dump:
                cmd += ['--dump-outputs', os.path.join(a.dump, f'{label}_r{r}')]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=240)
            if p.returncode:
                print(f'{label}: FAILED rc={p.returncode}\n{p.stderr[-2000:]}', flush=True)
                return 1
            d = json.loads(p.stdout.strip().splitlines()[-1])
            streams = [l.split('] ', 1)[1] for l in p.stderr.splitlines() if 'streams finished at' in l]
            rec = dict(label=label, build=lib, round=r, ms_per_step=d['ms_per_step'], rtfx=d['value'], steps=a.steps, warmup=a.warmup,
                       bench_args=a.extra, GPU_MAX_HW_QUEUES=env.get('GPU_MAX_HW_QUEUES', 'unset (bench.py sets 8)'),
                       queues_inherited=inherited, overrides=over, streams=streams[0] if streams else None, note=a.note)
            records.append(rec)
            print(f"{label:28s} round {r}  queues {rec['GPU_MAX_HW_QUEUES']:>3s}  {d['ms_per_step']:.4f} ms/step  {rec['streams']}", flush=True)
            with open(a.out, 'w') as fh:
                json.dump({'runs': records}, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
