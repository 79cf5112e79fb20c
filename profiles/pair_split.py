#!/usr/bin/env python3
"""Headline runs of several checkouts / launch plans in ONE session, interleaved (A B A B ...), each a fresh process with a
time limit of its own:
    python profiles/pair_split.py out.json [--rounds 3] [--steps 50] [--dump DIR] RUN [RUN ...]
    RUN = label,tree,queues[,NAME=VALUE ...]
      tree    directory of a built checkout whose bench.py is run (`.` = this one; a checkout of the parent commit for the A side)
      queues  `inherit` leaves GPU_MAX_HW_QUEUES as this process found it; a number exports that value
      NAME=VALUE  further environment of the run (QASR_PAIR_SPLIT=0 ...)
Appends one record per run to out.json: ms/step, RTFx, the environment and bench.py's `streams finished at` line (which says
how many launch chains overlapped, i.e. which regime was measured).  With --dump every run also writes its outputs to
DIR/<label>_r<round>, and the files of the runs of one round are compared byte by byte.  Stops at the first run that fails."""
import argparse
import filecmp
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_files(a, b):
    na, nb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return na == nb and all(filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False) for n in na)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('runs', nargs='+')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dump', metavar='DIR')
    ap.add_argument('--note', default='')
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {'runs': []}
    inherited = os.environ.get('GPU_MAX_HW_QUEUES')
    for r in range(a.rounds):
        dumps = []
        for spec in a.runs:
            label, tree, queues, *kv = spec.split(',')
            tree = os.path.abspath(os.path.join(ROOT, tree))
            env = dict(os.environ)
            env.pop('QASR_LIB', None)
            if queues != 'inherit':
                env['GPU_MAX_HW_QUEUES'] = queues
            over = dict(x.split('=', 1) for x in kv)
            env.update(over)
            cmd = [sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(a.steps), '--warmup', str(a.warmup)]
            if a.dump:
                dumps.append((label, os.path.abspath(os.path.join(a.dump, f'{label}_r{r}'))))
                cmd += ['--dump-outputs', dumps[-1][1]]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree, timeout=240)
            except subprocess.TimeoutExpired:
                print(f'{label}: no result within 240 s', flush=True)
                return 1
            if p.returncode:
                print(f'{label}: FAILED rc={p.returncode}\n{p.stderr[-2000:]}', flush=True)
                return 1
            d = json.loads(p.stdout.strip().splitlines()[-1])
            streams = [l.split('] ', 1)[1] for l in p.stderr.splitlines() if 'streams finished at' in l]
            rec = dict(label=label, round=r, ms_per_step=d['ms_per_step'], rtfx=d['value'], steps=a.steps, warmup=a.warmup,
                       GPU_MAX_HW_QUEUES=env.get('GPU_MAX_HW_QUEUES', 'unset (bench.py sets 8)'), queues_inherited=inherited,
                       overrides=over, streams=streams[0] if streams else None, note=a.note)
            doc['runs'].append(rec)
            print(f"{label:20s} round {r}  queues {rec['GPU_MAX_HW_QUEUES']:>3s}  {d['ms_per_step']:.4f} ms/step  {rec['streams']}", flush=True)
            with open(a.out, 'w') as fh:
                json.dump(doc, fh, indent=1)
        for label, d in dumps[1:]:
            same = same_files(dumps[0][1], d)
            doc.setdefault('outputs_identical', []).append(dict(round=r, a=dumps[0][0], b=label, identical=same, note=a.note))
            print(f'outputs of {dumps[0][0]} and {label}, round {r}: {"byte-identical" if same else "DIFFERENT"}', flush=True)
            with open(a.out, 'w') as fh:
                json.dump(doc, fh, indent=1)
            if not same:
                return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
