#!/usr/bin/env python3
"""Protocol of the halved ops: the parent commit's library (through QASR_LIB) against this build, one session,
every run a fresh process with a time limit of its own, the chain ends at the first failure.
    python profiles/half_tiles.py OUT.json --parent-lib LIB --work DIR STAGE [STAGE ...]
Stages (each appends to OUT.json; run them in any split over several calls):
  stats      rocprofv3 --kernel-trace --stats of the default `bench.py --gpus 1`, two runs per build, each on its own; the first
             table of each build is copied to DIR/half_tiles_kernel_stats_{parent,this}.csv
  pair0      one such run of this build with QASR_PAIR_SPLIT=0 QASR_HALF_TILES=1: the plain 512 layers as 64-frame launches
  headline   `bench.py --gpus 1 --steps 50 --warmup 5`, ten rounds (--rounds), alternating which build goes first, with
             --dump-outputs compared byte by byte in every round
  logits     one round with --gather logits, outputs compared
  full       `bench.py --full --no-cpu-baseline --no-other-configs` of this build (its in-flight-equals-serial check)
  q8         three rounds with GPU_MAX_HW_QUEUES=8, and the plan of a 128-frame engine there (no op halved)
  decide     the rule's terms from what OUT.json holds
GPU_MAX_HW_QUEUES is left as found everywhere but in q8."""
import argparse
import csv
import filecmp
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
# label of the op in the plan -> the kernel that serves it in a halved plan
CLASSES = {'k_sep2<33, 2, 0, 1, false, 128, 1>': 'k_sep2<33, 2, 0, 1, false, 64, 1>',
           'k_sep2<39, 2, 0, 1, false, 128, 1>': 'k_sep2<39, 2, 0, 1, false, 64, 1>',
           'k_sep2<51, 2, 0, 2, false, 128, 1>': 'k_sep2<51, 2, 0, 2, false, 64, 1>',
           'k_sep2<87, 4, 0, 2, false, 128, 2>': 'k_sep2<87, 4, 0, 2, false, 64, 2>'}
PER_FORWARD = {'k_sep2<33, 2, 0, 1, false, 128, 1>': 12, 'k_sep2<39, 2, 0, 1, false, 128, 1>': 12,
               'k_sep2<51, 2, 0, 2, false, 128, 1>': 1, 'k_sep2<87, 4, 0, 2, false, 128, 2>': 1}
PAIRS = {f'k_sep2p<{k}>': f'k_sep2<{k}, 4, 0, 2, false, 64, 1>' for k in (51, 63, 75)}


class Failed(Exception):
    pass


def save(doc, path):
    with open(path, 'w') as fh:
        json.dump(doc, fh, indent=1)


def run(cmd, env, limit, what):
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=limit)
    except subprocess.TimeoutExpired:
        raise Failed(f'{what}: no result within {limit} s')
    if p.returncode:
        raise Failed(f'{what}: rc={p.returncode}\n{p.stderr[-3000:]}')
    return p


def build_env(build, a, over=None):
    env = dict(os.environ)
    for name in ('QASR_LIB', 'QASR_HALF_TILES', 'QASR_PAIR_SPLIT'):
        env.pop(name, None)
    if build == 'parent':
        env['QASR_LIB'] = os.path.abspath(a.parent_lib)
    env.update(over or {})
    return env


def kernel_table(path):
    """rocprofv3's kernel table: kernel name (without `void qasr::` and the argument list) -> calls, average / min / max us"""
    out = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name'].replace('void qasr::', '').split('(')[0]
            out[name] = dict(calls=int(row['Calls']), us=float(row['AverageNs']) / 1e3, min_us=int(row['MinNs']) / 1e3,
                             max_us=int(row['MaxNs']) / 1e3)
    return out


def stats_run(a, build, tag, over=None, keep_as=None):
    d = os.path.join(a.work, f'prof_{tag}')
    shutil.rmtree(d, ignore_errors=True)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'p', '--', sys.executable, BENCH, '--gpus', '1']
    p = run(cmd, build_env(build, a, over), 300, f'rocprofv3 {tag}')
    found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if len(found) != 1:
        raise Failed(f'rocprofv3 {tag}: kernel tables found: {found}')
    t = kernel_table(found[0])
    if keep_as:
        shutil.copy(found[0], os.path.join(a.work, keep_as))
    shutil.rmtree(d, ignore_errors=True)                        # the trace itself is large and not kept
    ms =json.loads(p.stdout.strip().splitlines()[-1])['ms_per_step']
    keep = {k: v for k, v in t.items() if k.startswith('k_sep2')}
    print(f'{tag}: {len(t)} kernels, {ms:.4f} ms/step under the profiler', flush=True)
    for k in sorted(keep):
        print(f'   {k:44s} {keep[k]["calls"]:6d} x {keep[k]["us"]:7.3f} us', flush=True)
    return dict(build=build, tag=tag, overrides=over or {}, ms_per_step_under_profiler=ms, k_sep2=keep)


def stage_stats(a, doc):
    for build in ('parent', 'this'):
        for r in range(2):
            rec = stats_run(a, build, f'{build}_{r}', keep_as=f'half_tiles_kernel_stats_{build}.csv' if r == 0 else None)
            doc.setdefault('kernel_stats', []).append(rec)
            save(doc, a.out)


def stage_pair0(a, doc):
    rec = stats_run(a, 'this', 'this_pair0', {'QASR_PAIR_SPLIT': '0', 'QASR_HALF_TILES': '1'})
    doc['kernel_stats_pair_split_0'] = rec
    save(doc, a.out)


def same_files(x, y):
    nx, ny = sorted(os.listdir(x)), sorted(os.listdir(y))
    return bool(nx) and nx == ny and all(filecmp.cmp(os.path.join(x, n), os.path.join(y, n), shallow=False) for n in nx)


def bench_round(a, doc, key, r, order, over=None, extra=()):
    dumps = {}
    for build in order:
        dumps[build] = os.path.join(a.work, f'dump_{key}_{build}_r{r}')
        shutil.rmtree(dumps[build], ignore_errors=True)
        env = build_env(build, a, over)
        cmd = [sys.executable, BENCH, '--gpus', '1', '--steps', '50', '--warmup', '5', '--dump-outputs', dumps[build], *extra]
        p = run(cmd, env, 240, f'{key} {build} round {r}')
        d = json.loads(p.stdout.strip().splitlines()[-1])
        streams = [l.split('] ', 1)[-1] for l in p.stderr.splitlines() if 'streams finished at' in l]
        rec = dict(build=build, round=r, first=order[0], ms_per_step=d['ms_per_step'], rtfx=d['value'],
                   GPU_MAX_HW_QUEUES=env.get('GPU_MAX_HW_QUEUES', 'unset (bench.py sets 8)'), overrides=over or {}, extra=list(extra),
                   streams=streams)
        doc.setdefault(key, []).append(rec)
        print(f'{key:9s} {build:6s} round {r}  {d["ms_per_step"]:.4f} ms/step  {streams[-1] if streams else ""}', flush=True)
        save(doc, a.out)
    same = same_files(dumps['parent'], dumps['this'])
    doc.setdefault('outputs_identical', []).append(dict(stage=key, round=r, identical=same))
    save(doc, a.out)
    for d in dumps.values():
        shutil.rmtree(d, ignore_errors=True)
    if not same:
        raise Failed(f'{key} round {r}: outputs DIFFER')
    print(f'{key:9s} round {r}: outputs byte-identical', flush=True)


def stage_headline(a, doc):
    for r in range(a.rounds):
        bench_round(a, doc, 'headline', r, ('parent', 'this') if r % 2 == 0 else ('this', 'parent'))


def stage_logits(a, doc):
    bench_round(a, doc, 'logits', 0, ('parent', 'this'), extra=('--gather', 'logits'))


def stage_full(a, doc):
    p = run([sys.executable, BENCH, '--full', '--no-cpu-baseline', '--no-other-configs'], build_env('this', a), 420, 'bench.py --full')
    doc['full'] = dict(rc=0, result=json.loads(p.stdout.strip().splitlines()[-1]),
                       checks=[l.split('] ', 1)[-1] for l in p.stderr.splitlines() if 'serial' in l or 'in flight' in l])
    save(doc, a.out)
    print('bench.py --full: passed', flush=True)


PLAN_CHILD = """
import json, os, sys
sys.path[:0] = [os.path.join(%r, 'q-asr_amd'), %r]
import numpy as np, torch
from qasr import engine, pack, synth, topology
d = np.load(os.path.join(%r, 'tests', 'golden', 'net_quartznet_w8a8.npz'))
cfg = topology.quartznet15x5()
blob, _ = pack.pack_model(cfg, synth.make_state_dict(cfg, json.loads(str(d['meta']))['seed']), d['act_min'], d['act_max'], 8, 8)
e = engine.Engine(blob, 0, tile=128)
e.forward(torch.from_numpy(synth.make_features(3, cfg.feat_in, 500, 1)).cuda(), torch.tensor([500, 258, 2], dtype=torch.int32).cuda())
torch.cuda.synchronize()
print(json.dumps(dict(halved=sum(e.op_halved()), paired=sum(e.op_paired()), launches=e.num_launches())))
e.close()
""" % (ROOT, ROOT, ROOT)


def stage_q8(a, doc):
    over = {'GPU_MAX_HW_QUEUES': '8'}
    p = run([sys.executable, '-c', PLAN_CHILD], build_env('this', a, over), 120, 'plan with 8 queues')
    doc['plan_8_queues'] = json.loads(p.stdout.strip().splitlines()[-1])
    save(doc, a.out)
    print('plan with 8 queues:', doc['plan_8_queues'], flush=True)
    if doc['plan_8_queues']['halved']:
        raise Failed('ops halved with 8 queues')
    for r in range(3):
        bench_round(a, doc, 'queues8', r, ('parent', 'this') if r % 2 == 0 else ('this', 'parent'), over)


def spread(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v), n=len(v))


def stage_decide(a, doc):
    out = {}
    ks = doc.get('kernel_stats', [])
    par = [r['k_sep2'] for r in ks if r['build'] == 'parent']
    this = [r['k_sep2'] for r in ks if r['build'] == 'this']
    if len(par) == 2 and len(this) == 2:
        per = {}
        for label, kernel in CLASSES.items():
            p = [t[label]['us'] for t in par]
            h = [t[kernel]['us'] for t in this]
            noise = abs(p[0] - p[1])
            per[label] = dict(parent_us=p, this_us=h, parent_run_to_run_us=noise, per_forward=PER_FORWARD[label],
                              stays=all(min(p) - x > noise for x in h), saved_us_per_forward=(min(p) - max(h)) * PER_FORWARD[label])
        out['per_launch'] = per
        out['per_launch_saved_us_per_forward'] = sum(v['saved_us_per_forward'] for v in per.values())
    if 'kernel_stats_pair_split_0' in doc and this:
        t0 = doc['kernel_stats_pair_split_0']['k_sep2']
        out['pair_against_plain_64'] = {p: dict(k_sep2p_us=[t[p]['us'] for t in this], plain_64_us=t0[k]['us']) for p, k in PAIRS.items()}
    for key in ('headline', 'queues8'):
        runs = doc.get(key, [])
        if runs:
            out[key] = {b: spread([r['ms_per_step'] for r in runs if r['build'] == b]) for b in ('parent', 'this')}
    if 'headline' in out:
        p, t = out['headline']['parent'], out['headline']['this']
        out['default_stays_on'] = t['median'] < p['median']
        out['speedup_claimed'] = t['max'] < p['min']
        out['median_change_percent'] = 100.0 * (t['median'] / p['median'] - 1.0)
    if 'queues8' in out:
        p, t = out['queues8']['parent'], out['queues8']['this']
        out['queues8_inside_parent_range'] = p['min'] <= t['median'] <= p['max']
    out['outputs_identical_every_round'] = all(r['identical'] for r in doc.get('outputs_identical', [])) and bool(doc.get('outputs_identical'))
    doc['decision'] = out
    save(doc, a.out)
    print(json.dumps(out, indent=1), flush=True)


STAGES = dict(stats=stage_stats, pair0=stage_pair0, headline=stage_headline, logits=stage_logits, full=stage_full, q8=stage_q8,
              decide=stage_decide)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('stages', nargs='+', choices=list(STAGES))
    ap.add_argument('--parent-lib', required=True, help="the parent commit's libqasr_hip.so")
    ap.add_argument('--work', required=True, help='directory for traces, dumps and the two kernel tables')
    ap.add_argument('--rounds', type=int, default=10)
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.setdefault('queues_as_found', os.environ.get('GPU_MAX_HW_QUEUES'))
    try:
        for s in a.stages:
            STAGES[s](a, doc)
    except Failed as f:
        print(f'FAILED: {f}', flush=True)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
