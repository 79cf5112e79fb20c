#!/usr/bin/env python3
"""Keyword spotting (k_spot), measured on one GPU.

  spot     k_spot at 32 x 500 frames with K = 10 / 100 / 1000 keywords of 8 labels, for En (29 classes) and Zh (5207), and one
           stitched hour (1 x 180 000 frames, 100 keywords): device events around --steps launches on one stream, --rounds
           rounds.  In every round, after k_spot and on the same inputs: k_star (the plane k_spot reads), and - for the 32 x 500
           shapes - k_align<1> with want_total=False on the same P = 32 K problems (the keywords replicated per utterance).
           k_align is what one would launch today and does a different job (pinned ends, backpointers, a back-walk): context,
           not a gate.  Medians over the rounds; ns per problem and frame = time / (P T).
  bench    `bench.py --gpus 1`, fresh processes alternating this build / a build of the parent commit (QASR_LIB), --ab-runs
           each, the order inside a pair alternating as well.  Each process runs under its own time limit, and the script
           stops at the first one that fails.

    python profiles/ctc_spot.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_spot.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
SHAPES = (('en', 29), ('zh', 5207))
KEYWORDS = (10, 100, 1000)
LABELS = 8
HOUR = (1, 180000, 100)
TAG = 'CTC_SPOT_CHILD '
SPOT = dict(threshold=-1.0, max_span=500, max_hits=16)


def _round(torch, fn, steps):
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    t.record()
    t.synchronize()
    return s.elapsed_time(t) / steps * 1e3


def _logp(torch, B, T, C_, seed):
    """peaky synthetic posteriors: the frame's own class raised by 4 over unit Gaussian noise; (logp [B, T, C], classes [T])"""
    g = torch.Generator().manual_seed(seed)
    own = torch.randint(0, C_ - 1, (T,), generator=g)
    z = torch.randn(T, C_, generator=g).cuda()
    z[torch.arange(T).cuda(), own.cuda()] += 4.0
    return torch.log_softmax(z, dim=-1)[None].expand(B, T, C_).contiguous(), own


def _keywords(torch, own, K, seed):
    """K keywords of LABELS labels: runs of the frames' own classes from random offsets (so some occur), repeats allowed"""
    g = torch.Generator().manual_seed(seed)
    at = torch.randint(0, len(own) - LABELS, (K,), generator=g)
    tg = torch.stack([own[a:a + LABELS] for a in at.tolist()]).to(torch.int32)
    return tg.cuda(), torch.full((K,), LABELS, dtype=torch.int32).cuda()


def child_spot(a):
    import torch

    from qasr import engine
    if not torch.cuda.is_available():
        sys.exit('ctc_spot.py measures on the GPU; no GPU found')
    out = {}
    for name, C_ in SHAPES:
        for B, T, Ks in ((32, 500, KEYWORDS), HOUR[:2] + ((HOUR[2],),)):
            logp, own = _logp(torch, B, T, C_, 1)
            plane = torch.empty(B, T, device='cuda')
            engine.ctc_star(logp, None, 0.0, out=plane)
            for K in Ks:
                tg, tl = _keywords(torch, own, K, K)
                buf = {}

                def run_spot():
                    buf['s'] = engine.ctc_spot(logp, None, plane, tg, tl, C_ - 1, out=buf.get('s'), **SPOT)
                fns = dict(k_spot_us=run_spot, k_star_us=lambda: engine.ctc_star(logp, None, 0.0, out=plane))
                steps = a.steps if T <= 65536 else 1
                if T <= 65536:                                      # (k_align holds at most MAX_T frames)
                    P = B * K
                    tga, tla = tg.repeat(B, 1), tl.repeat(B)
                    ws = torch.empty(engine.ctc_align_workspace_bytes(P, T, LABELS), dtype=torch.uint8, device='cuda')

                    def run_align():
                        buf['a'] = engine.ctc_align(logp, None, tga, tla, C_ - 1, problems_per_utt=K, want_total=False, workspace=ws,
                                                    out=buf.get('a'))
                    fns['k_align1_us'] = run_align
                for fn in fns.values():                             # warm every shape the timed window uses
                    fn()
                torch.cuda.synchronize()
                rec = {k: [] for k in fns}
                for _ in range(a.rounds):                           # alternating: one sample of each per round
                    for k, fn in fns.items():
                        rec[k].append(_round(torch, fn, steps))
                rec.update(P=B * K, T=T, C=C_, K=K, hits=int(buf['s'].n_hits.sum()), ok=int(buf['s'].ok.sum()),
                           gather_bytes_per_launch=int(B * K * T * (2 * LABELS) * 4))
                out[f'{name}_{B}x{T}_K{K}'] = rec
                buf.clear()
            del logp, plane
    print(TAG + json.dumps(out), flush=True)


def _child(a, stage, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', stage, '--steps', str(a.steps), '--rounds', str(a.rounds)]
    env = dict(os.environ, QASR_LIB=os.path.abspath(lib)) if lib else dict(os.environ)
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout, env=env)
    except subprocess.TimeoutExpired:
        sys.exit(f'child {stage} ran past {a.child_timeout} s: stopping')
    line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
    if p.returncode or not line:
        sys.exit(f'child {stage} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
    return json.loads(line[0][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['spot'], default=None)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (A/B of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: spot, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_spot(a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='device events around `steps` launches on one stream, microseconds per launch, one sample of each kernel per '
                    'round; synthetic posteriors, not speech')
    if 'spot' not in skip:
        r = _child(a, 'spot')
        for k, v in r.items():
            pt = v['P'] * v['T']
            v['k_spot_median_us'], v['k_star_median_us'] = med(v['k_spot_us']), med(v['k_star_us'])
            v['k_spot_ns_per_problem_frame'] = v['k_spot_median_us'] * 1e3 / pt
            v['k_spot_gather_GBps'] = v['gather_bytes_per_launch'] / v['k_spot_median_us'] * 1e-3
            show = ['P', 'T', 'hits', 'k_spot_median_us', 'k_star_median_us', 'k_spot_ns_per_problem_frame', 'k_spot_gather_GBps']
            if 'k_align1_us' in v:
                v['k_align1_median_us'] = med(v['k_align1_us'])
                v['k_align1_ns_per_problem_frame'] = v['k_align1_median_us'] * 1e3 / pt
                v['k_align1_over_k_spot'] = v['k_align1_median_us'] / v['k_spot_median_us']
                show += ['k_align1_median_us', 'k_align1_over_k_spot']
            print('k_spot', k, json.dumps({x: v[x] for x in show}), flush=True)
        res['k_spot'] = r
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    if a.parent_lib and 'bench' not in skip:
        bench = dict(note='`bench.py --gpus 1`, fresh processes alternating this build / the parent commit\'s library (QASR_LIB)',
                     this=[], parent=[])
        for r in range(a.ab_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib))[::1 if r % 2 == 0 else -1]:      # who goes first alternates too
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
                print(f'bench {tag} run {r}: ' + json.dumps(bench[tag][-1]), flush=True)
        bench['this_median_ms'] = med([b['ms_per_step'] for b in bench['this']])
        bench['parent_min_ms'] = float(np.min([b['ms_per_step'] for b in bench['parent']]))
        bench['parent_max_ms'] = float(np.max([b['ms_per_step'] for b in bench['parent']]))
        bench['not_slower'] = bool(bench['this_median_ms'] <= bench['parent_max_ms'])
        res['bench'] = bench
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
