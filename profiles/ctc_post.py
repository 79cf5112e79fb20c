#!/usr/bin/env python3
"""CTC posteriors (k_post: forward-backward along an alignment), measured on one GPU against k_align with total.

  post     k_post and k_align (with total: Viterbi + forward, its own two serial passes over the same frame step) in the same
           build, on the same inputs, in one process: device events around --steps launches on one stream; --rounds rounds that
           alternate k_align / k_post, medians reported.  Shapes: 32 x 500 frames at En (29 classes) and Zh (5207 classes) with
           targets of about 100 labels, and 1 x 4097 frames at 2048 labels (the label cap: 17 states per thread).
  bench    `bench.py --gpus 1`, fresh processes alternating this build / a build of the parent commit (QASR_LIB), --ab-runs each;
           which of the two goes first alternates from pair to pair.  Each process runs under its own time limit, and the
           script stops at the first one that fails.

    python profiles/ctc_post.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_post.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
# (name, classes, utterances, frames, labels)
SHAPES = (('en_32x500_100', 29, 32, 500, 100), ('zh_32x500_100', 5207, 32, 500, 100), ('cap_1x4097_2048', 29, 1, 4097, 2048))
TAG = 'CTC_POST_CHILD '


def _events(torch, fn, steps):
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


def _targets(torch, own, n, P):
    """n labels in the order the frames carry them, no adjacent repeats"""
    y = []
    for c in own.tolist():
        if len(y) == n:
            break
        if not y or c != y[-1]:
            y.append(c)
    return torch.tensor([y] * P, dtype=torch.int32).cuda(), torch.full((P,), len(y), dtype=torch.int32).cuda()


def child_post(a):
    import torch

    from qasr import engine
    if not torch.cuda.is_available():
        sys.exit('ctc_post.py measures on the GPU; no GPU found')
    out = {}
    for name, C_, B, T, n in SHAPES:
        logp, own = _logp(torch, B, T, C_, 1)
        tg, tl = _targets(torch, own, n, B)
        ML = tg.shape[1]
        ws_a = torch.empty(engine.ctc_align_workspace_bytes(B, T, ML), dtype=torch.uint8, device='cuda')
        ws_p = torch.empty(engine.ctc_post_workspace_bytes(B, T), dtype=torch.uint8, device='cuda')
        buf = {}

        def run_align():
            buf['a'] = engine.ctc_align(logp, None, tg, tl, C_ - 1, workspace=ws_a, out=buf.get('a'))

        def run_post():
            buf['p'] = engine.ctc_post(logp, None, tg, tl, C_ - 1, buf['a'], workspace=ws_p, out=buf.get('p'))
        run_align(), run_post()
        torch.cuda.synchronize()
        al, po = [], []
        for _ in range(a.rounds):                                   # alternating rounds: drift hits both alike
            al.append(_events(torch, run_align, a.steps))
            po.append(_events(torch, run_post, a.steps))
        same_total = bool((buf['a'].total == buf['p'].total).all())
        out[name] = dict(classes=C_, utterances=B, frames=T, labels=int(tl[0]), k_align_total_us=al, k_post_us=po,
                         ok=int(buf['p'].ok.sum()), total_equal=same_total,
                         mean_posterior=float(torch.exp(buf['p'].frame_post.double() / 65536.0).mean()))
        del logp
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
    ap.add_argument('--child', choices=['post'], default=None)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (A/B of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: post, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_post(a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='device events around `steps` launches on one stream, microseconds per launch, rounds alternating k_align (with '
                    'total) / k_post; synthetic posteriors, not speech')
    if 'post' not in skip:
        r = _child(a, 'post')
        for k, v in r.items():
            v['k_align_total_median_us'], v['k_post_median_us'] = med(v['k_align_total_us']), med(v['k_post_us'])
            v['k_post_over_k_align_total'] = v['k_post_median_us'] / v['k_align_total_median_us']
            print('post', k, json.dumps({x: v[x] for x in ('labels', 'k_align_total_median_us', 'k_post_median_us',
                                                            'k_post_over_k_align_total', 'ok', 'total_equal')}), flush=True)
        res['post'] = r
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    if a.parent_lib and 'bench' not in skip:
        bench = dict(note='`bench.py --gpus 1`, fresh processes alternating this build / the parent commit\'s library (QASR_LIB)',
                     this=[], parent=[])
        for r in range(a.ab_runs):
            pair = (('this', this_lib), ('parent', a.parent_lib))
            for tag, lib in (pair if r % 2 == 0 else pair[::-1]):   # who goes first alternates too
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
