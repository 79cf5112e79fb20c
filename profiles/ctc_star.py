#!/usr/bin/env python3
"""The wildcard ("star") for untranscribed audio, measured on one GPU.

  k_star   the plane for En (29 classes) and Zh (5207 classes) at 32 x 500 frames and at 1 x 180 000 frames: device events
           around --steps launches on one stream, --rounds samples; next to each a device-to-device copy of the same byte count
           (4 B T C), timed in the same run.  k_star reads what the copy reads and writes 1 / C of it: the ratio is reported,
           not gated.
  star     k_align (32 x 500 frames, 150 labels) and k_align_band (1 x 180 000 frames, 1024 states) with a plane - the STAR
           instantiations - against the same launches without one, on identical targets that hold no wildcard
  parent   the same launches without a plane under this build and under a build of the parent commit (QASR_LIB), fresh
           processes alternating this / parent, --ab-runs each; then `bench.py --gpus 1` the same way.  Each process runs under
           its own time limit, and the script stops at the first one that fails.

    python profiles/ctc_star.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_star.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
SHAPES = (('en', 29), ('zh', 5207))
SIZES = ((32, 500), (1, 180000))
TAG = 'CTC_STAR_CHILD '


def _timed(torch, fn, steps, rounds):
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(rounds):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            fn()
        t.record()
        t.synchronize()
        samples.append(s.elapsed_time(t) / steps * 1e3)
    return samples


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


def child_star(a):
    import torch

    from qasr import engine
    if not torch.cuda.is_available():
        sys.exit('ctc_star.py measures on the GPU; no GPU found')
    out = {}
    for name, C_ in SHAPES:
        for B, T in SIZES:
            logp, _ = _logp(torch, B, T, C_, 1)
            plane = torch.empty(B, T, device='cuda')
            dst = torch.empty_like(logp)
            key = f'{name}_{B}x{T}'
            out[key] = dict(bytes=int(logp.numel() * 4),
                            k_star_us=_timed(torch, lambda: engine.ctc_star(logp, None, 1.0, out=plane), a.steps, a.rounds),
                            copy_us=_timed(torch, lambda: dst.copy_(logp), a.steps, a.rounds))
            del logp, dst
    print(TAG + json.dumps(out), flush=True)


def child_align(a):
    """k_align and k_align_band without a plane and (where the library has k_star) with one, targets without a wildcard"""
    import torch

    from qasr import engine
    if not torch.cuda.is_available():
        sys.exit('ctc_star.py measures on the GPU; no GPU found')
    has_star = hasattr(engine.load_library(), 'qasr_ctc_star')
    C_, out = 29, {}
    logp, own = _logp(torch, 32, 500, C_, 2)
    tg, tl = _targets(torch, own, 150, 32)
    ws = torch.empty(engine.ctc_align_workspace_bytes(32, 500, tg.shape[1]), dtype=torch.uint8, device='cuda')
    buf = {}

    def run_align(star=None):
        kw = {} if star is None else dict(star=star)
        buf['a'] = engine.ctc_align(logp, None, tg, tl, C_ - 1, workspace=ws, out=buf.get('a'), **kw)
    out['k_align_32x500_us'] = _timed(torch, run_align, a.steps, a.rounds)
    ok = int(buf['a'].ok.sum())
    if has_star:
        plane = engine.ctc_star(logp, None, 1.0)
        out['k_align_star_32x500_us'] = _timed(torch, lambda: run_align(plane), a.steps, a.rounds)
    logp1, own1 = _logp(torch, 1, 180000, C_, 3)
    tg1, tl1 = _targets(torch, own1, 54000, 1)
    ws1 = torch.empty(engine.ctc_align_band_workspace_bytes(1, 180000, 1024), dtype=torch.uint8, device='cuda')

    def run_band(star=None):
        kw = {} if star is None else dict(star=star)
        buf['b'] = engine.ctc_align_band(logp1, None, tg1, tl1, C_ - 1, band_states=1024, workspace=ws1, out=buf.get('b'), **kw)
    out['k_align_band_1x180000_us'] = _timed(torch, run_band, a.steps, a.rounds)
    ok_band = int(buf['b'].ok.sum())
    if has_star:
        plane1 = engine.ctc_star(logp1, None, 1.0)
        out['k_align_band_star_1x180000_us'] = _timed(torch, lambda: run_band(plane1), a.steps, a.rounds)
    out['ok'] = dict(k_align=ok, k_align_band=ok_band, labels=int(tl[0]), band_labels=int(tl1[0]))
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
    ap.add_argument('--child', choices=['star', 'align'], default=None)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (A/B of the launches without a plane, and of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: star, align, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_star(a) if a.child == 'star' else child_align(a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='device events around `steps` launches on one stream, microseconds per launch; synthetic posteriors, not speech')
    if 'star' not in skip:
        r = _child(a, 'star')
        for k, v in r.items():
            v['k_star_median_us'], v['copy_median_us'] = med(v['k_star_us']), med(v['copy_us'])
            v['k_star_over_copy'] = v['k_star_median_us'] / v['copy_median_us']
            v['k_star_read_GBps'] = v['bytes'] / v['k_star_median_us'] * 1e-3
            print('k_star', k, json.dumps({x: v[x] for x in ('bytes', 'k_star_median_us', 'copy_median_us', 'k_star_over_copy', 'k_star_read_GBps')}), flush=True)
        res['k_star'] = r
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    if 'align' not in skip:
        runs = dict(this=[], parent=[])
        for i in range(a.ab_runs if a.parent_lib else 1):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib)):
                if lib:
                    runs[tag].append(_child(a, 'align', lib))
        summ = {}
        for key in ('k_align_32x500_us', 'k_align_band_1x180000_us'):
            t = [med(r[key]) for r in runs['this']]
            s = [med(r[key.replace('_32', '_star_32').replace('_1x', '_star_1x')]) for r in runs['this']]
            summ[key] = dict(this_runs=t, this_with_a_plane_runs=s, star_over_false=med(s) / med(t))
            if runs['parent']:
                q = [med(r[key]) for r in runs['parent']]
                summ[key].update(parent_runs=q, this_median=med(t), parent_min=float(np.min(q)), parent_max=float(np.max(q)),
                                 inside_parent_spread=bool(np.min(q) <= med(t) <= np.max(q)))
        res['align'] = dict(runs=runs, summary=summ)
        print('align', json.dumps(summ), flush=True)
    if a.parent_lib and 'bench' not in skip:
        bench = dict(note='`bench.py --gpus 1`, fresh processes alternating this build / the parent commit\'s library (QASR_LIB)',
                     this=[], parent=[])
        for r in range(a.ab_runs):
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
