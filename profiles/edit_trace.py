#!/usr/bin/env python3
"""The edit path on the device (qasr_edit_trace: k_edit_cut, k_edit_trace), measured on one GPU.

  trace    one qasr_edit_trace call against (a) one qasr_edit_distance call of the same build on the same rows - the forward pass
           without the plane, with k_edit_totals - and (b) the host alternative a user has today: a full-matrix back-trace in
           Python on the same strings (one core; not run for the hour: minutes).  Device events around --steps calls on one
           stream (1 for the hour), the two calls alternating inside a round, --rounds rounds, medians.  `us`: the calls
           through the Python binding; `replay_us`: the same calls captured once in a graph and replayed, the device's own
           time.  32 x 40 words; 32 x 250 characters; one stitched hour in words (~9 000).  The strings are those of
           profiles/edit.py: the references with about 15 % of the units substituted, dropped or doubled.  `same_path`: the
           device's ops equal the host back-trace's.
           Forward pass and walk apart: run this stage under `rocprofv3 --kernel-trace --stats -- python profiles/edit_trace.py
           --child trace` in a run of its own; the walk is k_edit_trace's time less k_edit's of the same shape.
  bench    `bench.py --gpus 1`, fresh processes alternating this build / a build of the parent commit (QASR_LIB), --ab-runs each,
           the order inside a pair alternating as well.  Each process runs under its own time limit, and the script stops at the
           first one that fails.

    python profiles/edit_trace.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/edit_trace.json
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
TAG = 'EDIT_TRACE_CHILD '

_spec = importlib.util.spec_from_file_location('profiles_edit', os.path.join(ROOT, 'profiles', 'edit.py'))
pe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pe)                                        # its strings and rows: the same inputs as the edit paragraph's


def host_backtrace(h, r):
    """what a user writes today: the whole matrix in Python lists, then the walk under the same tie order"""
    n, m = len(h), len(r)
    M = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        M[0][j] = j
    for i in range(1, n + 1):
        M[i][0] = i
        row, up = M[i], M[i - 1]
        for j in range(1, m + 1):
            row[j] = min(up[j - 1] + (h[i - 1] != r[j - 1]), row[j - 1] + 1, up[j] + 1)
    ops, i, j = [], n, m
    while i or j:
        if i and j and M[i][j] == M[i - 1][j - 1] + (h[i - 1] != r[j - 1]):
            ops.append(int(h[i - 1] != r[j - 1]))
            i, j = i - 1, j - 1
        elif j and M[i][j] == M[i][j - 1] + 1:
            ops.append(2)
            j -= 1
        else:
            ops.append(3)
            i -= 1
    return ops[::-1]


def child_trace(a):
    import numpy as np
    import torch

    from qasr import edit, engine
    if not torch.cuda.is_available():
        sys.exit('edit_trace.py measures on the GPU; no GPU found')
    mask = torch.from_numpy(edit.space_mask(pe.VOCAB)).cuda()
    cases = {}
    for name, rows, words, mode, host in (('words_32x40', 32, 40, 'word', True), ('chars_32x250', 32, 45, 'char', True),
                                          ('hour_words_1x9000', 1, 9000, 'word', False)):
        refs = pe._texts(np, 1, rows, words)
        if name == 'chars_32x250':
            refs = [t[:250] for t in refs]
        hyps = pe._edited(np, 2, refs, mode)
        (h, hl), (r, rl) = pe._rows(np, torch, hyps), pe._rows(np, torch, refs)
        P, md = len(hyps), edit.MODES[mode]
        new = lambda n, dt=torch.uint8: torch.empty(n, dtype=dt, device='cuda')      # noqa: E731
        common = dict(mode=mode, is_space=mask)
        cases[name] = dict(
            args=(h, hl, r, rl, len(pe.VOCAB)),
            dist=dict(common, workspace=new(engine.edit_workspace_bytes(P, h.shape[1], r.shape[1], mode)),
                      totals=torch.zeros(16, dtype=torch.int64, device='cuda'), out=new((P, 8), torch.int32)),
            trace=dict(common, workspace=new(engine.edit_trace_workspace_bytes(P, h.shape[1], r.shape[1], mode)),
                       ops=new((P, edit.unit_bound(h.shape[1], md) + edit.unit_bound(r.shape[1], md))), n_ops=new(P, torch.int32),
                       out=new((P, 8), torch.int32)),
            steps=a.steps if rows > 1 else 1, hyps=hyps, refs=refs, host=host, mode=mode,
            rec=dict(P=P, hyp_ids=int(h.shape[1]), ref_ids=int(r.shape[1]), distance_us=[], trace_us=[]))
        cases[name]['rec']['trace_workspace_bytes'] = int(cases[name]['trace']['workspace'].numel())
    calls = dict(distance=lambda c: engine.edit_distance(*c['args'], **c['dist']), trace=lambda c: engine.edit_trace(*c['args'], **c['trace']))
    side = torch.cuda.Stream()
    for c in cases.values():                                        # warm every case before any is timed
        c['graphs'] = {}
        for which, call in calls.items():
            call(c)
            torch.cuda.synchronize()
            if c['steps'] > 1:                                      # the binding's Python costs more than a small batch's launches
                side.wait_stream(torch.cuda.current_stream())
                g = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(g, stream=side):
                        for _ in range(c['steps']):
                            call(c)
                g.replay()
                c['graphs'][which] = g
                c['rec'][which + '_replay_us'] = []
    torch.cuda.synchronize()

    def sample(fn, steps):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / steps * 1e3

    def eager(call, c):
        for _ in range(c['steps']):
            call(c)
    for rnd in range(a.rounds):
        for c in cases.values():
            for which in (('distance', 'trace') if rnd % 2 == 0 else ('trace', 'distance')):       # who goes first alternates
                c['rec'][which + '_us'].append(sample(lambda: eager(calls[which], c), c['steps']))
                if which in c['graphs']:
                    c['rec'][which + '_replay_us'].append(sample(c['graphs'][which].replay, c['steps']))
    out = {}
    for name, c in cases.items():
        rec = c['rec']
        res = calls['trace'](c)
        torch.cuda.synchronize()
        rows, ops, n_ops = res.rows.cpu().numpy(), res.ops.cpu().numpy(), res.n_ops.cpu().numpy()
        rec.update(errors=int(rows[:, 0].sum()), ops=int(n_ops.sum()), cells=int((rows[:, 4].astype(np.int64) * rows[:, 5]).sum()))
        rec['host_backtrace_ms'], rec['same_path'] = None, None     # not measured
        if c['host']:
            cut = (lambda t: list(t)) if c['mode'] == 'char' else (lambda t: t.split())
            t0 = time.perf_counter()
            paths = [host_backtrace(cut(h), cut(r)) for h, r in zip(c['hyps'], c['refs'])]
            rec['host_backtrace_ms'] = (time.perf_counter() - t0) * 1e3
            rec['same_path'] = all(ops[p, :n_ops[p]].tolist() == paths[p] for p in range(len(paths)))
        out[name] = rec
    print(TAG + json.dumps(out), flush=True)


def _child(a, stage):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', stage, '--steps', str(a.steps), '--rounds', str(a.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f'child {stage} ran past {a.child_timeout} s: stopping')
    line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
    if p.returncode or not line:
        sys.exit(f'child {stage} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
    return json.loads(line[0][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['trace'], default=None)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (A/B of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: trace, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_trace(a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='device events around `steps` calls on one stream, microseconds per call; qasr_edit_distance (three launches) and '
                    'qasr_edit_trace (two launches) alternate inside a round on the same rows; random strings over 28 characters, not speech')

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
    if 'trace' not in skip:
        r = _child(a, 'trace')
        for k, v in r.items():
            for which in ('distance', 'trace'):
                v[which + '_median_us'] = med(v[which + '_us'])
                if which + '_replay_us' in v:
                    v[which + '_replay_median_us'] = med(v[which + '_replay_us'])
            d, t = (v.get(w + '_replay_median_us', v[w + '_median_us']) for w in ('distance', 'trace'))
            v['trace_over_distance'] = t / d
            v['walk_le_forward'] = bool(t - d <= d)                  # the expectation of DESIGN: the walk costs at most a forward pass
            if v['host_backtrace_ms'] is not None:
                v['host_over_call'] = v['host_backtrace_ms'] * 1e3 / v['trace_median_us']
            print('k_edit_trace', k, json.dumps({x: v.get(x) for x in ('P', 'distance_median_us', 'trace_median_us', 'distance_replay_median_us',
                                                                       'trace_replay_median_us', 'trace_over_distance', 'host_backtrace_ms',
                                                                       'same_path', 'ops')}), flush=True)
        res['k_edit_trace'] = r
        save()
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
    save()


if __name__ == '__main__':
    main()
