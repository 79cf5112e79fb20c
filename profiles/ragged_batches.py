#!/usr/bin/env python3
"""Ragged batches, measured on one GPU: full-size QuartzNet15x5 En (random weights, the fixture's ranges), batch 32, a
fixed-seed sequence of batches whose utterance durations are drawn uniformly from 2 - 16 s, each batch padded to its own
longest utterance as the reference's collate function pads it.

Per batch, the call the facade makes (audio in; log-probs, tokens, encoded lengths out; fresh outputs per call):
  a  build of the parent commit (QASR_LIB), Engine.forward_audio
  b  this build, the same call, no reserve()
  c  this build, Engine.reserve(32, 16 s) once, then forward_ragged_audio + the clones EncDecCTCModel makes of its views
Host wall time per batch (perf_counter around the call and the synchronise) and device time per batch (events on the
stream around the call).  One sample = the mean over one pass of the whole sequence; the first pass of a process (plan,
graph captures, allocator warm-up) is not timed.  Fresh child processes, a / b / c interleaved, --process-rounds times.

Fixed shape (no figure of the ragged path): per library, 32 x 500 frames through the unreserved engine with all lengths
500 and all lengths 250, qasr_engine_time_ops per op; the k_sep2 rows are summed (`fixed`).

    python profiles/ragged_batches.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ragged_batches.json
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ragged -- python profiles/ragged_batches.py --child c
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o fixed -- python profiles/ragged_batches.py --child fixed500
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
SR, HOP = 16000, 160


def sequence(seed, n, batch, lo_s, hi_s):
    """[(samples per utterance)] per batch; a batch is padded to its own maximum"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return [np.sort(rng.integers(int(lo_s * SR), int(hi_s * SR) + 1, batch))[::-1].copy() for _ in range(n)]


def _blob():
    import numpy as np
    from qasr import pack, synth, topology
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_quartznet_w8a8.npz'))
    cfg = topology.quartznet15x5()
    return pack.pack_model(cfg, synth.make_state_dict(cfg, 0), d['act_min'], d['act_max'], 8, 8)[0]


def child_fixed(a):
    import torch
    from qasr import engine, synth
    full = a.child == 'fixed500'
    e = engine.Engine(_blob(), 0, tile=128 if a.tile128 else None)
    x = torch.from_numpy(synth.make_features(32, 64, 500, 2)).cuda()
    lens = torch.full((32,), 500 if full else 250, dtype=torch.int32).cuda()
    for _ in range(3):
        e.forward(x, lens)
    torch.cuda.synchronize()
    ms = e.time_ops(reps=a.reps)
    labels = e.op_labels()
    sep2 = [(l, float(m)) for l, m in zip(labels, ms) if l.startswith('k_sep2<')]
    for _ in range(a.reps):                                  # plain forwards for a kernel trace of this process
        e.forward(x, lens)
    torch.cuda.synchronize()
    res = dict(child=a.child, lib=os.path.basename(os.environ.get('QASR_LIB', 'libqasr_hip.so')), lens=int(lens[0]),
               k_sep2_sum_us=1e3 * sum(m for _, m in sep2), k_sep2_launches=len(sep2),
               k_sep2_max_us=1e3 * max(m for _, m in sep2), k_sep2_max_label=max(sep2, key=lambda t: t[1])[0],
               all_ops_sum_us=1e3 * float(sum(ms)))
    e.close()
    print('RAGGED_CHILD ' + json.dumps(res), flush=True)


def child(a):
    import numpy as np
    import torch
    from qasr import engine, melbank
    if not torch.cuda.is_available():
        sys.exit('ragged_batches.py measures on the GPU; no GPU found')
    if a.child.startswith('fixed'):
        return child_fixed(a)
    fb = torch.from_numpy(melbank.mel_filterbank(SR, 512, 64, 0.0, 8000.0).astype(np.float32)).cuda().contiguous()
    win = torch.hann_window(320, periodic=False).cuda()
    plan = engine.frontend_plan(fb)
    seq = sequence(a.seed, a.batches, a.batch, a.min_s, a.max_s)
    gen = torch.Generator(device='cuda').manual_seed(a.seed)
    data = []
    for lens in seq:
        S = int(lens.max())
        audio = 0.1 * torch.randn(a.batch, S, device='cuda', generator=gen)
        alen = torch.tensor(lens, dtype=torch.int32).cuda()
        audio *= (torch.arange(S, device='cuda')[None, :] < alen[:, None])       # zero padding, as the collate function pads
        data.append((audio.contiguous(), alen))
    e = engine.Engine(_blob(), 0)
    side = torch.cuda.Stream()
    if a.child == 'c':
        e.reserve(a.batch, max_samples=int(a.max_s * SR), want_logp=True, decode=False)

    def call(audio, alen):
        if a.child == 'c':
            lp, tk, el = e.forward_ragged_audio(audio, alen, fb, win, plan, 0.97, 16, stream=side)
            return lp.clone(), tk.long(), el.long()
        lp, tk, el = e.forward_audio(audio, alen, fb, win, plan, 0.97, 16, stream=side)
        return lp, tk.long(), el.long()

    host, dev, checksum = [], [], 0
    for p in range(a.passes + 1):
        h, d = [], []
        for audio, alen in data:
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(side):
                s.record()
                out = call(audio, alen)
                t.record()
            torch.cuda.synchronize()
            h.append((time.perf_counter() - t0) * 1e3)
            d.append(s.elapsed_time(t))
            if p == 0:
                checksum += int(out[2].sum())
        if p:
            host.append(float(np.mean(h)))
            dev.append(float(np.mean(d)))
    frames = [int(sum((int(l) + HOP - 1) // HOP for l in lens)) for lens in seq]
    padded = [a.batch * ((1 + int(lens.max()) // HOP + 15) // 16 * 16) for lens in seq]
    res = dict(child=a.child, lib=os.path.basename(os.environ.get('QASR_LIB', 'libqasr_hip.so')), host_ms=host, dev_ms=dev,
               tokens_checksum=checksum, padded_frame_share=1.0 - sum(frames) / sum(padded),
               stats=e.ragged_stats() if hasattr(e.lib, 'qasr_engine_ragged_stats') else None)
    e.close()
    print('RAGGED_CHILD ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['a', 'b', 'c', 'fixed500', 'fixed250'], default=None)
    ap.add_argument('--seed', type=int, default=20261016)
    ap.add_argument('--batches', type=int, default=40)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--min-s', type=float, default=2.0)
    ap.add_argument('--max-s', type=float, default=16.0)
    ap.add_argument('--passes', type=int, default=3, help='timed passes over the sequence per process (one more warms up)')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--tile128', action='store_true', help='fixed-shape children: 128-frame tiles (the benchmark\'s engine option)')
    ap.add_argument('--process-rounds', type=int, default=2)
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    plan = ([('a', a.parent_lib)] if a.parent_lib else []) + [('b', this_lib), ('c', this_lib)]
    fixed = [(c, tag, lib, t) for c in ('fixed500', 'fixed250') for tag, lib in
             ([('parent', a.parent_lib)] if a.parent_lib else []) + [('this', this_lib)] for t in (False, True)]
    runs = []

    def spawn(tag, which, lib, extra=()):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', which, '--seed', str(a.seed), '--batches', str(a.batches),
               '--batch', str(a.batch), '--min-s', str(a.min_s), '--max-s', str(a.max_s), '--passes', str(a.passes),
               '--reps', str(a.reps)] + list(extra)
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout, env=dict(os.environ, QASR_LIB=os.path.abspath(lib)))
        except subprocess.TimeoutExpired:
            sys.exit(f'child {tag} ran past {a.child_timeout} s: stopping')
        line = [l for l in p.stdout.splitlines() if l.startswith('RAGGED_CHILD ')]
        if p.returncode or not line:
            sys.exit(f'child {tag} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
        return json.loads(line[0][len('RAGGED_CHILD '):])

    for r in range(a.process_rounds):
        for which, lib in plan:
            runs.append(dict(round=r, **spawn(which, which, lib)))
            print(f"{which} round {r}: host {np.median(runs[-1]['host_ms']):.3f} ms  device {np.median(runs[-1]['dev_ms']):.3f} ms per batch", flush=True)
    fixed_runs = []
    for which, tag, lib, t128 in fixed:
        fixed_runs.append(dict(build=tag, tile128=t128, **spawn(f'{which}/{tag}', which, lib, ['--tile128'] if t128 else [])))
        print(f"{which} {tag} tile128={t128}: k_sep2 sum {fixed_runs[-1]['k_sep2_sum_us']:.1f} us, max {fixed_runs[-1]['k_sep2_max_us']:.2f} us", flush=True)

    def stat(v):
        return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v)) if len(v) else None

    summary = {}
    for which in 'abc':
        rs = [r for r in runs if r['child'] == which]
        if rs:
            summary[which] = dict(host_ms=stat([x for r in rs for x in r['host_ms']]), dev_ms=stat([x for r in rs for x in r['dev_ms']]),
                                  lib=rs[0]['lib'], stats=rs[-1]['stats'])
    if 'a' in summary:
        for k in ('host_ms', 'dev_ms'):
            summary[f'c_over_a_{k}'] = summary['c'][k]['median'] / summary['a'][k]['median']
            summary[f'b_over_a_{k}'] = summary['b'][k]['median'] / summary['a'][k]['median']
            summary[f'c_median_below_a_min_{k}'] = summary['c'][k]['median'] < summary['a'][k]['min']
    cs = {r['tokens_checksum'] for r in runs}
    res = dict(workload=dict(model='QuartzNet15x5Base-En (random weights)', batch=a.batch, batches=a.batches, seed=a.seed,
                             seconds=[a.min_s, a.max_s], padded_frame_share=runs[0]['padded_frame_share'] if runs else None,
                             passes=a.passes, process_rounds=a.process_rounds, same_encoded_lengths_everywhere=len(cs) == 1),
               note='one sample = mean per batch over one pass of the sequence; host: perf_counter around the call + synchronise; '
                    'device: events on the stream around the call', summary=summary, fixed=fixed_runs, runs=runs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    print(json.dumps(dict(workload=res['workload'], summary=summary), indent=1))


if __name__ == '__main__':
    main()
