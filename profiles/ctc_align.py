#!/usr/bin/env python3
"""CTC forced alignment on the device, measured on one GPU: QuartzNet15x5 En (29 classes) and Zh (5207 classes) at
32 utterances x 500 frames (250 encoder frames), targets = the greedy strings of the run.

  kernels  k_align per launch on the engine's own log-probabilities: device events around --steps launches on one stream,
           --rounds samples, median / min / max, and per frame; with and without `total` (the forward pass), at K = 1 and K = 4
           problems per utterance (K = 4: every target four times, as decode(beam_width=, n_best=4, timestamps=True) lays
           them out).  One long case: 1 utterance x 8000 frames x 2000 labels (random log-probabilities, the 17-states-per-
           thread instantiation).  The per-kernel table of rocprofv3 comes from a run of its own:
             rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o align -- python profiles/ctc_align.py --child En
  twin     qasr.align.align_host on the same batches, host seconds: context, not a bar
  bench    `bench.py --gpus 1` on this build and on a build of the parent commit (QASR_LIB), fresh processes alternating this /
           parent, --bench-runs each, each under its own time limit, stopping at the first one that fails

    python profiles/ctc_align.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_align.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]


def child(a):
    import numpy as np
    import torch

    from qasr import align, engine, pack, synth, topology
    if not torch.cuda.is_available():
        sys.exit('ctc_align.py measures on the GPU; no GPU found')

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

    def same(got, want, total):
        return all(np.array_equal(getattr(got, f).cpu().numpy().view(np.int32) if f == 'score' else getattr(got, f).cpu().numpy(),
                                  getattr(want, f).view(np.int32) if f == 'score' else getattr(want, f))
                   for f in ('start', 'nframes', 'score', 'path_score', 'ok') + (('total',) if total else ()))

    if a.child == 'long':
        T, L, C_ = a.long_frames, a.long_labels, 29
        g = torch.Generator().manual_seed(1)
        logp = torch.log_softmax(3.0 * torch.randn(1, T, C_, generator=g), dim=-1).cuda()
        tg = torch.randint(0, C_ - 1, (1, L), generator=g, dtype=torch.int32).cuda()
        tl = torch.tensor([L], dtype=torch.int32).cuda()
        ws = torch.empty(engine.ctc_align_workspace_bytes(1, T, L), dtype=torch.uint8, device='cuda')
        buf, kern = {}, {}
        for total in (True, False):
            def run(total=total):
                buf[total] = engine.ctc_align(logp, None, tg, tl, C_ - 1, want_total=total, workspace=ws, out=buf.get(total))
            kern['k_align_total_us' if total else 'k_align_us'] = timed(run)
        t0 = time.perf_counter()
        twin = align.align_host(logp.cpu().numpy(), None, tg.cpu().numpy(), tl.cpu().numpy(), C_ - 1)
        twin_s = time.perf_counter() - t0
        res = dict(model='long', classes=C_, enc_frames=T, labels=L, problems=1, workspace_bytes=int(ws.numel()), kernels_us=kern,
                   twin_host_s=twin_s, equals_twin=bool(same(buf[True], twin, True) and same(buf[False], twin, False)),
                   ok=int(twin.ok.sum()))
        print('CTC_ALIGN_CHILD ' + json.dumps(res), flush=True)
        return

    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_quartznet_w8a8.npz'))
    cfg = topology.quartznet15x5() if a.child == 'En' else topology.quartznet15x5_zh()
    blob = pack.pack_model(cfg, synth.make_state_dict(cfg, 0), d['act_min'], d['act_max'], 8, 8)[0]
    B, T, ncls = a.batch, a.frames, cfg.num_classes + 1
    x = torch.from_numpy(synth.make_features(B, 64, T, 2)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    e = engine.Engine(blob, 0, graph=True)
    logp, _, enc_len = e.forward(x, lens, want_logp=True)[:3]
    logp, enc_len = logp.clone(), enc_len.clone()
    greedy = e.forward(x, lens, want_logp=False, decode=True)[3]
    torch.cuda.synchronize()
    To = int(logp.shape[1])
    labels, n_labels = greedy.labels.clone(), greedy.n_labels.clone()          # [B, To] / [B]: the targets, row pitch To
    kern, buf, equal = {}, {}, True
    twin_s = None
    for K in (1, 4):
        tg = labels.repeat_interleave(K, dim=0).contiguous()
        tl = n_labels.repeat_interleave(K, dim=0).contiguous()
        ws = torch.empty(engine.ctc_align_workspace_bytes(B * K, To, To), dtype=torch.uint8, device='cuda')
        for total in (True, False):
            key = (K, total)

            def run(key=key, tg=tg, tl=tl, ws=ws, K=K, total=total):
                buf[key] = engine.ctc_align(logp, enc_len, tg, tl, ncls - 1, problems_per_utt=K, want_total=total, workspace=ws,
                                            out=buf.get(key))
            kern[f'k_align_k{K}' + ('_total' if total else '') + '_us'] = timed(run)
        if K == 1:
            t0 = time.perf_counter()
            twin = align.align_host(logp.cpu().numpy(), enc_len.cpu().numpy(), tg.cpu().numpy(), tl.cpu().numpy(), ncls - 1)
            twin_s = time.perf_counter() - t0
            equal = same(buf[(1, True)], twin, True) and same(buf[(1, False)], twin, False)
    res = dict(model=a.child, classes=ncls, enc_frames=To, problems=B, mean_labels=float(n_labels.float().mean()),
               max_labels=int(n_labels.max()), kernels_us=kern, twin_host_s=twin_s, equals_twin=bool(equal),
               ok=int(buf[(1, True)].ok.sum()))
    e.close()
    print('CTC_ALIGN_CHILD ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['En', 'Zh', 'long'], default=None)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--long-frames', type=int, default=8000)
    ap.add_argument('--long-labels', type=int, default=2000)
    ap.add_argument('--steps', type=int, default=10)
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

    summary, runs = {}, []
    for model in ('En', 'Zh', 'long'):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', model, '--batch', str(a.batch), '--frames', str(a.frames),
               '--long-frames', str(a.long_frames), '--long-labels', str(a.long_labels), '--steps', str(a.steps),
               '--rounds', str(a.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f'child {model} ran past {a.child_timeout} s: stopping')
        line = [l for l in p.stdout.splitlines() if l.startswith('CTC_ALIGN_CHILD ')]
        if p.returncode or not line:
            sys.exit(f'child {model} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
        r = json.loads(line[0][len('CTC_ALIGN_CHILD '):])
        runs.append(r)
        s = {k: stat(v) for k, v in r['kernels_us'].items()}
        for k in list(s):
            s[k + '_per_frame'] = s[k]['median'] / r['enc_frames']
        s.update({k: r[k] for k in r if k not in ('kernels_us', 'model')})
        summary[model] = s
        print(model, json.dumps(s), flush=True)
    bench = {}
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        bench = dict(note='`bench.py --gpus 1` in the same session, fresh processes alternating this build / the parent '
                          'commit\'s library (QASR_LIB)', this=[], parent=[])
        for r in range(a.bench_runs):
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
                print(f'bench {tag} run {r}: ' + json.dumps(bench[tag][-1]), flush=True)
        bench['this_median_ms'] = float(np.median([b['ms_per_step'] for b in bench['this']]))
        bench['parent_slowest_ms'] = float(np.max([b['ms_per_step'] for b in bench['parent']]))
        bench['not_slower'] = bool(bench['this_median_ms'] <= bench['parent_slowest_ms'])
    res = dict(shape=dict(batch=a.batch, frames=a.frames, long_frames=a.long_frames, long_labels=a.long_labels), steps=a.steps,
               rounds=a.rounds,
               note='kernel times: device events around `steps` launches on one stream (microseconds per launch); synthetic random '
                    'weights, so the greedy strings (the targets) are longer and the distributions flatter than a trained model\'s',
               summary=summary, bench=bench, runs=runs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
