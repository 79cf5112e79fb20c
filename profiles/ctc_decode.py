#!/usr/bin/env python3
"""On-device greedy CTC decoding, measured on one GPU: QuartzNet15x5 En (29 classes, k_dec) and Zh (5207 classes,
k_decw) at 32 utterances x 500 frames (250 encoder frames), one stream, graph replay, caller-owned buffers.

Device step, variants interleaved after warm-up (mean of --steps replays between device events per sample, --rounds
samples per variant and process, median / min / max over all samples reported):
  a  tokens only, nothing attached - on this build AND on a build of the parent commit (a library is chosen per
     process: QASR_LIB), fresh child processes interleaved this / parent / this / parent ..., each under its own time
     limit, stopping at the first child that fails
  b  tokens only + frame_score + decode attached (k_ctc inside the graph)
  c  with log-probabilities, nothing attached
End to end to strings, host milliseconds per batch (perf_counter around enqueue, copies, synchronise and Python):
  today   tokens to the host + WER.ctc_decoder_predictions_tensor (one Python step per frame)
  decode  variant b, compact labels / times / scores to the host + qasr.ctc.to_hypotheses (one step per label)

    python profiles/ctc_decode.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_decode.json
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ctc -- python profiles/ctc_decode.py --child Zh --variants b
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

    from nemo.collections.asr.metrics.wer import WER
    from qasr import ctc, engine, pack, synth, topology
    if not torch.cuda.is_available():
        sys.exit('ctc_decode.py measures on the GPU; no GPU found')
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_quartznet_w8a8.npz'))
    cfg = topology.quartznet15x5() if a.child == 'En' else topology.quartznet15x5_zh()
    blob = pack.pack_model(cfg, synth.make_state_dict(cfg, 0), d['act_min'], d['act_max'], 8, 8)[0]
    B, T, ncls = a.batch, a.frames, cfg.num_classes + 1
    x = torch.from_numpy(synth.make_features(B, 64, T, 2)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    side = torch.cuda.Stream()
    V = {}
    for v in a.variants.split(','):                      # one engine per variant: each keeps its own captured graph
        e = engine.Engine(blob, 0, graph=True)
        To = e.out_frames(T)
        out = (torch.empty(B, To, ncls, device='cuda') if v == 'c' else None,
               torch.empty(B, To, dtype=torch.int32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'))
        bufs = None
        if v == 'b':
            bufs = engine.ctc_buffers(B, To, 'cuda', scores=True, blank=ncls - 1)
            e.attach_ctc(bufs.frame_score, bufs, use_lens=True)
        V[v] = (e, out, bufs)

    def run(v, n):
        e, out, _ = V[v]
        with torch.cuda.stream(side):
            for _ in range(n):
                e.forward(x, lens, want_logp=v == 'c', out=out)

    for v in V:                                          # direct, capture, replays: every variant warm before any is timed
        run(v, 5)
    torch.cuda.synchronize()
    samples = {v: [] for v in V}
    for _ in range(a.rounds):
        for v in V:
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                s.record()
            run(v, a.steps)
            with torch.cuda.stream(side):
                t.record()
            t.synchronize()
            samples[v].append(s.elapsed_time(t) / a.steps)
    res = dict(model=a.child, lib=os.path.basename(os.environ.get('QASR_LIB', 'libqasr_hip.so')), step_ms=samples,
               launches={v: V[v][0].num_launches() for v in V})
    if 'a' in V and 'b' in V and a.e2e:
        wer = WER(vocabulary=cfg.vocabulary)
        spf = ctc.seconds_per_frame(cfg, 0.01)
        today, decode, texts = [], [], None
        for _ in range(a.e2e):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run('a', 1)
            side.synchronize()
            hy0 = wer.ctc_decoder_predictions_tensor(V['a'][1][1])
            t1 = time.perf_counter()
            run('b', 1)
            side.synchronize()
            hy1 = ctc.to_hypotheses(V['b'][2], cfg.vocabulary, spf)
            t2 = time.perf_counter()
            today.append((t1 - t0) * 1e3)
            decode.append((t2 - t1) * 1e3)
            texts = (hy0, [h.text for h in hy1])
        res['e2e_host_ms'] = dict(today=today, decode=decode, same_strings=texts[0] == texts[1],
                                  labels_per_batch=int(V['b'][2].n_labels.sum()), frames_per_batch=B * V['b'][1][1].shape[1])
    for e, _, _ in V.values():
        e.close()
    print('CTC_DECODE_CHILD ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['En', 'Zh'], default=None)
    ap.add_argument('--variants', default='a,b,c')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--e2e', type=int, default=10, help='batches of the end-to-end host timing (0: skip)')
    ap.add_argument('--process-rounds', type=int, default=2)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (variant a only)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    plan = [('this', this_lib, 'a,b,c')] + ([('parent', a.parent_lib, 'a')] if a.parent_lib else [])
    runs = []
    for r in range(a.process_rounds):
        for model in ('En', 'Zh'):
            for tag, lib, variants in plan:
                cmd = [sys.executable, os.path.abspath(__file__), '--child', model, '--variants', variants, '--batch', str(a.batch),
                       '--frames', str(a.frames), '--steps', str(a.steps), '--rounds', str(a.rounds), '--e2e', str(a.e2e)]
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout,
                                       env=dict(os.environ, QASR_LIB=os.path.abspath(lib)))
                except subprocess.TimeoutExpired:
                    sys.exit(f'child {tag}/{model} ran past {a.child_timeout} s: stopping')
                line = [l for l in p.stdout.splitlines() if l.startswith('CTC_DECODE_CHILD ')]
                if p.returncode or not line:
                    sys.exit(f'child {tag}/{model} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
                runs.append(dict(build=tag, round=r, **json.loads(line[0][len('CTC_DECODE_CHILD '):])))
                print(f'{tag:6s} {model} round {r}: ' + '  '.join(f'{v} {np.median(s):.4f}' for v, s in runs[-1]['step_ms'].items()), flush=True)

    def stat(v):
        return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v)) if len(v) else None

    summary = {}
    for model in ('En', 'Zh'):
        rs = [r for r in runs if r['model'] == model]
        s = {}
        for tag in ('this', 'parent'):
            for v in 'abc':
                vals = [x for r in rs if r['build'] == tag and v in r['step_ms'] for x in r['step_ms'][v]]
                if vals:
                    s[f'{tag}/{v}_ms'] = stat(vals)
        per_process_a = {tag: [float(np.median(r['step_ms']['a'])) for r in rs if r['build'] == tag] for tag in ('this', 'parent')}
        s['a_per_process_median_ms'] = per_process_a
        if 'this/b_ms' in s:
            s['b_minus_a_us'] = (s['this/b_ms']['median'] - s['this/a_ms']['median']) * 1e3
            s['c_minus_a_us'] = (s['this/c_ms']['median'] - s['this/a_ms']['median']) * 1e3
        e2e = [r['e2e_host_ms'] for r in rs if 'e2e_host_ms' in r]
        if e2e:
            s['e2e_host_ms'] = dict(today=stat([x for e in e2e for x in e['today']]), decode=stat([x for e in e2e for x in e['decode']]),
                                    same_strings=all(e['same_strings'] for e in e2e), labels_per_batch=e2e[0]['labels_per_batch'],
                                    frames_per_batch=e2e[0]['frames_per_batch'])
        s['launches'] = {r['build']: r['launches'] for r in rs}
        summary[model] = s
    res = dict(shape=dict(batch=a.batch, frames=a.frames), steps=a.steps, rounds=a.rounds, process_rounds=a.process_rounds,
               note='step times: device events around `steps` graph replays on one stream; synthetic random weights, so the '
                    'token rows carry far more labels than speech does (labels_per_batch)', summary=summary, runs=runs)
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    print(json.dumps(summary, indent=1))


if __name__ == '__main__':
    main()
