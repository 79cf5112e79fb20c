#!/usr/bin/env python3
"""Streaming endpointing (qasr.stream_ep, k_stream_endpoint), measured.  NOT RUN YET: no stream_endpoint.json is committed.

  --device     (one GPU) k_stream_endpoint against k_stream_emit per launch at 1 / 8 / 32 streams x 48 final frames, from the
               same stored state every time (the copy that restores it is timed alone and subtracted): device events around
               --steps launches, the median of --rounds samples.  For the kernel trace run it under a profiler, in a run of
               its own: rocprofv3 --kernel-trace --stats -- python profiles/stream_endpoint.py --device
  --session    (one GPU) host wall time per step of EncDecCTCModel.stream on the calibrated mini net at 1 / 8 / 32 streams,
               with and without endpoint=: the difference is one launch, one upload of flags and the read-back of the records
  --bench DIR  bench.py --gpus 1 of this tree and of the parent's tree at DIR (built there), alternating, three runs each;
               the expectation is that they read alike within the spread of the parent's own three runs, because no
               existing kernel's text changed

    python profiles/stream_endpoint.py --device --session --out profiles/stream_endpoint.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests'), ROOT]


def _timed(a, fn):
    import numpy as np
    import torch
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) * 1000.0 / a.steps)
    return float(np.median(samples))


def device(a):
    import numpy as np
    import torch

    import stream_cases as sc
    from qasr import engine, stream as st, stream_ep as se
    plan = sc.plan_frames(48, 5, 1)
    eplan = se.EndpointPlan(plan, 3, 7, 12, 16)
    rows = []
    for S in (1, 8, 32):
        rng = np.random.default_rng(S)
        state, ep = engine.stream_state(S, plan, 'cuda'), engine.stream_ep_state(S, 'cuda')
        blk = np.zeros((S, st.STATE_WORDS), np.int32)
        blk[:, 0:2].view(np.int64)[:, 0] = 48 * plan.samples_per_frame + plan.Rr          # 48 frames are final
        engine.stream_block(state, S).copy_(torch.from_numpy(blk).cuda())
        saved, ep_saved = state.clone(), ep.clone()
        sl = torch.arange(S, dtype=torch.int32, device='cuda')
        i32 = lambda v: torch.full((S,), v, dtype=torch.int32, device='cuda')               # noqa: E731
        tok = torch.from_numpy(np.stack([sc.token_row(rng, plan.Tw, 0.5, 3) for _ in range(S)])).cuda()
        fs = torch.from_numpy(np.stack([sc.score_row(rng, plan.Tw) for _ in range(S)])).cuda()
        fl, enc, first = i32(0), i32(plan.Tw), i32(0)
        out, eout = engine.stream_emit_buffers(S, plan, 'cuda'), engine.stream_endpoint_buffers(S, eplan, 'cuda')

        def emit():
            state.copy_(saved)
            engine.stream_emit(state, S, plan, sl, fl, tok, fs, enc, first, sc.BLANK, out=out)

        def both():
            state.copy_(saved), ep.copy_(ep_saved)
            engine.stream_emit(state, S, plan, sl, fl, tok, fs, enc, first, sc.BLANK, out=out)
            engine.stream_endpoint(state, ep, S, plan, eplan, sl, fl, tok, fs, enc, first, out, sc.BLANK, out=eout)

        t_copy = _timed(a, lambda: state.copy_(saved))
        t_copy2 = _timed(a, lambda: (state.copy_(saved), ep.copy_(ep_saved)))
        t_emit = _timed(a, emit) - t_copy
        t_both = _timed(a, both) - t_copy2
        row = dict(streams=S, final_frames=48, k_stream_emit_us=round(t_emit, 1), k_stream_endpoint_us=round(t_both - t_emit, 1),
                   records=int(eout.n_records.sum().item()))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return dict(note='device events, median of rounds; launch overhead included on both sides', rows=rows)


def session(a):
    import torch

    import stream_cases as sc
    import stream_ep_cases as ec
    import test_gpu_stream_facade as plain
    from qasr import synth
    torch.set_grad_enabled(False)
    m = plain.model('static')
    rows = []
    for S in (1, 8, 32):
        audio = torch.from_numpy(synth.make_audio(S, 90000, seed=8)).cuda()
        row = dict(streams=S)
        for name, ep in (('plain', None), ('endpoint', ec.facade_endpointing())):
            m.reserve(None, None)
            with m.stream(max_streams=S, endpoint=ep, **sc.FACADE_KW) as sess:
                slots = [sess.open() for _ in range(S)]
                C, walls = sess.plan.C, []
                for k in range(90000 // C):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sess.push(slots, audio[:, k * C:(k + 1) * C])
                    torch.cuda.synchronize()
                    walls.append(time.perf_counter() - t0)
                    if ep is not None:
                        sess.take_utterances()
            walls = sorted(walls[4:])                                            # full windows only
            row[name + '_step_ms'] = round(1000.0 * walls[len(walls) // 2], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return dict(note='median host wall time of one push = one step of full windows, mini net, synchronised', rows=rows)


def bench(a):
    runs = {'this': [], 'parent': []}
    for _ in range(3):
        for name, tree in (('parent', a.bench), ('this', ROOT)):
            out = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1'], capture_output=True, text=True, cwd=tree,
                                 check=True).stdout
            runs[name].append(json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1]))
            print(name, runs[name][-1], flush=True)
    return runs


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--device', action='store_true')
    p.add_argument('--session', action='store_true')
    p.add_argument('--bench', default=None, metavar='PARENT_TREE')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    rec = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.device:
        rec['device'] = device(a)
    if a.session:
        rec['session'] = session(a)
    if a.bench:
        rec['bench'] = bench(a)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
