#!/usr/bin/env python3
"""The streaming beam search (qasr.stream_beam, k_stream_beam), measured.

  --agreement  (CPU, the NumPy twin, the committed case lists of tests/beam_cases.py) for commit lags of 25 / 50 / 100 / 200
               frames, rounds every 32 frames: the share of utterances whose best string equals the offline search's
               (qasr.beam.beam_search_host over the same candidates) and the largest difference of the best scores.  A
               description of these synthetic lists - a competing class on every frame, denser than speech - not a gate
               and not a claim about speech.
  --device     (one GPU) k_stream_beam per launch at 1 / 8 / 32 streams x 48 final frames, W = 16 / 128, without a model
               and with the committed word 3-gram, against k_beam / k_beam_lm over the same 48 frames: device events around
               --steps launches, the median of --rounds samples.  The margin over the offline kernels is the state load /
               store and one or two rounds.  Under a profiler: rocprofv3 --kernel-trace --stats -- python
               profiles/stream_beam.py --device, in a run of its own.

    python profiles/stream_beam.py --agreement --out profiles/stream_beam.json
    python profiles/stream_beam.py --device --out profiles/stream_beam.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests'), ROOT]

LISTS = ('en_t250_w16_n20', 'en_t1000_w16_n20', 'zh_t250_w16_n20_blend', 'en_t250_w128_n20')
LAGS = (25, 50, 100, 200)


def agreement(a):
    import beam_cases
    from qasr import beam as qb, stream_beam as sb
    out = {}
    for name in LISTS:
        rows = {str(lag): dict(equal=0, of=0, max_score_diff=0.0) for lag in LAGS}
        for lp, blank, W, N in beam_cases.case_list(name):
            cid, cq = qb.topn_host(lp[None], N)
            off = qb.beam_search_host(cid, cq, None, blank, W, 1)
            best = off.labels[0, 0, :off.n_labels[0, 0]].tolist()
            for lag in LAGS:
                r = sb.lagged_search_host(cid[0], cq[0], lp.shape[0], blank, W, 1, lag=lag, check=False)
                row = rows[str(lag)]
                row['of'] += 1
                row['equal'] += int(r.hyps[0][0] == best)
                row['max_score_diff'] = max(row['max_score_diff'], abs(r.hyps[0][1] - int(off.score[0, 0])) / qb.ONE)
        out[name] = rows
        print(name, json.dumps(rows), flush=True)
    return dict(rounds_every=sb.K_ROUND, lags_frames=list(LAGS), lists=out,
                note='share of best strings equal to the offline search, NumPy twin, synthetic lists; not a gate')


def device(a):
    import numpy as np
    import torch

    import stream_beam_cases as cases
    import stream_cases as sc
    from qasr import beam as qb, engine, stream as st, stream_beam as sb
    lm = cases.load_lm(cases.GOLDEN, 'en3')
    splan = sc.plan_frames(48, 5, 1)
    Tw, F, N = splan.Tw, 232, 40
    res = []

    def timed(fn):
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

    for S in (1, 8, 32):
        for W in (16, 128):
            for model in (None, lm):
                lps = [cases.lm_stream_logp('en3', 100 + s, 200 + Tw) for s in range(S)]
                blank = lps[0].shape[1] - 1
                cand = qb.topn_host(np.stack(lps), N)
                bplan = sb.StreamBeamPlan(W, 1, N, F - sb.K_ROUND, splan.max_final_frames)
                ds, db = engine.stream_state(S, splan, 'cuda'), engine.stream_beam_state(S, bplan, 'cuda')
                blk = np.zeros((S, st.STATE_WORDS), np.int32)
                blk[:, 0:2].view(np.int64)[:, 0] = 10 ** 9
                sl = torch.arange(S, dtype=torch.int32, device='cuda')
                i32 = lambda v: torch.full((S,), v, dtype=torch.int32, device='cuda')      # noqa: E731
                out = engine.stream_beam_buffers(S, bplan, 'cuda', model is not None)
                kw = dict(lm=model, alpha=0.5, beta=0.5)
                # warm the beams over 200 frames, then time the step over frames [200, 248) from the same stored state
                done = 0
                for lo in range(0, 200, 40):
                    engine.stream_block(ds, S).copy_(torch.from_numpy(blk).cuda())
                    w = [torch.from_numpy(np.ascontiguousarray(c[:, lo:lo + Tw])).cuda() for c in cand]
                    engine.stream_beam(ds, db, S, splan, bplan, sl, i32(st.BEGIN if lo == 0 else 0), w[0], w[1], i32(40), i32(lo), blank, out=out, **kw)
                    done = lo + 40
                    blk[:, 2] = done
                engine.stream_block(ds, S).copy_(torch.from_numpy(blk).cuda())
                saved = db.clone()
                w = [torch.from_numpy(np.ascontiguousarray(c[:, 200:200 + Tw])).cuda() for c in cand]
                fl, enc, first = i32(0), i32(48), i32(200)

                def step():
                    db.copy_(saved)
                    engine.stream_beam(ds, db, S, splan, bplan, sl, fl, w[0], w[1], enc, first, blank, out=out, **kw)

                t_copy = timed(lambda: db.copy_(saved))
                t_stream = timed(step) - t_copy
                c48 = [torch.from_numpy(np.ascontiguousarray(c[:, 200:248])).cuda() for c in cand]
                ws = torch.empty(max(engine.ctc_beam_workspace_bytes(S, 48, W), 8), dtype=torch.uint8, device='cuda')
                t_off = timed(lambda: engine.ctc_beam(c48[0], c48[1], None, blank, W, 1, workspace=ws, **kw))
                row = dict(streams=S, W=W, model=model is not None, final_frames=48, k_stream_beam_us=round(t_stream, 1),
                           offline_kernel_us=round(t_off, 1), ratio=round(t_stream / t_off, 3))
                print(json.dumps(row), flush=True)
                res.append(row)
    return dict(note='device events, median of rounds; the offline kernel starts from an empty beam, the streaming one '
                     'from the beam after 200 frames, so the ratio also carries the fuller beam', rows=res)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--agreement', action='store_true')
    p.add_argument('--device', action='store_true')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    rec = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    t0 = time.time()
    if a.agreement:
        rec['agreement'] = agreement(a)
    if a.device:
        rec['device'] = device(a)
    print('seconds', round(time.time() - t0, 1))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
