#!/usr/bin/env python3
"""Streaming phrase boosting (qasr.stream_beam with boost=, k_stream_beam_boost), measured.

  --device   (one GPU) k_stream_beam_boost<false/true> per launch against k_stream_beam<false/true> over the SAME candidates
             and the same warmed beams' frames: 1 / 8 / 32 streams x 48 final frames, W = 16 / 128, without a model and
             with the committed word 3-gram; sets of 10 / 1 000 / 10 000 phrases (words of the streams' own greedy text
             first, random words behind them) and set 0 (a boosted session's stream without a set).  Device events around
             --steps launches, the median of --rounds samples.  The yardstick is k_stream_beam in the same run; boosting is
             one more global look-up per live candidate, so the expectation is between it and k_stream_beam with a
             character model.  An expectation, not a gate.  Under a profiler (a run of its own, no counters):
             rocprofv3 --kernel-trace --stats -- python profiles/stream_boost.py --device
  --session  (one GPU) host wall time per session step (push of one chunk for every stream) of EncDecCTCModel.stream(beam=)
             with and without boost, 8 streams, the synthetic MiniQuartzNet on the static engine.
  --bench    bench.py --gpus 1 of this tree alternating with a checkout of the parent commit (--parent DIR), three runs
             each; no existing kernel changed, so the two should agree within the spread of the parent's own runs.

    python profiles/stream_boost.py --device --session --out profiles/stream_boost.json
    python profiles/stream_boost.py --bench --parent ../parent --out profiles/stream_boost.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests'), ROOT]

SET_SIZES = (10, 1000, 10000)


def phrase_set(lps, blank, space, n, seed=1):
    """n whole-word phrases: words of the streams' greedy text first (they match), random words of 3 .. 8 labels behind"""
    import numpy as np

    import beam_cases
    from qasr import boost as qboost
    rng = np.random.Generator(np.random.PCG64(seed))
    words = []
    for lp in lps:
        cur = []
        for c in beam_cases.greedy(lp, blank) + [space]:
            if c == space:
                if 2 <= len(cur) <= 64:
                    words.append(tuple(cur))
                cur = []
            else:
                cur.append(c)
    out = list(dict.fromkeys(words))[:max(n // 2, 1)]
    labels = [c for c in range(blank) if c != space]
    while len(out) < n:
        out.append(tuple(int(labels[i]) for i in rng.integers(0, len(labels), size=int(rng.integers(3, 9)))))
    return qboost.PhraseSet([(list(p), 1.5) for p in out[:n]], n_labels=blank, space=space, whole_words=True)


def device(a):
    import numpy as np
    import torch

    import boost_cases
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
        lps = [cases.lm_stream_logp('en3', 100 + s, 200 + Tw) for s in range(S)]
        blank = lps[0].shape[1] - 1
        cand = qb.topn_host(np.stack(lps), N)
        sets = {n: phrase_set(lps, blank, boost_cases.EN_SPACE, n) for n in SET_SIZES}
        for W in (16, 128):
            for model in (None, lm):
                kw = dict(lm=model, alpha=0.5, beta=0.5)
                blk = np.zeros((S, st.STATE_WORDS), np.int32)
                blk[:, 0:2].view(np.int64)[:, 0] = 10 ** 9
                sl = torch.arange(S, dtype=torch.int32, device='cuda')
                i32 = lambda v: torch.full((S,), v, dtype=torch.int32, device='cuda')      # noqa: E731
                ds = engine.stream_state(S, splan, 'cuda')

                def measure(call, state):
                    """warm the beams over 200 frames, then time the step over frames [200, 248) from the same stored state"""
                    blk[:, 2] = 0
                    for lo in range(0, 200, 40):
                        engine.stream_block(ds, S).copy_(torch.from_numpy(blk).cuda())
                        w = [torch.from_numpy(np.ascontiguousarray(c[:, lo:lo + Tw])).cuda() for c in cand]
                        call(i32(st.BEGIN if lo == 0 else 0), w, i32(40), i32(lo))
                        blk[:, 2] = lo + 40
                    engine.stream_block(ds, S).copy_(torch.from_numpy(blk).cuda())
                    saved = state.clone()
                    w = [torch.from_numpy(np.ascontiguousarray(c[:, 200:200 + Tw])).cuda() for c in cand]
                    fl, enc, first = i32(0), i32(48), i32(200)

                    def step():
                        state.copy_(saved)
                        call(fl, w, enc, first)
                    return timed(step) - timed(lambda: state.copy_(saved))

                pplan = sb.StreamBeamPlan(W, 1, N, F - sb.K_ROUND, splan.max_final_frames)
                pdb = engine.stream_beam_state(S, pplan, 'cuda')
                pout = engine.stream_beam_buffers(S, pplan, 'cuda', model is not None)
                t_plain = measure(lambda fl, w, enc, first: engine.stream_beam(ds, pdb, S, splan, pplan, sl, fl, w[0], w[1], enc, first,
                                                                               blank, out=pout, **kw), pdb)
                bplan = sb.StreamBeamPlan(W, 1, N, F - sb.K_ROUND, splan.max_final_frames, boost=True)
                bout = engine.stream_beam_boost_buffers(S, bplan, 'cuda', model is not None)
                row = dict(streams=S, W=W, model=model is not None, final_frames=48, k_stream_beam_us=round(t_plain, 1))
                for n in (0,) + SET_SIZES:
                    bs = sets[n or SET_SIZES[0]]
                    bdb = engine.stream_beam_boost_state(S, bplan, 'cuda')
                    blobs = [engine.boost_device(bs, 'cuda')]
                    bset = i32(-1 if n == 0 else 0)
                    t = measure(lambda fl, w, enc, first: engine.stream_beam_boost(ds, bdb, S, splan, bplan, sl, fl, w[0], w[1], enc, first,
                                                                                   blank, [bs], bset, out=bout, blobs=blobs, **kw), bdb)
                    row[f'k_stream_beam_boost_us_set{n}'] = round(t, 1)
                    row[f'ratio_set{n}'] = round(t / t_plain, 3)
                print(json.dumps(row), flush=True)
                res.append(row)
    return dict(note='device events, median of rounds; both kernels step frames [200, 248) from beams warmed over 200 frames; '
                     'set0: a stream of a boosted session without a set (no look-up)', rows=res)


def session(a):
    import torch

    import stream_cases as sc
    from nemo.collections.asr.models import EncDecCTCModel
    import nemo.quantization.utils.quantize_model as qm
    from qasr import stream_beam as sb, synth
    torch.set_grad_enabled(False)
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([96] * 4).cuda()
    for c in synth.make_calibration(3, 4, 16, 96, 2):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    S = 8
    audio = torch.from_numpy(synth.make_audio(S, 160000, seed=4)).cuda()
    rows = {}
    for name, boost in (('without_boost', None), ('with_boost', ['hello', 'world', ('the cat', 2.0)])):
        with m.stream(max_streams=S, beam=sb.StreamBeam(width=16, lag_s=1.0, boost=boost), **sc.FACADE_KW) as sess:
            slots = [sess.open() for _ in range(S)]
            C = sess.plan.C
            times = []
            for k in range(160000 // C):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sess.push(slots, audio[:, k * C:(k + 1) * C])
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            for s in slots:
                sess.close(s)
        steady = sorted(times[len(times) // 2:])
        rows[name] = dict(streams=S, steps=len(times), median_step_ms=round(1000 * steady[len(steady) // 2], 3))
        print(name, json.dumps(rows[name]), flush=True)
    return dict(note='host wall time of one push (one step for every stream), second half of the steps, median', rows=rows)


def bench(a):
    def run(root):
        out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(a.bench_steps), '--warmup',
                              str(a.bench_warmup)], capture_output=True, text=True, check=True, cwd=root)
        return json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    rows = dict(this=[], parent=[])
    for _ in range(3):                                   # alternating, so that drift hits both alike
        rows['parent'].append(run(a.parent))
        rows['this'].append(run(ROOT))
    return dict(note='bench.py --gpus 1, parent and this tree alternating, three runs each', rows=rows)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--device', action='store_true')
    p.add_argument('--session', action='store_true')
    p.add_argument('--bench', action='store_true')
    p.add_argument('--parent', default=None, help='a checkout of the parent commit, built (--bench)')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--bench_steps', type=int, default=20)
    p.add_argument('--bench_warmup', type=int, default=5)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if a.bench and not a.parent:
        p.error('--bench needs --parent DIR')
    rec = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    t0 = time.time()
    if a.device:
        rec['device'] = device(a)
    if a.session:
        rec['session'] = session(a)
    if a.bench:
        rec['bench'] = bench(a)
    print('seconds', round(time.time() - t0, 1))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
