#!/usr/bin/env python3
"""Streaming beam endpointing (qasr.stream_beam's STREAM_BEAM_EP_RULES, k_stream_beam_ep<LM, BOOST>), measured.

  --device   (one GPU) k_stream_beam_ep per launch at 1 / 8 / 32 streams x 48 final frames, W = 16 / 128, the four
             instantiations (without a model / with the committed word 3-gram, without sets / with one set of 1 000 phrases):
             on record-free steps against k_stream_beam / k_stream_beam_boost of the SAME build and run over the SAME
             candidates and the same warmed beams' frames, and with one and with two cuts inside the step.  Device events
             around --steps launches, the median of --rounds samples.  Expectation: a record-free step costs what the
             existing kernel costs (the addition is one read of n_records), a cut costs about one END pass.  An expectation,
             not a gate.  Under a profiler (a run of its own, no counters):
             rocprofv3 --kernel-trace --stats -- python profiles/stream_beam_ep.py --device
  --session  (one GPU) host wall time per session step (push of one chunk for every stream) of EncDecCTCModel.stream(beam=)
             with and without StreamBeam.endpoint, 8 streams, the synthetic MiniQuartzNet on the static engine.
  --bench    bench.py --gpus 1 of this tree alternating with a checkout of the parent commit (--parent DIR), three runs
             each, medians; no existing kernel changed, so the two should agree within the spread of the parent's own runs.

    python profiles/stream_beam_ep.py --device --session --out profiles/stream_beam_ep.json
    python profiles/stream_beam_ep.py --bench --parent ../parent --out profiles/stream_beam_ep.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests'), ROOT]


def phrase_set(lps, blank, space, n, seed=1):
    """n whole-word phrases: words of the streams' greedy text first (they match), random words of 3 .. 8 labels behind"""
    import numpy as np

    import beam_cases
    from qasr import boost as qboost
    rng = np.random.Generator(np.random.PCG64(seed))
    words = []
    for lp in lps:
        cur = []
        for c in list(beam_cases.greedy(lp, blank)) + [space]:
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
    from qasr import beam as qb, engine, stream as st, stream_beam as sb, stream_ep as se
    lm = cases.load_lm(cases.GOLDEN, 'en3')
    splan = sc.plan_frames(48, 5, 1)
    Tw, F, N, E = splan.Tw, 232, 40, 2
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

    def records(S, ends, first_index=0):
        rec = np.zeros((S, E, se.REC_WORDS), np.int32)
        for k, e in enumerate(ends):
            rec[:, k] = se._record(first_index + k, 0, e, 0, 0, 0, se.HARD, np.float32(0), 0)
        i32 = lambda v: torch.full((S,), v, dtype=torch.int32, device='cuda')      # noqa: E731
        return se.EpStepBatch(torch.from_numpy(rec).cuda(), i32(len(ends)), i32(0))

    for S in (1, 8, 32):
        lps = [cases.lm_stream_logp('en3', 100 + s, 200 + Tw) for s in range(S)]
        blank = lps[0].shape[1] - 1
        cand = qb.topn_host(np.stack(lps), N)
        bs = phrase_set(lps, blank, boost_cases.EN_SPACE, 1000)
        for W in (16, 128):
            for model in (None, lm):
                for boosted in (False, True):
                    kw = dict(lm=model, alpha=0.5, beta=0.5)
                    blk = np.zeros((S, st.STATE_WORDS), np.int32)
                    blk[:, 0:2].view(np.int64)[:, 0] = 10 ** 9
                    sl = torch.arange(S, dtype=torch.int32, device='cuda')
                    i32 = lambda v: torch.full((S,), v, dtype=torch.int32, device='cuda')      # noqa: E731
                    ds = engine.stream_state(S, splan, 'cuda')
                    plan = sb.StreamBeamPlan(W, 1, N, F - sb.K_ROUND, splan.max_final_frames, boost=boosted)
                    sets, blobs, bset = ([bs], [engine.boost_device(bs, 'cuda')], i32(0)) if boosted else (None, None, None)
                    new_state = engine.stream_beam_boost_state if boosted else engine.stream_beam_state

                    def set_done(v):
                        blk[:, 2] = v
                        engine.stream_block(ds, S).copy_(torch.from_numpy(blk).cuda())

                    def old_call(state, out):
                        if boosted:
                            return lambda fl, w, enc, first: engine.stream_beam_boost(ds, state, S, splan, plan, sl, fl, w[0], w[1], enc, first,
                                                                                      blank, sets, bset, out=out, blobs=blobs, **kw)
                        return lambda fl, w, enc, first: engine.stream_beam(ds, state, S, splan, plan, sl, fl, w[0], w[1], enc, first, blank,
                                                                            out=out, **kw)

                    def ep_call(state, out, ep):
                        return lambda fl, w, enc, first: engine.stream_beam_ep(ds, state, S, splan, plan, sl, fl, w[0], w[1], enc, first, blank,
                                                                               ep, sets, bset, out=out, blobs=blobs, **kw)

                    def measure(kind, ends=()):
                        """warm the beams over 200 frames with the kernel under test, then time its step over the frames
                        [200, 248) from the same stored state; the stream block says what each kernel expects of it
                        (frames_done before emit for the existing kernels, after emit for the new one)"""
                        state = new_state(S, plan, 'cuda')
                        if kind == 'old':
                            out = (engine.stream_beam_boost_buffers if boosted else engine.stream_beam_buffers)(S, plan, 'cuda', model is not None)
                            warm = call = old_call(state, out)
                        else:
                            out = engine.stream_beam_ep_buffers(S, plan, E, 'cuda', model is not None)
                            warm, call = ep_call(state, out, records(S, ())), ep_call(state, out, records(S, ends))
                        for lo in range(0, 200, 40):
                            set_done(lo if kind == 'old' else lo + 40)
                            w = [torch.from_numpy(np.ascontiguousarray(c[:, lo:lo + Tw])).cuda() for c in cand]
                            warm(i32(st.BEGIN if lo == 0 else 0), w, i32(40), i32(lo))
                        set_done(200 if kind == 'old' else 248)
                        saved = state.clone()
                        w = [torch.from_numpy(np.ascontiguousarray(c[:, 200:200 + Tw])).cuda() for c in cand]
                        fl, enc, first = i32(0), i32(48), i32(200)

                        def step():
                            state.copy_(saved)
                            call(fl, w, enc, first)
                        return timed(step) - timed(lambda: state.copy_(saved))

                    t_old = measure('old')
                    row = dict(streams=S, W=W, model=model is not None, boosted=boosted, final_frames=48,
                               existing_kernel='k_stream_beam_boost' if boosted else 'k_stream_beam', existing_us=round(t_old, 1))
                    for name, ends in (('no_record', ()), ('one_cut', (224,)), ('two_cuts', (216, 240))):
                        t = measure('ep', ends)
                        row[f'k_stream_beam_ep_us_{name}'] = round(t, 1)
                        row[f'ratio_{name}'] = round(t / t_old, 3)
                    print(json.dumps(row), flush=True)
                    res.append(row)
    return dict(note='device events, median of rounds; every kernel steps frames [200, 248) from beams warmed over 200 frames; '
                     'cuts at frame 224, or at 216 and 240', rows=res)


def session(a):
    import torch

    import stream_cases as sc
    from nemo.collections.asr.models import EncDecCTCModel
    import nemo.quantization.utils.quantize_model as qm
    from qasr import stream_beam as sb, stream_ep as se, synth
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
    for name, ep in (('without_endpoint', None), ('with_endpoint', se.Endpointing(0.04, 0.2, 0.5, 0.6))):
        with m.stream(max_streams=S, beam=sb.StreamBeam(width=16, lag_s=1.0, endpoint=ep), **sc.FACADE_KW) as sess:
            slots = [sess.open() for _ in range(S)]
            C = sess.plan.C
            times, n_utts = [], 0
            for k in range(160000 // C):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sess.push(slots, audio[:, k * C:(k + 1) * C])
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                n_utts += len(sess.take_utterances()) if ep is not None else 0
            for s in slots:
                sess.close(s)
        steady = sorted(times[len(times) // 2:])
        rows[name] = dict(streams=S, steps=len(times), utterances=n_utts, median_step_ms=round(1000 * steady[len(steady) // 2], 3))
        print(name, json.dumps(rows[name]), flush=True)
    return dict(note='host wall time of one push (one step for every stream), second half of the steps, median', rows=rows)


def bench(a):
    def run(root):
        out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(a.bench_steps), '--warmup',
                              str(a.bench_warmup)], capture_output=True, text=True, check=True, cwd=root)
        rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
        return dict(ms_per_step=rec['ms_per_step'], value=rec['value'])      # RTFx; the rest of bench.py's line is its own configuration
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
