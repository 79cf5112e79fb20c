#!/usr/bin/env python3
"""Streaming keyword spotting (k_stream_spot), measured on one GPU.

  kernel   k_stream_spot per step at 1 / 8 / 32 streams x 10 / 100 / 1000 keywords of 8 labels, on En (29 classes) and Zh (5207)
           widths, over the max_final_frames frames that a step of the default plan (0.96 / 4.0 / 0.96 s) makes final, every
           block carrying a lattice row from an earlier step (so the load is paid).  Against k_spot of the same build over the
           same final frames only: the comparison that isolates the state round trip and the per-frame ballot.  Device events
           around every single launch (the spot state is put back before each), summed over --steps, medians of --rounds
           alternating rounds.
  session  host wall time per step of a session on the static engine, 8 streams, with and without spot= (100 keywords).
  kspot    k_spot<1 / 2 / 4> (keywords of 8 labels at a row pitch of 8 / 40 / 100) on the inputs of profiles/ctc_spot.py at
           32 x 500 frames, 100 keywords, this build against a build of the parent commit (QASR_LIB), fresh processes
           alternating: the header move of the frame step is kept only if the two agree within the spread of the parent's runs.
  bench    `bench.py --gpus 1`, fresh processes alternating this build / the parent's, --ab-runs each.
Each child process runs under its own time limit, and the script stops at the first one that fails.

    python profiles/stream_spot.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/stream_spot.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT, os.path.join(ROOT, 'profiles')]
SHAPES = (('en', 29), ('zh', 5207))
STREAMS = (1, 8, 32)
KEYWORDS = (10, 100, 1000)
LABELS = 8
TAG = 'STREAM_SPOT_CHILD '
SPOT = dict(threshold=-1.0, max_span=500)


def _timed(torch, prepare, fn, steps):
    """microseconds per launch: events around every launch on its own, `prepare` in between and outside the events"""
    pairs = []
    for _ in range(steps):
        prepare()
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        pairs.append((s, t))
    torch.cuda.synchronize()
    return sum(s.elapsed_time(t) for s, t in pairs) / steps * 1e3


def child_kernel(a):
    import numpy as np
    import torch

    import ctc_spot as offline
    from qasr import engine, spot, stream as st, stream_spot as ss
    plan = st.StreamPlan()
    nf, Tw = plan.max_final_frames, plan.Tw
    out = dict(max_final_frames=nf, Tw=Tw)
    for name, C_ in SHAPES:
        for S in STREAMS:
            logp, own = offline._logp(torch, S, Tw, C_, 1)
            enc = torch.full((S,), Tw, dtype=torch.int32, device='cuda')
            plane = engine.ctc_star(logp, enc, 0.0)
            for K in KEYWORDS:
                tg, tl = offline._keywords(torch, own, K, K)
                splan = ss.StreamSpotPlan(plan, tg.cpu().numpy(), tl.cpu().numpy(), spot.check_threshold(SPOT['threshold'], 'p'), SPOT['max_span'])
                state = engine.stream_state(S, plan, 'cuda')
                sp = engine.stream_spot_state(S, splan, 'cuda')
                sl = torch.arange(S, dtype=torch.int32, device='cuda')
                zero = torch.zeros(S, dtype=torch.int32, device='cuda')
                buf = engine.stream_spot_buffers(S, splan, 'cuda')
                blocks = engine.stream_block(state, S)

                def step(flags, done):
                    blocks[:, st._W_DONE] = done
                    engine.stream_spot(state, sp, S, plan, splan, sl, flags, logp, plane, enc, zero, zero, C_ - 1, keywords=(tg, tl), out=buf)
                step(torch.full_like(zero, st.BEGIN), nf)             # an earlier step: every block now carries a row
                blocks[:, st._W_DONE] = 2 * nf
                first = torch.full_like(zero, nf)                     # the window begins where the earlier step ended
                sp0 = sp.clone()
                res = {}

                def run_stream():
                    engine.stream_spot(state, sp, S, plan, splan, sl, zero, logp, plane, enc, first, zero, C_ - 1, keywords=(tg, tl), out=buf)

                def run_offline():
                    res['s'] = engine.ctc_spot(logp[:, :nf], None, plane[:, :nf], tg, tl, C_ - 1, SPOT['threshold'], SPOT['max_span'],
                                               splan.hit_pitch, out=res.get('s'))
                fns = dict(k_stream_spot_us=run_stream, k_spot_same_frames_us=run_offline)
                for fn in fns.values():
                    sp.copy_(sp0)
                    fn()
                torch.cuda.synchronize()
                assert int(buf.status.max()) == 0 and int(buf.ok.min()) == 1
                rec = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for k, fn in fns.items():
                        rec[k].append(_timed(torch, lambda: sp.copy_(sp0), fn, a.steps))
                rec.update(S=S, K=K, C=C_, frames=nf, state_bytes_per_problem=4 * splan.block_words, hits=int(buf.n_new_hits.sum()))
                out[f'{name}_S{S}_K{K}'] = rec
    print(TAG + json.dumps(out), flush=True)


def child_kspot(a):
    import torch

    import ctc_spot as offline
    from qasr import engine
    out = {}
    logp, own = offline._logp(torch, 32, 500, 29, 1)
    plane = engine.ctc_star(logp, None, 0.0)
    for pitch in (8, 40, 100):                                       # k_spot<1>, <2>, <4>
        tg8, tl = offline._keywords(torch, own, 100, 100)
        tg = torch.full((100, pitch), 28, dtype=torch.int32, device='cuda')
        tg[:, :LABELS] = tg8
        buf = {}

        def run():
            buf['s'] = engine.ctc_spot(logp, None, plane, tg, tl, 28, -1.0, 500, 16, out=buf.get('s'))
        run()
        torch.cuda.synchronize()
        out[f'pitch{pitch}'] = [offline._round(torch, run, a.steps) for _ in range(a.rounds)]
    print(TAG + json.dumps(out), flush=True)


def child_session(a):
    import torch

    from nemo.collections.asr.models import EncDecCTCModel
    import nemo.quantization.utils.quantize_model as qm
    from qasr import stream_spot as ss, synth
    torch.set_grad_enabled(False)
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En').cuda()
    m.preprocessor.featurizer.dither = 0.0
    m.eval()
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([96] * 4).cuda()
    for c in synth.make_calibration(3, 4, 64, 96, 0):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    S, n_steps = 8, 12
    g = torch.Generator().manual_seed(3)
    labels = [torch.randint(0, 28, (LABELS,), generator=g).tolist() for _ in range(100)]
    out = {}
    for tag, sp in (('without', None), ('with_spot', ss.StreamSpot(labels=labels))):
        with m.stream(max_streams=S, tail=False, spot=sp) as sess:
            slots = [sess.open() for _ in range(S)]
            x = 0.1 * torch.randn(S, sess.plan.C, generator=g).cuda()
            ts = []
            for k in range(n_steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sess.push(slots, x)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[tag + '_ms_per_step'] = ts[2:]
            out['served'] = type(getattr(m, '_ragged_engine', None) or getattr(m, '_engine', None)).__name__
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
    ap.add_argument('--child', choices=['kernel', 'kspot', 'session'], default=None)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (the A/B of k_spot and of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: kernel, session, kspot, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return dict(kernel=child_kernel, kspot=child_kspot, session=child_session)[a.child](a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='microseconds per launch, device events around single launches, medians over alternating rounds; synthetic '
                    'posteriors, not speech')

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')

    if 'kernel' not in skip:
        r = _child(a, 'kernel')
        for k, v in r.items():
            if not isinstance(v, dict):
                continue
            v['k_stream_spot_median_us'], v['k_spot_median_us'] = med(v['k_stream_spot_us']), med(v['k_spot_same_frames_us'])
            v['ratio'] = v['k_stream_spot_median_us'] / v['k_spot_median_us']
            print('kernel', k, json.dumps({x: v[x] for x in ('frames', 'k_stream_spot_median_us', 'k_spot_median_us', 'ratio')}), flush=True)
        res['kernel'] = r
        save()
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    if a.parent_lib and 'kspot' not in skip:
        ab = dict(this=[], parent=[])
        for r in range(a.ab_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib))[::1 if r % 2 == 0 else -1]:
                ab[tag].append({k: med(v) for k, v in _child(a, 'kspot', lib).items()})
                print(f'kspot {tag} run {r}: ' + json.dumps(ab[tag][-1]), flush=True)
        res['k_spot_ab'] = ab
        save()
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

    if 'session' not in skip:
        r = _child(a, 'session')
        r['without_median_ms'], r['with_spot_median_ms'] = med(r['without_ms_per_step']), med(r['with_spot_ms_per_step'])
        print('session', json.dumps({k: r[k] for k in ('without_median_ms', 'with_spot_median_ms', 'served')}), flush=True)
        res['session'] = r
        save()

if __name__ == '__main__':
    main()
