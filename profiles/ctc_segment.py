#!/usr/bin/env python3
"""CTC segmentation of long recordings, measured on one GPU.

  kernel   k_align_band per launch and per frame for each band width (256, 1024, 4352 states) at 1 and 32 recordings of
           --frames synthetic frames (an hour: 180 000; 29 classes; the posteriors of tests/align_band_cases.py: the true class's
           logit raised by 4, unit Gaussian noise; 0.3 labels per frame): device events around --steps launches on one stream,
           --rounds samples.  The back-walk's share: the same launch with 300 labels appended that have no audio - the band ends
           short of the final state, so the frame loop runs whole and no back-walk follows - taken from the full time.
  twin     qasr.align.align_band_host on a row of --twin-frames frames at 1024 states, host seconds: context, not a bar
  e2e      EncDecCTCModel.align_long on --seconds of synthetic audio through full-size QuartzNet15x5Base-En (synthetic
           weights, calibrated) at the defaults, the transcript = decode_long's greedy text cut into utterances of 40 labels;
           wall seconds, and the reserved engine's allocation and graph counters around the timed calls
  bench    `bench.py --gpus 1` on this build and on a build of the parent commit (QASR_LIB), fresh processes alternating this /
           parent, --bench-runs each, each under its own time limit, stopping at the first one that fails

    python profiles/ctc_segment.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_segment.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
C_ = 29


def _posteriors(T, seed, extra=0):
    """(logp cuda float32 [1, T, C], labels list): about 0.3 labels per frame, each 1 .. 3 frames with 0 .. 4 blanks behind"""
    import numpy as np
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    y, frames = [], []
    while len(frames) < T - 8:
        c = int(rng.integers(0, C_ - 1))
        if y and c == y[-1]:
            c = (c + 1) % (C_ - 1)
        y.append(c)
        frames += [c] * int(rng.integers(1, 4)) + [C_ - 1] * int(rng.integers(0, 5))
    frames = (frames + [C_ - 1] * T)[:T]
    z = torch.randn(T, C_, generator=torch.Generator().manual_seed(seed)).cuda()
    z[torch.arange(T).cuda(), torch.tensor(frames).cuda()] += 4.0
    return torch.log_softmax(z, dim=-1)[None].contiguous(), y + [int(rng.integers(0, C_ - 1)) for _ in range(extra)]


def child_kernel(a):
    import numpy as np
    import torch

    from qasr import align, engine
    if not torch.cuda.is_available():
        sys.exit('ctc_segment.py measures on the GPU; no GPU found')

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

    T = a.frames
    logp1, y = _posteriors(T, 1)
    kern, info = {}, {}
    for P in (1, 32):
        logp = logp1.expand(P, T, C_).contiguous()
        for bw in align.BAND_STATES:
            ws = torch.empty(engine.ctc_align_band_workspace_bytes(P, T, bw), dtype=torch.uint8, device='cuda')
            for tag, rows in (('', y), ('_no_backwalk', y + [(c + 1) % (C_ - 1) for c in y[-300:]])):
                tg = torch.tensor([rows] * P, dtype=torch.int32).cuda()
                tl = torch.full((P,), len(rows), dtype=torch.int32).cuda()
                buf = {}

                def run():
                    buf['o'] = engine.ctc_align_band(logp, None, tg, tl, C_ - 1, band_states=bw, workspace=ws, out=buf.get('o'))
                kern[f'k_align_band_p{P}_bw{bw}{tag}_us'] = timed(run)
                info[f'p{P}_bw{bw}{tag}'] = dict(ok=int(buf['o'].ok.sum()), labels=len(rows), workspace_bytes=int(ws.numel()),
                                                 last_base=int(buf['o'].band_base[0].max()))
            del ws
        del logp
    # the twin on a shorter row, and the kernel against it
    Tt = a.twin_frames
    lp, yt = _posteriors(Tt, 2)
    tg, tl = np.array([yt], dtype=np.int32), np.array([len(yt)], dtype=np.int32)
    t0 = time.perf_counter()
    twin = align.align_band_host(lp.cpu().numpy(), None, tg, tl, C_ - 1, band_states=1024)
    twin_s = time.perf_counter() - t0
    got = engine.ctc_align_band(lp, None, torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), C_ - 1, band_states=1024)
    equal = all(np.array_equal(getattr(got, f).cpu().numpy().view(np.int32), getattr(twin, f).view(np.int32))
                for f in ('start', 'nframes', 'score', 'frame_logp', 'band_base', 'ok')) and \
        np.array_equal(got.path_score.cpu().numpy(), twin.path_score)
    print('CTC_SEGMENT_CHILD ' + json.dumps(dict(frames=T, labels=len(y), classes=C_, kernels_us=kern, cases=info, twin_frames=Tt,
                                                 twin_labels=len(yt), twin_host_s=twin_s, equals_twin=bool(equal))), flush=True)


def child_e2e(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit('ctc_segment.py measures on the GPU; no GPU found')
    import longform as lf_profile                       # profiles/longform.py: the model and the audio of the decode_long record
    m = lf_profile._model()
    audio, lens = lf_profile._audio(a.seconds)
    plan = m._long_plan(lens.cpu().numpy())
    head, head_len = audio[:, :plan.Wl * 8].contiguous(), torch.tensor([plan.Wl * 8]).cuda()
    ids = m.decode_long(audio, lens)[0].labels
    utts = [ids[i:i + 40] for i in range(0, len(ids), 40)]
    m.align_long(head, head_len, labels=[ids[:200]])       # builds and reserves the engine with log-probabilities
    s0 = m._ragged_engine.ragged_stats()
    walls = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hyp = m.align_long(audio, lens, labels=[utts])[0]
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    s1 = m._ragged_engine.ragged_stats()
    rec = dict(seconds=a.seconds, windows=plan.Wn, stitched_frames=plan.Tmax, labels=len(hyp.labels), utterances=len(utts),
               aligned=bool(hyp.start_s), align_long_s=walls, stats_after_first_call=s0, stats_at_end=s1,
               device_allocs_after_first_call=s1['device_allocs'] - s0['device_allocs'],
               torch_max_memory_allocated=torch.cuda.max_memory_allocated())
    print('CTC_SEGMENT_CHILD ' + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['kernel', 'e2e'], default=None)
    ap.add_argument('--frames', type=int, default=180000)
    ap.add_argument('--twin-frames', type=int, default=9000)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--steps', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--child-timeout', type=int, default=500)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (bench.py A/B)')
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: kernel, e2e')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.join(ROOT, 'profiles'))
        return child_kernel(a) if a.child == 'kernel' else child_e2e(a)
    import numpy as np
    res = dict(note='kernel times: device events around `steps` launches on one stream (microseconds per launch); synthetic '
                    'posteriors and synthetic random weights, not speech')
    for stage in ('kernel', 'e2e'):
        if stage in a.skip.split(','):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), '--child', stage, '--frames', str(a.frames), '--twin-frames',
               str(a.twin_frames), '--seconds', str(a.seconds), '--repeats', str(a.repeats), '--steps', str(a.steps),
               '--rounds', str(a.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f'child {stage} ran past {a.child_timeout} s: stopping')
        line = [l for l in p.stdout.splitlines() if l.startswith('CTC_SEGMENT_CHILD ')]
        if p.returncode or not line:
            sys.exit(f'child {stage} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
        r = json.loads(line[0][len('CTC_SEGMENT_CHILD '):])
        if stage == 'kernel':
            s = {}
            for k, v in r['kernels_us'].items():
                s[k] = dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v),
                            per_frame=float(np.median(v)) / r['frames'])
            for k in [k for k in s if k.endswith('_no_backwalk_us')]:
                full = s[k.replace('_no_backwalk', '')]['median']
                s[k.replace('_no_backwalk_us', '_backwalk_share')] = (full - s[k]['median']) / full
            r['summary'] = s
        res[stage] = r
        print(stage, json.dumps(r.get('summary', r)), flush=True)
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        bench = dict(note='`bench.py --gpus 1` in the same session, fresh processes alternating this build / the parent commit\'s '
                          'library (QASR_LIB)', this=[], parent=[])
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
        res['bench'] = bench
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
