#!/usr/bin/env python3
"""decode_long on one hour of audio, measured on one GPU: full-size QuartzNet15x5Base-En (synthetic weights, calibrated), one
recording of --seconds of synthetic 16 kHz audio, the defaults of decode_long (30 s windows, 4 s overlap, 1 s guard, batches
of 32).

  long     wall time of decode_long (device synchronised before and after; the first call builds and reserves the engine and
           is reported apart from the --repeats calls that follow), windows and batches, and the reserved engine's counters
           after the first batch's worth of work and at the end: graphs captured, replays, device allocations.
  stages   the per-stage split (cut, forwards, stitch, collapse) needs a rocprofv3 run of its own:
             rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o longform -- python profiles/longform.py --child long
           then --stats-csv <the kernel_stats.csv it wrote> folds the table into the four stages.
  whole    (--whole) the same recording through plain decode() as ONE row, in a process of its own under a time limit, on the
           library --parent-lib names (the parent commit's; no path of it changed here): its wall time, or the fact that it
           did not fit.
  bench    `bench.py --gpus 1` on this build and on a build of the parent commit (QASR_LIB), fresh processes alternating this /
           parent, --bench-runs each, each under its own time limit, stopping at the first one that fails.

    python profiles/longform.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/longform.json
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
STAGES = (('cut', ('k_cut',)), ('stitch', ('k_stitch',)), ('collapse', ('k_ctc',)))


def _model():
    import torch

    import nemo.quantization.utils.quantize_model as qm
    from nemo.collections.asr.models import EncDecCTCModel
    from qasr import synth
    torch.set_grad_enabled(False)
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En').cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    length = torch.tensor([500] * 4).cuda()
    for c in synth.make_calibration(2, 4, 64, 500):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=length)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    return m


def _audio(seconds):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    S = int(seconds * 16000)
    return torch.from_numpy(rng.uniform(-0.5, 0.5, (1, S)).astype(np.float32)).cuda(), torch.tensor([S]).cuda()


def child_long(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit('longform.py measures on the GPU; no GPU found')
    m = _model()
    audio, lens = _audio(a.seconds)
    plan = m._long_plan(lens.cpu().numpy())
    head, head_len = audio[:, :plan.Wl * 8].contiguous(), torch.tensor([plan.Wl * 8]).cuda()

    def run(x, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hyps = m.decode_long(x, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, hyps

    first_s, _ = run(head, head_len)                       # builds and reserves the engine; a few batches
    s0 = m._ragged_engine.ragged_stats()
    walls = []
    for _ in range(a.repeats):
        w, hyps = run(audio, lens)
        walls.append(w)
    s1 = m._ragged_engine.ragged_stats()
    mem = torch.cuda.max_memory_allocated()
    rec = dict(seconds=a.seconds, windows=plan.Wn, batches=-(-plan.Wn // 32), window_frames=plan.window_frames,
               stitched_frames=plan.Tmax, first_call_8_windows_s=first_s, decode_long_s=walls, labels=len(hyps[0].labels),
               seams=len(hyps[0].seams_s or []), stats_after_first_call=s0, stats_at_end=s1,
               device_allocs_after_first_call=s1['device_allocs'] - s0['device_allocs'], torch_max_memory_allocated=mem)
    print('LONGFORM_CHILD ' + json.dumps(rec), flush=True)


def child_whole(a):
    import torch
    m = _model()
    audio, lens = _audio(a.seconds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hyps = m.decode(input_signal=audio, input_signal_length=lens)
    torch.cuda.synchronize()
    print('LONGFORM_CHILD ' + json.dumps(dict(seconds=a.seconds, decode_one_row_s=time.perf_counter() - t0, labels=len(hyps[0].labels),
                                              torch_max_memory_allocated=torch.cuda.max_memory_allocated())), flush=True)


def fold_stats(path):
    """the kernel table of rocprofv3 --stats folded into cut / forwards / stitch / collapse (nanoseconds, calls)"""
    out = {k: dict(ns=0, calls=0, kernels=[]) for k in ('cut', 'forwards', 'stitch', 'collapse')}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name']
            stage = next((s for s, keys in STAGES if any(f'::{k}(' in name or name.startswith(k + '(') for k in keys)), 'forwards')
            out[stage]['ns'] += int(row['TotalDurationNs'])
            out[stage]['calls'] += int(row['Calls'])
            out[stage]['kernels'].append(name.split('(')[0])
    for v in out.values():
        v['kernels'] = sorted(set(v['kernels']))[:12]
    return out


def _child(args, timeout, env=None):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        return None, f'ran past {timeout} s'
    line = [l for l in p.stdout.splitlines() if l.startswith('LONGFORM_CHILD ')]
    if p.returncode or not line:
        return None, f'rc {p.returncode}: {p.stderr[-800:]}'
    return json.loads(line[0][len('LONGFORM_CHILD '):]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['long', 'whole'], default=None)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--child-timeout', type=int, default=420)
    ap.add_argument('--whole', action='store_true')
    ap.add_argument('--stats-csv', default=None, help='kernel_stats.csv of a rocprofv3 run of `--child long`')
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (bench.py A/B, --whole)')
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_long(a) if a.child == 'long' else child_whole(a)
    import numpy as np
    common = ['--seconds', str(a.seconds), '--repeats', str(a.repeats)]
    long_rec, why = _child(['--child', 'long'] + common, a.child_timeout)
    if long_rec is None:
        sys.exit(f'the decode_long child failed ({why}): stopping')
    print(json.dumps(long_rec), flush=True)
    res = dict(note='QuartzNet15x5Base-En, synthetic weights and audio, decode_long at its defaults (30 s / 4 s / 1 s, batches of 32); '
                    'wall seconds with the device synchronised before and after', long=long_rec)
    res['long']['decode_long_median_s'] = float(np.median(long_rec['decode_long_s']))
    res['long']['rtfx'] = a.seconds / res['long']['decode_long_median_s']
    if a.stats_csv:
        res['stages'] = dict(note='rocprofv3 --kernel-trace --stats of `--child long` in a run of its own: device time per stage over '
                                  'that whole run (the first call of 8 windows and the repeats)', **fold_stats(a.stats_csv))
    if a.whole:
        env = dict(os.environ, QASR_LIB=os.path.abspath(a.parent_lib)) if a.parent_lib else None
        whole, why = _child(['--child', 'whole'] + common, a.child_timeout, env)
        res['whole_file_decode'] = whole if whole is not None else dict(fits=False, why=why)
        print(json.dumps(res['whole_file_decode']), flush=True)
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        bench = dict(note='`bench.py --gpus 1` in the same session, fresh processes alternating this build / the parent '
                          'commit\'s library (QASR_LIB)', this=[], parent=[])
        for k in range(a.bench_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib)):
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
                print(f'bench {tag} run {k}: ' + json.dumps(bench[tag][-1]), flush=True)
        bench['this_median_ms'] = float(np.median([b['ms_per_step'] for b in bench['this']]))
        bench['parent_median_ms'] = float(np.median([b['ms_per_step'] for b in bench['parent']]))
        bench['parent_slowest_ms'] = float(np.max([b['ms_per_step'] for b in bench['parent']]))
        bench['not_slower'] = bool(bench['this_median_ms'] <= bench['parent_slowest_ms'])
        res['bench'] = bench
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
