#!/usr/bin/env python3
"""CTC posteriors inside the band (k_post_band: forward-backward over the cells k_align_band kept), measured on one GPU against
k_align_band of the same build.

  post     k_align_band (Viterbi, backpointers, back-walk) and k_post_band (forward and backward pass, two table look-ups per
           cell each) in the same build, on the same inputs, in one process: device events around --steps launches on one
           stream; --rounds rounds that alternate the two, medians reported.  Shapes: the three device cases of the tests
           (tests/align_band_cases.DEVICE: the smallest at which each instantiation's band moves) and an hour - 180 000 frames,
           54 000 labels - at 1024 and at 4352 states.
  bench    `bench.py --gpus 1`, fresh processes alternating this build / a build of the parent commit (QASR_LIB), --ab-runs each;
           which of the two goes first alternates from pair to pair.  Each process runs under its own time limit, and the
           script stops at the first one that fails.

    python profiles/ctc_post_band.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_post_band.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT, os.path.join(ROOT, 'tests')]
# (name, band states, labels, frames per label from .. to, blank frames between labels from .. to)
HOURS = (('hour_bw1024', 1024, 54000, (1, 3), (0, 2)), ('hour_bw4352', 4352, 54000, (1, 3), (0, 2)))
HOUR_FRAMES = 180000
TAG = 'CTC_POST_BAND_CHILD '


def _events(torch, fn, steps):
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    t.record()
    t.synchronize()
    return s.elapsed_time(t) / steps * 1e3


def _cases():
    """(name, band states, logp float32 [1, T, C], targets [1, L], target_lens [1]) - NumPy, synthetic posteriors"""
    import numpy as np

    import align_band_cases as abc
    for name, bw, _ in abc.DEVICE:
        _, lp, tg, tl = abc.device_case(name)
        yield name, bw, lp, tg, tl
    for name, bw, L, per_label, gap in HOURS:
        lp, y = abc.synth(61, L, a=4.0, per_label=per_label, gap=gap, lead=50)
        T = lp.shape[0]
        assert T <= HOUR_FRAMES, T
        pad = np.full((HOUR_FRAMES - T, abc.C), -8.0, dtype=np.float32)       # the rest of the hour: silence
        pad[:, abc.BLANK] = np.float32(np.log1p(-(abc.C - 1) * np.exp(-8.0)))
        yield name, bw, np.concatenate([lp, pad])[None], np.array([y], dtype=np.int32), np.array([L], dtype=np.int32)


def child_post(a):
    import torch

    import align_band_cases as abc
    from qasr import engine
    if not torch.cuda.is_available():
        sys.exit('ctc_post_band.py measures on the GPU; no GPU found')
    out = {}
    for name, bw, lp, tg, tl in _cases():
        logp, tg_d, tl_d = torch.from_numpy(lp).cuda(), torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda()
        T = logp.shape[1]
        ws_a = torch.empty(engine.ctc_align_band_workspace_bytes(1, T, bw), dtype=torch.uint8, device='cuda')
        ws_p = torch.empty(engine.ctc_post_band_workspace_bytes(1, T), dtype=torch.uint8, device='cuda')
        buf = {}

        def run_align():
            buf['a'] = engine.ctc_align_band(logp, None, tg_d, tl_d, abc.BLANK, band_states=bw, workspace=ws_a, out=buf.get('a'))

        def run_post():
            buf['p'] = engine.ctc_post_band(logp, None, tg_d, tl_d, abc.BLANK, buf['a'], workspace=ws_p, out=buf.get('p'))
        run_align(), run_post()
        torch.cuda.synchronize()
        steps = 1 if T >= HOUR_FRAMES else a.steps
        al, po = [], []
        for _ in range(a.rounds):                                   # alternating rounds: drift hits both alike
            al.append(_events(torch, run_align, steps))
            po.append(_events(torch, run_post, steps))
        out[name] = dict(band_states=bw, frames=T, labels=int(tl[0]), bases=len(set(buf['a'].band_base[0].tolist())),
                         k_align_band_us=al, k_post_band_us=po, align_ok=int(buf['a'].ok.sum()), ok=int(buf['p'].ok.sum()),
                         path_score=int(buf['a'].path_score[0]), total=int(buf['p'].total[0]),
                         mean_posterior=float(torch.exp(buf['p'].frame_post.double() / 65536.0).mean()))
        del logp, ws_a, ws_p
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
    ap.add_argument('--child', choices=['post'], default=None)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=420)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (A/B of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: post, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_post(a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='device events around `steps` launches on one stream (one launch for the hours), microseconds per launch, rounds '
                    'alternating k_align_band / k_post_band; one recording per launch; synthetic posteriors, not speech')
    if 'post' not in skip:
        r = _child(a, 'post')
        for k, v in r.items():
            v['k_align_band_median_us'], v['k_post_band_median_us'] = med(v['k_align_band_us']), med(v['k_post_band_us'])
            v['k_post_band_over_k_align_band'] = v['k_post_band_median_us'] / v['k_align_band_median_us']
            print('post', k, json.dumps({x: v[x] for x in ('band_states', 'frames', 'labels', 'bases', 'k_align_band_median_us',
                                                            'k_post_band_median_us', 'k_post_band_over_k_align_band', 'ok')}), flush=True)
        res['post'] = r
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    if a.parent_lib and 'bench' not in skip:
        bench = dict(note='`bench.py --gpus 1`, fresh processes alternating this build / the parent commit\'s library (QASR_LIB)',
                     this=[], parent=[])
        for r in range(a.ab_runs):
            pair = (('this', this_lib), ('parent', a.parent_lib))
            for tag, lib in (pair if r % 2 == 0 else pair[::-1]):   # who goes first alternates too
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
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
