#!/usr/bin/env python3
"""The beam kernels after they moved onto the shared headers (csrc/qasr_beam_dev.h, csrc/qasr_stream_beam_dev.h), against a
library built from the parent commit (QASR_BUILD_TAG=parent python qasr/build.py in a checkout of it): fresh processes
alternating this build and the parent's in one session, --runs each, device events inside the children (no counters).

  --offline DIR  k_beam, k_beam_lm and k_beam_boost at W = 16 / 128: the `existing` and `boost:en` children of
                 profiles/ctc_boost.py over its prepared inputs (python profiles/ctc_boost.py --prepare DIR, CPU)
  --stream       k_stream_beam, k_stream_beam_boost and k_stream_beam_ep at 1 / 8 / 32 streams x W = 16 / 128 x the four
                 instantiations on identical candidates: profiles/stream_beam_ep.py --device per library
  --bench        bench.py --gpus 1

A row's verdict: the median of this build may exceed the parent's median by at most the larger of the parent's own
max / min spread over its runs of that row and 3 %.

    python profiles/beam_dev_ab.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --offline build/boost_profile --out profiles/beam_dev_ab.json
    python profiles/beam_dev_ab.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --stream --out profiles/beam_dev_ab.json
    python profiles/beam_dev_ab.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --bench --out profiles/beam_dev_ab.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1.03


def child(cmd, lib, timeout):
    """one fresh process on one library; any failure or time limit ends the session (nothing more is started on the GPU)"""
    try:
        p = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                           env=dict(os.environ, QASR_LIB=os.path.abspath(lib)))
    except subprocess.TimeoutExpired:
        sys.exit(f'{cmd[0]} ran past {timeout} s: stopping')
    if p.returncode:
        sys.exit(f'{cmd[0]} failed (rc {p.returncode}): stopping\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}')
    return p.stdout


def verdicts(series):
    """series[tag][row] = [one figure per run]; lower is better"""
    import numpy as np
    out = {}
    for row, par in series['parent'].items():
        this = series['this'][row]
        allowed = max(max(par) / min(par), MARGIN)
        ratio = float(np.median(this) / np.median(par))
        out[row] = dict(this_median=float(np.median(this)), parent_median=float(np.median(par)), ratio=round(ratio, 4),
                        allowed=round(float(allowed), 4), ok=bool(ratio <= allowed))
    return out


def offline(a, libs):
    import numpy as np
    series = dict(this={}, parent={})
    base = [os.path.join(ROOT, 'profiles', 'ctc_boost.py'), '--data', a.offline, '--widths', '16,128']
    for k in range(a.runs):
        for tag, lib in libs:
            for case in ('existing', 'boost:en'):
                line = [l for l in child(base + ['--child', case], lib, a.timeout).splitlines() if l.startswith('CTC_BOOST_CHILD ')]
                for row, v in json.loads(line[0][len('CTC_BOOST_CHILD '):])['us'].items():
                    series[tag].setdefault(row, []).append(float(np.median(v)))
            print(f'offline {tag} run {k}: ' + json.dumps({r: v[-1] for r, v in series[tag].items()}), flush=True)
            a.save('offline', dict(series_us=series))
    return dict(note='microseconds per launch (32 utterances x 250 frames, N = 40), the median of 5 samples of 10 launches per run',
                series_us=series, verdict=verdicts(series))


def stream(a, libs):
    series = dict(this={}, parent={})
    for k in range(a.runs):
        for tag, lib in libs:
            with tempfile.TemporaryDirectory() as d:
                out = os.path.join(d, 'rows.json')
                child([os.path.join(ROOT, 'profiles', 'stream_beam_ep.py'), '--device', '--out', out], lib, a.timeout)
                with open(out) as f:
                    rows = json.load(f)['device']['rows']
            for r in rows:
                name = f"S{r['streams']}_w{r['W']}_{'lm' if r['model'] else 'nolm'}_{'boost' if r['boosted'] else 'plain'}"
                series[tag].setdefault(f"{r['existing_kernel']}_{name}", []).append(r['existing_us'])
                for kind in ('no_record', 'one_cut', 'two_cuts'):
                    series[tag].setdefault(f'k_stream_beam_ep_{kind}_{name}', []).append(r[f'k_stream_beam_ep_us_{kind}'])
            print(f'stream {tag} run {k}: done', flush=True)
            a.save('stream', dict(series_us=series))
    return dict(note='microseconds per step of 48 final frames from beams warmed over 200 frames, device events, the median of 7 '
                     'samples of 20 launches per run', series_us=series, verdict=verdicts(series))


def bench(a, libs):
    """--runs pairs with this build first, then --runs pairs with the parent's first: the second process of a pair finds the
    device as the first left it, so one order alone is biased.  The verdict pools both orders; each order is kept too."""
    import numpy as np
    orders = dict(this_first=dict(this=[], parent=[]), parent_first=dict(this=[], parent=[]))
    for order, pair in (('this_first', libs), ('parent_first', libs[::-1])):
        for k in range(a.runs):
            for tag, lib in pair:
                line = [l for l in child([os.path.join(ROOT, 'bench.py'), '--gpus', '1'], lib, a.timeout).splitlines() if l.startswith('{')]
                rec = json.loads(line[-1])
                orders[order][tag].append(rec['ms_per_step'])
                print(f'bench {order} {tag} run {k}: ' + json.dumps(dict(ms_per_step=rec['ms_per_step'], value=rec['value'])), flush=True)
    series = {tag: dict(ms_per_step=orders['this_first'][tag] + orders['parent_first'][tag]) for tag in ('this', 'parent')}
    per_order = {o: round(float(np.median(v['this']) / np.median(v['parent'])), 4) for o, v in orders.items()}
    return dict(note='bench.py --gpus 1, milliseconds per step; series_ms pools the two orders, ratio_per_order is this / parent of each',
                orders_ms=orders, ratio_per_order=per_order, series_ms=series, verdict=verdicts(series))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-lib', required=True)
    ap.add_argument('--offline', default=None, metavar='DIR')
    ap.add_argument('--stream', action='store_true')
    ap.add_argument('--bench', action='store_true')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--timeout', type=int, default=600, help='seconds for one child')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    libs = (('this', os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))), ('parent', a.parent_lib))
    rec = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)

    def save(name, part):                       # after every child, so that a session cut short keeps what it measured
        rec[name] = part
        if a.out:
            with open(a.out, 'w') as f:
                f.write(json.dumps(rec, indent=1, sort_keys=True) + '\n')
    a.save = save
    for name, fn in (('offline', offline), ('stream', stream), ('bench', bench)):
        if getattr(a, name):
            save(name, fn(a, libs))
            bad = [r for r, v in rec[name]['verdict'].items() if not v['ok']]
            print(f'{name}: {len(rec[name]["verdict"])} rows, over the margin: {bad}', flush=True)


if __name__ == '__main__':
    main()
