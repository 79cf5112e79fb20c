#!/usr/bin/env python3
"""The CTC lattice kernels after they moved onto the shared headers (csrc/qasr_fixed_dev.h, csrc/qasr_lattice_dev.h), against a
library built from the parent commit (QASR_BUILD_TAG=parent python qasr/build.py in a checkout of it): fresh processes
alternating this build and the parent's in one session, --runs each, device events inside the children (no counters).  The
children are the existing --child modes of the lattice profiles at their own shapes; the session's rules (one process at a
time, the first failure or time limit ends it, the verdict's margin) are profiles/beam_dev_ab.py's.

  --rows NAMES   comma-separated, of: align_En, align_Zh, align_long (ctc_align.py), star_align (ctc_star.py), post (ctc_post.py),
                 post_band (ctc_post_band.py), segment (ctc_segment.py --child kernel), spot (ctc_spot.py)
  --parent-first the parent's library first in every pair of --rows (the second process of a pair finds the device as the first
                 left it: a row near the margin is measured in both orders); recorded under its own key
  --bench        bench.py --gpus 1, --runs pairs in each order

A row of the verdict is one timed launch of one child: every list under a key k_*_us, its median per run.

    python profiles/lattice_ab.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --rows align_En,align_Zh,star_align,post --out profiles/lattice_ab.json
    python profiles/lattice_ab.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --bench --out profiles/lattice_ab.json
"""
import argparse
import json
import os

from beam_dev_ab import MARGIN, ROOT, bench, child, verdicts

CHILDREN = dict(align_En=('ctc_align.py', 'En'), align_Zh=('ctc_align.py', 'Zh'), align_long=('ctc_align.py', 'long'),
                star_align=('ctc_star.py', 'align'), post=('ctc_post.py', 'post'), post_band=('ctc_post_band.py', 'post'),
                segment=('ctc_segment.py', 'kernel'), spot=('ctc_spot.py', 'spot'))


def timings(node, path=()):
    """(name, samples) for every list of numbers under a key k_*_us of a child's record"""
    for k, v in sorted(node.items()) if isinstance(node, dict) else ():
        if isinstance(v, dict):
            yield from timings(v, path + (k,))
        elif k.startswith('k_') and k.endswith('_us') and isinstance(v, list):
            yield '/'.join(path + (k[:-3],)), v


def kernels(a, libs, names):
    import numpy as np
    series = dict(this={}, parent={})
    for k in range(a.runs):
        for tag, lib in libs:
            for name in names:
                script, mode = CHILDREN[name]
                out = child([os.path.join(ROOT, 'profiles', script), '--child', mode], lib, a.timeout)
                line = [l for l in out.splitlines() if l.startswith('CTC_') and '_CHILD ' in l]
                for row, v in timings(json.loads(line[0].split('_CHILD ', 1)[1])):
                    series[tag].setdefault(f'{name}/{row}', []).append(float(np.median(v)))
            print(f'kernels {tag} run {k}: ' + json.dumps({r: v[-1] for r, v in series[tag].items()}), flush=True)
            a.save(dict(series_us=series))
    return dict(note=f'microseconds per launch, device events, the median of a child\'s samples per run; allowed = max(parent max / min, {MARGIN})',
                series_us=series, verdict=verdicts(series))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-lib', required=True)
    ap.add_argument('--rows', default='')
    ap.add_argument('--parent-first', action='store_true')
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
    names = [n for n in a.rows.split(',') if n]
    order = libs[::-1] if a.parent_first else libs
    todo = [('kernels_' + '_'.join(names) + ('_parent_first' if a.parent_first else ''), lambda: kernels(a, order, names))] if names else []
    if a.bench:
        todo.append(('bench', lambda: bench(a, libs)))
    for name, fn in todo:
        a.save = lambda part, name=name: save(name, part)
        save(name, fn())
        bad = [r for r, v in rec[name]['verdict'].items() if not v['ok']]
        print(f'{name}: {len(rec[name]["verdict"])} rows, over the margin: {bad}', flush=True)


if __name__ == '__main__':
    main()
