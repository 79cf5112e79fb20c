#!/usr/bin/env python3
"""Golden fixture of the CTC forced alignment: the outputs of the fixed-point twin qasr.align.align_host (which k_align
follows bit for bit) on the seeded lists align_cases.FIXTURE_LISTS, so that it does not drift unnoticed.  NumPy only.

    python tests/golden/gen_golden_align.py      # -> align.npz

Per list: the lengths and targets, the twin's start / nframes / score / path_score / total / ok, and - instead of the
log-probabilities, which tests/align_cases.py regenerates from the seed - a probe of them: four classes per frame and
their float32 values, so that a change of the generator shows as such."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import align_cases  # noqa: E402
from qasr import align  # noqa: E402


def main():
    out, cases = {}, []
    for spec in align_cases.FIXTURE_LISTS:
        name, C, T, B, K, seed = spec
        lp, lens, tg, tl = align_cases.fixture_inputs(spec)
        res = align.align_host(lp, lens, tg, tl, C - 1, problems_per_utt=K)
        assert res.ok.sum() >= B, name
        probe = np.random.Generator(np.random.PCG64(seed + 1000)).integers(0, C, size=(B, T, 4)).astype(np.int32)
        out.update({'lens_' + name: lens, 'targets_' + name: tg, 'target_lens_' + name: tl, 'probe_' + name: probe,
                    'probe_lp_' + name: np.take_along_axis(lp, probe.astype(np.int64), axis=2)})
        out.update({f + '_' + name: getattr(res, f) for f in ('start', 'nframes', 'score', 'path_score', 'total', 'ok')})
        cases.append(dict(name=name, classes=C, T=T, utterances=B, problems_per_utt=K, seed=seed))
    out['meta'] = np.array(json.dumps(dict(cases=cases)))
    path = os.path.join(HERE, 'align.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
