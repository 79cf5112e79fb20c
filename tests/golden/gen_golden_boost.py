#!/usr/bin/env python3
"""Golden fixture of the phrase boosting: the outputs of the fixed-point twin qasr.beam with a qasr.boost.PhraseSet on the
seeded lists boost_cases.FIXTURE_LISTS (two without a model, one with the committed En 3-gram), so that neither the
generator, the automaton nor the twin drifts unnoticed.  NumPy only.

    python tests/golden/gen_golden_boost.py      # -> boost.npz"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import beam_lm_cases as lm_cases  # noqa: E402
import boost_cases as cases  # noqa: E402
from qasr import beam, boost, ngram  # noqa: E402


def run(spec, golden_dir=HERE):
    name, model, C, T, W, N, n, seed = spec
    lp, lens, phrases = cases.fixture_inputs(spec)
    lm = None if model is None else ngram.NgramLM.from_arpa(lm_cases.model_path(golden_dir, model), lm_cases.vocab_of(model))
    ps = boost.PhraseSet(phrases, cases.vocab_for(C))
    return beam.search_host(lp, lens, C - 1, W, None, N, lm, 1.0, 0.5, boost=ps), ps


def main():
    out, meta = {}, []
    for spec in cases.FIXTURE_LISTS:
        res, ps = run(spec)
        for f in ('labels', 'n_labels', 'score', 'boost_score', 'n_hyps') + (('lm_score',) if res.lm_score is not None else ()):
            out[f'{f}_{spec[0]}'] = getattr(res, f)
        out[f'blob_{spec[0]}'] = np.frombuffer(ps.pack(), np.uint8)
        meta.append(dict(name=spec[0], model=spec[1], classes=spec[2], T=spec[3], W=spec[4], N=spec[5], utterances=spec[6], seed=spec[7]))
    out['meta'] = np.array(json.dumps(dict(cases=meta)))
    path = os.path.join(HERE, 'boost.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
