#!/usr/bin/env python3
"""Golden fixtures of the beam search with a language model: the small ARPA models that tests/beam_lm_cases.py generates
(lm_en_word3.arpa, lm_en_word1.arpa, lm_en_word5.arpa, lm_zh_char2.arpa.gz) and the outputs of the fixed-point twin
qasr.beam with qasr.ngram on the seeded lists beam_lm_cases.FIXTURE_LISTS, so that neither the generator, the loader nor
the twin drifts unnoticed.  NumPy only.

    python tests/golden/gen_golden_beam_lm.py      # -> lm_*.arpa[.gz], beam_lm.npz"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import beam_lm_cases as cases  # noqa: E402
from qasr import beam, ngram  # noqa: E402


def main():
    cases.write_models(HERE)
    out, meta = {}, []
    for name, model, T, W, N, alpha, beta, n, seed in cases.FIXTURE_LISTS:
        lm = ngram.NgramLM.from_arpa(cases.model_path(HERE, model), cases.vocab_of(model))
        lp, lens = cases.batch_inputs(model, T, n, seed)
        res = beam.search_host(lp, lens, lp.shape[2] - 1, W, None, N, lm, alpha, beta)
        for f in ('labels', 'n_labels', 'score', 'lm_score', 'n_hyps'):
            out[f'{f}_{name}'] = getattr(res, f)
        meta.append(dict(name=name, model=model, T=T, W=W, N=N, alpha=alpha, beta=beta, utterances=n, seed=seed))
    out['meta'] = np.array(json.dumps(dict(cases=meta)))
    path = os.path.join(HERE, 'beam_lm.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
