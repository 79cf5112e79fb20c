#!/usr/bin/env python3
"""Golden fixture of the CTC prefix beam search: the outputs of this repository's own two implementations - the fixed-point
twin qasr.beam (which the kernels follow bit for bit) and the float64 search of tests/beam_cases.py - on the seeded lists
beam_cases.FIXTURE_LISTS, so that neither drifts unnoticed.  NumPy only; parity with ctc_decoders itself is not pinned
(the package is not available).

    python tests/golden/gen_golden_beam.py      # -> beam.npz

Per list: each frame's N best classes and their float32 log-probabilities (all a search reads of a distribution;
beam_cases.dense rebuilds a [B, T, C] tensor from them), the lengths, the twin's labels / n_labels / score / n_hyps and the
oracle's final beams (JSON text: [[labels, float64 score], ...] per utterance)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import beam_cases  # noqa: E402
from qasr import beam  # noqa: E402


def main():
    out, cases = {}, []
    for spec in beam_cases.FIXTURE_LISTS:
        name, C, T, W, N, n, seed, blend = spec
        lp, lens = beam_cases.fixture_inputs(spec)
        top_id, _ = beam.topn_host(lp, N)
        top_lp = np.take_along_axis(lp, top_id.astype(np.int64), axis=2)
        again = beam_cases.dense(top_id, top_lp, C)
        cid, cq = beam.topn_host(again, N, lens)
        assert np.array_equal(beam.topn_host(again, N)[0], top_id)
        res = beam.beam_search_host(cid, cq, lens, C - 1, W)
        oracle, waived = [], 0
        for b in range(n):
            o = beam_cases.oracle_beam(again[b, :lens[b]], W, N, C - 1)
            waived += len(o) > 1 and o[0][1] - o[1][1] < beam_cases.GAP
            oracle.append([[list(p), s] for p, s in o])
        assert waived <= beam_cases.MAX_WAIVED * n, (name, waived)
        out.update({'top_id_' + name: top_id, 'top_lp_' + name: top_lp, 'lens_' + name: lens, 'labels_' + name: res.labels,
                    'n_labels_' + name: res.n_labels, 'score_' + name: res.score, 'n_hyps_' + name: res.n_hyps,
                    'oracle_' + name: np.array(json.dumps(oracle))})
        cases.append(dict(name=name, classes=C, T=T, W=W, N=N, utterances=n, seed=seed, blend=blend))
    out['meta'] = np.array(json.dumps(dict(cases=cases)))
    path = os.path.join(HERE, 'beam.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
