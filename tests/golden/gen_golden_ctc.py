#!/usr/bin/env python3
"""Golden fixture of greedy CTC decoding: the reference's own WER.ctc_decoder_predictions_tensor
(nemo/collections/asr/metrics/wer.py, loaded by file path from the reference tree, unmodified) run on the CPU over the
seeded token matrices of tests/ctc_cases.py.  Runs only where the reference tree is available; never on the GPU machine.

    python tests/golden/gen_golden_ctc.py <reference root>      # -> ctc_decode.npz

The reference module imports three packages that are not installed here and that the decoding helper does not use:
`editdistance` (word_error_rate only), `pytorch_lightning.metrics.Metric` (the base class: state registration) and
`nemo.utils.logging` (update() only).  They get empty stand-ins.  The fixture holds data only: the token matrices, the
vocabulary sizes and the reference's hypothesis strings (JSON text)."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import ctc_cases  # noqa: E402


def load_reference_wer(ref_root):
    class Metric:                                       # pytorch_lightning.metrics.Metric: only what WER.__init__ calls
        def __init__(self, *a, **k):
            pass

        def add_state(self, name, default, **k):
            setattr(self, name, default)

    stubs = {'editdistance': types.ModuleType('editdistance'), 'pytorch_lightning': types.ModuleType('pytorch_lightning'),
             'pytorch_lightning.metrics': types.ModuleType('pytorch_lightning.metrics'),
             'nemo': types.ModuleType('nemo'), 'nemo.utils': types.ModuleType('nemo.utils')}
    stubs['pytorch_lightning.metrics'].Metric = Metric
    stubs['pytorch_lightning'].metrics = stubs['pytorch_lightning.metrics']
    stubs['nemo.utils'].logging = types.SimpleNamespace(info=print, warning=print)
    stubs['nemo'].utils = stubs['nemo.utils']
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location(
            '_reference_wer', os.path.join(ref_root, 'nemo', 'collections', 'asr', 'metrics', 'wer.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('QASR_REFERENCE_ROOT')
    if not ref_root:
        sys.exit('usage: gen_golden_ctc.py <root of the reference tree>   (or QASR_REFERENCE_ROOT)')
    ref = load_reference_wer(ref_root)
    out, cases = {}, []
    for vi, n_labels in enumerate(ctc_cases.FIXTURE_VOCAB):
        wer = ref.WER(vocabulary=ctc_cases.vocabulary(n_labels))
        for T in ctc_cases.FIXTURE_T:
            name = f'v{n_labels}_t{T}'
            tok = ctc_cases.token_matrix(1000 * vi + T, T, n_labels)
            hyps = wer.ctc_decoder_predictions_tensor(torch.from_numpy(tok).long())
            assert len(hyps) == tok.shape[0]
            out['tokens_' + name] = tok
            out['hyps_' + name] = np.array(json.dumps(hyps))
            cases.append(dict(name=name, n_labels=n_labels, T=T, rows=int(tok.shape[0])))
    out['meta'] = np.array(json.dumps(dict(cases=cases)))
    path = os.path.join(HERE, 'ctc_decode.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(cases), 'cases')


if __name__ == '__main__':
    main()
