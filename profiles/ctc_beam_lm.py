#!/usr/bin/env python3
"""CTC prefix beam search with an n-gram language model on the device, measured on one GPU: k_beam / k_beam_lm per launch and
per frame at 32 utterances x 250 encoder frames (500 input frames), N = 40 candidates, beam widths 16 and 128, for
  En without a model (k_beam, the launch this change must not slow),
  En with a word 3-gram and Zh with a character 3-gram (k_beam_lm).
The models are synthetic ones of the test generator (tests/beam_lm_cases.py) scaled to a few hundred thousand n-grams, so
that their tables do not sit in L1; the log-probabilities spell sentences of those models (tests/beam_lm_cases.lm_logp), so
that the look-ups hit n-grams of every order instead of ending at "out of vocabulary".

  prepare  (CPU, once) generate the models, load and pack them, draw the inputs:   --prepare DIR
  measure  device events around --steps launches on one stream, --rounds samples.  With --parent-lib (a library built from
           the parent commit) the no-model launch is measured in fresh processes alternating this / parent, --ab-runs each;
           the margin of the comparison is the spread of the parent's own runs.

    python profiles/ctc_beam_lm.py --prepare build/lm_profile
    python profiles/ctc_beam_lm.py --data build/lm_profile --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_beam_lm.json
"""
import argparse
import json
import os
import pickle
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests'), ROOT]

# (name, mode, order, tokens, training tokens, seed)
SCALED = (('en_word3', 'word', 3, 20000, 260000, 21), ('zh_char3', 'char', 3, 3000, 300000, 22))


def prepare(a):
    import numpy as np

    import beam_lm_cases as cases
    from qasr import beam, ngram
    os.makedirs(a.prepare, exist_ok=True)
    for name, mode, order, n_tok, n_train, seed in SCALED:
        text, tokens = cases.scaled_model_text(mode, order, n_tok, n_train, seed)
        path = os.path.join(a.prepare, name + '.arpa')
        with open(path, 'w', encoding='utf-8') as f:
            f.write(text)
        vocab = cases.EN_VOCAB if mode == 'word' else cases.ZH_VOCAB
        lm = ngram.NgramLM.from_arpa(path, vocab)
        blob = lm.pack()
        lm._memo = {}
        rng = np.random.Generator(np.random.PCG64(seed + 100))
        spec = (name, '', mode, order, n_tok, n_train, seed)
        lp = np.stack([cases.lm_logp(rng, spec, a.enc_frames, 1.5, tokens) for _ in range(a.batch)])
        cid, cq = beam.topn_host(lp, a.top_n)
        with open(os.path.join(a.prepare, name + '.pkl'), 'wb') as f:
            pickle.dump(dict(lm=lm, cand_id=cid, cand_q=cq, classes=lp.shape[2]), f, protocol=4)
        hdr = np.frombuffer(blob[:128], '<i4')
        print(name, 'n-grams', len(lm.trans), 'nodes', len(lm.backoff), 'blob bytes', len(blob), 'probe bound', int(hdr[7]), flush=True)


def child(a):
    import numpy as np
    import torch

    from qasr import beam, engine
    if not torch.cuda.is_available():
        sys.exit('ctc_beam_lm.py measures on the GPU; no GPU found')
    name = {'plain': 'en_word3', 'en': 'en_word3', 'zh': 'zh_char3'}[a.child]
    with open(os.path.join(a.data, name + '.pkl'), 'rb') as f:
        d = pickle.load(f)
    lm = None if a.child == 'plain' else d['lm']
    cid, cq = torch.from_numpy(d['cand_id']).cuda(), torch.from_numpy(d['cand_q']).cuda()
    B, T, N = cid.shape
    blank = d['classes'] - 1
    widths = [int(w) for w in a.widths.split(',')]
    ws = {W: torch.empty(engine.ctc_beam_workspace_bytes(B, T, W), dtype=torch.uint8, device='cuda') for W in widths}
    res = {}

    def run(W):
        res[W] = engine.ctc_beam(cid, cq, None, blank, W, W, workspace=ws[W], out=res.get(W), lm=lm, alpha=a.alpha, beta=a.beta) \
            if lm is not None else engine.ctc_beam(cid, cq, None, blank, W, W, workspace=ws[W], out=res.get(W))

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

    out = dict(case=a.child, frames=int(T), batch=int(B), top_n=int(N), us={f'w{W}': timed(lambda: run(W)) for W in widths})
    if lm is not None:                                    # the device results are the twin's (first utterance, narrowest beam)
        W = widths[0]
        twin = beam.beam_search_host(d['cand_id'][:1], d['cand_q'][:1], None, blank, W, W, lm, a.alpha, a.beta)
        out['equals_twin'] = bool(all(np.array_equal(getattr(res[W], f)[:1].cpu().numpy(), getattr(twin, f))
                                      for f in ('labels', 'n_labels', 'score', 'lm_score', 'n_hyps')))
        out['model'] = dict(order=lm.order, ngrams=len(lm.trans), nodes=len(lm.backoff), blob_bytes=len(lm.pack()),
                            scored_terms_best=int(round(float(twin.lm_score[0, 0]) / 65536.0)))
    print('CTC_BEAM_LM_CHILD ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prepare', default=None, metavar='DIR')
    ap.add_argument('--data', default=None, metavar='DIR')
    ap.add_argument('--child', choices=['plain', 'en', 'zh'], default=None)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--enc-frames', type=int, default=250)
    ap.add_argument('--top-n', type=int, default=40)
    ap.add_argument('--widths', default='16,128')
    ap.add_argument('--alpha', type=float, default=1.0)
    ap.add_argument('--beta', type=float, default=0.5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--ab-runs', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.prepare:
        return prepare(a)
    if a.child:
        return child(a)
    import numpy as np

    def run_child(case, lib=None):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', case, '--data', a.data, '--widths', a.widths, '--alpha', str(a.alpha),
               '--beta', str(a.beta), '--steps', str(a.steps), '--rounds', str(a.rounds)]
        env = dict(os.environ, QASR_LIB=os.path.abspath(lib)) if lib else dict(os.environ)
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout, env=env)
        except subprocess.TimeoutExpired:
            sys.exit(f'child {case} ran past {a.child_timeout} s: stopping')
        line = [l for l in p.stdout.splitlines() if l.startswith('CTC_BEAM_LM_CHILD ')]
        if p.returncode or not line:
            sys.exit(f'child {case} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
        return json.loads(line[0][len('CTC_BEAM_LM_CHILD '):])

    def stat(v):
        return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))

    runs = [run_child(c) for c in ('plain', 'en', 'zh')]
    summary = {}
    for r in runs:
        s = {k: stat(v) for k, v in r['us'].items()}
        for k in list(s):
            s[k + '_per_frame_us'] = s[k]['median'] / r['frames']
        for k in ('equals_twin', 'model'):
            if k in r:
                s[k] = r[k]
        summary[r['case']] = s
        print(r['case'], json.dumps(s), flush=True)
    ab = {}
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        series = dict(this={}, parent={})
        for k in range(a.ab_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib)):
                r = run_child('plain', lib)
                for w, v in r['us'].items():
                    series[tag].setdefault(w, []).append(float(np.median(v)))
                print(f'no-model {tag} run {k}: ' + json.dumps({w: float(np.median(v)) for w, v in r['us'].items()}), flush=True)
        ab = dict(series_us=series, verdict={})
        for w in series['parent']:
            par, this = series['parent'][w], series['this'][w]
            margin = max(par) - min(par)
            ab['verdict'][w] = dict(parent_median=float(np.median(par)), this_median=float(np.median(this)), parent_spread=margin,
                                    not_slower=bool(np.median(this) <= np.median(par) + margin))
        print('no-model A/B', json.dumps(ab['verdict']), flush=True)
    res = dict(shape=dict(batch=a.batch, enc_frames=a.enc_frames, top_n=a.top_n, alpha=a.alpha, beta=a.beta), steps=a.steps,
               rounds=a.rounds,
               note='microseconds per launch: device events around `steps` launches on one stream; `plain` is k_beam without a model on '
                    'the En inputs, `en` / `zh` are k_beam_lm; no_model_ab: medians of fresh processes alternating this build and '
                    'the parent commit\'s, margin = max - min of the parent\'s own runs',
               summary=summary, no_model_ab=ab, runs=runs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
