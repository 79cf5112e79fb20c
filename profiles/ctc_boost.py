#!/usr/bin/env python3
"""CTC prefix beam search with phrase boosting on the device, measured on one GPU: k_beam_boost per launch and per frame at
32 utterances x 250 encoder frames (500 input frames), N = 40 candidates, beam widths 16 and 128, with synthetic sets of
10 / 1 000 / 10 000 phrases, En (whole words) and Zh, without and with the n-gram models of profiles/ctc_beam_lm.py; and
k_beam / k_beam_lm of this build and of a build of the parent commit, in alternating fresh processes.

The inputs are those of profiles/ctc_beam_lm.py (log-probabilities that spell sentences of the scaled models); the phrases
are drawn from the same token lists (En: 1 .. 3 words, Zh: 2 .. 6 characters), so that matches begin, continue and end on
the searched prefixes instead of never leaving the root.

  prepare  (CPU, once) the models and inputs of ctc_beam_lm.py, then the phrase sets:       --prepare DIR
  measure  device events around --steps launches on one stream, --rounds samples.

    python profiles/ctc_boost.py --prepare build/boost_profile
    python profiles/ctc_boost.py --data build/boost_profile --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_boost.json
"""
import argparse
import importlib.util
import json
import os
import pickle
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests'), ROOT]
SET_SIZES = (10, 1000, 10000)
LANGS = dict(en='en_word3', zh='zh_char3')
TAG = 'CTC_BOOST_CHILD '


def _lm_profile():
    spec = importlib.util.spec_from_file_location('ctc_beam_lm_profile', os.path.join(ROOT, 'profiles', 'ctc_beam_lm.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def prepare(a):
    import numpy as np

    import beam_lm_cases as cases
    from qasr import boost
    lmp = _lm_profile()
    if not all(os.path.exists(os.path.join(a.prepare, n + '.pkl')) for n in LANGS.values()):
        lmp.prepare(a)
    for lang, (name, mode, order, n_tok, n_train, seed) in zip(('en', 'zh'), lmp.SCALED):
        _, tokens = cases.scaled_model_text(mode, order, n_tok, n_train, seed)
        vocab = cases.EN_VOCAB if mode == 'word' else cases.ZH_VOCAB
        rng = np.random.Generator(np.random.PCG64(seed + 200))
        sets = {}
        for n in SET_SIZES:
            phrases = set()
            while len(phrases) < n:
                k = int(rng.integers(1, 4)) if mode == 'word' else int(rng.integers(2, 7))
                pick = [tokens[int(i)] for i in rng.integers(0, len(tokens), size=k)]
                phrases.add((' ' if mode == 'word' else '').join(pick)[:64])
            ps = boost.PhraseSet([(p, float(rng.uniform(0.5, 3.0))) for p in sorted(phrases)], vocab)
            blob = ps.pack()
            hdr = np.frombuffer(blob[:128], '<i4')
            sets[n] = ps
            print(lang, n, 'phrases: nodes', ps.n_nodes, 'table capacity', int(hdr[7]), 'probe bound', int(hdr[8]), 'blob bytes', len(blob), flush=True)
        with open(os.path.join(a.prepare, f'boost_{lang}.pkl'), 'wb') as f:
            pickle.dump(sets, f, protocol=4)


def child(a):
    import numpy as np
    import torch

    from qasr import beam, engine
    if not torch.cuda.is_available():
        sys.exit('ctc_boost.py measures on the GPU; no GPU found')
    widths = [int(w) for w in a.widths.split(',')]

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

    out = dict(case=a.child, us={})
    langs = ('en', 'zh') if a.child == 'existing' else (a.child.split(':')[1],)
    for lang in langs:
        with open(os.path.join(a.data, LANGS[lang] + '.pkl'), 'rb') as f:
            d = pickle.load(f)
        cid, cq = torch.from_numpy(d['cand_id']).cuda(), torch.from_numpy(d['cand_q']).cuda()
        B, T, N = cid.shape
        blank = d['classes'] - 1
        out.update(frames=int(T), batch=int(B), top_n=int(N))
        ws = {W: torch.empty(engine.ctc_beam_workspace_bytes(B, T, W), dtype=torch.uint8, device='cuda') for W in widths}
        if a.child == 'existing':                           # k_beam and k_beam_lm, as this library has them
            for W in widths:
                res = {}

                def run(lm):
                    kw = dict(lm=lm, alpha=a.alpha, beta=a.beta) if lm is not None else {}
                    res[lm is None] = engine.ctc_beam(cid, cq, None, blank, W, W, workspace=ws[W], out=res.get(lm is None), **kw)
                if lang == 'en':
                    out['us'][f'k_beam_en_w{W}'] = timed(lambda: run(None))
                out['us'][f'k_beam_lm_{lang}_w{W}'] = timed(lambda: run(d['lm']))
            continue
        with open(os.path.join(a.data, f'boost_{lang}.pkl'), 'rb') as f:
            sets = pickle.load(f)
        out['sets'] = {}
        for n, ps in sets.items():
            out['sets'][str(n)] = dict(nodes=ps.n_nodes, blob_bytes=len(ps.pack()), probe_bound=int(np.frombuffer(ps.pack()[:128], '<i4')[8]))
            for lm in (None, d['lm']):
                for W in widths:
                    res = {}

                    def run():
                        kw = dict(lm=lm, alpha=a.alpha, beta=a.beta) if lm is not None else {}
                        res[0] = engine.ctc_beam(cid, cq, None, blank, W, W, workspace=ws[W], out=res.get(0), boost=ps, **kw)
                    out['us'][f'k_beam_boost_{lang}_{n}_{"lm" if lm is not None else "nolm"}_w{W}'] = timed(run)
                    if W == widths[0] and n == SET_SIZES[1]:    # the device results are the twin's (first utterance, narrowest beam)
                        twin = beam.beam_search_host(d['cand_id'][:1], d['cand_q'][:1], None, blank, W, W, lm, a.alpha, a.beta, boost=ps)
                        fields = ('labels', 'n_labels', 'score', 'boost_score', 'n_hyps') + (('lm_score',) if lm is not None else ())
                        out.setdefault('equals_twin', {})['lm' if lm is not None else 'nolm'] = bool(all(
                            np.array_equal(getattr(res[0], f)[:1].cpu().numpy(), getattr(twin, f)) for f in fields))
                        out.setdefault('boost_of_best_nats', {})['lm' if lm is not None else 'nolm'] = float(twin.boost_score[0, 0]) / 65536.0
    print(TAG + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prepare', default=None, metavar='DIR')
    ap.add_argument('--data', default=None, metavar='DIR')
    ap.add_argument('--child', default=None)
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
    ap.add_argument('--ab-runs', type=int, default=3)
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
        line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
        if p.returncode or not line:
            sys.exit(f'child {case} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
        return json.loads(line[0][len(TAG):])

    runs = [run_child('boost:en'), run_child('boost:zh')]
    frames = runs[0]['frames']
    summary = {}
    for r in runs:
        for k, v in r['us'].items():
            summary[k] = dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)),
                              per_frame_us=float(np.median(v)) / frames)
            print(k, json.dumps(summary[k]), flush=True)
        print(r['case'], 'equals_twin', r.get('equals_twin'), 'sets', r.get('sets'), flush=True)
    ab = {}
    if a.parent_lib:
        this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
        series = dict(this={}, parent={})
        for k in range(a.ab_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib)):
                r = run_child('existing', lib)
                for w, v in r['us'].items():
                    series[tag].setdefault(w, []).append(float(np.median(v)))
                print(f'existing kernels, {tag} run {k}: ' + json.dumps({w: float(np.median(v)) for w, v in r['us'].items()}), flush=True)
        ab = dict(series_us=series, verdict={})
        for w in series['parent']:
            par, this = series['parent'][w], series['this'][w]
            ab['verdict'][w] = dict(parent_mean=float(np.mean(par)), this_mean=float(np.mean(this)), parent_min=min(par), parent_max=max(par),
                                    per_frame_us=float(np.mean(this)) / frames,
                                    within_parent_spread=bool(min(par) <= np.mean(this) <= max(par)),
                                    not_slower=bool(np.mean(this) <= max(par)))
        print('existing kernels A/B', json.dumps(ab['verdict']), flush=True)
    res = dict(shape=dict(batch=a.batch, enc_frames=a.enc_frames, top_n=a.top_n, alpha=a.alpha, beta=a.beta), steps=a.steps, rounds=a.rounds,
               note='microseconds per launch: device events around `steps` launches on one stream, the median of `rounds` samples; '
                    'k_beam_boost_<lang>_<phrases>_<lm|nolm>_w<W>; existing_ab: k_beam / k_beam_lm in fresh processes alternating this '
                    'build and the parent commit\'s, the yardstick is the parent\'s own min .. max',
               summary=summary, sets={r['case']: r.get('sets') for r in runs}, equals_twin={r['case']: r.get('equals_twin') for r in runs},
               boost_of_best_nats={r['case']: r.get('boost_of_best_nats') for r in runs}, existing_ab=ab)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
