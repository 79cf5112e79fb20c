#!/usr/bin/env python3
"""Word / character error counts on the device (qasr_edit_distance: k_edit_cut, k_edit, k_edit_totals), measured on one GPU.

  edit     the three launches of one call between device events, --steps calls per sample on one stream (1 for the hour), one
           sample of each case per round, --rounds rounds, medians - `us`: the calls through the Python binding, which for a small
           batch is what the host can enqueue; `replay_us`: the same --steps calls captured once in a graph and replayed, the
           device's own time: 32 x 40 words; 32 x 250 characters; 32 references x 16 n-best
           rows of 40 words; one stitched hour in words (~9 000) and in characters (~54 000).  Hypotheses are the references with
           about 15 % of the units substituted, dropped or doubled.  Next to each of the 32-row cases: the host wall time of
           word_error_rate on the same strings (one core, Python), and whether the two rates are equal.  The hour on the host is
           not run here (minutes to tens of minutes).
  loop     the greedy evaluation loop of examples/asr/quantization/inference.py, host wall milliseconds per batch: a
           random-weight QuartzNet15x5 En engine (as profiles/ctc_decode.py builds it) at 32 x 500 frames, then the metric -
           today: tokens to the host, WER.update (a Python step per frame and per cell); device: WER(device=True).update
           (k_ctc + k_edit behind the forward, nothing read back until compute()).
  bench    `bench.py --gpus 1`, fresh processes alternating this build / a build of the parent commit (QASR_LIB), --ab-runs each,
           the order inside a pair alternating as well.  Each process runs under its own time limit, and the script stops at the
           first one that fails.

    python profiles/edit.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/edit.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT]
TAG = 'EDIT_CHILD '
VOCAB = [' '] + list("abcdefghijklmnopqrstuvwxyz'")


def _texts(np, seed, rows, words):
    g = np.random.default_rng(seed)
    return [' '.join(''.join(VOCAB[c] for c in g.integers(1, len(VOCAB), int(g.integers(2, 9)))) for _ in range(words)) for _ in range(rows)]


def _edited(np, seed, texts, unit):
    """about 15 % of the units (words, or characters) substituted, dropped or doubled"""
    g = np.random.default_rng(seed)
    out = []
    for t in texts:
        us, keep = (t.split() if unit == 'word' else list(t)), []
        for u in us:
            x = g.random()
            if x < 0.05:
                continue
            keep.append(us[int(g.integers(len(us)))] if x < 0.10 else u)
            if x > 0.95:
                keep.append(u)
        out.append((' ' if unit == 'word' else '').join(keep))
    return out


def _rows(np, torch, texts):
    at = {ch: i for i, ch in enumerate(VOCAB)}
    n = max(1, max(len(t) for t in texts))
    m = np.zeros((len(texts), n), dtype=np.int32)
    for r, t in enumerate(texts):
        m[r, :len(t)] = [at[ch] for ch in t]
    return torch.from_numpy(m).cuda(), torch.tensor([len(t) for t in texts], dtype=torch.int32).cuda()


def child_edit(a):
    import numpy as np
    import torch

    from nemo.collections.asr.metrics.wer import word_error_rate
    from qasr import edit, engine
    if not torch.cuda.is_available():
        sys.exit('edit.py measures on the GPU; no GPU found')
    mask = torch.from_numpy(edit.space_mask(VOCAB)).cuda()
    cases = {}
    for name, rows, words, K, mode, host in (('words_32x40', 32, 40, 1, 'word', True), ('chars_32x250', 32, 45, 1, 'char', True),
                                             ('nbest16_32x40', 32, 40, 16, 'word', True), ('hour_words_1x9000', 1, 9000, 1, 'word', False),
                                             ('hour_chars_1x54000', 1, 9000, 1, 'char', False)):
        refs = _texts(np, 1, rows, words)
        if name == 'chars_32x250':
            refs = [t[:250] for t in refs]
        hyps = [h for k in range(K) for h in _edited(np, 2 + k, refs, mode)]
        hyps = [hyps[k * rows + b] for b in range(rows) for k in range(K)]          # row p = b * K + k
        (h, hl), (r, rl) = _rows(np, torch, hyps), _rows(np, torch, refs)
        ws = torch.empty(engine.edit_workspace_bytes(len(hyps), h.shape[1], r.shape[1], mode), dtype=torch.uint8, device='cuda')
        cases[name] = dict(args=(h, hl, r, rl, len(VOCAB)), kw=dict(mode=mode, is_space=mask, rows_per_ref=K, workspace=ws,
                           totals=torch.zeros(16, dtype=torch.int64, device='cuda'), out=torch.empty(len(hyps), 8, dtype=torch.int32, device='cuda')),
                           steps=a.steps if rows > 1 else 1, hyps=hyps, refs=refs, host=host, K=K, mode=mode,
                           rec=dict(P=len(hyps), hyp_ids=int(h.shape[1]), ref_ids=int(r.shape[1]), workspace_bytes=int(ws.numel()), us=[]))
    side = torch.cuda.Stream()
    for c in cases.values():                                        # warm every case before any is timed
        engine.edit_distance(*c['args'], **c['kw'])
        torch.cuda.synchronize()
        c['graph'] = None
        if c['steps'] > 1:                                          # the binding's Python costs more than the three launches of a small
            side.wait_stream(torch.cuda.current_stream())           # batch: the same calls captured once and replayed give the device time
            c['graph'] = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(c['graph'], stream=side):
                    for _ in range(c['steps']):
                        engine.edit_distance(*c['args'], **c['kw'])
            c['graph'].replay()
            c['rec']['replay_us'] = []
    torch.cuda.synchronize()

    def sample(fn, steps):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / steps * 1e3

    def eager(c):
        for _ in range(c['steps']):
            engine.edit_distance(*c['args'], **c['kw'])
    for _ in range(a.rounds):
        for c in cases.values():
            c['rec']['us'].append(sample(lambda: eager(c), c['steps']))
            if c['graph'] is not None:
                c['rec']['replay_us'].append(sample(c['graph'].replay, c['steps']))
    out = {}
    for name, c in cases.items():
        rec = c['rec']
        c['kw']['totals'].zero_()
        res = engine.edit_distance(*c['args'], **c['kw'])
        tot = res.totals.cpu().numpy()
        rec.update(errors=int(tot[0]), ref_units=int(tot[1]), S=int(tot[2]), D=int(tot[3]), I=int(tot[4]), oracle_errors=int(tot[7]),
                   cells=int((res.rows[:, 4].long() * res.rows[:, 5].long()).sum()))
        if c['host']:
            first = c['hyps'][::c['K']]
            t0 = time.perf_counter()
            rate = word_error_rate(first, c['refs'], use_cer=c['mode'] == 'char')
            rec['host_word_error_rate_ms'] = (time.perf_counter() - t0) * 1e3
            rec['same_rate'] = bool(rate == tot[0] / tot[1])
        else:
            rec['host_word_error_rate_ms'] = None                   # not measured
        out[name] = rec
    print(TAG + json.dumps(out), flush=True)


def child_loop(a):
    import numpy as np
    import torch

    from nemo.collections.asr.metrics.wer import WER
    from qasr import engine, pack, synth, topology
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_quartznet_w8a8.npz'))
    cfg = topology.quartznet15x5()
    blob = pack.pack_model(cfg, synth.make_state_dict(cfg, 0), d['act_min'], d['act_max'], 8, 8)[0]
    B, T = 32, 500
    x = torch.from_numpy(synth.make_features(B, 64, T, 2)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    e = engine.Engine(blob, 0, graph=True)
    To = e.out_frames(T)
    outb = (None, torch.empty(B, To, dtype=torch.int32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'))
    g = torch.Generator().manual_seed(3)
    tg = torch.randint(0, len(cfg.vocabulary), (B, 120), generator=g, dtype=torch.int32).cuda()
    tl = torch.randint(60, 121, (B,), generator=g, dtype=torch.int32).cuda()
    res = {}
    metrics = dict(today=WER(vocabulary=cfg.vocabulary), device=WER(vocabulary=cfg.vocabulary, device=True))
    for _ in range(3):
        e.forward(x, lens, want_logp=False, out=outb)
    metrics['device'].update(outb[1], tg, tl)
    metrics['device'].reset()
    torch.cuda.synchronize()
    for name in ('today', 'device') * a.rounds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.batches):
            e.forward(x, lens, want_logp=False, out=outb)
            metrics[name].update(outb[1], tg, tl)
        torch.cuda.synchronize()
        res.setdefault(name + '_ms_per_batch', []).append((time.perf_counter() - t0) * 1e3 / a.batches)
    rates = {k: float(m.compute()[0]) for k, m in metrics.items()}
    res.update(batch=B, frames=T, encoder_frames=To, batches_per_sample=a.batches, same_rate=rates['today'] == rates['device'], rate=rates['today'])
    e.close()
    print(TAG + json.dumps(res), flush=True)


def _child(a, stage):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', stage, '--steps', str(a.steps), '--rounds', str(a.rounds), '--batches', str(a.batches)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f'child {stage} ran past {a.child_timeout} s: stopping')
    line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
    if p.returncode or not line:
        sys.exit(f'child {stage} failed (rc {p.returncode}): stopping\n{p.stderr[-1500:]}')
    return json.loads(line[0][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['edit', 'loop'], default=None)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (A/B of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: edit, loop, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_edit(a) if a.child == 'edit' else child_loop(a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='device events around `steps` calls (three launches each) on one stream, microseconds per call, one sample of each '
                    'case per round; random strings over 28 characters, not speech')

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
    if 'edit' not in skip:
        r = _child(a, 'edit')
        for k, v in r.items():
            v['median_us'] = med(v['us'])
            v['ns_per_cell'] = v['median_us'] * 1e3 / max(v['cells'], 1)
            if 'replay_us' in v:
                v['replay_median_us'] = med(v['replay_us'])
                v['ns_per_cell'] = v['replay_median_us'] * 1e3 / max(v['cells'], 1)
            if v['host_word_error_rate_ms'] is not None:
                v['host_over_call'] = v['host_word_error_rate_ms'] * 1e3 / v['median_us']
            print('k_edit', k, json.dumps({x: v.get(x) for x in ('P', 'median_us', 'replay_median_us', 'ns_per_cell', 'host_word_error_rate_ms', 'same_rate', 'errors')}), flush=True)
        res['k_edit'] = r
        save()
    if 'loop' not in skip:
        r = _child(a, 'loop')
        r['today_median_ms'], r['device_median_ms'] = med(r['today_ms_per_batch']), med(r['device_ms_per_batch'])
        print('loop', json.dumps(r), flush=True)
        res['greedy_loop'] = r
        save()
    this_lib = os.environ.get('QASR_LIB', os.path.join(ROOT, 'q-asr_amd', 'qasr', 'libqasr_hip.so'))
    if a.parent_lib and 'bench' not in skip:
        bench = dict(note='`bench.py --gpus 1`, fresh processes alternating this build / the parent commit\'s library (QASR_LIB)',
                     this=[], parent=[])
        for r in range(a.ab_runs):
            for tag, lib in (('this', this_lib), ('parent', a.parent_lib))[::1 if r % 2 == 0 else -1]:      # who goes first alternates too
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
    save()


if __name__ == '__main__':
    main()
