#!/usr/bin/env python3
"""MBR re-ranking of n-best rows on the device (qasr_ctc_mbr: k_edit_cut, k_mbr_pair, k_mbr_pick), measured on one GPU.

  mbr      one call at 32 utterances x K = 4 / 16 / 64 / 128 rows, on rows of 40 words and of 250 characters, between device
           events: --steps calls captured once in a graph and replayed (the device's own time; `us`: the same calls through the
           Python binding), one sample of each case per round, --rounds rounds, medians.  Rows are one random row per utterance
           with about 15 % of the units substituted, dropped or doubled per copy.  Next to it: qasr_edit_distance on the same
           number of problems (32 K (K - 1) / 2 hypothesis rows, the same rows as references) and rerank_texts(device=None), the
           twin on the host (one core), on the same strings up to --host-max-k.  The split between the three launches comes
           from a kernel trace of this child on one case
           (rocprofv3 --kernel-trace --stats -- python profiles/ctc_mbr.py --child mbr --only words40_K16).
  decode   host wall milliseconds per batch of EncDecCTCModel.decode(beam_width=16, n_best=16) with and without mbr='word': a
           random-weight QuartzNet15x5 En engine at 32 x 500 frames.
  bench    `bench.py --gpus 1`, fresh processes alternating this build / a build of the parent commit (QASR_LIB), --ab-runs each.
           Each process runs under its own time limit, and the script stops at the first one that fails.

    python profiles/ctc_mbr.py --parent-lib q-asr_amd/qasr/libqasr_parent.so --out profiles/ctc_mbr.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'q-asr_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
TAG = 'MBR_CHILD '


def child_mbr(a):
    import numpy as np
    import torch

    import edit as pe                                               # profiles/edit.py: the strings and their rows
    from qasr import edit, engine, mbr
    if not torch.cuda.is_available():
        sys.exit('ctc_mbr.py measures on the GPU; no GPU found')
    B = 32
    mask = torch.from_numpy(edit.space_mask(pe.VOCAB)).cuda()
    engine.mbr_table_device('cuda')
    side = torch.cuda.Stream()

    def replayed(fn, steps):
        """fn captured `steps` times in one graph; returns the graph"""
        fn()
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for _ in range(steps):
                    fn()
        g.replay()
        torch.cuda.synchronize()
        return g

    def sample(fn, steps):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / steps * 1e3

    cases = {}
    for unit, mode in (('words40', 'word'), ('chars250', 'char')):
        base = pe._texts(np, 1, B, 40 if mode == 'word' else 45)
        if mode == 'char':
            base = [t[:250] for t in base]
        for K in (4, 16, 64, 128):
            if a.only and a.only != f'{unit}_K{K}':
                continue
            steps = max(1, a.steps // (1 if K <= 16 else (4 if K == 64 else 16)))
            texts = [pe._edited(np, 2 + k, base, mode) for k in range(K)]                  # [K][B]
            nbest = [[texts[k][b] for k in range(K)] for b in range(B)]
            flat = [t for row in nbest for t in row]
            lab, nl = pe._rows(np, torch, flat)
            L = lab.shape[1]
            lab3, nl2 = lab.view(B, K, L), nl.view(B, K)
            g = np.random.default_rng(5 + K)
            sc_h = np.sort(np.rint(-g.random((B, K)) * 6 * 65536 - 30 * 65536).astype(np.int64), axis=1)[:, ::-1].copy()
            sc = torch.from_numpy(sc_h).cuda()
            ws = torch.empty(engine.mbr_workspace_bytes(B, K, L, mode), dtype=torch.uint8, device='cuda')
            out = mbr.MbrResult(None, *(torch.empty(s, dtype=d, device='cuda') for s, d in (((B, K), torch.int32), ((B,), torch.int64),
                                ((B, K), torch.int64), ((B, K), torch.int32), ((B, K), torch.int32))))
            call = lambda lab3=lab3, nl2=nl2, sc=sc, ws=ws, out=out, mode=mode: engine.mbr_rerank(
                lab3, nl2, sc, None, len(pe.VOCAB), mode=mode, is_space=mask, workspace=ws, out=out)
            rec = dict(B=B, K=K, ids=int(L), pairs=B * K * (K - 1) // 2, steps=steps, workspace_bytes=int(ws.numel()), us=[], replay_us=[])
            c = dict(call=call, rec=rec, steps=steps, graph=replayed(call, steps), nbest=nbest, scores=(sc_h / 65536.0).tolist(), mode=mode)
            # qasr_edit_distance on as many problems: every pair's first row against its second as the reference
            ia, ib = np.triu_indices(K, 1)
            hyp_rows = torch.from_numpy(np.concatenate([b * K + ia for b in range(B)])).cuda()
            ref_rows = torch.from_numpy(np.concatenate([b * K + ib for b in range(B)])).cuda()
            h, hl, r, rl = lab[hyp_rows].contiguous(), nl[hyp_rows].contiguous(), lab[ref_rows].contiguous(), nl[ref_rows].contiguous()
            P = int(h.shape[0])
            ews = torch.empty(engine.edit_workspace_bytes(P, L, L, mode), dtype=torch.uint8, device='cuda')
            ekw = dict(mode=mode, is_space=mask, workspace=ews, totals=torch.zeros(16, dtype=torch.int64, device='cuda'),
                       out=torch.empty(P, 8, dtype=torch.int32, device='cuda'))
            ecall = lambda h=h, hl=hl, r=r, rl=rl, ekw=ekw: engine.edit_distance(h, hl, r, rl, len(pe.VOCAB), **ekw)
            c['egraph'], rec['edit_replay_us'] = replayed(ecall, steps), []
            # the distances of the two calls agree
            call(), ecall()
            torch.cuda.synchronize()
            full = mbr.mbr_device(lab3, nl2, sc, None, len(pe.VOCAB), mode=mode, is_space=mask, dist=True)
            ia_d, ib_d = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
            rec['same_distances'] = bool((full.dist[:, ia_d, ib_d].reshape(-1) == ekw['out'][:, 0]).all())
            rec['picks_not_first'] = int((out.order[:, 0] != 0).sum())
            cases[f'{unit}_K{K}'] = c
    for _ in range(a.rounds):
        for c in cases.values():
            c['rec']['us'].append(sample(lambda: [c['call']() for _ in range(c['steps'])], c['steps']))
            c['rec']['replay_us'].append(sample(c['graph'].replay, c['steps']))
            c['rec']['edit_replay_us'].append(sample(c['egraph'].replay, c['steps']))
    out = {}
    for name, c in cases.items():
        rec = c['rec']
        if rec['K'] <= a.host_max_k:
            t0 = time.perf_counter()
            host = mbr.rerank_texts(c['nbest'], c['scores'], use_cer=c['mode'] == 'char')
            rec['host_rerank_texts_ms'] = (time.perf_counter() - t0) * 1e3
            dev = mbr.rerank_texts(c['nbest'], c['scores'], use_cer=c['mode'] == 'char', device='cuda')
            rec['same_as_host'] = bool(host == dev)
        else:
            rec['host_rerank_texts_ms'] = None                      # not measured
        out[name] = rec
    print(TAG + json.dumps(out), flush=True)


def child_decode(a):
    import numpy as np
    import torch

    import nemo.quantization.utils.quantize_model as qm
    from nemo.collections.asr.models import EncDecCTCModel
    from qasr import synth
    torch.set_grad_enabled(False)
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En', seed=0).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([200] * 4).cuda()
    for c in synth.make_calibration(2, 4, 64, 200, 0):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    B, T = 32, 500
    io = dict(processed_signal=torch.from_numpy(synth.make_features(B, 64, T, 2)).cuda(),
              processed_signal_length=torch.full((B,), T, dtype=torch.int64).cuda())
    kws = dict(plain=dict(), mbr=dict(mbr='word'))
    for kw in kws.values():
        m.decode(**io, beam_width=16, n_best=16, **kw)
    res = {}
    for name in ('plain', 'mbr') * a.rounds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.batches):
            hyps = m.decode(**io, beam_width=16, n_best=16, **kws[name])
        torch.cuda.synchronize()
        res.setdefault(name + '_ms_per_batch', []).append((time.perf_counter() - t0) * 1e3 / a.batches)
    res.update(batch=B, frames=T, rows=sum(len(r) for r in hyps), picks_not_first=sum(r[0].beam_rank != 0 for r in hyps),
               served=type(getattr(m, '_engine', None)).__name__)
    print(TAG + json.dumps(res), flush=True)


def _child(a, stage):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', stage, '--steps', str(a.steps), '--rounds', str(a.rounds), '--batches',
           str(a.batches), '--host-max-k', str(a.host_max_k)] + (['--only', a.only] if a.only else [])
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
    ap.add_argument('--child', choices=['mbr', 'decode'], default=None)
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--host-max-k', type=int, default=16, help='the host twin is timed up to this K')
    ap.add_argument('--only', default=None, help='one case of the mbr stage, such as words40_K16 (for a kernel trace)')
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--parent-lib', default=None, help='library built from the parent commit (A/B of bench.py)')
    ap.add_argument('--ab-runs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=300)
    ap.add_argument('--skip', default='', help='comma-separated stages to leave out: mbr, decode, bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child_mbr(a) if a.child == 'mbr' else child_decode(a)
    import numpy as np
    med = lambda v: float(np.median(v))                              # noqa: E731
    skip = a.skip.split(',')
    res = dict(note='device events around `steps` calls on one stream, microseconds per call, one sample of each case per round; '
                    'random strings over 28 characters, not speech')

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
    if 'mbr' not in skip:
        r = _child(a, 'mbr')
        for k, v in r.items():
            v['median_us'], v['replay_median_us'], v['edit_replay_median_us'] = med(v['us']), med(v['replay_us']), med(v['edit_replay_us'])
            v['mbr_over_edit'] = v['replay_median_us'] / v['edit_replay_median_us']
            if v['host_rerank_texts_ms'] is not None:
                v['host_over_call'] = v['host_rerank_texts_ms'] * 1e3 / v['replay_median_us']
            print('mbr', k, json.dumps({x: v.get(x) for x in ('pairs', 'replay_median_us', 'edit_replay_median_us', 'median_us',
                                                              'host_rerank_texts_ms', 'same_distances', 'same_as_host')}), flush=True)
        res['qasr_ctc_mbr'] = r
        save()
    if 'decode' not in skip:
        r = _child(a, 'decode')
        r['plain_median_ms'], r['mbr_median_ms'] = med(r['plain_ms_per_batch']), med(r['mbr_ms_per_batch'])
        print('decode', json.dumps(r), flush=True)
        res['decode_beam16_nbest16'] = r
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
