#!/usr/bin/env python3
"""Phase stamps of one work-group of the fused separable-layer kernels (qasr_debug_prof: s_memtime at the phase
boundaries of work-group (0, 1), thread 0).  Usage: python profiles/phase_stamps.py [--tile 32|64] [--gen 1|2]
Prints, per selected op, the cycle deltas between consecutive stamps: k_sep2 = start | per 256-channel chunk: window
committed, depthwise done | after the post-depthwise barrier(s) | per 256-channel pass: main GEMM, (residual GEMM,) epilogue.
--prologue (a library built with -DSEP2_PSTAMP=1, named by QASR_LIB; add -DSEP2_EARLY=0 for the prologue order before DESIGN.md
5.8): also the points inside the prologue, in cycles from the wave's first instruction - start stamp | kernel arguments (old
order: and lens[b]) there | per-lane constants done | group 0 requested | depthwise parameters requested | group 0 back |
rows on their way to LDS | first depthwise MFMA.  The stamped wave waits at `arguments` and `group 0 back`, a production wave
does not.  --json FILE --tag NAME adds the figures to FILE under NAME."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'q-asr_amd'))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--tile', type=int, default=32, choices=[32, 64, 128])
ap.add_argument('--gen', type=int, default=2)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--prologue', action='store_true')
ap.add_argument('--json')
ap.add_argument('--tag', default='run')
args = ap.parse_args()
from qasr import engine, pack, synth, topology  # noqa: E402

d = np.load(os.path.join(ROOT, 'tests/golden/net_quartznet_w8a8.npz'))
meta = json.loads(str(d['meta']))
cfg = topology.quartznet15x5()
sd = synth.make_state_dict(cfg, meta['seed'])
blob, pm = pack.pack_model(cfg, sd, d['act_min'], d['act_max'], 8, 8)
e = engine.Engine(blob, 0, tile=args.tile, sep_gen=getattr(args, "gen", 2))
B, T = args.batch, 512
x = torch.from_numpy(synth.make_features(B, 64, T, 1)).cuda()
lens = torch.full((B,), 500)
for _ in range(3):
    e.forward(x, lens)
torch.cuda.synchronize()
lib = engine.load_library()
buf = torch.zeros(32, dtype=torch.int64, device='cuda')
lib.qasr_debug_prof(C.c_void_p(buf.data_ptr()))
labels = e.op_labels()
paired = e.op_paired()
seen = {}
for oi, lab in enumerate(labels):
    if lab.startswith('k_sep'):
        seen[lab + (' paired' if paired[oi] else '')] = oi    # last op of every instantiation
PRO = ('start', 'arguments', 'constants', 'group0_requested', 'dw_params_requested', 'group0_back', 'rows_to_lds', 'first_mfma')
rec = {}
for lab, oi in seen.items():
    buf.zero_()
    for _ in range(3):
        e.run_op(oi)
    torch.cuda.synchronize()
    st = buf.cpu().numpy()
    n = int(st[31])
    deltas = [int(st[i + 1] - st[i]) for i in range(n - 1)]
    print(f'{lab:41s} op {oi:3d} stamps {n:2d} total {int(st[n - 1] - st[0]):6d}  deltas {deltas}')
    rec[lab] = dict(op=oi, total=int(st[n - 1] - st[0]), deltas=deltas)
    if args.prologue and st[29]:
        # slots 24.. hold the prologue's own points, slot 29 the wave's first instruction; stamps 1 - 3 of the ordinary list
        # are `group 0 requested`, `group 0 back` and `first MFMA` (a bare 1x1 layer has no depthwise stage: stamp 1 only)
        t = dict(start=st[0], arguments=st[24], constants=st[25], group0_requested=st[1], dw_params_requested=st[26],
                 group0_back=st[2], rows_to_lds=st[27], first_mfma=st[3])
        if lab.startswith('k_sep2<0,'):
            t = dict(start=st[0], arguments=st[24], constants=st[25], group0_requested=st[1], dw_params_requested=st[26])
        pro = {k: int(t[k] - st[29]) for k in PRO if k in t and t[k]}
        print(f'{"":41s} prologue, cycles from the first instruction: {pro}')
        rec[lab]['prologue'] = pro
if args.json:
    doc = json.load(open(args.json)) if os.path.exists(args.json) else {}
    doc.setdefault('phase_stamps', {})[args.tag] = dict(tile=args.tile, batch=args.batch, lib=os.environ.get('QASR_LIB', 'default'),
                                                        GPU_MAX_HW_QUEUES=os.environ.get('GPU_MAX_HW_QUEUES'), kernels=rec)
    with open(args.json, 'w') as fh:
        json.dump(doc, fh, indent=1)
lib.qasr_debug_prof(C.c_void_p(0))
e.close()
