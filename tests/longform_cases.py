"""Shared inputs of the long-recording tests (CPU and GPU): small plans in frames, random global rows cut into window rows
(the slice property), windows that disagree everywhere (structure only) and the checks both test files apply."""
import numpy as np

from qasr import longform as lf

SPF = 320
RATE = 16000
BLANK = 28


def plan_frames(lens_samples, window_f, overlap_f, guard_f, frames_of=None):
    """a WindowPlan stated in frames (times that round to exactly these counts)"""
    return lf.WindowPlan(lens_samples, window_f * SPF / RATE, overlap_f * SPF / RATE, guard_f * SPF / RATE, RATE, SPF, frames_of)


def rec_lens(plan_args, windows, ragged=True):
    """sample counts of recordings with the given window counts (the last window ragged: neither full nor frame-aligned)"""
    Wl, H, Ov = plan_args['window_f'] * SPF, (plan_args['window_f'] - plan_args['overlap_f']) * SPF, plan_args['overlap_f'] * SPF
    out = []
    for i, n in enumerate(windows):
        if n == 1:
            out.append(Wl - 37 * (i + 1) if ragged else Wl)
        else:
            tail = Ov + 1 + (53 * (i + 3)) % (H - 1) if ragged else H      # the last window: Ov < samples <= Ov + H
            out.append(Wl + (n - 2) * H + tail - Ov)
    return out


def plane_rows(rng, shape, bpf):
    """random bytes as int32 words [..., bpf / 4]"""
    return rng.integers(-2 ** 31, 2 ** 31 - 1, size=shape + (bpf // 4,), dtype=np.int64).astype(np.int32)


def scores(rng, shape, ties=False):
    """negative float32 'log-probabilities'; ties: a few distinct values with both zeros among them, so equal sums abound"""
    if ties:
        return rng.choice(np.array([-0.0, 0.0, -0.5, -0.25, -1.0], dtype=np.float32), size=shape)
    return -np.abs(rng.standard_normal(shape)).astype(np.float32)


def slice_case(plan, Tw, seed, bpfs=(), ties=False, p_blank=0.5):
    """Global rows per recording cut into window rows: window w holds global frames first_frame(w) .. + enc[w]) and noise
    behind them.  Returns dict(tokens, frame_score, planes, enc, want=[tokens, frame_score, *planes] global, total)."""
    rng = np.random.default_rng(seed)
    G = plan.Tmax + Tw + 1
    gtok = np.where(rng.random((plan.R, G)) < p_blank, BLANK, rng.integers(0, BLANK, (plan.R, G))).astype(np.int32)
    gfs = scores(rng, (plan.R, G), ties)
    gpl = [plane_rows(rng, (plan.R, G), b) for b in bpfs]
    tok = rng.integers(0, BLANK + 1, (plan.Wn, Tw)).astype(np.int32)
    fs = scores(rng, (plan.Wn, Tw), ties)
    pls = [plane_rows(rng, (plan.Wn, Tw), b) for b in bpfs]
    enc = np.zeros(plan.Wn, dtype=np.int32)
    total = np.zeros(plan.R, dtype=np.int32)
    Hf, Of, g = plan.hop_frames, plan.overlap_frames, plan.guard
    for w, (r, _, n, f0) in enumerate(plan.table.tolist()):
        last = w == plan.first[r] + plan.count[r] - 1
        hi = min(Tw, plan.frames_of(n), 2 * Hf)
        lo = min(hi, max(1, n // SPF)) if last else Hf + 2 * g + 1   # a window reaches its right neighbour, past the guards
        enc[w] = rng.integers(lo, hi + 1)
        e = int(enc[w])
        tok[w, :e], fs[w, :e] = gtok[r, f0:f0 + e], gfs[r, f0:f0 + e]
        for p, gp in zip(pls, gpl):
            p[w, :e] = gp[r, f0:f0 + e]
        if last:
            total[r] = f0 + e
    want = []
    for i, gp in enumerate([gtok, gfs] + gpl):
        o = np.zeros((plan.R, plan.Tmax) + gp.shape[2:], dtype=gp.dtype)
        if i == 0:
            o[...] = BLANK
        for r in range(plan.R):
            o[r, :total[r]] = gp[r, :total[r]]
        want.append(o)
    return dict(tokens=tok, frame_score=fs, planes=pls, enc=enc, want=want, total=total)


def garbage_case(plan, Tw, seed, ties=True):
    """windows that agree on nothing, lengths of every kind (negative, 0, beyond Tw); plane 0 tags every frame with its
    (window, frame) so the owner of each output frame can be read back"""
    rng = np.random.default_rng(seed)
    tok = rng.integers(0, BLANK + 1, (plan.Wn, Tw)).astype(np.int32)
    fs = scores(rng, (plan.Wn, Tw), ties)
    enc = rng.integers(-2, Tw + 4, plan.Wn).astype(np.int32)
    tag = ((np.arange(plan.Wn)[:, None] + 1) * 65536 + np.arange(Tw)[None, :]).astype(np.int32)[:, :, None]
    return dict(tokens=tok, frame_score=fs, planes=[tag], enc=enc)


def check_structure(plan, Tw, case, out, total, seams):
    """what holds for ANY inputs: seams ascend from each window's first frame, every frame before total_frames comes from the
    one window that owns it (or is fill where that window is too short), and the tails are blank / zero"""
    enc = np.clip(case['enc'].astype(np.int64), 0, min(Tw, 2 * plan.hop_frames))
    tag = out[-1][:, :, 0]
    for r in range(plan.R):
        w0, n = int(plan.first[r]), int(plan.count[r])
        last = w0 + n - 1
        assert seams[w0] == 0
        assert total[r] == min(plan.table[last, 3] + enc[last], plan.Tmax)
        edges = [int(seams[w]) for w in range(w0, w0 + n)] + [int(total[r])]
        for k, w in enumerate(range(w0, w0 + n)):
            f0 = int(plan.table[w, 3])
            assert f0 <= edges[k] <= edges[k + 1], (r, w, edges)
            for g in range(min(edges[k], plan.Tmax), min(edges[k + 1], plan.Tmax)):
                if g < f0 + enc[w]:
                    assert tag[r, g] == (w + 1) * 65536 + g - f0, (r, w, g)
                    assert out[0][r, g] == case['tokens'][w, g - f0]
                else:
                    assert tag[r, g] == 0 and out[0][r, g] == BLANK, (r, w, g)
        assert (out[0][r, total[r]:] == BLANK).all()
        for o in out[1:]:
            assert not o[r, total[r]:].view(np.uint8).any()


def window_outputs(m, plan, audio, lens, batch_size):
    """(tokens, frame scores, encoded lengths) of every window of the plan from the model's own forward, in decode_long's
    batches: windows cut by the twin, each batch through the path the model serves"""
    import torch
    win, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
    toks, fss, encs = [], [], []
    for i in range(0, plan.Wn, batch_size):
        sig = torch.from_numpy(win[i:i + batch_size]).to(audio.device)
        ln = torch.from_numpy(wl[i:i + batch_size]).to(audio.device).long()
        t, f, e = m._forward(sig, ln, decode='frames')
        toks.append(t.cpu().numpy().astype(np.int32))
        fss.append(f.cpu().numpy().astype(np.float32))
        encs.append(e.cpu().numpy().astype(np.int32))
    return np.concatenate(toks), np.concatenate(fss), np.concatenate(encs)


def compose_on_host(m, audio, lens, window_s, overlap_s, guard_s, batch_size, seam='blank'):
    """decode_long restated with the twins over the model's own per-window forward outputs"""
    from qasr import ctc
    plan = m._long_plan(lens.cpu().numpy(), window_s, overlap_s, guard_s)
    tok, fs, enc = window_outputs(m, plan, audio, lens, batch_size)
    blank = len(m.decoder.vocabulary)
    out, total, seams = lf.stitch_host(plan, enc, tok, fs, (), blank, seam)
    spf = m.seconds_per_frame()
    hyps = ctc.to_hypotheses(ctc.collapse_host(out[0], out[1], total, blank=blank), m.decoder.vocabulary, spf)
    for r, h in enumerate(hyps):
        if plan.count[r] > 1:
            h.seams_s = [float(seams[w]) * spf for w in range(plan.first[r] + 1, plan.first[r] + plan.count[r])]
    return plan, hyps, dict(tokens=tok, frame_score=fs, enc=enc, out=out, total=total, seams=seams)
