"""Shared by the banded posterior tests on the CPU and on the GPU (qasr.align.post_band_host, k_post_band): an independent
float64 forward-backward over the lattice restricted to a band trajectory, helpers that chain align_band_host -> post_band_host,
and the rows that POST_BAND_RULES calls invalid.  NumPy only.

The oracle is written plainly: one loop over frames, every state addressed by its own number, a mask for the cells that exist,
numpy.logaddexp, no table, no fixed point, no window that shifts.  It shares nothing with qasr/align.py but the rules."""
import math

import numpy as np

import align_band_cases as abc
import post_cases as pc
from qasr import align

NEGF = -math.inf
BLOCK = 32


def frame_bases(band_base_row, T):
    """base(t) for t < T from one row of band_base"""
    return np.asarray(band_base_row, dtype=np.int64)[np.arange(T) // BLOCK]


def oracle_post_band(logp, y, blank, bases, BW):
    """float64 log-posteriors gamma [T, S] (-inf where there is no cell) given y and the restricted lattice, and its total;
    bases: base(t) for every frame of logp.  None when no alignment stays inside the band."""
    lp = np.asarray(logp, dtype=np.float64)
    T = lp.shape[0]
    L = len(y)
    S = 2 * L + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    may_skip = np.zeros(S, dtype=bool)                              # s may be entered from s - 2
    if L > 1:
        may_skip[3::2] = np.asarray(y[1:]) != np.asarray(y[:-1])
    s_all = np.arange(S)
    cell = [(s_all >= int(bases[t])) & (s_all < min(int(bases[t]) + BW, S)) for t in range(T)]
    al = np.full((T, S), NEGF)
    be = np.full((T, S), NEGF)
    al[0, :min(2, S)] = lp[0, lab[:min(2, S)]]
    al[0, ~cell[0]] = NEGF
    for t in range(1, T):
        src = np.where(cell[t - 1] & (s_all >= int(bases[t])), al[t - 1], NEGF)      # an edge leaves only these cells
        acc = src.copy()
        acc[1:] = np.logaddexp(acc[1:], src[:-1])
        acc[2:] = np.logaddexp(acc[2:], np.where(may_skip[2:], src[:-2], NEGF))
        al[t] = np.where(cell[t], acc + lp[t, lab], NEGF)
    for s in range(max(S - 2, 0), S):
        if cell[T - 1][s]:
            be[T - 1, s] = lp[T - 1, lab[s]]
    for t in range(T - 2, -1, -1):
        dst = be[t + 1]                                             # -inf outside the band of t + 1
        acc = dst.copy()
        acc[:-1] = np.logaddexp(acc[:-1], dst[1:])
        acc[:-2] = np.logaddexp(acc[:-2], np.where(may_skip[2:], dst[2:], NEGF))
        acc[s_all < int(bases[t + 1])] = NEGF                       # no edge leaves a cell below the next base
        be[t] = np.where(cell[t], acc + lp[t, lab], NEGF)
    total = float(np.logaddexp.reduce(al[T - 1, max(S - 2, 0):]))
    if total == NEGF:
        return None
    with np.errstate(invalid='ignore'):
        gamma = al + be - lp[:, lab] - total
    gamma[np.isnan(gamma)] = NEGF
    return gamma, total


def band_and_post(lp, lens, tg, tl, blank, bw, star=None):
    """(align_band_host's result, post_band_host's result on its path and its band)"""
    res = align.align_band_host(lp, lens, tg, tl, blank, band_states=bw, star=star)
    return res, post_band(lp, lens, tg, tl, blank, res, star=star)


def post_band(lp, lens, tg, tl, blank, res, star=None, start=None, nframes=None, ok=None, band_base=None):
    """post_band_host on `res`, any of its four arrays replaced"""
    return align.post_band_host(lp, lens, tg, tl, blank, res.start if start is None else start,
                                res.nframes if nframes is None else nframes, res.ok if ok is None else ok,
                                res.band_base if band_base is None else band_base, res.band_states, star=star)


def n_bases(res, p=0):
    return len(set(np.asarray(res.band_base)[p].tolist()))


_made = {}


def noisy_case(a=0.5):
    """the issue's noisy recording: (logp [1, T, C], targets, target_lens); T = 1421 at band 256"""
    key = ('noisy', a)
    if key not in _made:
        lp, y = abc.synth(31, 400, a=a, per_label=(1, 3), gap=(0, 3), tail=4)
        _made[key] = (lp[None], np.array([y], dtype=np.int32), np.array([len(y)], dtype=np.int32))
    return _made[key]


def pair_case():
    """Two recordings in one batch at band 256, both with a moving band: (lp [2, T, C], lens, tg, tl, res, good).  Row 1 is the
    one the invalid-row tests break: one label frame and one blank frame per label (the path climbs one state per frame), its
    labels 1 and 2 equal, and 200 frames of slack behind the last label."""
    if 'pair' not in _made:
        lp0, y0 = abc.synth(41, 330, a=4.0, per_label=(1, 3), gap=(0, 2), tail=3)
        lp1, y1 = abc.synth(42, 300, a=4.0, per_label=(1, 1), gap=(1, 1), tail=200)
        y1[2] = y1[1]
        T = max(lp0.shape[0], lp1.shape[0])
        lp = np.full((2, T, abc.C), np.float32(-math.log(abc.C)), dtype=np.float32)
        lp[0, :lp0.shape[0]], lp[1, :lp1.shape[0]] = lp0, lp1
        lens = np.array([lp0.shape[0], lp1.shape[0]], dtype=np.int32)
        tg = np.full((2, max(len(y0), len(y1))), abc.BLANK, dtype=np.int32)
        tg[0, :len(y0)], tg[1, :len(y1)] = y0, y1
        tl = np.array([len(y0), len(y1)], dtype=np.int32)
        res, good = band_and_post(lp, lens, tg, tl, abc.BLANK, 256)
        assert res.ok.tolist() == [1, 1] and good.ok.tolist() == [1, 1] and n_bases(res, 0) > 3 and n_bases(res, 1) > 3
        _made['pair'] = (lp, lens, tg, tl, res, good)
    return _made['pair']


def _trajectory(states, nblk, top, margin, at=None, value=None):
    """a band_base row that keeps `states` (the path, one per frame) `margin` states above the base; block `at` gets `value`"""
    bb = np.zeros(nblk, dtype=np.int64)
    for k in range(1, nblk):
        bb[k] = max(bb[k - 1], min(top, max(0, int(states[BLOCK * k]) - margin)))
        if k == at:
            bb[k] = value
    return bb.astype(np.int32)


def invalid_bands(res, tg, tl, p, lim, BW=256):
    """name -> (start, nframes, ok, band_base) with row p invalid in each of the ways POST_BAND_RULES adds to POST_RULES, and
    'control: ...' entries that are valid (the same construction without the fault)"""
    L = int(tl[p])
    top = 2 * L + 1 - BW
    nblk = (lim + BLOCK - 1) // BLOCK
    base = np.asarray(res.band_base)
    assert top > 0 and res.ok[p] == 1
    j = int(np.flatnonzero(base[p, :nblk] > 0)[0])                  # the first block whose base has moved
    assert 1 <= j < nblk - 2
    out = {}

    def variant(name):
        st, nf, ok, bb = res.start.copy(), res.nframes.copy(), res.ok.copy(), base.copy()
        out[name] = (st, nf, ok, bb)
        return st, nf, bb
    _, _, bb = variant('a decreasing base')
    bb[p, j + 1] = bb[p, j] - 1
    _, _, bb = variant('a step of BW / 2')
    bb[p, j:nblk] = np.maximum(bb[p, j:nblk], bb[p, j - 1] + BW // 2)
    assert bb[p, j] - bb[p, j - 1] == BW // 2 and bb[p, :nblk].max() <= top
    _, _, bb = variant('control: a step of BW / 2 - 1')
    bb[p, j:nblk] = np.maximum(bb[p, j:nblk], bb[p, j - 1] + BW // 2 - 1)
    _, _, bb = variant('a base above top')
    bb[p, nblk - 1] = top + 1
    _, _, bb = variant('a negative base')
    bb[p, 1] = -1
    _, _, bb = variant('INT_MAX')
    bb[p, nblk - 2] = 2 ** 31 - 1
    _, _, bb = variant('INT_MIN')
    bb[p, nblk - 2] = -2 ** 31
    _, _, bb = variant('base[0] != 0')
    bb[p, 0] = 1
    # the path 180 frames late: still a CTC alignment of the target over lim frames, but 180 states below where the band is
    st, nf, _ = variant('a path shifted out of the band')
    st[p, :L] += 180
    assert pc.align_cases.path_is_valid(st[p, :L], nf[p, :L], [int(c) for c in tg[p, :L]], lim)
    # another trajectory around the same path (64 states of margin), valid; then with one base put exactly on the state the path
    # has at the first frame of block k: if the path climbed into that state at that frame, its cell of the frame before lies
    # below the new base and has no edge out
    states = pc.path_states(res.start[p], res.nframes[p], L, lim)
    k = next(k for k in range(j + 1, nblk - 1) if states[BLOCK * k] > states[BLOCK * k - 1] and states[BLOCK * k] <= top)
    _, _, bb = variant('control: another trajectory')
    bb[p, :nblk] = _trajectory(states, nblk, top, 64)
    _, _, bb = variant('control: a base on the state the path leaves')
    bb[p, :nblk] = _trajectory(states, nblk, top, 64, k, int(states[BLOCK * k - 1]))
    _, _, bb = variant('a path through a dead-end cell')
    bb[p, :nblk] = _trajectory(states, nblk, top, 64, k, int(states[BLOCK * k]))
    return out


# ---- the façade: align_long(posteriors=True) against the host chain, shared by the CPU and the GPU test
def host_chain(m, audio, lens, rows, band_states=None):
    """the host statement of align_long(posteriors=True) over the model's own per-window forward outputs: align_long_cases'
    twin_chain (cut_host, forward per batch, stitch_host, align_band_host) and post_band_host behind it on the same stitched
    log-probabilities: (BandResult, PostResult, frames per recording)"""
    import torch

    import align_long_cases as alc
    from qasr import longform as lf
    plan = m._long_plan(lens.cpu().numpy(), **alc.KW)
    win, wl = lf.cut_host(audio.cpu().numpy(), lens.cpu().numpy(), plan)
    toks, fss, encs, lps = [], [], [], []
    for i in range(0, plan.Wn, alc.BATCH):
        logp, e, t = m(input_signal=torch.from_numpy(win[i:i + alc.BATCH]).to(audio.device),
                       input_signal_length=torch.from_numpy(wl[i:i + alc.BATCH]).to(audio.device).long())
        toks.append(t.cpu().numpy().astype(np.int32)), encs.append(e.cpu().numpy().astype(np.int32))
        fss.append(logp.float().gather(2, t.long().unsqueeze(-1)).squeeze(-1).cpu().numpy())
        lps.append(logp.float().cpu().numpy())
    blank = len(m.decoder.vocabulary)
    out, total, _ = lf.stitch_host(plan, np.concatenate(encs), np.concatenate(toks), np.concatenate(fss), [np.concatenate(lps)], blank)
    tg = np.full((len(rows), max(1, max(len(r) for r in rows))), blank, dtype=np.int32)
    for i, r in enumerate(rows):
        tg[i, :len(r)] = r
    tl = np.array([len(r) for r in rows], dtype=np.int32)
    res, post = band_and_post(out[2], total, tg, tl, blank, align.pick_band_states(tg.shape[1], band_states))
    return res, post, total


def check_facade(m, device):
    """align_long(posteriors=True): every new field is the host chain's, nothing else changes, and without the argument the
    call returns what it did"""
    import torch

    import align_long_cases as alc
    ONE = align.ONE
    audio, lens = alc.recordings(device)
    greedy = m.decode_long(audio, lens, batch_size=alc.BATCH, **alc.KW)
    ids = greedy[0].labels
    a, b = len(ids) // 3, 2 * len(ids) // 3
    parts = [ids[:a], ids[a:b], ids[b:]]
    vocab = list(m.decoder.vocabulary)
    gap = [vocab.index(' ')] if ' ' in vocab else []
    joined = parts[0] + gap + parts[1] + gap + parts[2]
    rows = [parts, greedy[1].labels]
    plain = m.align_long(audio, lens, labels=rows, batch_size=alc.BATCH, **alc.KW)
    off = m.align_long(audio, lens, labels=rows, batch_size=alc.BATCH, posteriors=False, **alc.KW)
    got = m.align_long(audio, lens, labels=rows, batch_size=alc.BATCH, posteriors=True, **alc.KW)

    def fields(h):
        return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words, h.lm_score, h.boost_score, h.seams_s,
                None if h.segments is None else [(s.text, s.start_s, s.end_s, s.score) for s in h.segments])
    assert [fields(h) for h in plain] == [fields(h) for h in off] == [fields(h) for h in got]
    for h in plain + off:                                           # without the argument: what it was
        assert h.ctc_score is None and h.post is None and h.post_min is None and h.word_post is None and h.frame_post is None
        assert h.segments is None or all(s.post is None for s in h.segments)
    res, post, frames = host_chain(m, audio, lens, [joined, greedy[1].labels])
    assert res.ok.tolist() == [1, 1] and post.ok.tolist() == [1, 1] and post.frame_post.min() < 0
    for r, h in enumerate(got):
        lim, n = int(frames[r]), len(h.labels)
        assert h.frame_post.dtype == np.float32 and h.frame_post.tolist() == (post.frame_post[r, :lim] / ONE).astype(np.float32).tolist()
        assert h.ctc_score == post.total[r] / ONE and h.utt_score <= h.ctc_score + 1e-3
        pr = np.exp(post.frame_post[r, :lim].astype(np.float64) / ONE)
        assert len(h.post) == len(h.post_min) == n and len(h.word_post) == len(h.words)
        for i in range(n):
            run = pr[res.start[r, i]:res.start[r, i] + res.nframes[r, i]]
            assert h.post[i] == float(run.mean()) and h.post_min[i] == float(run.min()) and 0.0 <= h.post_min[i] <= h.post[i] <= 1.0
        assert all(0.0 <= w <= 1.0 for w in h.word_post)
    assert got[1].segments is None and len(got[0].segments) == 3
    pr = np.exp(post.frame_post[0].astype(np.float64) / ONE)
    at = 0
    for seg, part in zip(got[0].segments, parts):
        f0 = int(res.start[0, at])
        f1 = int(res.start[0, at + len(part) - 1] + res.nframes[0, at + len(part) - 1])
        assert seg.post == float(pr[f0:f1].mean()) and 0.0 <= seg.post <= 1.0
        at += len(part) + len(gap)
    # a lost alignment keeps empty lists, and its segments have no value
    lost = m.align_long(audio[1:, :8000].contiguous(), torch.tensor([8000]).to(device), labels=[[ids[:20], ids[20:40]]],
                        posteriors=True, **alc.KW)[0]
    assert lost.start_s == [] and lost.post == [] and lost.post_min == [] and lost.word_post == [] and len(lost.frame_post) == 0
    assert lost.ctc_score == float('-inf')
    assert [(s.start_s, s.end_s, s.score, s.post) for s in lost.segments] == [(None, None, float('-inf'), None)] * 2
    # with a wildcard between the utterances: values for the wildcards' words too, ctc_score None as in align
    star = m.align_long(audio[:1], lens[:1], labels=[parts], batch_size=alc.BATCH, star_between=True, posteriors=True, **alc.KW)[0]
    assert star.ctc_score is None and len(star.word_post) == len(star.words) and len(star.post) == len(star.labels)
    assert all(0.0 <= v <= 1.0 for v in star.post + star.word_post) and all(0.0 <= s.post <= 1.0 for s in star.segments)
    return got
