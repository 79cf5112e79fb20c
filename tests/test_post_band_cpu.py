"""CTC posteriors inside the band on the host: qasr.align.post_band_host (the NumPy statement k_post_band follows) against
post_host where the band is the whole lattice or costs nothing, against an independent float64 forward-backward over the
restricted lattice where it does cost, its exact cases, the star identity, invalid rows, and align_long(posteriors=True) on
host modules."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_band_cases as abc  # noqa: E402
import align_cases  # noqa: E402
import align_long_cases as alc  # noqa: E402
import post_band_cases as pbc  # noqa: E402
import post_cases as pc  # noqa: E402
import star_cases as sc  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import align  # noqa: E402
from qasr.beam import NEG, ONE, Q_FLOOR  # noqa: E402


def _zero_row(post, p):
    return post.ok[p] == 0 and post.total[p] == NEG and not post.frame_post[p].any() and not post.label_post[p].any()


# --------------------------------------------------------------------------------------------------------- static band
def test_a_band_that_holds_every_state_is_post_host_on_every_byte():
    lp, y = abc.synth(5, 60, a=3.0, per_label=(1, 3), gap=(0, 2), tail=2)
    T = lp.shape[0]
    rng = np.random.Generator(np.random.PCG64(3))
    rows = [y, [], y[:17], sc.labels_without_blank(rng, 127, abc.C, abc.BLANK, repeats=0.3), y[:5], []]       # S = 255 is the widest
    tg, tl = align_cases.pad_targets(rows, abc.BLANK)
    batch = np.stack([lp, lp, lp[::-1], lp, lp, lp])
    for lens in (None, np.array([T, T - 9, 40, T, 0, 0], dtype=np.int32), np.array([T + 5, 1, T, 254, 4, -3], dtype=np.int32)):
        for bw in (256, 1024):
            res, got = pbc.band_and_post(batch, lens, tg, tl, abc.BLANK, bw)
            assert not res.band_base.any()
            full, want = pc.align_and_post(batch, lens, tg, tl, abc.BLANK)
            sc.same_bytes(res, full, ('start', 'nframes', 'ok'))
            pc.same_bytes(got, want, (bw, None if lens is None else lens.tolist()))
            assert got.ok.sum() >= 4 and got.ok[1] == got.ok[5] == 1
    assert got.total[5] == 0 and got.total[4] == NEG                # lim == 0: without labels the empty path, with labels none


# --------------------------------------------------------------------------------------------------------- moving band
def _committed(name):
    if name in abc.MOVING:
        lp, lens, tg, tl = abc.moving_case(name)
        return 256, lp, lens, tg, tl
    bw, lp, tg, tl = abc.device_case(name)
    return bw, lp, None, tg, tl


@pytest.mark.parametrize('name', list(abc.MOVING) + ['bw256_S1201', 'bw1024_S2401'])
def test_the_band_costs_nothing_on_the_committed_cases(name):
    """the mass outside the band lies below the table's 16-nat cutoff at every cell that matters: total, frame_post and
    label_post are the full lattice's on every byte, although the base takes many values"""
    bw, lp, lens, tg, tl = _committed(name)
    res, got = pbc.band_and_post(lp, lens, tg, tl, abc.BLANK, bw)
    full, want = pc.align_and_post(lp, lens, tg, tl, abc.BLANK)
    print(name, 'T', lp.shape[1], 'S', 2 * int(tl[0]) + 1, 'bases', pbc.n_bases(res), 'lowest frame_post / 2^16', got.frame_post.min() / ONE)
    assert pbc.n_bases(res) >= 10 and res.ok[0] == 1 and got.ok[0] == 1
    sc.same_bytes(res, full, ('start', 'nframes', 'ok'))
    assert got.total.dtype == np.int64 and got.total.tobytes() == full.total.tobytes()
    pc.same_bytes(got, want, name)
    assert got.frame_post.min() < 0


def test_the_noisy_case_against_the_float64_oracle_of_the_restricted_lattice():
    """At a = 0.5 the band follows another path than the full lattice's and total is that of the restricted lattice, so the
    yardstick is the float64 forward-backward over the same cells and edges.  The bound is post_cases.bound(lim) = 131 lim /
    2^16 nat, and its derivation (test_post_cpu.test_frame_post_against_the_float64_oracle) carries over unchanged: per frame
    each pass still rounds q once and looks the table up at most twice per cell, over a subset of the terms of the full step
    (a missing term is NEG on both sides, where lae is exact), lae is 1-Lipschitz in each argument, and total adds one more
    look-up - so e_A(t) <= 0.5 + 65.5 t, e_B(t) <= 0.5 + 65.5 (lim - 1 - t), e_total <= 65.5 lim - 32.5 as there."""
    lp, tg, tl = pbc.noisy_case()
    T, L = lp.shape[1], int(tl[0])
    assert T == 1421
    res, post = pbc.band_and_post(lp, None, tg, tl, abc.BLANK, 256)
    full = align.align_host(lp, None, tg, tl, abc.BLANK)
    assert res.ok[0] == 1 and post.ok[0] == 1 and pbc.n_bases(res) >= 10
    got = pbc.oracle_post_band(lp[0], tg[0, :L], abc.BLANK, pbc.frame_bases(res.band_base[0], T), 256)
    assert got is not None
    gamma, total = got
    states = pc.path_states(res.start[0], res.nframes[0], L, T)
    want = gamma[np.arange(T), states]
    fp = post.frame_post[0].astype(np.int64)
    free = (fp < 0) & (fp > Q_FLOOR)                                # the clamp is inactive
    diff = float(np.abs(fp[free] / ONE - want[free]).max())
    print(f'T {T} L {L}: largest |frame_post - oracle| {diff:.6f} nat, bound {pc.bound(T):.4f}; {int((~free).sum())} frames at the clamp; '
          f'total {post.total[0] / ONE:.4f}, oracle {total:.4f}, full lattice {full.total[0] / ONE:.4f}, path {res.path_score[0] / ONE:.4f}')
    assert free.sum() > T // 2 and np.isfinite(want).all()
    assert (want[~free] >= -pc.bound(T)).all()
    assert diff <= pc.bound(T)
    assert abs(post.total[0] / ONE - total) <= pc.bound(T)
    assert res.path_score[0] <= post.total[0] <= full.total[0] + int(np.ceil(pc.bound(T) * ONE))
    assert post.total[0] < full.total[0]                            # the restriction is exercised
    for i in range(L):
        a, n = int(res.start[0, i]), int(res.nframes[0, i])
        assert post.label_post[0, i] == post.frame_post[0, a:a + n].min()


def test_the_oracle_of_the_restricted_lattice_passes_its_own_checks():
    """with a band that holds every state it is post_cases.oracle_post; per frame the posteriors over the band's cells sum to 1"""
    lp, y = abc.synth(6, 40, a=1.0, per_label=(1, 2), gap=(0, 2), tail=2)
    T = lp.shape[0]
    gamma, total = pbc.oracle_post_band(lp, y, abc.BLANK, np.zeros(T, dtype=np.int64), 256)
    g2, t2 = pc.oracle_post(lp, y, abc.BLANK)
    assert abs(total - t2) <= 1e-9 * abs(t2) and np.abs(np.exp(gamma) - np.exp(g2)).max() <= 1e-9
    lp, tg, tl = pbc.noisy_case()                                   # 150 labels on 400 frames: S = 301, top = 45
    bases = pbc.frame_bases(np.minimum(np.arange(13) * 5, 45), 400)
    gamma, _ = pbc.oracle_post_band(lp[0, :400], tg[0, :150], abc.BLANK, bases, 256)
    assert np.abs(np.exp(gamma).sum(axis=1) - 1.0).max() <= 1e-9
    assert (gamma[390:, :45] == -np.inf).all() and (gamma[:32, 256:] == -np.inf).all()


@pytest.mark.parametrize('L', [129, 200])
def test_equal_labels_on_the_fewest_frames_have_one_path(L):
    T, C, blank = 2 * L - 1, 3, 2
    rng = np.random.Generator(np.random.PCG64(L))
    z = rng.standard_normal((T, C))
    z[np.arange(T), np.where(np.arange(T) % 2 == 0, 1, blank)] += 4.0   # the one path is also the likely one: the band keeps it
    lp = (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)[None]
    tg, tl = align_cases.pad_targets([[1] * L], blank)
    res, post = pbc.band_and_post(lp, None, tg, tl, blank, 256)
    assert 2 * L + 1 > 256 and res.ok[0] == 1 and res.nframes[0].tolist() == [1] * L and pbc.n_bases(res) > 1
    assert post.ok[0] == 1 and post.total[0] == res.path_score[0]
    assert not post.frame_post.any() and not post.label_post.any()


# ------------------------------------------------------------------------------------------------------- star identity
def test_with_a_plane_it_is_the_call_on_the_augmented_matrix():
    lp, tg, tl, blank, bw = sc.moving_band_case()
    T = lp.shape[1]
    for lens in (None, np.array([T - 100], dtype=np.int32)):
        star = align.star_host(lp, lens, 1.5)
        res, got = pbc.band_and_post(lp, lens, tg, tl, blank, bw, star=star)
        res2, want = pbc.band_and_post(sc.augmented(lp, star), lens, tg, tl, blank, bw)
        assert res.ok[0] == 1 and got.ok[0] == 1 and pbc.n_bases(res) > 3 and got.frame_post.min() < 0
        sc.same_bytes(res, res2, sc.BAND_FIELDS)
        pc.same_bytes(got, want, 'star')
        bare = pbc.post_band(lp, lens, tg, tl, blank, res)          # without the plane the wildcard's id is no label
        assert _zero_row(bare, 0)


# -------------------------------------------------------------------------------------------------------- invalid rows
def test_invalid_rows_are_zero_and_leave_the_other_row_alone():
    lp, lens, tg, tl, res, good = pbc.pair_case()
    lim = int(lens[1])
    variants = pbc.invalid_bands(res, tg, tl, 1, lim)
    for name, (st, nf, ok) in pc.invalid_paths(res, tg, tl, 1, lim).items():
        variants[name] = (st, nf, ok, res.band_base)
    assert len(variants) == 18
    n_control = 0
    for name, (st, nf, ok, bb) in variants.items():
        got = pbc.post_band(lp, lens, tg, tl, abc.BLANK, res, start=st, nframes=nf, ok=ok, band_base=bb)
        for f in pc.POST_FIELDS:
            assert getattr(got, f)[0].tobytes() == getattr(good, f)[0].tobytes(), (name, f)
        if name.startswith('control'):
            n_control += 1
            assert got.ok[1] == 1 and got.total[1] != NEG and got.total[1] <= good.total[1] + 64, name
        else:
            assert _zero_row(got, 1), name
    assert n_control == 3
    # the targets align_band_host refuses are refused here, whatever the path says
    for bad_tl in (None, -1, tg.shape[1] + 1):
        tg2, tl2 = tg.copy(), tl.copy()
        if bad_tl is None:
            tg2[1, 3] = abc.BLANK
        else:
            tl2[1] = bad_tl
        got = pbc.post_band(lp, lens, tg2, tl2, abc.BLANK, res, ok=np.ones(2, dtype=np.int32))
        assert got.ok.tolist() == [1, 0] and _zero_row(got, 1)
    with pytest.raises(ValueError, match='band_base'):
        pbc.post_band(lp, lens, tg, tl, abc.BLANK, res, band_base=res.band_base[:, :5])
    with pytest.raises(ValueError, match='band_states'):
        align.post_band_host(lp, lens, tg, tl, abc.BLANK, res.start, res.nframes, res.ok, res.band_base, 512)


# ---------------------------------------------------------------------------------------------------------- the facade
_m = None


def _model():
    global _m
    if _m is None:
        torch.set_grad_enabled(False)
        _m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
        _m.eval()
        _m.preprocessor.featurizer.dither = 0.0
        _m.set_quant_mode('none')
    return _m


def test_facade_align_long_with_posteriors_on_host_modules():
    pbc.check_facade(_model(), 'cpu')


def test_the_tool_appends_the_segments_posterior(tmp_path):
    """--posteriors: one more field per line; without the flag the file is byte for byte what it was"""
    extra = ['--no_quant', '--device', 'cpu']
    (tmp_path / 'a').mkdir(), (tmp_path / 'b').mkdir()
    alc.check_tool_output(tmp_path / 'a', extra)
    plain = (tmp_path / 'a' / 'out' / 'segments' / '8000_talk_segments.txt').read_text(encoding='utf-8').splitlines()
    import subprocess
    data = tmp_path / 'a' / 'data'
    out = subprocess.run([sys.executable, alc.TOOL, '--data', str(data), '--output_dir', str(tmp_path / 'b'), '--model', 'MiniQuartzNet',
                          '--synthetic_model', '--window_s', '4', '--window_len', '8000', '--posteriors'] + extra,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = (tmp_path / 'b' / 'segments' / '8000_talk_segments.txt').read_text(encoding='utf-8').splitlines()
    assert lines[0] == plain[0] and len(lines) == len(plain) == 4
    for ln, was in zip(lines[1:], plain[1:]):
        head, _, post = ln.rpartition(' | ')
        assert head == was and 0.0 <= float(post) <= 1.0
