"""What the Python bindings of the seven CTC lattice entry points (qasr.engine.ctc_align, ctc_post, ctc_align_band,
ctc_post_band, ctc_star, ctc_spot, stream_spot) refuse before they launch anything, and in which words: the exception's type and
its whole message, written out here as they stood before the bindings' argument filling was shared.  Every call below is a
valid one with one thing wrong, and every one raises in Python: no call gets as far as the library.  The bindings assert on
cuda tensors, hence the mark.  (T above BAND_MAX_FRAMES is asked with an expanded tensor, which owns 20 bytes.)"""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_spot_cases as pc  # noqa: E402
from qasr import align, spot, stream_spot as ss  # noqa: E402

B, T, CN, K, ML = 2, 6, 5, 2, 3
P, BLANK = B * K, CN - 1
I32, I64, F32 = torch.int32, torch.int64, torch.float32


@pytest.fixture(scope='module')
def engine():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    return engine


def z(dt, *shape):
    return torch.zeros(*shape, device='cuda', dtype=dt)


def refused(exc, msg, fn, kw, **wrong):
    with pytest.raises(exc, match=re.escape(msg)) as e:
        fn(**{**kw, **wrong})
    assert str(e.value) == msg


def log_probs_cases(fn, kw, who, shape='[B, T, C]'):
    msg = f'{who}: log_probs must be a cuda float32 tensor {shape}'
    refused(AssertionError, msg, fn, kw, log_probs=kw['log_probs'].double())
    refused(AssertionError, msg, fn, kw, log_probs=kw['log_probs'][0])


def align_result(rows):
    return align.AlignResult(labels=None, n_labels=None, start=z(I32, rows, ML), nframes=z(I32, rows, ML), score=z(F32, rows, ML),
                             path_score=z(I64, rows), total=z(I64, rows), ok=z(I32, rows))


def band_result():
    return align.BandResult(labels=None, n_labels=None, start=z(I32, B, ML), nframes=z(I32, B, ML), score=z(F32, B, ML),
                            path_score=z(I64, B), total=None, ok=z(I32, B), frame_logp=z(F32, B, T), band_base=z(I32, B, 1),
                            band_states=256)


def post_result(rows):
    return align.PostResult(frame_post=z(I32, rows, T), label_post=z(I32, rows, ML), total=z(I64, rows), ok=z(I32, rows))


def test_ctc_align_refusals(engine):
    fn, rep = engine.ctc_align, dataclasses.replace
    kw = dict(log_probs=z(F32, B, T, CN), lens=None, targets=z(I32, P, ML), target_lens=z(I32, P), blank=BLANK, problems_per_utt=K)
    log_probs_cases(fn, kw, 'ctc_align')
    refused(AssertionError, 'ctc_align: targets must be [P, max_labels], target_lens [P]', fn, kw, targets=z(I32, P))
    refused(ValueError, 'ctc_align: 4 target rows but 3 lengths', fn, kw, target_lens=z(I32, P - 1))
    refused(ValueError, 'ctc_align: max_labels (the row pitch of targets) must be 1 .. 2048, got 2049', fn, kw, targets=z(I32, P, 2049))
    out = align_result(P)
    refused(AssertionError, 'ctc_align: out.start', fn, kw, out=rep(out, start=z(I64, P, ML)))
    refused(AssertionError, 'ctc_align: out.total', fn, kw, out=rep(out, total=z(I64, P + 1)))
    refused(AssertionError, 'ctc_align: out.ok is required', fn, kw, out=rep(out, ok=None))
    refused(AssertionError, 'ctc_align: star must be a cuda float32 plane [2, 6]', fn, kw, star=z(F32, B, T + 1))


def test_ctc_post_refusals(engine):
    fn, rep = engine.ctc_post, dataclasses.replace
    kw = dict(log_probs=z(F32, B, T, CN), lens=None, targets=z(I32, P, ML), target_lens=z(I32, P), blank=BLANK,
              align_result=align_result(P), problems_per_utt=K)
    log_probs_cases(fn, kw, 'ctc_post')
    refused(AssertionError, 'ctc_post: targets must be [P, max_labels], target_lens [P]', fn, kw, targets=z(I32, P))
    refused(ValueError, 'ctc_post: 4 target rows but 5 lengths', fn, kw, target_lens=z(I32, P + 1))
    refused(ValueError, 'ctc_post: max_labels (the row pitch of targets) must be 1 .. 2048, got 2049', fn, kw, targets=z(I32, P, 2049))
    refused(AssertionError, 'ctc_post: align_result.start must be [4, 3]', fn, kw, align_result=rep(kw['align_result'], start=z(I32, P, ML + 1)))
    refused(AssertionError, 'ctc_post: align_result.ok must be [4]', fn, kw, align_result=rep(kw['align_result'], ok=None))
    out = post_result(P)
    refused(AssertionError, 'ctc_post: out.frame_post', fn, kw, out=rep(out, frame_post=z(I64, P, T)))
    refused(AssertionError, 'ctc_post: out.label_post', fn, kw, out=rep(out, label_post=z(I64, P, ML)))
    refused(AssertionError, 'ctc_post: out.ok', fn, kw, out=rep(out, ok=None))
    refused(AssertionError, 'ctc_post: star must be a cuda float32 plane [2, 6]', fn, kw, star=z(F32, B, T).double())


def test_ctc_align_band_refusals(engine):
    fn, rep = engine.ctc_align_band, dataclasses.replace
    kw = dict(log_probs=z(F32, B, T, CN), lens=None, targets=z(I32, B, ML), target_lens=z(I32, B), blank=BLANK)
    log_probs_cases(fn, kw, 'ctc_align_band', '[P, T, C]')
    refused(AssertionError, 'ctc_align_band: targets must be [P, max_labels], target_lens [P]', fn, kw, targets=z(I32, B))
    refused(ValueError, 'ctc_align_band: 2 recordings but 3 target rows and 2 lengths', fn, kw, targets=z(I32, B + 1, ML))
    refused(ValueError, 'ctc_align_band: 2 recordings but 2 target rows and 1 lengths', fn, kw, target_lens=z(I32, 1))
    refused(ValueError, 'ctc_align_band: max_labels (the row pitch of targets) must be 1 .. 1048576, got 1048577', fn, kw,
            targets=z(I32, 1, 1).expand(B, (1 << 20) + 1))
    refused(ValueError, 'ctc_align_band: max_labels (the row pitch of targets) must be 1 .. 1048576, got 0', fn, kw, targets=z(I32, B, 0))
    refused(ValueError, 'ctc_align_band: at most 4194304 frames, got 4194305', fn, kw, log_probs=z(F32, 1, 1, CN).expand(B, (1 << 22) + 1, CN))
    refused(ValueError, 'band_states must be one of (256, 1024, 4352), got 512', fn, kw, band_states=512)
    out = band_result()
    refused(AssertionError, 'ctc_align_band: out.frame_logp', fn, kw, out=rep(out, frame_logp=z(I32, B, T)))
    refused(AssertionError, 'ctc_align_band: out.band_base', fn, kw, out=rep(out, band_base=z(I32, B, 2)))
    refused(AssertionError, 'ctc_align_band: out.ok is required', fn, kw, out=rep(out, ok=None))
    refused(AssertionError, 'ctc_align_band: star must be a cuda float32 plane [2, 6]', fn, kw, star=z(F32, B + 1, T))


def test_ctc_post_band_refusals(engine):
    fn, rep = engine.ctc_post_band, dataclasses.replace
    kw = dict(log_probs=z(F32, B, T, CN), lens=None, targets=z(I32, B, ML), target_lens=z(I32, B), blank=BLANK, band_result=band_result())
    log_probs_cases(fn, kw, 'ctc_post_band', '[P, T, C]')
    refused(AssertionError, 'ctc_post_band: targets must be [P, max_labels], target_lens [P]', fn, kw, targets=z(I32, B))
    refused(ValueError, 'ctc_post_band: 2 recordings but 2 target rows and 3 lengths', fn, kw, target_lens=z(I32, B + 1))
    refused(ValueError, 'ctc_post_band: max_labels (the row pitch of targets) must be 1 .. 1048576, got 1048577', fn, kw,
            targets=z(I32, 1, 1).expand(B, (1 << 20) + 1))
    refused(ValueError, 'ctc_post_band: at most 4194304 frames, got 4194305', fn, kw, log_probs=z(F32, 1, 1, CN).expand(B, (1 << 22) + 1, CN))
    refused(ValueError, 'ctc_post_band: band_result.band_states must be one of (256, 1024, 4352), got 512', fn, kw,
            band_result=rep(kw['band_result'], band_states=512))
    refused(AssertionError, 'ctc_post_band: band_result.nframes must be [2, 3]', fn, kw, band_result=rep(kw['band_result'], nframes=z(I32, B, ML + 1)))
    refused(AssertionError, 'ctc_post_band: band_result.band_base must be [2, 1]', fn, kw, band_result=rep(kw['band_result'], band_base=None))
    out = post_result(B)
    refused(AssertionError, 'ctc_post_band: out.frame_post', fn, kw, out=rep(out, frame_post=z(I32, B, T + 1)))
    refused(AssertionError, 'ctc_post_band: out.total', fn, kw, out=rep(out, total=z(I32, B)))
    refused(AssertionError, 'ctc_post_band: star must be a cuda float32 plane [2, 6]', fn, kw, star=z(F32, B, T - 1))


def test_ctc_star_refusals(engine):
    fn = engine.ctc_star
    kw = dict(log_probs=z(F32, B, T, CN), lens=None, penalty=0.5)
    log_probs_cases(fn, kw, 'ctc_star')
    refused(AssertionError, 'ctc_star: out', fn, kw, out=z(F32, B, T + 1))
    refused(AssertionError, 'ctc_star: out', fn, kw, out=z(I32, B, T))


def test_ctc_spot_refusals(engine):
    fn, rep = engine.ctc_spot, dataclasses.replace
    kw = dict(log_probs=z(F32, B, T, CN), lens=None, star=z(F32, B, T), targets=z(I32, K, ML), target_lens=z(I32, K), blank=BLANK,
              threshold=-4.0, max_span=T, max_hits=4)
    log_probs_cases(fn, kw, 'ctc_spot')
    refused(ValueError, 'ctc_spot: max_hits must be at least 1, got 0', fn, kw, max_hits=0)
    refused(AssertionError, 'ctc_spot: targets must be [K, max_labels], target_lens [K]', fn, kw, targets=z(I32, K))
    refused(ValueError, 'ctc_spot: max_labels (the row pitch of targets) must be 1 .. 127, got 128', fn, kw, targets=z(I32, K, 128))
    refused(ValueError, 'ctc_spot: 2 target rows but 3 lengths', fn, kw, target_lens=z(I32, K + 1))
    out = spot.SpotResult(z(I32, P, 4), z(I32, P, 4), z(I64, P, 4), z(I32, P), z(I32, P), z(I64, P, T), z(I32, P, T), K)
    refused(AssertionError, 'ctc_spot: out.hit_score', fn, kw, out=rep(out, hit_score=z(I32, P, 4)))
    refused(AssertionError, 'ctc_spot: out.ok', fn, kw, out=rep(out, ok=None))
    refused(AssertionError, 'ctc_spot: out.trace_score and out.trace_start go together', fn, kw, out=rep(out, trace_start=None))
    refused(AssertionError, 'ctc_spot: out.trace_start', fn, kw, out=rep(out, trace_start=z(I64, P, T)))
    refused(AssertionError, 'ctc_spot: the two trace planes must share one row pitch', fn, kw, out=rep(out, trace_start=z(I32, P, T + 2)[:, :T]))
    refused(AssertionError, 'ctc_spot: star must be a cuda float32 plane [2, 6]', fn, kw, star=z(F32, B, T, 1))


def test_stream_spot_refusals(engine):
    name, Cn, ml, k, plan_name, threshold, max_span = pc.KERNEL_CASES[0]              # the smallest session of stream_spot_cases
    plan = pc.plan_of(plan_name)
    tg, tl, _ = pc.keyword_set(np.random.default_rng(1), Cn, Cn - 1, ml, k)
    splan = ss.StreamSpotPlan(plan, tg, tl, spot.check_threshold(threshold, name), max_span)
    S, Tw, rep = 3, plan.Tw, dataclasses.replace
    keywords = engine.stream_spot_keywords(splan, 'cuda')
    kw = dict(state=engine.stream_state(S, plan, 'cuda'), spot_state=engine.stream_spot_state(S, splan, 'cuda'), S=S, plan=plan,
              splan=splan, slots=z(I32, B), flags=z(I32, B), log_probs=z(F32, B, Tw, Cn), star=z(F32, B, Tw), enc_lens=z(I32, B),
              first_frame=z(I32, B), emit_status=z(I32, B), blank=Cn - 1, keywords=keywords)
    fn = engine.stream_spot
    log_probs_cases(fn, kw, 'stream_spot', '[B, Tw, C]')
    refused(AssertionError, 'stream_spot: slots', fn, kw, slots=z(I32, B + 1))
    refused(AssertionError, 'stream_spot: emit_status', fn, kw, emit_status=z(I64, B))
    refused(AssertionError, 'stream_spot: spot_state', fn, kw, spot_state=kw['spot_state'].float())
    refused(AssertionError, 'stream_spot: targets', fn, kw, keywords=(keywords[0].long(), keywords[1]))
    refused(AssertionError, 'stream_spot: targets', fn, kw, keywords=(keywords[0][:, :-1].contiguous(), keywords[1]))
    refused(AssertionError, 'stream_spot: target_lens', fn, kw, keywords=(keywords[0], keywords[1][:-1]))
    out = engine.stream_spot_buffers(B, splan, 'cuda')
    refused(AssertionError, 'stream_spot: out.hit_score', fn, kw, out=rep(out, hit_score=out.hit_score.int()))
    refused(AssertionError, 'stream_spot: out.status', fn, kw, out=rep(out, status=z(I32, B * splan.K + 1)))
    refused(AssertionError, f'stream_spot: star must be a cuda float32 plane [2, {Tw}]', fn, kw, star=z(F32, B, Tw + 1))
