"""The wildcard ("star") for untranscribed audio on the host: qasr.align.star_host against a plain statement, the
augmented-matrix statement of STAR_RULES on every byte of every output of both twins, planted recordings whose transcript
skips a stretch, and the facade (align, align_long) on CPU tensors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases  # noqa: E402
import align_long_cases as alc  # noqa: E402
import star_cases as sc  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import align, synth  # noqa: E402
from qasr.beam import NEG, ONE  # noqa: E402


# ---------------------------------------------------------------------------------------------------------- star_host
def _special_logp():
    rng = np.random.Generator(np.random.PCG64(21))
    lp = np.log(rng.dirichlet(np.ones(7), size=(3, 9))).astype(np.float32)
    lp[0, 0, :] = lp[0, 0, 3]                                       # a tie over the whole row
    lp[0, 1, [2, 5]] = lp[0, 1].max() + np.float32(0.25)            # a tie of two
    lp[0, 2, :] = -np.inf                                           # a row of all -inf
    lp[1, 0, :] = -0.0                                              # -0.0 everywhere ...
    lp[1, 1, :] = -0.0
    lp[1, 1, 4] = 0.0                                               # ... and +0.0 above it in the key order
    lp[1, 2, :] = [-np.inf, -3.0, -np.inf, -3.0, -np.inf, -200.0, -np.inf]
    return lp


@pytest.mark.parametrize('penalty', [0.0, 1.5])
@pytest.mark.parametrize('lens', [None, [0, 9, 4], [9, 9, 9], [12, -3, 1]])
def test_star_host_is_the_row_maximum_less_one_float32_subtraction(lens, penalty):
    lp = _special_logp()
    got = align.star_host(lp, lens, penalty)
    want = sc.star_brute(lp, lens, penalty)
    assert got.dtype == np.float32 and got.shape == (3, 9) and got.tobytes() == want.tobytes()
    if lens is None:
        assert got[0, 2] == -np.inf and got[0, 0] == np.float32(lp[0, 0, 3] - np.float32(penalty))
        assert got[1, 0] == -np.float32(penalty) and np.signbit(align.star_host(lp, None, 0.0)[1, 0])   # max(-0.0 ...) - 0 = -0.0
        assert not np.signbit(align.star_host(lp, None, 0.0)[1, 1])                                 # +0.0 wins over -0.0
        assert align.quantize(got[0, 2:3])[0] == align.quantize(np.array([-np.inf], dtype=np.float32))[0]   # the floor, as today


def test_star_host_refuses_by_name():
    lp = _special_logp()
    for bad in (-0.001, 16.5, float('nan'), float('inf'), -float('inf'), None, 'x'):
        with pytest.raises(ValueError, match='penalty'):
            align.star_host(lp, None, bad)
    assert align.star_host(lp, None, 16.0).shape == (3, 9)
    with pytest.raises(ValueError, match='log_probs'):
        align.star_host(lp[0], None, 1.0)
    for twin in (align.align_host, align.align_band_host):
        with pytest.raises(ValueError, match='star'):
            twin(lp, None, np.zeros((3, 2), dtype=np.int32), np.zeros(3, dtype=np.int32), 6, star=np.zeros((3, 8), dtype=np.float32))


# ---------------------------------------------------------------------------------- the augmented-matrix statement, every byte
@pytest.fixture(scope='module')
def full_case():
    """B = 3 utterances (lens: full, short, 1), C = 29, T = 60, with the plane and the augmented matrix"""
    C, T, B, blank = 29, 60, 3, 28
    rng = np.random.Generator(np.random.PCG64(31))
    lp = sc.logp(rng, B, T, C, blank)
    lens = np.array([T, 41, 1], dtype=np.int32)
    star = align.star_host(lp, lens, 1.5)
    return lp, lens, star, sc.augmented(lp, star), C, blank


@pytest.mark.parametrize('want_total', [True, False])
@pytest.mark.parametrize('K', [1, 2])
def test_align_host_with_a_plane_is_align_host_on_the_augmented_matrix(full_case, K, want_total):
    lp, lens, star, aug, C, blank = full_case
    rng = np.random.Generator(np.random.PCG64(32 + K))
    n_ok = 0
    for n in (1, 6, 14):
        tg, tl = sc.position_targets(rng, n, C, blank, pitch=20)
        for r in range(0, len(sc.POSITIONS), 3 * K):                # B * K problems per call: different positions per row
            rows = [(r + i) % len(sc.POSITIONS) for i in range(3 * K)]
            for use_lens in (lens, None):
                got = align.align_host(lp, use_lens, tg[rows], tl[rows], blank, problems_per_utt=K, want_total=want_total, star=star)
                want = align.align_host(aug, use_lens, tg[rows], tl[rows], blank, problems_per_utt=K, want_total=want_total)
                sc.same_bytes(got, want, sc.ALIGN_FIELDS, (n, rows))
                n_ok += int(got.ok.sum())
    assert n_ok >= 20                                               # (lim = 1 aligns only the lone wildcard)


def test_lim_of_one_frame_aligns_the_lone_wildcard(full_case):
    lp, lens, star, aug, C, blank = full_case
    tg, tl = align_cases.pad_targets([[C], [C], [C]], blank)
    got = align.align_host(lp, lens, tg, tl, blank, star=star)
    sc.same_bytes(got, align.align_host(aug, lens, tg, tl, blank), sc.ALIGN_FIELDS)
    assert got.ok.tolist() == [1, 1, 1] and got.nframes[2, 0] == 1 and got.start[2, 0] == 0
    assert got.score[2, 0] == star[2, 0] and got.path_score[2] == int(align.quantize(star[2, :1])[0])
    two, tl2 = align_cases.pad_targets([[C, C]] * 3, blank)          # two adjacent wildcards are a repeat: three frames at least
    assert align.align_host(lp, np.array([3, 2, 1]), two, tl2, blank, star=star).ok.tolist() == [1, 0, 0]


def test_the_wildcards_id_without_a_plane_is_a_bad_label_as_before(full_case):
    lp, lens, star, aug, C, blank = full_case
    tg, tl = align_cases.pad_targets([[1, C, 2], [C], [3]], blank)
    for res in (align.align_host(lp, lens, tg, tl, blank), align.align_band_host(lp, lens, tg, tl, blank)):
        assert res.ok.tolist() == [0, 0, 1] and res.path_score[0] == NEG and not res.start[:2].any()
    tg[0, 1] = C + 1                                                # one past the wildcard stays outside with a plane too
    assert align.align_host(lp, lens, tg, tl, blank, star=star).ok.tolist() == [0, 1, 1]
    assert align.align_band_host(lp, lens, tg, tl, blank, star=star).ok.tolist() == [0, 1, 1]


def test_band_twin_with_the_band_fixed(full_case):
    """256 states hold every lattice here: the band never moves, and the per-label outputs are align_host(star=)'s"""
    lp, lens, star, aug, C, blank = full_case
    rng = np.random.Generator(np.random.PCG64(41))
    for n in (1, 6, 14):
        tg, tl = sc.position_targets(rng, n, C, blank, pitch=20)
        for r in (0, 3):
            for use_lens in (lens, None):
                got = align.align_band_host(lp, use_lens, tg[r:r + 3], tl[r:r + 3], blank, band_states=256, star=star)
                want = align.align_band_host(aug, use_lens, tg[r:r + 3], tl[r:r + 3], blank, band_states=256)
                sc.same_bytes(got, want, sc.BAND_FIELDS, (n, r))
                full = align.align_host(lp, use_lens, tg[r:r + 3], tl[r:r + 3], blank, want_total=False, star=star)
                sc.same_bytes(got, full, ('start', 'nframes', 'score', 'path_score', 'ok'), (n, r))
                assert not got.band_base.any()


def test_band_twin_with_the_band_moving():
    lp, tg, tl, blank, bw = sc.moving_band_case()
    lens = np.array([lp.shape[1] - 7], dtype=np.int32)
    star = align.star_host(lp, lens, 1.0)
    got = align.align_band_host(lp, lens, tg, tl, blank, band_states=bw, star=star)
    want = align.align_band_host(sc.augmented(lp, star), lens, tg, tl, blank, band_states=bw)
    sc.same_bytes(got, want, sc.BAND_FIELDS)
    assert got.ok[0] == 1 and got.band_base.max() > 100 and (np.diff(got.band_base[0, :lens[0] // 32]) >= 0).all()
    C = lp.shape[2]
    for i in np.flatnonzero(tg[0] == C):                            # the wildcard's score and frame_logp read the plane
        a, n = int(got.start[0, i]), int(got.nframes[0, i])
        assert n >= 1 and got.frame_logp[0, a:a + n].tobytes() == star[0, a:a + n].tobytes()
        assert got.score[0, i] == star[0, a:a + n].max()


# ------------------------------------------------------------------------------------------------------ planted cases
@pytest.mark.parametrize('name', [p[0] for p in sc.PLANTED])
def test_a_wildcard_at_a_planted_stretch_keeps_every_other_label_in_place(name):
    lp, y, yw, starts, (s0, s1), k = sc.planted(name)
    kind = next(p[3] for p in sc.PLANTED if p[0] == name)
    C = lp.shape[2]
    blank, n = C - 1, len(y)
    tg, tl = align_cases.pad_targets([y], blank)
    tgw, tlw = align_cases.pad_targets([yw], blank)
    star = align.star_host(lp, None, 1.0)
    if kind == 'full':
        without = align.align_host(lp, None, tg, tl, blank, want_total=False)
        got = align.align_host(lp, None, tgw, tlw, blank, want_total=False, star=star)
    else:
        without = align.align_band_host(lp, None, tg, tl, blank, band_states=256)
        got = align.align_band_host(lp, None, tgw, tlw, blank, band_states=256, star=star)
    # the transcript alone: aligned "successfully", with at least one label in the wrong place (what the wildcard is for)
    assert without.ok[0] == 1 and (without.start[0, :n] != np.array(starts)).any()
    assert got.ok[0] == 1
    real = np.delete(got.start[0, :n + 1], k)
    for i in range(n):
        if i not in (k - 1, k):                                     # every label that does not touch the wildcard
            assert real[i] == starts[i], (name, i, int(real[i]), starts[i])
    a, b = int(got.start[0, k]), int(got.start[0, k] + got.nframes[0, k])
    assert abs(a - s0) <= 2 and abs(b - s1) <= 2, (name, a, b, s0, s1)


# ---------------------------------------------------------------------------------------------------------- the facade
_m = None


def _model():
    global _m
    if _m is None:
        _m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
        _m.eval()
        _m.preprocessor.featurizer.dither = 0.0
        _m.set_quant_mode('none')                                   # float modules on the CPU: the same forward on every call
    return _m


def _tuples(h):
    return (h.text, h.labels, h.start_s, h.end_s, h.score, h.utt_score, h.words, h.lm_score, h.ctc_score, h.segments, h.seams_s)


def test_token_splitting_and_joining():
    m = _model()
    vocab = list(m.decoder.vocabulary)
    from nemo.collections.asr.parts import parsers
    parser = parsers.make_parser(labels=vocab, name='en', unk_id=-1, blank_id=-1, do_normalize=True)
    W, sp = len(vocab) + 1, vocab.index(' ')
    ids = lambda s: [vocab.index(ch) for ch in s]                   # noqa: E731

    def row(text, space=sp, token='*'):
        return m._star_join([m._star_pieces(text, token, parser, 'align', 'text 0')], space, W)[0]
    assert row('ab * cd') == ids('ab') + [sp, W, sp] + ids('cd')
    assert row('ab*cd') == ids('ab') + [sp, W, sp] + ids('cd')        # phrases stay whole words
    assert row('* Ab, c') == [W, sp] + ids('ab c') and row('ab c *') == ids('ab c') + [sp, W]
    assert row('*') == [W] and row(' * ') == [W] and row('') == [] and row('ab') == ids('ab')
    assert row('ab ** * cd') == row('ab * cd') and row('***') == [W]  # consecutive tokens collapse to one
    assert row('ab * cd * e') == ids('ab') + [sp, W, sp] + ids('cd') + [sp, W, sp] + ids('e')
    assert row('ab<skip>cd', token='<skip>') == row('ab*cd')
    # a vocabulary without a space: the pieces touch the wildcard
    assert row('ab*cd', space=None) == ids('ab') + [W] + ids('cd') and row('*ab**', space=None) == [W] + ids('ab') + [W]


def _inputs():
    x = torch.from_numpy(synth.make_features(3, 16, 96, 7))
    return dict(processed_signal=x, processed_signal_length=torch.tensor([96, 70, 41]))


def test_facade_align_with_a_token_on_host_modules():
    m = _model()
    vocab = list(m.decoder.vocabulary)
    W, blank, sp = len(vocab) + 1, len(vocab), vocab.index(' ')
    inputs = _inputs()
    with torch.no_grad():
        logp, enc_len, _ = m(**inputs)
    spf = m.seconds_per_frame()
    texts = ['ab * c', '* hello', 'a']
    hyps = m.align(**inputs, texts=texts, star='*', star_penalty=1.5)
    assert [h.text for h in hyps] == ['ab * c', '* hello', 'a']
    rows = [[vocab.index(ch) if ch != '*' else W for ch in t] for t in texts]
    assert [h.labels for h in hyps] == rows
    tg, tl = align_cases.pad_targets(rows, blank)
    star = align.star_host(logp.numpy(), enc_len.numpy(), 1.5)
    want = align.align_host(logp.numpy(), enc_len.numpy(), tg, tl, blank, star=star)
    assert want.ok.all()
    for b, h in enumerate(hyps):
        n = len(rows[b])
        assert h.start_s == (want.start[b, :n] * spf).tolist() and h.end_s == ((want.start[b, :n] + want.nframes[b, :n]) * spf).tolist()
        assert h.score == want.score[b, :n].astype(np.float64).tolist()
        assert h.utt_score == want.path_score[b] / ONE                # the wildcard's emissions are in it
        assert (h.ctc_score is None) == (W in rows[b])                # None exactly with a wildcard
        assert [w[0] for w in h.words] == h.text.split()
        for i in (i for i, c in enumerate(rows[b]) if c == W):        # the token is a word with the wildcard's times and score
            a, k = int(want.start[b, i]), int(want.nframes[b, i])
            assert ('*', h.start_s[i], h.end_s[i], h.score[i]) in h.words and h.score[i] == float(star[b, a:a + k].max())
    assert hyps[2].ctc_score == want.total[2] / ONE
    # the same through labels=, where the id one past the blank is the wildcard
    same = m.align(**inputs, labels=rows, star='*', star_penalty=1.5)
    assert [_tuples(h) for h in same] == [_tuples(h) for h in hyps]
    # another penalty is another alignment score
    assert m.align(**inputs, texts=texts, star='*', star_penalty=0.0)[0].utt_score > hyps[0].utt_score
    # the arguments at their defaults - and a token no transcript uses - are the call without them
    plain = m.align(**inputs, texts=['ab c', 'hello', 'a'])
    assert [_tuples(h) for h in m.align(**inputs, texts=['ab c', 'hello', 'a'], star=None, star_penalty=1.0)] == [_tuples(h) for h in plain]
    assert [_tuples(h) for h in m.align(**inputs, texts=['ab c', 'hello', 'a'], star='*')] == [_tuples(h) for h in plain]
    assert all(h.ctc_score is not None for h in plain)


def test_facade_align_refusals_name_their_argument():
    m = _model()
    vocab = list(m.decoder.vocabulary)
    inputs = _inputs()
    ok = dict(texts=['a', 'b', 'c'])
    for bad, word in ((dict(star=''), 'star'), (dict(star=5), 'star'), (dict(star='a*'), 'shares'), (dict(star=' '), 'shares'),
                      (dict(star='*', star_penalty=-1), 'star_penalty'), (dict(star='*', star_penalty=16.5), 'star_penalty'),
                      (dict(star='*', star_penalty=float('nan')), 'star_penalty'), (dict(star_penalty=99), 'star_penalty')):
        with pytest.raises(ValueError, match=word):
            m.align(**inputs, **ok, **bad)
    with pytest.raises(ValueError, match='transcript 1 holds the wildcard label'):
        m.align(**inputs, labels=[[1], [2, len(vocab) + 1], [3]])
    with pytest.raises(ValueError, match='transcript 2'):
        m.align(**inputs, labels=[[1], [2], [len(vocab) + 2]], star='*')
    with pytest.raises(ValueError, match='transcript 0'):            # MAX_LABELS counts wildcards
        m.align(**inputs, labels=[[1, len(vocab) + 1] * (align.MAX_LABELS // 2) + [1], [1], [1]], star='*')


def test_facade_align_long_with_star_between():
    m = _model()
    vocab = list(m.decoder.vocabulary)
    W, blank, sp = len(vocab) + 1, len(vocab), vocab.index(' ')
    audio, lens = alc.recordings('cpu')
    greedy = m.decode_long(audio[:1], lens[:1], batch_size=alc.BATCH, **alc.KW)[0]
    ids = greedy.labels
    a, b = len(ids) // 3, 2 * len(ids) // 3
    parts = [[c for c in p if c != sp] or [1] for p in (ids[:a], ids[a:b], ids[b:])]
    got = m.align_long(audio[:1], lens[:1], labels=[parts], batch_size=alc.BATCH, star_between=True, **alc.KW)[0]
    joined = [W, sp] + parts[0] + [sp, W, sp] + parts[1] + [sp, W, sp] + parts[2] + [sp, W]
    assert got.labels == joined and got.text.count('*') == 4 and got.ctc_score is None
    assert len(got.segments) == 3 and got.start_s and np.isfinite(got.utt_score)
    at = 2
    for seg, part in zip(got.segments, parts):                      # one per utterance, over its own labels only
        assert seg.text == ''.join(vocab[c] for c in part)
        assert seg.start_s == got.start_s[at] and seg.end_s == got.end_s[at + len(part) - 1] and np.isfinite(seg.score)
        at += len(part) + 3
    stars = [w for w in got.words if w[0] == '*']
    assert len(stars) == 4 and all(w[1] < w[2] for w in stars)
    for seg in got.segments:                                        # wildcard frames belong to no segment
        assert all(w[2] <= seg.start_s + 1e-9 or w[1] >= seg.end_s - 1e-9 for w in stars)
    # the token inside a text, with and without utterance lists; the default token of star_between is '*'
    text = ''.join(vocab[c] for c in parts[0]) + ' * ' + ''.join(vocab[c] for c in parts[2])
    one = m.align_long(audio[:1], lens[:1], texts=[text], batch_size=alc.BATCH, star='*', **alc.KW)[0]
    assert one.labels == parts[0] + [sp, W, sp] + parts[2] and one.segments is None and one.text == text
    lst = m.align_long(audio[:1], lens[:1], texts=[[text]], batch_size=alc.BATCH, star='*', **alc.KW)[0]
    assert lst.labels == one.labels and len(lst.segments) == 1 and lst.segments[0].start_s == lst.start_s[0]
    assert lst.segments[0].end_s == lst.end_s[-1] and lst.segments[0].text == text
    # defaults are the call without the arguments
    plain = m.align_long(audio[:1], lens[:1], labels=[parts], batch_size=alc.BATCH, **alc.KW)
    dflt = m.align_long(audio[:1], lens[:1], labels=[parts], batch_size=alc.BATCH, star=None, star_penalty=1.0, star_between=False, **alc.KW)
    assert [_tuples(h) for h in dflt] == [_tuples(h) for h in plain] and W not in plain[0].labels
    # refusals
    with pytest.raises(ValueError, match='holds the wildcard label'):
        m.align_long(audio[:1], lens[:1], labels=[[parts[0], [W]]], **alc.KW)
    with pytest.raises(ValueError, match='utterance 1 of transcript 0 is empty'):
        m.align_long(audio[:1], lens[:1], texts=[['ab', ' * ']], star='*', **alc.KW)
    with pytest.raises(ValueError, match='star_penalty'):
        m.align_long(audio[:1], lens[:1], labels=[parts], star_between=True, star_penalty=17, **alc.KW)
    with pytest.raises(ValueError, match='shares'):
        m.align_long(audio[:1], lens[:1], labels=[parts], star='b', **alc.KW)


def test_to_hypotheses_gives_the_token_a_word_of_its_own_without_a_space():
    vocab = ['a', 'b', 'c']                                         # blank 3, wildcard 4
    res = align.AlignResult(np.array([[0, 4, 1, 2]], dtype=np.int32), np.array([4], dtype=np.int32),
                            np.array([[0, 2, 5, 6]], dtype=np.int32), np.array([[2, 3, 1, 2]], dtype=np.int32),
                            np.array([[-0.1, -1.2, -0.3, -0.4]], dtype=np.float32), np.array([-5 * ONE]), np.array([-4 * ONE]),
                            np.array([1], dtype=np.int32), 3, 1)
    h = align.to_hypotheses(res, vocab, 0.5, star_token='<x>')[0]
    assert h.text == 'a<x>bc' and h.ctc_score is None and h.utt_score == -5.0
    assert [(w[0], w[1], w[2]) for w in h.words] == [('a', 0.0, 1.0), ('<x>', 1.0, 2.5), ('bc', 2.5, 4.0)]
    assert h.words[2][3] == min(h.score[2:]) and h.words[1][3] == h.score[1]


def test_the_segmentation_tool_takes_star_between(tmp_path):
    """the tool's file keeps one row per utterance; with wildcards around them the rows still come in order"""
    rows = alc.check_tool_output(tmp_path, ['--no_quant', '--device', 'cpu', '--star_between', '--star_penalty', '2.0'])
    assert len(rows) == 3
    import subprocess
    bad = subprocess.run([sys.executable, alc.TOOL, '--data', str(tmp_path), '--star_penalty', '2.0'], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode != 0 and '--star_penalty needs --star_between' in bad.stderr
