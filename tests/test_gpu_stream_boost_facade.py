"""EncDecCTCModel.stream(beam=StreamBeam(boost=)) on an MI355X: on the static engine, with a caller's reservation and on the
dynamic path a session with a boosted and an unboosted stream equals the host composition (qasr.stream_beam twins with
boost= over the same model's per-window log-probabilities), however the pushes are sliced; boost_score is filled;
full-window steps replay one graph without allocating."""
import os
import sys

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_lm_cases  # noqa: E402
import stream_beam_cases as sbc  # noqa: E402
import stream_boost_cases as cases  # noqa: E402
import stream_cases as sc  # noqa: E402
import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import boost as qboost  # noqa: E402
from qasr import ngram, synth  # noqa: E402
from qasr import stream_beam as sb  # noqa: E402

KW = sc.FACADE_KW
LM_PATH = beam_lm_cases.model_path(sbc.GOLDEN, 'en3')


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _model(mode, seed=2):
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=seed).cuda()
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    if mode == 'static':
        qm.calibrate(m)
        L = torch.tensor([96] * 4).cuda()
        for c in synth.make_calibration(3, 4, 16, 96, seed):
            e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
            m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, mode == 'dynamic')
    return m


_models = {}


def model(mode):
    if mode not in _models:
        _models[mode] = _model(mode)
    return _models[mode]


def _words(m, audio, lens):
    x = torch.from_numpy(audio).cuda()
    hyps = m.decode_stream(x, torch.tensor(lens), **KW)
    out = sorted({w[:64] for h in hyps for w in h.text.split(' ')[:6] if len(w) >= 2})
    return out or ['ab']


@pytest.mark.parametrize('mode,with_lm,n_best,lag_s,named', [('static', True, 3, 0.3, True), ('reserved', False, 1, 0.3, False),
                                                             ('dynamic', False, 2, 100.0, True)])
def test_stream_boost_equals_the_host_composition(mode, with_lm, n_best, lag_s, named):
    m = model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(2, 3.0) if mode == 'reserved' else m.reserve(None, None)
    before = m._reserve
    lm = ngram.NgramLM.from_arpa(LM_PATH, m.decoder.vocabulary) if with_lm else None
    audio, lens = sc.facade_audio()[:, :50000], [20000, 50000]
    try:
        words = _words(m, audio, lens)
        if named:                               # two named sets: stream 0 takes 'b' (index 1), stream 1 none
            boost = {'a': [(w, 2.0) for w in words[:2]], 'b': qboost.PhraseSet(words, m.decoder.vocabulary, weight=1.5, whole_words=False)}
            open_boost, set_of = ['b', None], [1, -1]
        else:                                   # one set: stream 0 uses it, stream 1 opts out
            boost, open_boost, set_of = [(w, 2.5) for w in words], [None, False], [0, -1]
        beam = sb.StreamBeam(width=8, n_best=n_best, cutoff_top_n=20, lm=lm, alpha=0.5, beta=0.5, lag_s=lag_s, boost=boost)
        slots, ups, hyps, steps, sess = cases.play_session(m, audio, lens, 11000, beam, open_boost, device='cuda', **KW)
        assert m._reserve == before and (mode == 'dynamic' or sess.served == 'Engine')
        sets = list(sess.beam.boost.values())
        plan, bplan, want = cases.compose_on_host(m, audio, lens, sess.beam, sets, set_of, device='cuda', **KW)
        assert (plan.C, bplan.Lg) == (8000, 15 if lag_s < 1 else 5000) and steps == 6 + 2 and bplan.boost
        cases.check_against_composition(m, slots, ups, hyps, want, beam)
        cases.check_boost_scores(hyps, want, beam)
        first = lambda h: h[0] if n_best > 1 else h                               # noqa: E731
        assert first(hyps[0]).boost_score > 0.0 and first(hyps[1]).boost_score == 0.0
        again = cases.play_session(m, audio, lens, 8000, beam, open_boost, device='cuda', **KW)
        assert repr(again[2]) == repr(hyps) and repr([again[1][s] for s in slots]) == repr([ups[s] for s in slots])
    finally:
        m.reserve(None, None)


def test_full_window_steps_replay_without_allocating():
    m = model('static')
    m.reserve(None, None)
    audio = torch.from_numpy(sc.facade_audio()).cuda()
    beam = sb.StreamBeam(width=16, lag_s=0.5, boost={'x': ['ab', ('the', 2.0)], 'y': ['cd']})
    with m.stream(max_streams=2, beam=beam, **KW) as sess:
        C, Wl = sess.plan.C, sess.plan.Wl
        slot = sess.open(boost='y')
        stats, text = [], ''
        for k in range(90000 // C):
            ups = sess.push([slot], audio[1:2, k * C:(k + 1) * C])
            assert len(ups) == 1
            text += ups[0].text
            if (k + 1) * C >= Wl:                                                # the window is full from here on
                stats.append(m._ragged_engine.ragged_stats())
        hyp = sess.close(slot)
    assert len(stats) >= 6 and len(text) > 0 and hyp.text.startswith(text) and hyp.boost_score is not None
    assert stats[-1]['device_allocs'] == stats[0]['device_allocs'] and stats[-1]['device_frees'] == stats[0]['device_frees']
    assert len(stats) - 2 <= stats[-1]['graph_replays'] - stats[0]['graph_replays'] <= len(stats) - 1      # one replay per step
