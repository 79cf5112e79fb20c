"""EncDecCTCModel.align_long on CPU inputs (the NumPy twins behind the float host modules): it equals the twin chain over the
same stitched log-probabilities, segments tile the labels, refusals name their argument, and the command-line tool writes
the segments file."""
import os
import sys

import pytest

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_long_cases as alc  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402

_m = None


def model():
    global _m
    if _m is None:
        torch.set_grad_enabled(False)
        _m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=2)
        _m.eval()
        _m.preprocessor.featurizer.dither = 0.0
        _m.set_quant_mode('none')
    return _m


@pytest.mark.parametrize('band_states', [None, 256, 4352])
def test_align_long_equals_the_twin_chain(band_states):
    alc.check_equals_the_twin_chain(model(), 'cpu', band_states)


def test_segments_tile_the_labels_and_a_lost_path_keeps_its_text():
    alc.check_segments(model(), 'cpu')


def test_texts_go_through_the_parser_and_join_with_the_space_label():
    m = model()
    audio, lens = alc.recordings('cpu')
    vocab = list(m.decoder.vocabulary)
    got = m.align_long(audio[:1], lens[:1], texts=[['ab c', 'de']], **alc.KW)[0]
    assert got.text == 'ab c de' and got.labels == [vocab.index(c) for c in 'ab c de']
    assert [s.text for s in got.segments] == ['ab c', 'de'] and [w[0] for w in got.words] == ['ab', 'c', 'de']
    one = m.align_long(audio[:1], lens[:1], texts=['ab c de'], **alc.KW)[0]
    assert one.segments is None and (one.start_s, one.utt_score) == (got.start_s, got.utt_score)


def test_refusals_name_their_argument():
    alc.check_refusals(model(), 'cpu')


def test_the_tool_writes_the_segments_file(tmp_path):
    alc.check_tool_output(tmp_path, ['--no_quant', '--device', 'cpu'])
