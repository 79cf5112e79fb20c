"""EncDecCTCModel.error_rate / error_rate_long with alignments=True on an MI355X: the Alignments the device chain reads back equal
the host composition - align_texts over decode()'s texts and the references - on the static engine, a reserved engine and the
dynamic path, greedy and beam; the totals and the oracle equal those without alignments."""
import os
import sys

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_edit_facade as tf  # noqa: E402  (its models and references)
from qasr import edit, synth  # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from qasr import engine
    engine.load_library()
    torch.set_grad_enabled(False)


def _check(rep, plain, hyp_texts, ref_texts, use_cer):
    want = edit.align_texts(hyp_texts, ref_texts, use_cer=use_cer)              # the twin over the strings
    assert rep.alignments == want and sum(a.counts.errors for a in want) > 0
    assert [a.counts for a in rep.alignments] == rep.per_utterance
    assert plain.alignments is None
    assert (rep.total, rep.oracle_errors, rep.per_utterance, rep.invalid) == (plain.total, plain.oracle_errors, plain.per_utterance, plain.invalid)
    for a in rep.alignments:
        assert [a.hyp_units[i] for i in a.hyp_index if i is not None] == a.hyp_units
        assert [a.ref_units[j] for j in a.ref_index if j is not None] == a.ref_units
        assert edit.listing(a).count('\n') == 1


@pytest.mark.parametrize('mode', ['static', 'reserved', 'dynamic'])
def test_error_rate_alignments_equal_the_host_composition(mode):
    m = tf.model('dynamic' if mode == 'dynamic' else 'static')
    m.reserve(5, 2.0) if mode == 'reserved' else m.reserve(None, None)
    try:
        audio = torch.from_numpy(synth.make_audio(5, 24000, seed=3)).cuda()
        alen = torch.tensor([24000, 20000, 16001, 9000, 4000]).cuda()
        m.preprocessor.featurizer.pad_to = 16
        io = dict(input_signal=audio, input_signal_length=alen)
        tg, tl, ref_texts = tf._references(m, 5, 5)
        greedy = [h.text for h in m.decode(**io)]
        for use_cer in (False, True):
            kw = dict(targets=tg, target_lengths=tl, use_cer=use_cer)
            _check(m.error_rate(**io, **kw, alignments=True), m.error_rate(**io, **kw), greedy, ref_texts, use_cer)
        nbest = m.decode(**io, beam_width=4, n_best=2)
        best = [row[0].text for row in nbest]
        for use_cer in (False, True):
            kw = dict(texts=ref_texts, use_cer=use_cer, beam_width=4, n_best=2)
            _check(m.error_rate(**io, **kw, alignments=True), m.error_rate(**io, **kw), best, ref_texts, use_cer)
        with pytest.raises(ValueError, match=r'edit_trace: .* needs a workspace of \d+ bytes, above max_workspace_bytes = 100'):
            m.error_rate(**io, texts=ref_texts, alignments=True, max_workspace_bytes=100)
    finally:
        m.reserve(None, None)


def test_error_rate_long_alignments_equal_the_host_composition():
    m = tf.model('static')
    m.reserve(None, None)
    S = 32000 + 2 * 24000 + 10000
    audio = torch.from_numpy(synth.make_audio(2, S, seed=8)).cuda()
    lens = torch.tensor([30000, S]).cuda()
    tg, tl, ref_texts = tf._references(m, 2, 9, width=90)
    texts = [h.text for h in m.decode_long(audio, lens, batch_size=2, **tf.KW)]
    kw = dict(targets=tg, target_lengths=tl, batch_size=2, **tf.KW)
    _check(m.error_rate_long(audio, lens, alignments=True, **kw), m.error_rate_long(audio, lens, **kw), texts, ref_texts, False)
    rows = m.decode_long(audio, lens, batch_size=2, beam_width=4, n_best=2, **tf.KW)
    kw.update(beam_width=4, n_best=2, use_cer=True)
    _check(m.error_rate_long(audio, lens, alignments=True, **kw), m.error_rate_long(audio, lens, **kw), [r[0].text for r in rows], ref_texts, True)


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_alignments_lists_every_entry_and_the_confusions(tmp_path):
    import json
    import re
    import subprocess
    n_utt, samples = 4, 24000
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=4)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            tf._write_wav(p, audio[i, :samples - 1000 * i])
            f.write(json.dumps(dict(audio_filepath=p, duration=(samples - 1000 * i) / 16000, text='hello wide world'[:16 - i])) + '\n')
    out = tmp_path / 'alignments.txt'
    dev = tf._cli(tmp_path, man, ['--device_wer', '--alignments', str(out)])
    text = out.read_text()
    blocks, tail = text.split('substitutions (ref -> hyp):\n')[0].strip('\n').split('\n\n'), text.split('substitutions (ref -> hyp):\n')[1]
    assert len(blocks) == n_utt and f'listed {n_utt} alignments' in dev
    got = [0, 0, 0]
    for i, blk in enumerate(blocks):
        path, counts, ref, hyp = blk.split('\n')
        assert path == str(tmp_path / f'u{i}.wav') and ref.startswith('REF:') and hyp.startswith('HYP:')
        e, s, d, ins, nr, nh = (int(x) for x in re.fullmatch(r'errors (\d+)  S (\d+)  D (\d+)  I (\d+)  ref (\d+)  hyp (\d+)', counts).groups())
        assert e == s + d + ins and len(ref[5:].split()) == len(hyp[5:].split()) == nr + ins
        got = [a + b for a, b in zip(got, (s, d, ins))]
    assert got == [int(x) for x in tf._printed(dev, 'S / D / I:').split(' / ')] and sum(got) > 0
    assert 'deletions:\n' in tail and 'insertions:\n' in tail
    n_listed = sum(int(ln.split()[0]) for ln in tail.split('\n') if ln[:6].strip().isdigit())
    assert 0 < n_listed <= sum(got)
    refused = subprocess.run([sys.executable, tf.CLI, '--asr_model', 'QuartzNet15x5Base-En', '--dataset', str(man), '--alignments', str(out)],
                             capture_output=True, text=True, timeout=300)
    assert refused.returncode == 2 and '--alignments OUT needs --device_wer' in refused.stderr
