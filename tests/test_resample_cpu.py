"""qasr.resample, the NumPy statement of the device resampler, without a GPU: the filter against scipy's polyphase resampler, the
fixed point against the float64 direct sum, tones, lengths, edges, the packed table's host check (qasr_resample_check through
the binding), read_wav / the dataset at any rate and the model facade on the host modules."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_cases as rc  # noqa: E402
from nemo.collections.asr.data import audio_to_text as a2t  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import resample as rs  # noqa: E402

_plans = {}


def plan(sr, quality='best'):
    if (sr, quality) not in _plans:
        _plans[sr, quality] = rs.ResamplePlan(sr, 16000, quality)
    return _plans[sr, quality]


def test_table_sizes_are_the_documented_ones():
    got = {sr: (plan(sr).L, plan(sr).M, plan(sr).W, plan(sr).L * 2 * plan(sr).W) for sr in (8000, 11025, 22050, 32000, 44100, 48000, 96000)}
    assert got == {8000: (2, 1, 68, 272), 11025: (640, 441, 68, 87040), 22050: (320, 441, 94, 60160), 32000: (1, 2, 136, 272),
                   44100: (160, 441, 187, 59840), 48000: (1, 3, 203, 406), 96000: (1, 6, 406, 812)}
    for sr in rc.RATES:
        for q in rc.QUALITIES:
            assert plan(sr, q).abs_sum() / 2 ** 30 <= 2.59 and plan(sr, q).table.dtype == np.int32


@pytest.mark.parametrize('quality', rc.QUALITIES)
@pytest.mark.parametrize('sr', rc.RATES)
def test_filter_identity_against_scipy(sr, quality):
    """the unrounded float64 direct sum is scipy.signal.resample_poly with this filter's taps (scipy multiplies a given tap
    array by `up`): an independent implementation pins q, phi, the tap order and the output length"""
    signal = pytest.importorskip('scipy.signal')
    p = plan(sr, quality)
    L, W = p.L, p.W
    taps = np.zeros(2 * W * L + 1)
    for phi in (0, L // 3, L - 1):                                  # taps[(d + W) L + phi] = h(phi / L + d)
        for d in (-W, -1, 0, W - 1):
            u = p.s * (phi / L + d)
            want = p.s * np.sinc(u) * np.i0(p.beta * np.sqrt(max(1 - (u / p.Z) ** 2, 0.0))) / np.i0(p.beta) if abs(u) < p.Z else 0.0
            assert p.h[phi, d + W] == pytest.approx(want, rel=1e-12, abs=1e-18)
    taps[:2 * W * L] = p.h.T.reshape(-1)
    for n in (1499, 2 * W + 3):
        xi = rc.pcm(1, n, 1, seed=sr + n)[0]                        # signals in [-1, 1): int16 / 32768
        want = signal.resample_poly(xi / 32768.0, p.L, p.M, window=taps) / L
        got = rs.resample_direct(xi, n, p)
        assert got.shape == want.shape == (p.out_len(n),)
        err = np.abs(got - want).max()
        print(f'{sr} {quality} n={n}: direct sum vs scipy {err:.3g}')
        assert err <= 1e-12


@pytest.mark.parametrize('quality', rc.QUALITIES)
@pytest.mark.parametrize('sr', rc.RATES)
def test_fixed_point_bound(sr, quality):
    """|twin - float64 direct sum| <= 2 W 2^-31 (half a unit of coefficient rounding per tap times |x| <= 1) + ulp32(|y|) / 2
    (the final rounding).  float32 input: the same, plus 2 W products and 2 W sums rounded in float64; no partial sum passes
    sum |h| |x| <= 2.59 < 4, so each rounding is below 4 * 2^-53: 4 W 2^-51 in all."""
    p = plan(sr, quality)
    n = 1777
    x = rc.pcm(1, n, 1, seed=sr)[0]
    d = rs.resample_direct(x, n, p)
    half_ulp = np.spacing(np.abs(d).astype(np.float32)).astype(np.float64) / 2
    y, ln = rs.resample_host(x[None], [n], p)
    assert ln.tolist() == [p.out_len(n)] and y.dtype == np.float32 and y.shape == (1, p.out_len(n))
    err = np.abs(y[0] - d)
    print(f'{sr} {quality}: int16 twin vs direct {err.max():.3g}')
    assert np.all(err <= 2 * p.W * 2.0 ** -31 + half_ulp)
    yf, _ = rs.resample_host(rc.to_float(x)[None], [n], p)
    errf = np.abs(yf[0] - d)
    print(f'{sr} {quality}: float32 twin vs direct {errf.max():.3g}')
    assert np.all(errf <= 2 * p.W * 2.0 ** -31 + 4 * p.W * 2.0 ** -51 + half_ulp)


@pytest.mark.parametrize('quality', rc.QUALITIES)
@pytest.mark.parametrize('sr', rc.RATES)
def test_tones(sr, quality):
    """int16 sines of amplitude 20000, RMS over the middle half of the output: pass band within 0.05 dB of the input, a tone
    just past the stop-band edge of a downsampling filter at most -80 dB"""
    p = plan(sr, quality)
    n = int(0.6 * sr)
    nyq = min(sr, 16000) / 2
    ref = rc.AMP / 32768 / np.sqrt(2)
    for f in (0.5 * nyq, 0.5 * p.rolloff * nyq, 0.85 * p.rolloff * nyq):
        y, _ = rs.resample_host(rc.tone(sr, f, n)[None], [n], p)
        db = 20 * np.log10(rc.mid_rms(y[0]) / ref)
        print(f'{sr} {quality}: {f:.0f} Hz passes at {db:+.4f} dB')
        assert abs(db) <= 0.05
    if sr > 16000:
        f = 8000 * (2 - p.rolloff) + 50
        assert f < sr / 2
        y, _ = rs.resample_host(rc.tone(sr, f, n)[None], [n], p)
        db = 20 * np.log10(max(rc.mid_rms(y[0]), 1e-30) / ref)
        print(f'{sr} {quality}: {f:.0f} Hz is stopped at {db:.1f} dB')
        assert db <= -80.0


def test_lengths():
    from qasr import engine
    for sr in rc.RATES + (16000,):
        p = plan(sr)
        for n in (0, 1, 2, 3, 7, 101, 997, 7919, 104729, 15485863):
            want = 0
            while want * p.M < n * p.L and n < 10000:               # ceil without a division (small n)
                want += 1
            if n >= 10000:
                want = int((n * p.L + p.M - 1) // p.M)
            assert p.out_len(n) == want
            assert engine.resample_out_samples(n, p.L, p.M) == want
    assert engine.resample_out_samples(-1, 1, 1) == -1 and engine.resample_out_samples(5, 0, 1) == -1
    assert engine.resample_out_samples(2 ** 31 - 1, 2, 1) == -1
    y, ln = rs.resample_host(np.zeros((2, 0), np.int16), [0, 0], plan(8000))
    assert y.shape == (2, 0) and ln.tolist() == [0, 0]


def test_equal_rates_return_read_wav_values():
    p = plan(16000)
    assert p.equal
    for ch in (1, 2, 3):
        x = rc.pcm(2, 501, ch, seed=ch)
        lens = [501, 77]
        y, ln = rs.resample_host(x, lens, p, channels=ch)
        assert ln.tolist() == lens and y.shape == (2, 501)
        for b, n in enumerate(lens):
            want = x[b, :n * ch].astype(np.float32) / 32768.0       # read_wav, verbatim
            if ch > 1:
                want = want.reshape(-1, ch).mean(axis=1)
            assert np.array_equal(y[b, :n], want) and not y[b, n:].any()
    xf = rc.to_float(rc.pcm(1, 300, 1, seed=9))
    assert np.array_equal(rs.resample_host(xf, [300], p)[0], xf)


@pytest.mark.parametrize('sr', (8000, 44100, 48000))
def test_channels_and_plain_statement(sr):
    """1, 2 and 3 channels with odd channel sums against a plain per-output Python-integer statement (exact), and copies of
    one channel against mono (exact: the sum and the divisor scale together)"""
    p = plan(sr, 'fast')
    n = 150
    for ch in (1, 2, 3):
        x = rc.pcm(1, n, ch, seed=10 * ch + 1)
        if ch > 1:
            x[0, ::ch] |= 1
            x[0, 1::ch] &= ~np.int16(1)                            # frame sums are odd wherever ch == 2
            assert ch != 2 or np.all(x[0].reshape(n, ch).astype(np.int64).sum(axis=1) % 2 == 1)
        y, _ = rs.resample_host(x, [n], p, channels=ch)
        assert np.array_equal(y[0], rc.brute_int16(x[0], n, p, ch))
        mean = x[0].reshape(n, ch).astype(np.float64).mean(axis=1) / 32768
        d = rs.resample_direct(x[0], n, p, channels=ch)
        assert np.all(np.abs(y[0] - d) <= 2 * p.W * 2.0 ** -31 + np.spacing(np.abs(d).astype(np.float32)) / 2) and np.abs(mean).max() <= 1
        mono = rc.pcm(1, n, 1, seed=3)
        ym, _ = rs.resample_host(mono, [n], p)
        yc, _ = rs.resample_host(np.repeat(mono, ch, axis=1), [n], p, channels=ch)
        assert np.array_equal(ym, yc)
        yf, _ = rs.resample_host(np.repeat(rc.to_float(mono), ch, axis=1), [n], p, channels=ch)
        assert np.abs(yf - ym).max() <= 2.0 ** -23


@pytest.mark.parametrize('sr,quality', [(8000, 'best'), (48000, 'best'), (11025, 'fast')])
def test_edges_padding_and_out_range(sr, quality):
    p = plan(sr, quality)
    W = p.W
    lens = [0, 1, 2, W - 1, W, 2 * W + 5, 700]
    S = 700
    x = rc.pcm(len(lens), S, 1, seed=5)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    y, ln = rs.resample_host(x, lens, p)
    assert ln.tolist() == [p.out_len(n) for n in lens] and y.shape == (len(lens), p.out_len(S))
    for b, n in enumerate(lens[:5]):                                # utterances shorter than the filter: the plain statement
        assert np.array_equal(y[b, :ln[b]], rc.brute_int16(x[b], n, p)) and not y[b, ln[b]:].any()
    # what lies behind a length is never read: full-scale fill does not change a byte
    for data in (x, rc.to_float(x)):
        a, la = rs.resample_host(data, lens, p)
        b_, lb = rs.resample_host(rc.fill_behind(data, lens), lens, p)
        assert a.tobytes() == b_.tobytes() and la.tobytes() == lb.tobytes()
    # a slice of outputs equals the full run's slice
    P = y.shape[1]
    for i0, i1 in ((0, P), (0, 1), (P - 1, P), (P // 7, P // 2 + 3), (P // 2, P // 2)):
        part = rs.resample_host(x, lens, p, out_range=(i0, i1))[0]
        assert part.shape == (len(lens), i1 - i0) and np.array_equal(part, y[:, i0:i1])
    with pytest.raises(ValueError, match='out_range'):
        rs.resample_host(x, lens, p, out_range=(0, P + 1))


def test_plans_refused_name_the_rate():
    for bad, word in ((16001, '16001 Hz'), (999, '999 Hz'), (44101, '44101 Hz'), (2000000, '2000000 Hz')):
        with pytest.raises(ValueError, match=word):
            rs.ResamplePlan(bad)
    with pytest.raises(ValueError, match='integers'):
        rs.ResamplePlan(8000.5)
    with pytest.raises(ValueError, match='quality'):
        rs.ResamplePlan(8000, quality='better')
    with pytest.raises(ValueError, match='channels'):
        rs.resample_host(np.zeros((1, 9), np.int16), [1], plan(8000), channels=9)
    with pytest.raises(ValueError, match='int16 or float32'):
        rs.resample_host(np.zeros((1, 9), np.float64), [9], plan(8000))


def test_blob_check_through_the_binding():
    """qasr_resample_check is host code: every plan's packed table passes; truncations, a wrong magic or version, a wrong
    table length and a table whose accumulator bound fails are rejected with the field named"""
    from qasr import engine
    for sr in rc.RATES + (16000,):
        for q in rc.QUALITIES:
            engine.resample_check(plan(sr, q).pack())
    blob = plan(8000).pack()
    words = np.frombuffer(blob, dtype=np.int32)
    assert words[0] == rs.MAGIC and words[2] == len(blob) and tuple(words[3:6]) == (2, 1, 68) and words[9] == 272
    # the device layout: column r holds the phase (r M) mod L
    p = plan(11025)
    body = np.frombuffer(p.pack(), dtype=np.int32)[rs.HDR_WORDS:].reshape(2 * p.W, p.L)
    for r in (0, 1, 5, p.L - 1):
        assert np.array_equal(body[:, r], p.table[(r * p.M) % p.L])

    def bad(mut, word):
        w = words.copy()
        out = mut(w)
        with pytest.raises(engine.QasrError, match=word):
            engine.resample_check((w if out is None else out).tobytes())

    for cut in (0, 4, 127, 128, len(blob) - 4):
        with pytest.raises(engine.QasrError):
            engine.resample_check(blob[:cut])
    with pytest.raises(engine.QasrError):
        engine.resample_check(blob + b'\0\0\0\0')
    bad(lambda w: w.__setitem__(0, rs.MAGIC + 1), 'magic')
    bad(lambda w: w.__setitem__(1, 2), 'version')
    bad(lambda w: w.__setitem__(9, 271), 'entries')
    bad(lambda w: w.__setitem__(5, 67), 'entries')                  # W no longer matches the table
    bad(lambda w: w.__setitem__(3, 4), 'reduce')                    # L / M no longer the rates' ratio
    bad(lambda w: w.__setitem__(5, 5000), 'W 5000')
    bad(lambda w: w.__setitem__(20, 1), 'reserved')
    bad(lambda w: w.__setitem__(slice(rs.HDR_WORDS, None, 2), 2 ** 30), 'column 0')      # 136 x 2^30 x 32768 x 8 >= 2^53


def _write_wav(path, pcm, sr, ch):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(ch)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.astype('<i2').tobytes())


def test_read_wav_and_dataset_at_any_rate(tmp_path):
    mono8, st44, mono16 = rc.pcm(1, 4000, 1, seed=1)[0], rc.pcm(1, 9000, 2, seed=2)[0], rc.pcm(1, 5000, 1, seed=3)[0]
    _write_wav(tmp_path / 'a.wav', mono8, 8000, 1)
    _write_wav(tmp_path / 'b.wav', st44, 44100, 2)
    _write_wav(tmp_path / 'c.wav', mono16, 16000, 1)
    _write_wav(tmp_path / 'd.wav', mono8, 16001, 1)
    for name, x, sr, ch in (('a', mono8, 8000, 1), ('b', st44, 44100, 2)):
        pcm, rate, chans = a2t.read_pcm(str(tmp_path / f'{name}.wav'))
        assert pcm.dtype == np.int16 and np.array_equal(pcm, x) and (rate, chans) == (sr, ch)
        want, ln = rs.resample_host(x[None], [x.size // ch], plan(sr), channels=ch)
        got = a2t.read_wav(str(tmp_path / f'{name}.wav'))
        assert got.dtype == np.float32 and got.shape == (int(ln[0]),) and np.array_equal(got, want[0])
    assert np.array_equal(a2t.read_wav(str(tmp_path / 'c.wav')), mono16.astype(np.float32) / 32768.0)
    assert np.array_equal(a2t.read_wav(str(tmp_path / 'a.wav'), quality='fast'),
                          rs.resample_host(mono8[None], [4000], plan(8000, 'fast'))[0][0])
    with pytest.raises(ValueError, match='d.wav.*16001 Hz'):
        a2t.read_wav(str(tmp_path / 'd.wav'))
    labels = [' ', 'a', 'b']
    man = tmp_path / 'm.json'
    with open(man, 'w') as f:
        for name in ('a', 'a'):
            f.write(json.dumps(dict(audio_filepath=str(tmp_path / f'{name}.wav'), duration=0.5, text='ab')) + '\n')
    with open(tmp_path / 'mixed.json', 'w') as f:
        for name in ('a', 'b'):
            f.write(json.dumps(dict(audio_filepath=str(tmp_path / f'{name}.wav'), duration=0.5, text='ab')) + '\n')
    ds = a2t.AudioToCharDataset(str(man), labels, input_rate=8000)
    x, n, t, m = ds[0]
    assert x.dtype == torch.int16 and int(n) == 4000 and np.array_equal(x.numpy(), mono8) and t.tolist() == [1, 2]
    batch = a2t.AudioToCharDataset.collate_fn([ds[0], (x[:3000], torch.tensor(3000), t, m)])
    assert batch[0].dtype == torch.int16 and batch[0].shape == (2, 4000) and not batch[0][1, 3000:].any() and batch[1].tolist() == [4000, 3000]
    loader = a2t.make_dataloader(dict(manifest_filepath=str(man), labels=labels, batch_size=2, input_rate=8000))
    assert next(iter(loader))[0].dtype == torch.int16
    mixed = a2t.AudioToCharDataset(str(tmp_path / 'mixed.json'), labels, input_rate=8000)
    with pytest.raises(ValueError, match='44100 Hz.*8000 Hz'):
        mixed[1]
    # without input_rate a manifest of mixed rates is resampled on the host while it is read
    plain = a2t.AudioToCharDataset(str(tmp_path / 'mixed.json'), labels)
    fb = a2t.AudioToCharDataset.collate_fn([plain[0], plain[1]])
    assert fb[0].dtype == torch.float32 and fb[1].tolist() == [8000, plan(44100).out_len(9000)]


def test_facade_on_the_host_modules(tmp_path):
    """forward / decode / align / transcribe on a mini QuartzNet's host modules: sample_rate=R is forward on the twin's output
    with converted lengths; the defaults leave the call untouched"""
    torch.manual_seed(0)
    m = EncDecCTCModel.from_synthetic('MiniQuartzNet', seed=4)
    m.set_quant_mode('none')
    m.eval()
    m.preprocessor.featurizer.dither = 0.0
    with torch.no_grad():
        for sr, ch, quality in ((8000, 1, 'best'), (44100, 2, 'fast')):
            m.resample_quality = quality
            S = sr // 2
            x = rc.pcm(2, S, ch, seed=sr)
            lens = [S, S - 1234]
            y, ln = rs.resample_host(x, lens, plan(sr, quality), channels=ch)
            want = m(input_signal=torch.from_numpy(y), input_signal_length=torch.tensor(ln.astype(np.int64)))
            got = m(input_signal=torch.from_numpy(x), input_signal_length=torch.tensor(lens), sample_rate=sr, channels=ch)
            assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[0].shape[0] == 2
            gotf = m(input_signal=torch.from_numpy(rc.to_float(x)), input_signal_length=torch.tensor(lens), sample_rate=sr, channels=ch)
            yf, _ = rs.resample_host(rc.to_float(x), lens, plan(sr, quality), channels=ch)
            wantf = m(input_signal=torch.from_numpy(yf), input_signal_length=torch.tensor(ln.astype(np.int64)))
            assert all(torch.equal(a, b) for a, b in zip(gotf, wantf))
            hyp = m.decode(input_signal=torch.from_numpy(x), input_signal_length=torch.tensor(lens), sample_rate=sr, channels=ch)
            hyp_want = m.decode(input_signal=torch.from_numpy(y), input_signal_length=torch.tensor(ln.astype(np.int64)))
            assert [(h.text, h.start_s, h.end_s, h.utt_score) for h in hyp] == [(h.text, h.start_s, h.end_s, h.utt_score) for h in hyp_want]
            al = m.align(input_signal=torch.from_numpy(x), input_signal_length=torch.tensor(lens), labels=[[1, 2], [3]], sample_rate=sr,
                         channels=ch)
            al_want = m.align(input_signal=torch.from_numpy(y), input_signal_length=torch.tensor(ln.astype(np.int64)), labels=[[1, 2], [3]])
            assert [(h.start_s, h.end_s, h.ctc_score) for h in al] == [(h.start_s, h.end_s, h.ctc_score) for h in al_want]
        m.resample_quality = 'best'
        # the model's own rate: float mono is untouched, int16 takes the equal-rate bypass (read_wav's values)
        x16 = rc.pcm(1, 8000, 1, seed=7)
        a = m(input_signal=torch.from_numpy(rc.to_float(x16)), input_signal_length=torch.tensor([8000]))
        b = m(input_signal=torch.from_numpy(rc.to_float(x16)), input_signal_length=torch.tensor([8000]), sample_rate=16000)
        c = m(input_signal=torch.from_numpy(x16), input_signal_length=torch.tensor([8000]), sample_rate=16000)
        assert all(torch.equal(u, v) and torch.equal(u, w) for u, v, w in zip(a, b, c))
        with pytest.raises(ValueError, match='16001 Hz'):
            m(input_signal=torch.from_numpy(x16), input_signal_length=torch.tensor([8000]), sample_rate=16001)
        with pytest.raises(ValueError, match='channels needs sample_rate'):
            m(input_signal=torch.from_numpy(x16), input_signal_length=torch.tensor([8000]), channels=2)
        # transcribe() on files of other rates: what it returns for the same audio resampled by the twin, written at 16 kHz... the
        # loader trims silence first, so compare with read_wav's own output fed through the same loader path
        _write_wav(tmp_path / 'a.wav', rc.pcm(1, 6000, 1, seed=1)[0], 8000, 1)
        _write_wav(tmp_path / 'b.wav', rc.pcm(1, 30000, 2, seed=2)[0], 44100, 2)
        hyps = m.transcribe([str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav')], batch_size=2)
        assert len(hyps) == 2 and all(isinstance(h, str) for h in hyps)
