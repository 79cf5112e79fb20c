"""CTC segmentation of long recordings: every utterance of a transcript gets its start time, end time and a confidence.

For each `name.wav` under --data (a wav file or a directory of them) the transcript `name.txt` next to it, one utterance per
line, is aligned against the whole recording by EncDecCTCModel.align_long - overlapped windows through the model, the
log-probabilities stitched on the device, one banded Viterbi alignment (k_align_band) per recording - and
`<output_dir>/segments/<window_len>_<name>_segments.txt` is written: the wav path on the first line, then per utterance

    start end score | text | text_with_punct

with times in seconds; `text_with_punct` is the matching line of `name_with_punct.txt` when that file exists, else the text
again.  The score is the min-mean confidence of qasr.align.segment_scores (natural-log probabilities); parity with the
`ctc_segmentation` package's own numbers is not pinned.  An utterance whose alignment was lost is written with times -1 and
score -inf.

--star_between puts a wildcard label in front of the first utterance, between every two and behind the last
(EncDecCTCModel.align_long(star_between=True)): audio the transcript does not cover - an introduction, a jingle, a skipped
sentence - goes to the wildcards instead of being pushed onto the neighbouring utterances; the segments stay one per
utterance.  --star_penalty is what a wildcard frame pays below the frame's best class, in nats (default 1.0, not tuned on speech).

--posteriors appends one more ` | `-separated field to every utterance line: the segment's posterior, 0 .. 1 - the mean over its
frames of the probability that the transcript, aligned anywhere inside the band, is where this alignment put it
(EncDecCTCModel.align_long(posteriors=True), k_post_band behind k_align_band); `nan` for a lost alignment.  No threshold is
suggested: nothing here has been tried on speech.  Without the flag the file is what it always was.
"""
import argparse
import glob
import os
import sys
import wave

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402


def read_wav(path):
    """(int16 PCM [frames * channels], interleaved; frames; channels; rate) of a 16-bit wav file"""
    with wave.open(path, 'rb') as w:
        if w.getsampwidth() != 2:
            raise ValueError(f'{path}: {8 * w.getsampwidth()}-bit samples; 16-bit PCM is read')
        n, ch, rate = w.getnframes(), w.getnchannels(), w.getframerate()
        pcm = np.frombuffer(w.readframes(n), dtype='<i2').astype(np.int16)
    return pcm, len(pcm) // ch, ch, rate


def read_lines(path):
    with open(path, encoding='utf-8') as f:
        return [ln.strip() for ln in f if ln.strip()]


def build_model(args):
    if args.model.endswith('.nemo'):
        model = EncDecCTCModel.restore_from(restore_path=args.model)
    elif args.synthetic_model:
        model = EncDecCTCModel.from_synthetic(args.model)
    else:
        model = EncDecCTCModel.from_pretrained(model_name=args.model)
    model = model.to(args.device)
    model.eval()
    model.preprocessor.featurizer.dither = 0.0
    if args.no_quant:
        model.set_quant_mode('none')
        return model
    model.set_quant_bit(8, mode='weight')
    model.set_quant_bit(8, mode='act')
    model.encoder.bn_folding()
    if not args.dynamic:
        if args.load:
            from qasr.calib_io import load_synthetic
            distilled = load_synthetic(args.load)
        else:
            from qasr import synth
            distilled = [torch.from_numpy(a) for a in synth.make_calibration(args.synthetic_calib, 4, int(model.preprocessor.featurizer.nfilt), 500)]
        qm.calibrate(model)
        bs, _, seqlen = distilled[0].shape
        length = torch.tensor([seqlen] * bs).to(args.device)
        for inputs in distilled:
            enc, _, enc_sf = model.encoder(audio_signal=inputs.to(args.device), length=length)
            model.decoder(encoder_output=enc, encoder_output_scaling_factor=enc_sf)
    qm.evaluate(model)
    qm.set_dynamic(model, args.dynamic)
    return model


def main(argv=None):
    p = argparse.ArgumentParser(description='CTC segmentation')
    p.add_argument('--output_dir', default='output', type=str, help='output directory; the files go to <output_dir>/segments')
    p.add_argument('--data', type=str, required=True,
                   help='a wav file, or a directory of wav files; name.txt (one utterance per line) lies next to name.wav, and '
                        'name_with_punct.txt, when present, holds the same lines as they should be printed')
    p.add_argument('--window_len', type=int, default=8000,
                   help='accepted for the reference tool\'s command lines and used in the output file\'s name only: the lattice is '
                        'pruned by --band_states here, not by a window of frames')
    p.add_argument('--sample_rate', type=int, default=16000, help='the rate the model works at; files at another rate are resampled')
    p.add_argument('--model', type=str, default='QuartzNet15x5Base-En', help='a .nemo checkpoint or the name of a registered model')
    p.add_argument('--band_states', type=int, default=None, choices=[256, 1024, 4352],
                   help='lattice states kept per frame (default: the smallest that holds the transcript whole, else 4352)')
    p.add_argument('--star_between', action='store_true',
                   help='a wildcard label around and between the utterances, for audio the transcript does not cover')
    p.add_argument('--star_penalty', type=float, default=None,
                   help='with --star_between: nats per frame the wildcard pays below the frame\'s best class, 0 .. 16 (default 1.0)')
    p.add_argument('--posteriors', action='store_true',
                   help='one more field per utterance line: the posterior of the segment, 0 .. 1 (a forward-backward pass in the band)')
    p.add_argument('--window_s', type=float, default=30.0, help='seconds of audio per window of the model (overlap: 4 s, less for short windows)')
    p.add_argument('--batch_size', type=int, default=32, help='windows per batch')
    p.add_argument('--synthetic_model', action='store_true', help='seeded random weights under the model\'s name (no checkpoint needed)')
    p.add_argument('--load', type=str, default=None, help='calibration data (a file of distilled inputs) of the integer model')
    p.add_argument('--synthetic_calib', type=int, default=2, help='without --load: this many seeded random calibration batches')
    p.add_argument('--dynamic', action='store_true', help='dynamic quantisation: no calibration')
    p.add_argument('--no_quant', action='store_true', help='the float model on the host modules')
    p.add_argument('--device', type=str, default='cuda', help='cuda, or cpu with --no_quant (the NumPy twins)')
    args = p.parse_args(argv)
    if args.device != 'cuda' and not args.no_quant:
        p.error('--device cpu needs --no_quant: the integer model runs on the HIP engine only')
    if args.star_penalty is not None and not args.star_between:
        p.error('--star_penalty needs --star_between')
    star_kw = dict(star_between=True, star_penalty=1.0 if args.star_penalty is None else args.star_penalty) if args.star_between else {}
    post_kw = dict(posteriors=True) if args.posteriors else {}
    wavs = sorted(glob.glob(os.path.join(args.data, '*.wav'))) if os.path.isdir(args.data) else [args.data]
    if not wavs or not all(w.endswith('.wav') and os.path.exists(w) for w in wavs):
        p.error(f'--data {args.data}: no wav file')
    torch.set_grad_enabled(False)
    model = build_model(args)
    if int(model.preprocessor._sample_rate) != args.sample_rate:
        p.error(f'--sample_rate {args.sample_rate}: the model works at {int(model.preprocessor._sample_rate)} Hz')
    overlap_s = min(4.0, args.window_s / 4)
    seg_dir = os.path.join(args.output_dir, 'segments')
    os.makedirs(seg_dir, exist_ok=True)
    for path in wavs:
        txt = path[:-4] + '.txt'
        if not os.path.exists(txt):
            p.error(f'{path}: its transcript {txt} is missing')
        text = read_lines(txt)
        punct = path[:-4] + '_with_punct.txt'
        shown = read_lines(punct) if os.path.exists(punct) else text
        if len(shown) != len(text):
            p.error(f'{punct} has {len(shown)} lines, {txt} has {len(text)}')
        pcm, n, ch, rate = read_wav(path)
        try:
            hyp = model.align_long(torch.from_numpy(pcm).to(args.device)[None], torch.tensor([n]).to(args.device), texts=[text],
                                   window_s=args.window_s, overlap_s=overlap_s, guard_s=overlap_s / 4, batch_size=args.batch_size,
                                   band_states=args.band_states, sample_rate=rate, channels=ch, **star_kw, **post_kw)[0]
        except ValueError as e:
            p.error(f'{path}: {e}')
        out = os.path.join(seg_dir, f'{args.window_len}_' + os.path.basename(path)[:-4] + '_segments.txt')
        with open(out, 'w', encoding='utf-8') as f:
            f.write(path + '\n')
            for seg, a, b in zip(hyp.segments, text, shown):
                start, end = (-1, -1) if seg.start_s is None else (round(seg.start_s, 4), round(seg.end_s, 4))
                tail = f" | {'nan' if seg.post is None else seg.post}" if args.posteriors else ''
                f.write(f'{start} {end} {seg.score} | {a} | {b}{tail}\n')
        lost = sum(1 for s in hyp.segments if s.start_s is None)
        print(f'{path}: {len(text)} utterances' + (f', alignment lost ({lost})' if lost else '') + f' -> {out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
