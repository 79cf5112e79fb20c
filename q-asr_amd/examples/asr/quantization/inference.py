#!/usr/bin/env python3
"""Calibrate + evaluate a quantised CTC model — the reference's entry point
(examples/asr/quantization/inference.py:46-159) with the same flags, running on one MI355X.

    python inference.py --asr_model QuartzNet15x5Base-En.nemo --dataset dev_clean.json \
        --load synthetic.pkl --weight_bit 8 --act_bit 8 --percentile 99.996 --batch_size 32

Flow (identical to the reference): load model -> set bit-widths -> percentile -> BN fold -> calibrate the
QuantAct ranges on the synthetic (mel-domain) batches in host PyTorch -> `qm.evaluate` -> evaluation loop, which
now runs mel front-end + integer encoder/decoder in the HIP engine -> greedy CTC decode -> WER.
`--load` reads what the reference's synthesize.py writes (`pickle.dump([x.cpu() ...])`, synthesize.py:103-104) through
a restricted unpickler that can only rebuild tensors, or a .pt / .npz written by this repo; `--synthetic_calib N`
generates N seeded batches instead.
"""
import os
import sys
import time
from argparse import ArgumentParser

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(_HERE, '..', '..', '..')))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.metrics.wer import WER, word_error_rate  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402

if not torch.cuda.is_available():
    raise Exception("Current implementation only supports GPU (MI355X / ROCm)")


from qasr.calib_io import load_synthetic  # noqa: E402  (restricted loader for --load)


def _add_report(counts, rep):
    """--device_wer: an ErrorReport's total and oracle into the run's counts (errors, S, D, I, ref, hyp, oracle)"""
    t = rep.total
    if rep.invalid:
        raise SystemExit(f'--device_wer: {rep.invalid} rows held an id outside the vocabulary')
    for k, v in enumerate((t.errors, t.substitutions, t.deletions, t.insertions, t.ref_units, t.hyp_units, rep.oracle_errors)):
        counts[k] += v


def main():
    p = ArgumentParser()
    p.add_argument("--asr_model", type=str, default="QuartzNet15x5Base-En", required=True)
    p.add_argument("--dataset", type=str, required=True, help="path to evaluation data (JSON-lines manifest)")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--normalize_text", default=True, type=bool,
                   help="English transcript normalisation; type=bool as in the reference: pass '' for False (non-English models)")
    p.add_argument("--shuffle", action='store_true')
    p.add_argument("--load", type=str, default=None, help="load path for the synthetic data")
    p.add_argument("--percentile", type=float, default=None)
    p.add_argument("--weight_bit", type=int, default=8)
    p.add_argument("--act_bit", type=int, default=8)
    p.add_argument("--dynamic", action='store_true')
    p.add_argument("--no_quant", action='store_true')
    p.add_argument("--eval_early_stop", type=int, default=None)
    p.add_argument("--calib_early_stop", type=int, default=None)
    p.add_argument("--synthetic_calib", type=int, default=0, help="(extension) generate N seeded calibration batches")
    p.add_argument("--synthetic_model", action='store_true', help="(extension) random-init weights of --asr_model")
    p.add_argument("--dither", type=float, default=None, help="(extension) override the preprocessor's dither (0: reproducible runs)")
    p.add_argument("--dump_hyps", type=str, default=None, help="(extension) write hypotheses, references and WER as JSON")
    p.add_argument("--reserve", type=float, default=None, metavar='SECONDS',
                   help="(extension) reserve the engine once for batches of --batch_size utterances of at most SECONDS "
                        "seconds: no allocation per batch, one captured graph per length bucket (EncDecCTCModel.reserve)")
    p.add_argument("--timestamps", action='store_true',
                   help="(extension) also decode every batch with EncDecCTCModel.decode: word times and confidences "
                        "(`words`, `utt_score` per utterance in the --dump_hyps JSON); hypotheses and WER are unchanged")
    p.add_argument("--beam_width", type=int, default=None, metavar='W',
                   help="(extension) CTC prefix beam search of width W (1 .. 128, no language model) instead of the arg-max: "
                        "hypotheses and WER come from the beam (EncDecCTCModel.decode(beam_width=W)); --dump_hyps gains `beam_score`")
    p.add_argument("--lm_path", type=str, default=None,
                   help="(extension, needs --beam_width) an n-gram language model as ARPA text (gzip too; KenLM binary files "
                        "are refused: export ARPA), fused into the beam on the device; --dump_hyps gains `lm_score`")
    p.add_argument("--alpha", type=float, default=None, help="(extension, needs --lm_path) weight of the model, 0 .. 16 (default 1.0)")
    p.add_argument("--beta", type=float, default=None, help="(extension, needs --lm_path) bonus per scored word or character, -16 .. 16 (default 0.0)")
    p.add_argument("--boost_file", type=str, default=None, metavar='FILE',
                   help="(extension, needs --beam_width) phrases to boost in the beam search (hot words): one per line with an "
                        "optional <tab>weight in nats per label, '#' lines and blank lines are skipped; works with or without "
                        "--lm_path, and with --stream_chunk_s (one set for all streams, kept per stream across steps); --dump_hyps "
                        "gains `boost_score`")
    p.add_argument("--boost_weight", type=float, default=None, help="(extension, needs --boost_file) weight of the phrases without one, 0 .. 16 (default 1.0)")
    p.add_argument("--device_wer", action='store_true',
                   help="(extension) score on the device: the label rows go through the edit-distance kernel (k_edit) where they "
                        "lie and only counts are read back per batch; WER is the number printed without the flag, a line "
                        "`S / D / I:` is added and, with --beam_width W --n_best K, a line `oracle WER:` (the best of the K rows of "
                        "every utterance).  With --stream_chunk_s or --window_s the hypotheses exist as strings and are scored "
                        "through qasr.edit.error_counts.  --dump_hyps still reads the strings")
    p.add_argument("--n_best", type=int, default=None, metavar='K',
                   help="(extension, needs --beam_width and --device_wer or --mbr) rows of the beam scored per utterance for "
                        "`oracle WER:`, and the list --mbr re-ranks")
    p.add_argument("--mbr", type=str, default=None, choices=['word', 'char'],
                   help="(extension, needs --beam_width W --n_best K, K >= 2) minimum Bayes risk re-ranking of every utterance's "
                        "K rows on the device (qasr.mbr.MBR_RULES; EncDecCTCModel.decode(mbr=)): the transcripts are the picks, the "
                        "rows with the fewest expected word (character) errors against the rest of the list.  With --device_wer "
                        "`WER:` stays the beam's first row and a line `MBR WER:` is printed between `WER:` and `oracle WER:`; "
                        "--dump_hyps gains `posterior` and `mbr_risk`.  Not with --stream_chunk_s or --window_s")
    p.add_argument("--mbr_scale", type=float, default=None, help="(extension, needs --mbr) the weight of the scores in the rows' "
                        "posteriors, 0 .. 16 (default 1.0, untuned)")
    p.add_argument("--cer", action='store_true', help="(extension) character error rate: WER is computed over characters")
    p.add_argument("--alignments", type=str, default=None, metavar='OUT',
                   help="(extension, needs --device_wer) which words were wrong: the edit path of every utterance's best "
                        "hypothesis from the device (k_edit_trace behind k_edit; with --stream_chunk_s or --window_s through "
                        "qasr.edit.align_texts on the device).  OUT gets per manifest entry the audio path, the counts and the "
                        "two-line REF: / HYP: listing (characters with --cer), then the 20 most frequent substitution pairs, "
                        "deletions and insertions of the run; WER and the other outputs are unchanged")
    p.add_argument("--align", type=str, default=None, metavar='OUT',
                   help="(extension) forced alignment of every manifest line's reference text against its batch's "
                        "log-probabilities (EncDecCTCModel.align): OUT gets one JSON line per utterance - audio_filepath, text, "
                        "ctc_score (log-likelihood of the text), utt_score (its best alignment) and words [word, start_s, end_s, "
                        "score]; hypotheses, WER and the other outputs are unchanged.  With --window_s the texts are aligned "
                        "against the stitched windows of the whole recording (EncDecCTCModel.align_long, a banded lattice: any "
                        "length of text; ctc_score is then null unless --posteriors fills it)")
    p.add_argument("--star_token", type=str, default=None, metavar='TOK',
                   help="(extension, needs --align) a token such as '*' in the manifest's texts that marks audio the text does not "
                        "cover: the texts are aligned as written, TOK as a wildcard label (EncDecCTCModel.align(star=)); OUT "
                        "shows TOK as a word with its times, and ctc_score is null for a text that holds it")
    p.add_argument("--star_penalty", type=float, default=None, metavar='X',
                   help="(extension, needs --star_token or --star_between) nats per frame the wildcard pays below the frame's best "
                        "class, 0 .. 16 (default 1.0: a starting point, not tuned on speech)")
    p.add_argument("--star_between", action='store_true',
                   help="(extension, needs --align and --window_s) a wildcard in front of and behind every recording's text")
    p.add_argument("--posteriors", action='store_true',
                   help="(extension, needs --align) how sure the alignment is: a backward pass behind the "
                        "alignment (EncDecCTCModel.align(posteriors=True), k_post behind k_align); every JSON line of OUT gains "
                        "\"post\", one value in 0 .. 1 per entry of words in their order - the mean posterior of the word's label "
                        "frames.  Goes with --star_token.  With --window_s the passes run inside the band of the banded alignment "
                        "(EncDecCTCModel.align_long(posteriors=True), k_post_band behind k_align_band): ctc_score is then the "
                        "log-likelihood inside the band, and with --star_between the line also gains \"segments\", [text, "
                        "start_s, end_s, score, post] per utterance")
    p.add_argument("--spot_file", type=str, default=None, metavar='FILE',
                   help="(extension, needs --spot) keywords to look for, one phrase per line (empty lines and lines that start "
                        "with # are skipped)")
    p.add_argument("--spot", type=str, default=None, metavar='OUT',
                   help="(extension, needs --spot_file) keyword spotting (EncDecCTCModel.spot, k_star and k_spot behind the forward): "
                        "OUT gets one JSON line per manifest entry - audio_filepath and hits [{keyword, start, end, score}], times "
                        "in seconds, score the mean likelihood ratio against the frame's best class in nats per frame (0: the "
                        "keyword is the greedy path there); hypotheses, WER and the other outputs are unchanged.  With --window_s "
                        "the keywords are searched in the stitched windows of the whole recording (EncDecCTCModel.spot_long).  With "
                        "--stream_chunk_s the manifest plays through streaming sessions that spot on the live stream "
                        "(EncDecCTCModel.stream(spot=), k_star and k_stream_spot behind k_stream_emit in every step): the same lines, "
                        "every hit with \"detected_s\", the stream time at which it became final; not with --beam_width")
    p.add_argument("--spot_threshold", type=float, default=None, metavar='X',
                   help="(extension, needs --spot) the lowest score a hit may have, -16 .. 0 nats per frame (default -1.0, untried on speech)")
    p.add_argument("--spot_max_span_s", type=float, default=None, metavar='S',
                   help="(extension, needs --spot) the longest hit in seconds (default 10.0, untried on speech)")
    p.add_argument("--input_rate", type=int, default=None, metavar='HZ',
                   help="(extension) every file of the manifest is 16-bit mono PCM at this rate (a telephone corpus at 8000, say): "
                        "the batches stay int16 and are resampled to the model's rate on the device (k_resample) in front of the "
                        "mel front-end; a file of another rate is an error.  Without it files of any rate are resampled on the "
                        "host while they are read")
    p.add_argument("--resample_quality", type=str, default=None, choices=['best', 'fast'],
                   help="(extension, needs --input_rate) filter preset of the device resampler (default best)")
    p.add_argument("--window_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, for long recordings) cut every manifest entry into windows of this many seconds, run them as "
                        "batches of --batch_size and stitch the results on the device (EncDecCTCModel.decode_long)")
    p.add_argument("--overlap_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --window_s) overlap of neighbouring windows (default 4.0)")
    p.add_argument("--stream_chunk_s", type=float, default=None, metavar='SECONDS',
                   help="(extension) play every manifest entry through a streaming session (EncDecCTCModel.stream), --batch_size "
                        "streams at a time in chunks of this many seconds; hypotheses and WER come from the sessions' final results.  "
                        "With --input_rate (and --resample_quality) the streams carry int16 PCM at that rate and every stream is "
                        "resampled on the device as it arrives")
    p.add_argument("--stream_left_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --stream_chunk_s) context in front of every chunk (default 4.0)")
    p.add_argument("--stream_right_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --stream_chunk_s) look-ahead behind every chunk (default 0.96)")
    p.add_argument("--stream_beam_lag_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --stream_chunk_s and --beam_width) the commit lag of the streaming beam search "
                        "(EncDecCTCModel.stream(beam=)): text older than this becomes final (default 4.0, untried on speech)")
    p.add_argument("--stream_endpoint_silence_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --stream_chunk_s) cut every stream into utterances on the device "
                        "(EncDecCTCModel.stream(endpoint=), decoder-driven: blank against non-blank final frames): an utterance "
                        "ends after this many seconds without speech behind speech.  The utterance count is printed and WER is "
                        "scored on each recording's utterance texts joined by a space (nothing for Zh).  With --beam_width the "
                        "endpointing goes into the StreamBeam (StreamBeam(endpoint=)): the beam is finalised and reset at "
                        "every cut and the utterance texts are the beam's.  Untried on speech")
    p.add_argument("--stream_endpoint_timeout_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --stream_endpoint_silence_s) an utterance without any speech ends after this long "
                        "(default 5.0, untried on speech)")
    p.add_argument("--stream_max_utt_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --stream_endpoint_silence_s) an utterance this long ends at the next blank frame "
                        "(default 30.0, untried on speech)")
    p.add_argument("--stream_hard_max_s", type=float, default=None, metavar='SECONDS',
                   help="(extension, needs --stream_endpoint_silence_s) an utterance this long ends wherever it stands "
                        "(default 40.0, untried on speech)")
    args = p.parse_args()
    if args.stream_endpoint_silence_s is not None and args.stream_chunk_s is None:
        p.error('--stream_endpoint_silence_s needs --stream_chunk_s')
    for flag in ('stream_endpoint_timeout_s', 'stream_max_utt_s', 'stream_hard_max_s'):
        if getattr(args, flag) is not None and args.stream_endpoint_silence_s is None:
            p.error(f'--{flag} needs --stream_endpoint_silence_s')
    if (args.stream_left_s is not None or args.stream_right_s is not None) and args.stream_chunk_s is None:
        p.error('--stream_left_s and --stream_right_s need --stream_chunk_s')
    if args.stream_beam_lag_s is not None and (args.stream_chunk_s is None or args.beam_width is None):
        p.error('--stream_beam_lag_s needs --stream_chunk_s and --beam_width')
    if args.stream_chunk_s is not None:
        for flag in ('window_s', 'align'):
            if getattr(args, flag) is not None:
                p.error(f'--stream_chunk_s does not go with --{flag}: a streaming session steps by chunks')
        if args.spot is not None and args.beam_width is not None:
            p.error('--stream_chunk_s with --spot does not go with --beam_width: keyword spotting in a streaming beam session '
                    '(stream(spot=) together with beam=) is not built')
    if (args.spot is None) != (args.spot_file is None):
        p.error('--spot OUT and --spot_file FILE go together')
    if (args.spot_threshold is not None or args.spot_max_span_s is not None) and args.spot is None:
        p.error('--spot_threshold and --spot_max_span_s need --spot')
    if args.spot_threshold is not None and not -16.0 <= args.spot_threshold <= 0.0:
        p.error(f'--spot_threshold must be -16 .. 0, got {args.spot_threshold}')
    if args.overlap_s is not None and args.window_s is None:
        p.error('--overlap_s needs --window_s')
    if args.alignments is not None and not args.device_wer:
        p.error('--alignments OUT needs --device_wer')
    if args.mbr is not None and args.beam_width is None:
        p.error('--mbr needs --beam_width W --n_best K (the greedy path has one hypothesis, nothing to re-rank)')
    if args.mbr is not None and (args.n_best is None or args.n_best < 2):
        p.error('--mbr needs --n_best K with K >= 2 (a list of one row has nothing to re-rank)')
    if args.mbr is not None and (args.stream_chunk_s is not None or args.window_s is not None):
        p.error('--mbr does not go with --stream_chunk_s or --window_s: MBR re-ranking is built for decode() alone')
    if args.mbr_scale is not None and (args.mbr is None or not 0.0 <= args.mbr_scale <= 16.0):
        p.error('--mbr_scale needs --mbr and a value in 0 .. 16')
    if args.n_best is not None and ((not args.device_wer and args.mbr is None) or args.beam_width is None
                                    or not 1 <= args.n_best <= args.beam_width):
        p.error('--n_best K needs --beam_width W, 1 <= K <= W, and --device_wer or --mbr')
    if args.star_token is not None and (args.align is None or args.shuffle):
        p.error('--star_token needs --align and does not go with --shuffle: the texts are read from the manifest in order')
    if args.star_between and (args.align is None or args.window_s is None):
        p.error('--star_between needs --align and --window_s')
    if args.posteriors and args.align is None:
        p.error('--posteriors needs --align')
    if args.star_penalty is not None and args.star_token is None and not args.star_between:
        p.error('--star_penalty needs --star_token or --star_between')
    if args.star_penalty is not None and not 0.0 <= args.star_penalty <= 16.0:
        p.error(f'--star_penalty must be 0 .. 16, got {args.star_penalty}')
    if args.window_s is not None and args.timestamps and args.beam_width is not None:
        p.error('--timestamps with --window_s and --beam_width is not offered: stitched beam hypotheses carry no times')
    if args.resample_quality is not None and args.input_rate is None:
        p.error('--resample_quality needs --input_rate')
    if args.beam_width is not None and not 1 <= args.beam_width <= 128:
        p.error(f'--beam_width must be 1 .. 128, got {args.beam_width}')
    if args.lm_path is not None and args.beam_width is None:
        p.error('--lm_path needs --beam_width')
    if (args.alpha is not None or args.beta is not None) and args.lm_path is None:
        p.error('--alpha and --beta need --lm_path')
    alpha, beta = 1.0 if args.alpha is None else args.alpha, 0.0 if args.beta is None else args.beta
    if not 0.0 <= alpha <= 16.0 or not abs(beta) <= 16.0:
        p.error(f'--alpha must be 0 .. 16 and --beta -16 .. 16, got {alpha} and {beta}')
    if args.boost_file is not None and args.beam_width is None:
        p.error('--boost_file needs --beam_width')
    if args.boost_weight is not None and args.boost_file is None:
        p.error('--boost_weight needs --boost_file')
    boost_weight = 1.0 if args.boost_weight is None else args.boost_weight
    if not 0.0 <= boost_weight <= 16.0:
        p.error(f'--boost_weight must be 0 .. 16, got {boost_weight}')
    if args.boost_file is not None and not os.path.isfile(args.boost_file):      # before the model is built
        p.error(f'--boost_file {args.boost_file}: no such file')
    torch.set_grad_enabled(False)

    if args.asr_model.endswith('.nemo'):
        asr_model = EncDecCTCModel.restore_from(restore_path=args.asr_model)
    elif args.synthetic_model:
        asr_model = EncDecCTCModel.from_synthetic(args.asr_model)
    else:
        asr_model = EncDecCTCModel.from_pretrained(model_name=args.asr_model)
    asr_model = asr_model.cuda()
    if args.dither is not None:
        asr_model.preprocessor.featurizer.dither = args.dither
    rate_kw = {}
    if args.input_rate is not None:
        from qasr import resample as qresample
        asr_model.resample_quality = args.resample_quality or 'best'
        try:                                                 # a rate without a plan is refused here, by name
            qresample.ResamplePlan(args.input_rate, asr_model.preprocessor._sample_rate, asr_model.resample_quality)
        except ValueError as e:
            p.error(f'--input_rate: {e}')
        rate_kw = dict(sample_rate=args.input_rate)
    asr_model.setup_test_data(test_data_config={
        'sample_rate': 16000, 'manifest_filepath': args.dataset, 'labels': asr_model.decoder.vocabulary,
        'batch_size': args.batch_size, 'normalize_transcripts': args.normalize_text, 'shuffle': args.shuffle,
        'input_rate': args.input_rate})

    distilled = None
    if args.load is not None:
        print('Data loaded from %s' % args.load)
        distilled = load_synthetic(args.load)
    elif args.synthetic_calib:
        from qasr import synth
        distilled = [torch.from_numpy(a) for a in synth.make_calibration(args.synthetic_calib, args.batch_size, 64, 500)]
    else:
        assert args.dynamic, "synthetic data must be loaded unless running with the dynamic quantization mode"

    asr_model.eval()
    asr_model.set_quant_bit(args.weight_bit, mode='weight')
    asr_model.set_quant_bit(args.act_bit, mode='act')
    if args.percentile is not None:
        qm.set_percentile(asr_model, args.percentile)
    if args.no_quant:
        asr_model.set_quant_mode('none')
    else:
        asr_model.encoder.bn_folding()

    if not args.dynamic and not args.no_quant:
        print('Calibrating...')
        qm.calibrate(asr_model)
        bs, _, seqlen = distilled[0].shape
        length = torch.tensor([seqlen] * bs).cuda()
        for i, inputs in enumerate(distilled):
            if args.calib_early_stop is not None and i == args.calib_early_stop:
                break
            enc, enc_len, enc_sf = asr_model.encoder(audio_signal=inputs.cuda(), length=length)
            asr_model.decoder(encoder_output=enc, encoder_output_scaling_factor=enc_sf)

    print('Evaluating...')
    qm.evaluate(asr_model)
    qm.set_dynamic(asr_model, args.dynamic)
    if args.reserve:
        asr_model.reserve(args.batch_size, args.reserve)
    labels_map = dict(enumerate(asr_model.decoder.vocabulary))
    wer = WER(vocabulary=asr_model.decoder.vocabulary)
    dev_wer = WER(vocabulary=asr_model.decoder.vocabulary, use_cer=args.cer, device=True) if args.device_wer else None
    dev_counts = [0] * 7                                     # --device_wer beyond the greedy path: errors, S, D, I, ref, hyp, oracle
    need_text = not args.device_wer or bool(args.dump_hyps)  # the strings are read only where something needs them
    hyps, refs, words, utt_scores, beam_scores, lm_scores, boost_scores = [], [], [], [], [], [], []
    mbr_kw = dict(mbr=args.mbr, mbr_scale=1.0 if args.mbr_scale is None else args.mbr_scale) if args.mbr is not None else {}
    mbr_errors, posteriors, mbr_risks = 0, [], []            # --mbr: the picks' errors (--device_wer), their posterior and expected errors
    lm_kw = dict(lm=args.lm_path, alpha=alpha, beta=beta) if args.lm_path is not None else {}
    if args.boost_file is not None:                          # compiled once for the run: the file does not change per batch
        from qasr import boost as qboost
        lm_kw['boost'] = qboost.PhraseSet(qboost.read_phrase_file(args.boost_file), asr_model.decoder.vocabulary, weight=boost_weight)
    aligned, items = [], getattr(asr_model.test_dataloader().dataset, 'items', [])
    listed = []                                              # --alignments: one qasr.ctc.Alignment (or None) per utterance
    spotted, spot_words = [], []
    if args.spot is not None:                                # read once for the run: the list does not change per batch
        with open(args.spot_file, encoding='utf-8') as f:
            spot_words = [ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith('#')]
        if not spot_words:
            p.error(f'--spot_file {args.spot_file} holds no keyword')
    audio_s, t0 = 0.0, time.time()
    stream_sess, n_utterances = None, 0
    for i, batch in enumerate(asr_model.test_dataloader()):
        if i == args.eval_early_stop:
            break
        batch = [x.cuda() for x in batch]
        signal = batch[0] if rate_kw else batch[0].float()   # --input_rate: int16 PCM, resampled inside the model's call
        if args.stream_chunk_s is not None:                  # one session per batch: k_stream_push / _window / _emit per step
            if stream_sess is None:                          # one session for the whole manifest: one reservation, one graph
                stream_beam = None
                if args.beam_width is not None:              # k_topn + k_stream_beam in front of k_stream_emit in every step
                    from qasr import stream_beam as qsb
                    stream_beam = qsb.StreamBeam(width=args.beam_width, lm=args.lm_path, alpha=alpha, beta=beta,
                                                 lag_s=4.0 if args.stream_beam_lag_s is None else args.stream_beam_lag_s,
                                                 boost=lm_kw.get('boost'),   # one set for all streams: k_stream_beam_boost
                                                 boost_weight=boost_weight)
                stream_ep = None
                if args.stream_endpoint_silence_s is not None:               # k_stream_endpoint behind k_stream_emit in every step
                    from qasr import stream_ep as qse
                    dflt = qse.Endpointing()
                    pick = lambda v, d: d if v is None else v
                    stream_ep = qse.Endpointing(args.stream_endpoint_silence_s, pick(args.stream_endpoint_timeout_s, dflt.start_timeout_s),
                                                pick(args.stream_max_utt_s, dflt.max_utt_s), pick(args.stream_hard_max_s, dflt.hard_max_s))
                if stream_beam is not None and stream_ep is not None:        # k_stream_beam_ep behind emit and endpoint in every step
                    stream_beam.endpoint, stream_ep = stream_ep, None
                stream_spot = None
                if args.spot is not None:                                    # k_star + k_stream_spot behind k_stream_emit in every step
                    from qasr import stream_spot as qss
                    stream_spot = qss.StreamSpot(keywords=spot_words, threshold=-1.0 if args.spot_threshold is None else args.spot_threshold,
                                                 max_span_s=10.0 if args.spot_max_span_s is None else args.spot_max_span_s)
                try:
                    stream_sess = asr_model.stream(max_streams=args.batch_size, chunk_s=args.stream_chunk_s, tail=False,
                                                   left_s=4.0 if args.stream_left_s is None else args.stream_left_s,
                                                   right_s=0.96 if args.stream_right_s is None else args.stream_right_s,
                                                   input_rate=args.input_rate,       # int16 PCM: resampled per stream on the device
                                                   beam=stream_beam, endpoint=stream_ep, spot=stream_spot)
                except ValueError as e:
                    p.error(f'--stream_chunk_s / --stream_left_s / --stream_right_s / --input_rate / --stream_beam_lag_s / '
                            f'--stream_endpoint_silence_s and its times / --spot and its arguments: {e}')
            stream_hyps = asr_model.decode_stream(signal, batch[1], session=stream_sess)
            if stream_sess.spot is not None:                     # the hits that closed while the recordings played, END included
                stream_hyps = stream_hyps[0]
                for row in stream_sess.decoded_hits:
                    k = len(spotted)
                    spotted.append(dict(audio_filepath=items[k][0] if not args.shuffle and k < len(items) else None,
                                        hits=[dict(keyword=h.hit.keyword, start=h.hit.start_s, end=h.hit.end_s, score=h.hit.score,
                                                   detected_s=h.detected_s) for h in row]))
            for h in stream_hyps:
                if stream_sess.endpoint is not None:             # a recording's utterances: texts joined (by nothing for Zh)
                    n_utterances += len(h)
                    sep = ' ' if ' ' in asr_model.decoder.vocabulary else ''     # (Zh: no space label)
                    hyps.append(sep.join(u.hypothesis.text for u in h if u.hypothesis.text))
                    if args.beam_width is not None:
                        beam_scores.append([u.hypothesis.utt_score for u in h])
                        lm_scores.append([u.hypothesis.lm_score for u in h])
                        boost_scores.append([u.hypothesis.boost_score for u in h])
                    elif args.timestamps:
                        words.append([list(w) for u in h for w in u.hypothesis.words])
                        utt_scores.append([u.hypothesis.utt_score for u in h])
                    continue
                hyps.append(h.text)
                if args.beam_width is not None:
                    beam_scores.append(h.utt_score)
                    lm_scores.append(h.lm_score)
                    boost_scores.append(h.boost_score)
                elif args.timestamps:
                    words.append([list(w) for w in h.words])
                    utt_scores.append(h.utt_score)
        elif args.window_s is not None:                      # k_cut, windows in batches, k_stitch, one collapse / search
            overlap_s = 4.0 if args.overlap_s is None else args.overlap_s
            try:
                long_hyps = asr_model.decode_long(signal, batch[1], window_s=args.window_s, overlap_s=overlap_s,
                                                  guard_s=min(1.0, overlap_s / 4), batch_size=args.batch_size,
                                                  beam_width=args.beam_width, **lm_kw, **rate_kw)
            except ValueError as e:
                p.error(f'--window_s / --overlap_s: {e}')
            for h in long_hyps:
                hyps.append(h.text)
                if args.beam_width is not None:
                    beam_scores.append(h.utt_score)
                    lm_scores.append(h.lm_score)
                    boost_scores.append(h.boost_score)
                elif args.timestamps:
                    words.append([list(w) for w in h.words])
                    utt_scores.append(h.utt_score)
        elif args.beam_width is not None:                    # k_topn + k_beam behind the forward, on the same stream
            if args.device_wer:                              # ... and k_edit behind them: only the counts are read back
                rep = asr_model.error_rate(input_signal=signal, input_signal_length=batch[1], targets=batch[2], use_cer=args.cer,
                                           beam_width=args.beam_width, n_best=args.n_best or 1,
                                           alignments=args.alignments is not None, **lm_kw, **rate_kw, **mbr_kw)
                _add_report(dev_counts, rep)
                mbr_errors += rep.mbr_total.errors if mbr_kw else 0
                listed += rep.alignments or []               # --alignments: k_edit_trace over the best rows
            for h in (asr_model.decode(input_signal=signal, input_signal_length=batch[1], beam_width=args.beam_width,
                                       **lm_kw, **rate_kw, **(dict(mbr_kw, n_best=args.n_best) if mbr_kw else {})) if need_text else ()):
                if mbr_kw:                                   # the list in MBR order: the transcript is the pick
                    h = h[0]
                    posteriors.append(h.posterior)
                    mbr_risks.append(h.mbr_risk)
                hyps.append(h.text)
                beam_scores.append(h.utt_score)
                lm_scores.append(h.lm_score)
                boost_scores.append(h.boost_score)
        else:
            log_probs, enc_len, greedy = asr_model(input_signal=signal, input_signal_length=batch[1], **rate_kw)
            if dev_wer is not None:                          # k_ctc over the padded rows, then k_edit against the padded targets
                dev_wer.update(greedy, batch[2], None)
            if need_text:
                hyps += wer.ctc_decoder_predictions_tensor(greedy)
            if args.alignments is not None:                  # the rows dev_wer scored (k_ctc over the padded rows), through k_edit_trace
                from qasr import edit as qedit, engine as qengine
                vocab, mode = list(asr_model.decoder.vocabulary), 'char' if args.cer else 'word'
                mask = None if args.cer else qedit.space_mask(vocab, '--alignments')
                col = qengine.ctc_collapse(greedy, lens=None, blank=dev_wer.blank_id)
                tg = batch[2] if batch[2].shape[1] else torch.zeros(batch[2].shape[0], 1, device=greedy.device, dtype=torch.int32)
                tr = qedit.trace_device(col.labels, col.n_labels, tg, None, len(vocab), mode=mode,
                                        is_space=None if mask is None else torch.from_numpy(mask).cuda())
                cpu = lambda t: t.cpu().numpy()
                listed += qedit.alignments_of(qedit.TraceResult(cpu(tr.rows), cpu(tr.ops), cpu(tr.n_ops), 1), cpu(col.labels),
                                              cpu(col.n_labels), cpu(tg), None, vocab, mode=mode, is_space=mask)
        if args.timestamps and args.window_s is None and args.stream_chunk_s is None:        # device-side collapse up to each utterance's encoded length
            for h in asr_model.decode(input_signal=signal, input_signal_length=batch[1], **rate_kw):
                words.append([list(w) for w in h.words])
                utt_scores.append(h.utt_score)
        if args.align:                                       # the reference texts' own labels, one k_align launch per batch
            ref_ids = [row[:int(n)].tolist() for row, n in zip(batch[2].cpu(), batch[3].cpu())]
            ref_kw = dict(labels=ref_ids)
            if args.star_token is not None or args.star_between:     # the wildcard: k_star in front of the alignment
                ref_kw.update(star=args.star_token, star_penalty=1.0 if args.star_penalty is None else args.star_penalty)
            if args.star_token is not None:                          # the texts as the manifest has them: the data layer drops the token
                raw = asr_model.test_dataloader().dataset.raw_texts[len(aligned):len(aligned) + len(ref_ids)]
                ref_kw.update(labels=None, texts=list(raw))
            if args.window_s is not None:                    # long recordings: windows, k_stitch, one k_align_band launch
                overlap_s = 4.0 if args.overlap_s is None else args.overlap_s
                if args.star_between:                        # one utterance per recording: a wildcard in front of it and behind it
                    ref_kw.update({k: [[v] for v in ref_kw[k]] for k in ('labels', 'texts') if ref_kw.get(k) is not None},
                                  star_between=True)
                if args.posteriors:                          # k_post_band behind k_align_band
                    ref_kw.update(posteriors=True)
                try:
                    got = asr_model.align_long(signal, batch[1], window_s=args.window_s, overlap_s=overlap_s,
                                               guard_s=min(1.0, overlap_s / 4), batch_size=args.batch_size, **ref_kw, **rate_kw)
                except ValueError as e:
                    p.error(f'--align with --window_s / --overlap_s: {e}')
            else:
                if args.posteriors:
                    ref_kw.update(posteriors=True)
                got = asr_model.align(input_signal=signal, input_signal_length=batch[1], **ref_kw, **rate_kw)
            for h in got:
                k = len(aligned)
                aligned.append(dict(audio_filepath=items[k][0] if not args.shuffle and k < len(items) else None, text=h.text,
                                    ctc_score=h.ctc_score, utt_score=h.utt_score, words=[list(w) for w in h.words]))
                if args.posteriors:
                    aligned[-1]['post'] = list(h.word_post)
                    if h.segments is not None:
                        aligned[-1]['segments'] = [[sg.text, sg.start_s, sg.end_s, sg.score, sg.post] for sg in h.segments]
        if args.spot is not None and args.stream_chunk_s is None:       # k_star + k_spot behind the forward (with --window_s: behind k_stitch)
            spot_kw = dict(keywords=spot_words, threshold=-1.0 if args.spot_threshold is None else args.spot_threshold,
                           max_span_s=10.0 if args.spot_max_span_s is None else args.spot_max_span_s)
            try:
                if args.window_s is not None:
                    overlap_s = 4.0 if args.overlap_s is None else args.overlap_s
                    found = asr_model.spot_long(signal, batch[1], window_s=args.window_s, overlap_s=overlap_s,
                                                guard_s=min(1.0, overlap_s / 4), batch_size=args.batch_size, **spot_kw, **rate_kw)
                else:
                    found = asr_model.spot(input_signal=signal, input_signal_length=batch[1], **spot_kw, **rate_kw)
            except ValueError as e:
                p.error(f'--spot: {e}')
            for row in found:
                k = len(spotted)
                spotted.append(dict(audio_filepath=items[k][0] if not args.shuffle and k < len(items) else None,
                                    hits=[dict(keyword=h.keyword, start=h.start_s, end=h.end_s, score=h.score) for h in row]))
        strings_scored = args.device_wer and (args.stream_chunk_s is not None or args.window_s is not None)
        if need_text or strings_scored:
            for row in batch[2].cpu().numpy():
                refs.append(''.join(labels_map[c] for c in row))
        if strings_scored:                                   # hypotheses that exist only as strings
            from qasr.edit import error_counts
            n = batch[2].shape[0]
            c = error_counts(hyps[-n:], refs[-n:], use_cer=args.cer, device='cuda')
            for k, v in enumerate((c.errors, c.substitutions, c.deletions, c.insertions, c.ref_units, c.hyp_units, c.errors)):
                dev_counts[k] += v
            if args.alignments is not None:
                from qasr.edit import align_texts
                listed += align_texts(hyps[-n:], refs[-n:], use_cer=args.cer, device='cuda')
        audio_s += float(batch[1].sum()) / float(args.input_rate or 16000)
    torch.cuda.synchronize()
    wall = time.time() - t0
    served = type(getattr(asr_model, '_engine', None) or getattr(asr_model, '_ragged_engine', None)).__name__
    if stream_sess is not None:                              # the session's engine leaves with its reservation
        stream_sess.close_all()
        served = stream_sess.served
    print('path:', {'Engine': 'static integer engine (HIP)', 'DynamicRunner': 'dynamic device path (HIP)'}.get(
        served, 'host modules'))
    if stream_sess is not None and stream_sess.endpoint is not None:
        print('utterances:', n_utterances)
    if args.device_wer:
        if dev_wer is not None and args.beam_width is None and args.stream_chunk_s is None and args.window_s is None:
            c = dev_wer.counts()                             # the one read of the metric's totals block
            dev_counts = [c.errors, c.substitutions, c.deletions, c.insertions, c.ref_units, c.hyp_units, c.errors]
        wer_value = 1.0 * dev_counts[0] / dev_counts[4] if dev_counts[4] != 0 else float('inf')
    else:
        wer_value = word_error_rate(hypotheses=hyps, references=refs, use_cer=args.cer)
    print('WER:', wer_value)
    if args.device_wer:
        print('S / D / I:', dev_counts[1], '/', dev_counts[2], '/', dev_counts[3])
        if args.mbr is not None:
            print('MBR WER:', 1.0 * mbr_errors / dev_counts[4] if dev_counts[4] != 0 else float('inf'))
        if args.beam_width is not None and args.n_best and args.stream_chunk_s is None and args.window_s is None:
            print('oracle WER:', 1.0 * dev_counts[6] / dev_counts[4] if dev_counts[4] != 0 else float('inf'))
    if args.dump_hyps:
        import json
        with open(args.dump_hyps, 'w') as f:
            extra = dict(words=words, utt_score=utt_scores) if args.timestamps else {}
            if args.beam_width is not None:
                extra.update(beam_width=args.beam_width, beam_score=beam_scores)
            if args.mbr is not None:
                extra.update(mbr=args.mbr, mbr_scale=mbr_kw['mbr_scale'], n_best=args.n_best, posterior=posteriors, mbr_risk=mbr_risks)
                if args.device_wer:                          # `wer` is the beam's first row there; the hypotheses are the picks
                    extra.update(mbr_wer=1.0 * mbr_errors / dev_counts[4] if dev_counts[4] != 0 else float('inf'))
            if args.lm_path is not None:
                extra.update(lm_path=args.lm_path, alpha=alpha, beta=beta, lm_score=lm_scores)
            if args.boost_file is not None:
                extra.update(boost_file=args.boost_file, boost_weight=boost_weight, boost_score=boost_scores)
            if stream_sess is not None and stream_sess.endpoint is not None:
                extra.update(utterances=n_utterances)
            json.dump(dict(hypotheses=hyps, references=refs, wer=wer_value, path=served, **extra), f)
    if args.alignments:
        from qasr.edit import confusions, listing
        with open(args.alignments, 'w', encoding='utf-8') as f:
            for k, a in enumerate(listed):
                f.write(f'{items[k][0] if not args.shuffle and k < len(items) else None}\n')
                if a is None:                                    # a row the kernel refused: an id outside the vocabulary
                    f.write('not scored\n\n')
                    continue
                c = a.counts
                f.write(f'errors {c.errors}  S {c.substitutions}  D {c.deletions}  I {c.insertions}  ref {c.ref_units}  hyp {c.hyp_units}\n')
                f.write(listing(a) + '\n\n')
            sub, dele, ins = confusions(listed, top=20)
            f.write('substitutions (ref -> hyp):\n' + ''.join(f'{n:6d}  {r!r} -> {h!r}\n' for (r, h), n in sub))
            f.write('deletions:\n' + ''.join(f'{n:6d}  {u!r}\n' for u, n in dele))
            f.write('insertions:\n' + ''.join(f'{n:6d}  {u!r}\n' for u, n in ins))
        print(f'listed {len(listed)} alignments -> {args.alignments}')
    if args.align:
        import json
        with open(args.align, 'w', encoding='utf-8') as f:
            for rec in aligned:                                  # a text that is not alignable has scores -inf: written as null
                rec = {k: (None if isinstance(v, float) and v == float('-inf') else v) for k, v in rec.items()}
                f.write(json.dumps(rec, ensure_ascii=False) + '\n')
        print(f'aligned {len(aligned)} transcripts ({sum(1 for r in aligned if r["words"])} with word times) -> {args.align}')
    if args.spot:
        import json
        with open(args.spot, 'w', encoding='utf-8') as f:
            for rec in spotted:
                f.write(json.dumps(rec, ensure_ascii=False) + '\n')
        print(f'spotted {sum(len(r["hits"]) for r in spotted)} hits of {len(spot_words)} keywords in {len(spotted)} recordings -> {args.spot}')
    print(f'RTFx (incl. host data loading): {audio_s / max(wall, 1e-9):.1f}  ({audio_s:.1f} s audio in {wall:.2f} s)')


if __name__ == '__main__':
    main()
