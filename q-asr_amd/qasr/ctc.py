"""Greedy CTC decoding past the arg-max: the host statement of k_ctc (csrc/qasr_ctc.hip, include/qasr.h) and the
step from compact labels to strings, timestamps and confidences.  NumPy only: no GPU, no native library.

`collapse_host` is the CPU fallback of EncDecCTCModel.decode and the yardstick the GPU tests compare k_ctc with, bit for
bit.  The rule is the loop of WER.ctc_decoder_predictions_tensor (nemo/collections/asr/metrics/wer.py): a frame's token p
is kept when `(p != previous or previous == blank) and p != blank`, i.e. every maximal run of one non-blank token emits
one label."""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np


@dataclass
class CtcResult:
    """Outputs of one collapse, row pitch T (arrays: NumPy on the host, torch tensors from the device binding).
    labels [B, T] int32 (tail: blank), n_labels [B] int32, start / nframes [B, T] int32 (tail 0), score [B, T] float32
    (tail 0) and utt_score [B] float32; the last two are None without frame scores."""
    labels: object
    n_labels: object
    start: object = None
    nframes: object = None
    score: object = None
    utt_score: object = None
    blank: int = -1
    frame_score: object = None              # [B, T] float32 the scores were taken from (the engine's decode= fills it)


@dataclass
class Segment:
    """One utterance of a transcript inside a long recording (EncDecCTCModel.align_long): from the first frame of its first
    label to the end of its last label's run, in seconds of the recording; score: qasr.align.segment_scores (-inf, with times
    None, when the alignment was lost); post: with align_long(posteriors=True) the mean over the segment's frames of
    exp(frame_post), in float64, 0 .. 1 - how much of the transcript's probability mass inside the band passes through the
    alignment there (None without posteriors and for a lost alignment)."""
    text: str
    start_s: Optional[float]
    end_s: Optional[float]
    score: float
    post: Optional[float] = None


@dataclass
class KeywordHit:
    """One occurrence of a keyword (EncDecCTCModel.spot / spot_long; qasr.spot.SPOT_RULES): keyword as it was given (the string,
    or the label ids), index: its position in the keyword list, start_s / end_s: from the start of its first frame to the end of
    its last, in seconds, frames: the span in frames, score: the mean over the span of the likelihood ratio against the frame's
    best class, in nats per frame, <= 0 - 0 means the keyword is the greedy path over its span."""
    keyword: object
    index: int
    start_s: float
    end_s: float
    score: float
    frames: int


@dataclass
class StreamHit:
    """One final keyword hit of a streaming session (EncDecCTCModel.stream(spot=), qasr.stream_spot.STREAM_SPOT_RULES): the
    stream's slot, the KeywordHit in seconds of the stream, and detected_s: the end of the final frame after which the hit
    closed - the stream time at which it became certain that nothing can replace it."""
    slot: int
    hit: KeywordHit
    detected_s: float


@dataclass
class StreamUpdate:
    """What one step of a streaming session (EncDecCTCModel.stream) made final for one stream: the labels whose runs closed,
    their text, start / end times in seconds of the stream and confidences (best frame log-probability of each run), and
    tail_text: the provisional text of the look-ahead frames, which the next step may change."""
    slot: int
    labels: List[int]
    text: str
    start_s: List[float]
    end_s: List[float]
    score: List[float]
    tail_text: str = ''


@dataclass
class Hypothesis:
    text: str
    labels: List[int]
    start_s: List[float]
    end_s: List[float]
    score: Optional[List[float]]            # per label: best frame log-probability inside the label's run
    utt_score: Optional[float]              # log-probability of the greedy path
    words: List[Tuple[str, float, float, Optional[float]]] = field(default_factory=list)
    lm_score: Optional[float] = None        # beam search with a language model: the model's share of utt_score
    ctc_score: Optional[float] = None       # forced alignment (qasr.align): the CTC log-likelihood of the text, all alignments
    boost_score: Optional[float] = None     # beam search with phrase boosting (qasr.boost): the boosting's share of utt_score
    segments: Optional[List[Segment]] = None  # align_long with a list of utterances: one Segment per utterance
    # align / decode(timestamps=True) with posteriors=True (qasr.align.POST_RULES): how much of the text's probability mass agrees
    post: Optional[List[float]] = None      # per label: the mean posterior of its state over its run, 0 .. 1
    post_min: Optional[List[float]] = None  # per label: the posterior at its least certain frame
    word_post: Optional[List[float]] = None  # one per entry of words: the mean over the frames of the word's labels
    frame_post: Optional[object] = None     # float32 [frames]: the log-posterior (nats) of the path's state at every frame
    # decode(mbr=) (qasr.mbr.MBR_RULES): the n-best list in minimum Bayes risk order
    posterior: Optional[float] = None       # the row's normalised weight among the rows of its list, 0 .. 1
    mbr_risk: Optional[float] = None        # its expected number of errors against the list, in the mode's units (words / characters)
    beam_rank: Optional[int] = None         # its place in the beam's list (0: the row with the best path score)
    seams_s: Optional[List[float]] = None   # decode_long (qasr.longform): the times at which neighbouring windows were joined


@dataclass
class StreamUtterance:
    """One finished utterance of a stream (EncDecCTCModel.stream(endpoint=), qasr.stream_ep.EP_RULES): its number in the
    stream, why it ended ('silence' | 'timeout' | 'max' | 'hard' | 'end'), its span and the span of its speech frames in
    seconds of the stream (None: no speech frame), and the Hypothesis of its labels - times in seconds of the stream,
    utt_score the greedy path's log-probability over the utterance's own frames.  A 'timeout' utterance has no text.
    In a beam session (StreamBeam(endpoint=)) the hypothesis is the beam's best for the utterance: label times are the
    frames at which the labels entered the beam, utt_score / lm_score / boost_score are the utterance's alone."""
    slot: int
    index: int
    reason: str
    start_s: float
    end_s: float
    speech_start_s: Optional[float]
    speech_end_s: Optional[float]
    hypothesis: Hypothesis
    n_best: Optional[List[Hypothesis]] = None   # beam sessions (StreamBeam(endpoint=)) with n_best > 1: the utterance's list, best first


@dataclass
class ErrorCounts:
    """Edit-distance counts of one utterance, or their sum over a set (qasr.edit.EDIT_RULES): errors = substitutions +
    deletions + insertions against ref_units reference words (characters with use_cer), hyp_units units in the hypotheses;
    rate = errors / ref_units, inf for ref_units == 0 as word_error_rate gives it."""
    errors: int
    substitutions: int
    deletions: int
    insertions: int
    ref_units: int
    hyp_units: int
    rate: float


@dataclass
class ErrorReport:
    """EncDecCTCModel.error_rate / error_rate_long: total over the best hypothesis of every utterance, oracle_errors: the sum
    over the utterances of the fewest errors of any of their n-best rows (n_best = 1: total.errors), per_utterance: the best
    hypothesis's counts, invalid: rows left out because an id or a length was out of range."""
    total: ErrorCounts
    oracle_errors: int
    per_utterance: List[ErrorCounts]
    invalid: int
    alignments: Optional[List[Optional['Alignment']]] = None   # alignments=True: one per utterance for its best row (None: not scored)
    mbr_total: Optional[ErrorCounts] = None                    # error_rate(mbr=): the counts of every utterance's MBR pick, summed
    mbr_pick: Optional[List[int]] = None                       # error_rate(mbr=): the row picked per utterance (-1: no present row)


@dataclass
class Alignment:
    """The edit path of one hypothesis against its reference (qasr.edit.TRACE_RULES): ops over 'CSDI' - correct, substitution,
    deletion, insertion - in forward order; ref_units / hyp_units: the words (characters with use_cer) of the two rows;
    ref_index / hyp_index: per op the unit it consumes of each row, None opposite an insertion / a deletion -
    Hypothesis.words[hyp_index[t]] is where an error lies in time; counts: the row's ErrorCounts."""
    ops: str
    ref_units: List[str]
    hyp_units: List[str]
    ref_index: List[Optional[int]]
    hyp_index: List[Optional[int]]
    counts: ErrorCounts


def _order_key(x):
    """float32 -> int32 that orders like the float on every bit pattern (-0 < +0); the order k_ctc takes maxima in"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def utt_score_host(frame_score_row) -> np.float32:
    """The fixed summation order of qasr_ctc_out.utt_score: part[l] = float32 sum, in increasing t, of the frames with
    t % 64 == l, then the float32 sum of part[0] .. part[63] in increasing l; both start from 0.0f."""
    x = np.ascontiguousarray(frame_score_row, dtype=np.float32)
    n = len(x)
    part = np.zeros(64, dtype=np.float32)
    for c in range(0, n, 64):                          # one vector add per 64-frame chunk = 64 independent sequential sums
        k = min(64, n - c)
        part[:k] = part[:k] + x[c:c + k]
    acc = np.float32(0.0)
    for l in range(64):
        acc = np.float32(acc + part[l])
    return acc


def collapse_host(tokens, frame_score=None, lens=None, blank=None) -> CtcResult:
    """tokens int [B, T]; frame_score float32 [B, T] or None; lens int [B] or None (None: the padded row, as the
    reference walks it); blank: the blank id (required)."""
    if blank is None:
        raise ValueError('collapse_host: blank is required (the decoder\'s last class)')
    tok = np.asarray(tokens)
    if tok.ndim != 2 or tok.shape[0] < 1 or tok.shape[1] < 1:
        raise ValueError(f'collapse_host: tokens must be [B, T] with B, T >= 1, got {tok.shape}')
    tok = tok.astype(np.int32)
    B, T = tok.shape
    fs = None if frame_score is None else np.ascontiguousarray(frame_score, dtype=np.float32)
    if fs is not None and fs.shape != tok.shape:
        raise ValueError('collapse_host: frame_score must have the shape of tokens')
    labels = np.full((B, T), blank, dtype=np.int32)
    n_labels = np.zeros(B, dtype=np.int32)
    start = np.zeros((B, T), dtype=np.int32)
    nframes = np.zeros((B, T), dtype=np.int32)
    score = None if fs is None else np.zeros((B, T), dtype=np.float32)
    utt = None if fs is None else np.zeros(B, dtype=np.float32)
    for b in range(B):
        lim = T if lens is None else int(min(max(int(lens[b]), 0), T))
        row = tok[b, :lim]
        if lim:
            change = np.flatnonzero(row[1:] != row[:-1]) + 1
            first_all = np.concatenate([[0], change])       # first frame of every run
            end_all = np.concatenate([change, [lim]])       # one past its last frame
            keep = row[first_all] != blank
            first, end = first_all[keep], end_all[keep]
            n = len(first)
            n_labels[b] = n
            labels[b, :n] = row[first]
            start[b, :n] = first
            nframes[b, :n] = end - first
            if fs is not None:
                best = np.maximum.reduceat(_order_key(fs[b, :lim]), first_all)[keep]   # per-run maximum, exact
                score[b, :n] = (best ^ ((best >> 31) & np.int32(0x7fffffff))).view(np.float32)
                utt[b] = utt_score_host(fs[b, :lim])
    return CtcResult(labels, n_labels, start, nframes, score, utt, int(blank))


def seconds_per_frame(cfg, hop_s: float) -> float:
    """Seconds one encoder output frame stands for: the featurizer's hop in seconds (hop_length / sample_rate of the
    model's preprocessor) times the product of the strides along the encoder's main path (qasr.topology.conv_plan of the
    model's ModelCfg): 0.01 s x 2 = 0.02 s for the registered models."""
    from . import topology
    stride = 1
    for sites in topology.conv_plan(cfg):
        for s in sites:
            if s.role in ('dw', 'dense'):
                stride *= int(s.stride)
    return float(hop_s) * stride


def _np(x):
    if x is None:
        return None
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def to_hypotheses(result: CtcResult, vocabulary: Sequence[str], seconds_per_frame: float) -> List[Hypothesis]:
    """Strings, times and word groups from compact labels: one Python step per emitted label (not per frame).  Times are
    start * seconds_per_frame and (start + nframes) * seconds_per_frame.  Words are the labels between ' ' labels, as
    (word, start_s, end_s, score) with the score the minimum of the word's label scores (None without scores); a
    vocabulary without ' ' gives one word per utterance."""
    labels, n_labels = _np(result.labels), _np(result.n_labels)
    start, nframes, score, utt = _np(result.start), _np(result.nframes), _np(result.score), _np(result.utt_score)
    vocab = list(vocabulary)
    spf = float(seconds_per_frame)
    hyps = []
    for b in range(labels.shape[0]):
        n = int(n_labels[b])
        ids = labels[b, :n].tolist()
        chars = [vocab[i] for i in ids]
        if start is not None and nframes is not None:
            st = (start[b, :n].astype(np.float64) * spf).tolist()
            en = ((start[b, :n] + nframes[b, :n]).astype(np.float64) * spf).tolist()
        else:
            st, en = [], []
        sc = None if score is None else score[b, :n].astype(np.float64).tolist()
        words = []
        if st:
            i = 0
            while i <= n:                                   # split on ' ' labels; empty groups (leading / double spaces) drop out
                j = i
                while j < n and chars[j] != ' ':
                    j += 1
                if j > i:
                    words.append((''.join(chars[i:j]), st[i], en[j - 1], None if sc is None else min(sc[i:j])))
                i = j + 1
        hyps.append(Hypothesis(''.join(chars), ids, st, en, sc, None if utt is None else float(utt[b]), words))
    return hyps
