"""CTC prefix beam search behind the reference's BeamSearchDecoderWithLM interface, with or without an n-gram model.

The search is the fixed-point one of qasr.beam (csrc/qasr_beam.hip on the device): CUDA log-probabilities run k_topn +
k_beam (k_beam_lm with a model) on the current stream, CPU tensors and the `input_tensor=False` form (a list of
per-utterance probability arrays) run the NumPy twin; both give the same hypotheses and scores, bit for bit.

`lm_path`: an ARPA text file (gzip too), read by qasr.ngram - neither ctc_decoders nor kenlm is used.  Of ctc_decoders'
Scorer this follows: the mode from the vocabulary (word-based if it has a space, else character-based), a word scored
when a space ends it, every extension adding alpha * ln p + beta (words that the model lacks: -1000, then an empty
history), the history starting at <s>, </s> never scored, and in word mode the unfinished last word scored after the
last frame with the beam re-ordered.  Not followed: the arithmetic (fixed point, qasr.beam.LM_RULES, so that device and
host agree on every bit), KenLM binary files (export ARPA), the dictionary FST that restricts prefixes to spellable
words, vocabulary pruning by cumulative probability (`cutoff_prob` must be 1.0), orders above 6.  The reference's
(score, string) tuples have no place for times: EncDecCTCModel.decode(beam_width=, timestamps=True) gives them.  The reported score is
the search score including the model's share, where ctc_decoders subtracts it again."""
import numpy as np
import torch
from torch import nn

from qasr import beam as qbeam


class BeamSearchDecoderWithLM(nn.Module):
    """forward(log_probs, log_probs_length) -> one list per utterance, best first and at most beam_width long, of
    (log-probability of the hypothesis, string).

    vocab: the model's labels (the CTC blank is the class after the last one); beam_width: 1 .. 128; cutoff_top_n:
    1 .. 64 classes considered per frame; num_cpus is accepted and unused (the device needs none, the twin is one loop);
    input_tensor: True for a tensor [B, T, D] of log-probabilities with lengths, False for a list of [T_i, D] arrays of
    probabilities, as the reference passes them on.  boost (keyword-only, an extension): a list of phrases (text or
    (text, weight); boost_weight nats per label where a phrase has none) or a qasr.boost.PhraseSet: phrase boosting by
    qasr.boost.BOOST_RULES (k_beam_boost on the device), with or without lm_path.  mbr (keyword-only, an extension): 'word' |
    'char' returns every list in minimum Bayes risk order (qasr.mbr.MBR_RULES; qasr_ctc_mbr behind the beam on the device,
    the twin otherwise) - the row with the fewest expected word (character) errors against the rest of its list first, the rows
    weighted by exp(mbr_scale * score), mbr_scale 0 .. 16; the tuples stay (log-probability, string).  Needs beam_width >= 2."""

    def __init__(self, vocab, beam_width, alpha, beta, lm_path, num_cpus, cutoff_prob=1.0, cutoff_top_n=40,
                 input_tensor=False, *, boost=None, boost_weight=1.0, mbr=None, mbr_scale=1.0):
        if float(cutoff_prob) != 1.0:
            raise ValueError(f'BeamSearchDecoderWithLM: cutoff_prob must be 1.0 (no cumulative pruning), got {cutoff_prob}')
        if not 1 <= int(beam_width) <= qbeam.MAX_W:
            raise ValueError(f'BeamSearchDecoderWithLM: beam_width must be 1 .. {qbeam.MAX_W}, got {beam_width}')
        if not 1 <= int(cutoff_top_n) <= qbeam.MAX_N:
            raise ValueError(f'BeamSearchDecoderWithLM: cutoff_top_n must be 1 .. {qbeam.MAX_N}, got {cutoff_top_n}')
        scorer = None
        if lm_path is not None:                     # (a KenLM binary file raises ModuleNotFoundError: export ARPA)
            from qasr import ngram
            try:
                ngram.fixed_weights(alpha, beta)
            except ValueError as e:
                raise ValueError(f'BeamSearchDecoderWithLM: {e}') from None
            scorer = lm_path if isinstance(lm_path, ngram.NgramLM) else ngram.NgramLM.from_arpa(lm_path, list(vocab))
            if scorer.n_labels != len(list(vocab)):
                raise ValueError(f'BeamSearchDecoderWithLM: the model was loaded for {scorer.n_labels} labels, vocab has {len(list(vocab))}')
        phrases = None
        if boost is not None:                       # (keyword-only: the positional signature is the reference's)
            from qasr import boost as qboost
            try:
                phrases = qboost.as_phrase_set(boost, list(vocab), boost_weight)
            except ValueError as e:
                raise ValueError(f'BeamSearchDecoderWithLM: {e}') from None
        mask = None
        if mbr is not None:                         # (keyword-only, likewise)
            from qasr import edit as qedit, mbr as qmbr
            if mbr not in ('word', 'char'):
                raise ValueError(f"BeamSearchDecoderWithLM: mbr must be None, 'word' or 'char', got {mbr!r}")
            if int(beam_width) < 2:
                raise ValueError('BeamSearchDecoderWithLM: mbr needs beam_width >= 2 (a list of one row has nothing to re-rank)')
            qmbr.check_scale(mbr_scale, 'BeamSearchDecoderWithLM')
            mask = qedit.space_mask(list(vocab), 'BeamSearchDecoderWithLM') if mbr == 'word' else None
        super().__init__()
        self.mbr, self.mbr_scale, self.mbr_mask = mbr, float(mbr_scale), mask
        self.scorer = scorer
        self.phrases = phrases
        self.vocab = list(vocab)
        self.beam_width = int(beam_width)
        self.alpha, self.beta = alpha, beta
        self.num_cpus = num_cpus
        self.cutoff_prob = float(cutoff_prob)
        self.cutoff_top_n = int(cutoff_top_n)
        self.input_tensor = bool(input_tensor)

    def search(self, log_probs, log_probs_length=None, n_best=None):
        """the qasr.beam.BeamResult of a [B, T, D] tensor of log-probabilities (cuda: the kernels, cpu: the twin)"""
        blank = len(self.vocab)
        if log_probs.shape[-1] != blank + 1:
            raise ValueError(f'BeamSearchDecoderWithLM: {log_probs.shape[-1]} classes for a vocabulary of {blank} labels + blank')
        if log_probs.is_cuda:
            from qasr import engine as qengine
            return qengine.ctc_beam_search(log_probs.float(), log_probs_length, blank, self.beam_width, n_best,
                                           self.cutoff_top_n, lm=self.scorer, alpha=self.alpha, beta=self.beta,
                                           boost=self.phrases)
        lens = None if log_probs_length is None else np.asarray(log_probs_length.cpu())
        return qbeam.search_host(log_probs.float().numpy(), lens, blank, self.beam_width, n_best, self.cutoff_top_n,
                                 self.scorer, self.alpha, self.beta, self.phrases)

    @torch.no_grad()
    def forward(self, log_probs, log_probs_length=None):
        if self.input_tensor:
            res = self.search(log_probs, log_probs_length)
        else:
            rows = [np.asarray(p.detach().cpu() if torch.is_tensor(p) else p, dtype=np.float32) for p in log_probs]
            T = max([r.shape[0] for r in rows] + [1])
            with np.errstate(divide='ignore'):
                lp = np.full((len(rows), T, len(self.vocab) + 1), -np.inf, dtype=np.float32)
                for i, r in enumerate(rows):
                    lp[i, :r.shape[0]] = np.log(r)              # a probability of 0 becomes the fixed-point floor
            res = self.search(torch.from_numpy(lp), torch.tensor([r.shape[0] for r in rows], dtype=torch.int64))
        lists = qbeam.to_hypotheses(res, self.vocab)
        if self.mbr is not None:
            lists = [[row[k] for k in order if 0 <= k < len(row)] for row, order in zip(lists, self._mbr_order(res))]
        return [[(h.utt_score, h.text) for h in hyps] for hyps in lists]

    def _mbr_order(self, res):
        """order [B][n_best] of MBR_RULES over a BeamResult where it lies (cuda: qasr_ctc_mbr, cpu: the twin)"""
        from qasr import mbr as qmbr
        if torch.is_tensor(res.labels) and res.labels.is_cuda:
            sp = None if self.mbr_mask is None else torch.from_numpy(self.mbr_mask).to(res.labels.device)
            return qmbr.mbr_device(res.labels, res.n_labels, res.score, res.n_hyps, len(self.vocab), mode=self.mbr, is_space=sp,
                                   scale=self.mbr_scale).order.cpu().tolist()
        return qmbr.mbr_host(res.labels, res.n_labels, res.score, res.n_hyps, len(self.vocab), mode=self.mbr, is_space=self.mbr_mask,
                             scale=self.mbr_scale).order.tolist()
