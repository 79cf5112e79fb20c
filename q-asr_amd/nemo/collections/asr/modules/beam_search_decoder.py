"""CTC prefix beam search behind the reference's BeamSearchDecoderWithLM interface, without a language model.

The search is the fixed-point one of qasr.beam (csrc/qasr_beam.hip on the device): CUDA log-probabilities run k_topn +
k_beam on the current stream, CPU tensors and the `input_tensor=False` form (a list of per-utterance probability arrays)
run the NumPy twin; both give the same hypotheses and scores, bit for bit.  There is no n-gram scorer here: `lm_path` must
be None (alpha and beta are kept for the signature and unused), and vocabulary pruning by cumulative probability is not
implemented (`cutoff_prob` must be 1.0)."""
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
    probabilities, as the reference passes them on."""

    def __init__(self, vocab, beam_width, alpha, beta, lm_path, num_cpus, cutoff_prob=1.0, cutoff_top_n=40,
                 input_tensor=False):
        if lm_path is not None:
            raise ModuleNotFoundError('BeamSearchDecoderWithLM with an n-gram model (lm_path) requires ctc_decoders, which '
                                      'this build does not use: pass lm_path=None for the search without a scorer')
        if float(cutoff_prob) != 1.0:
            raise ValueError(f'BeamSearchDecoderWithLM: cutoff_prob must be 1.0 (no cumulative pruning), got {cutoff_prob}')
        if not 1 <= int(beam_width) <= qbeam.MAX_W:
            raise ValueError(f'BeamSearchDecoderWithLM: beam_width must be 1 .. {qbeam.MAX_W}, got {beam_width}')
        if not 1 <= int(cutoff_top_n) <= qbeam.MAX_N:
            raise ValueError(f'BeamSearchDecoderWithLM: cutoff_top_n must be 1 .. {qbeam.MAX_N}, got {cutoff_top_n}')
        super().__init__()
        self.scorer = None
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
                                           self.cutoff_top_n)
        lens = None if log_probs_length is None else np.asarray(log_probs_length.cpu())
        return qbeam.search_host(log_probs.float().numpy(), lens, blank, self.beam_width, n_best, self.cutoff_top_n)

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
        return [[(h.utt_score, h.text) for h in hyps] for hyps in qbeam.to_hypotheses(res, self.vocab)]
