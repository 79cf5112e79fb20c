"""Greedy CTC decoding and word error rate (nemo/collections/asr/metrics/wer.py:26-59, 62-181).
The reference delegates the Levenshtein distance to the third-party `editdistance==0.5.3` C extension
(absent here); a dynamic-programming restatement is used and pinned by the reference's own known
answers (tests/collections/asr/test_asr_metrics.py:94-111)."""
from typing import List

import torch

__all__ = ['word_error_rate', 'WER']


def _levenshtein(a, b) -> int:
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[-1]


def word_error_rate(hypotheses: List[str], references: List[str], use_cer=False, device=None) -> float:
    """device=None: the host loop below.  device='cuda' (or 'cpu'): the same number from qasr.edit.error_counts - the strings
    as id rows through the edit-distance kernel (the NumPy twin on 'cpu')."""
    if len(hypotheses) != len(references):
        raise ValueError("In word error rate calculation, hypotheses and reference lists must have the same "
                         "number of elements. But I got:{0} and {1} correspondingly".format(len(hypotheses),
                                                                                          len(references)))
    if device is not None:
        from qasr.edit import error_counts
        return error_counts(hypotheses, references, use_cer=use_cer, device=device).rate
    scores = words = 0
    for h, r in zip(hypotheses, references):
        h_list, r_list = (list(h), list(r)) if use_cer else (h.split(), r.split())
        words += len(r_list)
        scores += _levenshtein(h_list, r_list)
    return 1.0 * scores / words if words != 0 else float('inf')


class WER:
    """Accumulating WER metric with the reference's decode helpers (no pytorch-lightning dependency)."""

    def __init__(self, vocabulary, batch_dim_index=0, use_cer=False, ctc_decode=True, log_prediction=True,
                 dist_sync_on_step=False, device=False):
        """device=True: update() scores label ids instead of strings - on CUDA tensors the padded prediction rows go through
        qasr_ctc_collapse and qasr_edit_distance into a totals block on the device that compute() reads once; on CPU tensors
        through their NumPy twins.  The numbers are those of device=False (qasr.edit.EDIT_RULES)."""
        self.batch_dim_index = batch_dim_index
        self.blank_id = len(vocabulary)
        self.labels_map = dict(enumerate(vocabulary))
        self.use_cer, self.ctc_decode, self.log_prediction = use_cer, ctc_decode, log_prediction
        self.scores = torch.tensor(0)
        self.words = torch.tensor(0)
        self.device = bool(device)
        self._totals = None                     # device=True: int64 [16], a cuda tensor or a NumPy array (qasr.edit)
        self._space = self._space_dev = None
        if self.device and not use_cer:
            from qasr.edit import space_mask
            self._space = space_mask(list(vocabulary), 'WER(device=True)')

    def ctc_decoder_predictions_tensor(self, predictions: torch.Tensor) -> List[str]:
        """Collapse repeats, drop blanks; walks the full padded row like the reference (it ignores lengths)."""
        rows = predictions.long().cpu()
        if self.batch_dim_index != 0:
            rows = rows.transpose(0, self.batch_dim_index)
        hyps = []
        for row in rows.tolist():
            out, prev = [], self.blank_id
            for p in row:
                if (p != prev or prev == self.blank_id) and p != self.blank_id:
                    out.append(p)
                prev = p
            hyps.append(''.join(self.labels_map[c] for c in out))
        return hyps

    def _update_device(self, predictions, targets, target_lengths):
        """the label rows scored where they lie: collapse of the padded prediction rows (no lengths, as
        ctc_decoder_predictions_tensor walks them), then the edit distance against targets[:, :target_lengths]"""
        import numpy as np
        from qasr import edit
        if not self.ctc_decode:
            raise NotImplementedError("Not supported. Use BeamSearch in the meantime")
        rows = predictions if self.batch_dim_index == 0 else predictions.transpose(0, self.batch_dim_index)
        mode = 'char' if self.use_cer else 'word'
        if rows.is_cuda:
            from qasr import engine
            dev = rows.device
            if self._totals is None or not torch.is_tensor(self._totals):
                held = None if self._totals is None else torch.from_numpy(self._totals).to(dev)
                self._totals = torch.zeros(edit.TOTAL_WORDS, device=dev, dtype=torch.int64) if held is None else held
            res = engine.ctc_collapse(rows, lens=None, blank=self.blank_id)
            if self._space is not None and (self._space_dev is None or self._space_dev.device != dev):
                self._space_dev = torch.from_numpy(self._space).to(dev)      # uploaded once per device
            sp = self._space_dev
            tg = targets.to(dev)
            if tg.shape[1] == 0:
                tg = torch.zeros(tg.shape[0], 1, device=dev, dtype=torch.int32)
            tl = None if target_lengths is None else target_lengths.to(dev)      # None: the padded target rows
            engine.edit_distance(res.labels, res.n_labels, tg, tl, self.blank_id, mode=mode, is_space=sp, totals=self._totals)
            return
        from qasr.ctc import collapse_host
        if self._totals is None:
            self._totals = np.zeros(edit.TOTAL_WORDS, dtype=np.int64)
        elif torch.is_tensor(self._totals):
            self._totals = self._totals.cpu().numpy()
        res = collapse_host(rows.cpu().numpy().astype(np.int32), lens=None, blank=self.blank_id)
        tg = targets.cpu().numpy()
        if tg.shape[1] == 0:
            tg = np.zeros((tg.shape[0], 1), dtype=np.int32)
        tl = None if target_lengths is None else target_lengths.cpu().numpy()
        self._totals = edit.edit_host(res.labels, res.n_labels, tg, tl, self.blank_id, mode=mode, is_space=self._space,
                                      totals=self._totals).totals

    def _read_totals(self):
        import numpy as np
        from qasr import edit
        if self._totals is None:
            return np.zeros(edit.TOTAL_WORDS, dtype=np.int64)
        t = self._totals.cpu().numpy() if torch.is_tensor(self._totals) else self._totals
        if int(t[edit.T_INVALID]):
            raise ValueError(f'WER(device=True): {int(t[edit.T_INVALID])} rows held an id outside the vocabulary or a length '
                             f'outside the row')
        return t

    def counts(self):
        """The ErrorCounts (qasr.ctc) of everything update() has seen: with device=True the substitution / deletion / insertion
        split from the totals block; otherwise errors and reference units only, the split as 0."""
        from qasr import edit
        if self.device:
            return edit.totals_counts(self._read_totals())
        return edit.counts_of(int(self.scores), 0, 0, 0, int(self.words), 0)

    def update(self, predictions, targets, target_lengths):
        if self.device:
            return self._update_device(predictions, targets, target_lengths)
        refs = []
        t = targets.long().cpu()
        n = target_lengths.long().cpu()
        for i in range(t.shape[0]):
            refs.append(''.join(self.labels_map[c] for c in t[i][:int(n[i])].tolist()))
        if not self.ctc_decode:
            raise NotImplementedError("Not supported. Use BeamSearch in the meantime")
        hyps = self.ctc_decoder_predictions_tensor(predictions)
        scores = words = 0
        for h, r in zip(hyps, refs):
            h_l, r_l = (list(h), list(r)) if self.use_cer else (h.split(), r.split())
            words += len(r_l)
            scores += _levenshtein(h_l, r_l)
        self.scores = self.scores + scores
        self.words = self.words + words

    def compute(self):
        if self.device:
            from qasr import edit
            t = self._read_totals()
            self.scores, self.words = torch.tensor(int(t[edit.T_ERRORS])), torch.tensor(int(t[edit.T_REF]))
        s, w = self.scores.detach().float(), self.words.detach().float()
        return s / w, s, w

    def reset(self):
        self.scores, self.words = torch.tensor(0), torch.tensor(0)
        self._totals = None
