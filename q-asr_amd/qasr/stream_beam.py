"""Streaming CTC prefix beam search: a per-stream beam that a step loads, advances over the frames that became final and
stores back, with a fixed-lag commit that prunes.  The host statement of k_stream_beam (csrc/qasr_stream_beam.hip,
include/qasr.h) and the CPU path of EncDecCTCModel.stream(beam=).  NumPy only: no GPU, no native library.

The search itself is qasr.beam's (`_search_one` without a model, `_search_one_lm` under LM_RULES with one); what is new is
where the beam lives between two steps and the rule for when text becomes final (STREAM_BEAM_RULES)."""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import stream as qs
from .beam import FRAC, MAX_N, MAX_W, NEG, _hmix, lae, lae_table

K_ROUND = 32                            # a commit round runs after every global frame t with (t + 1) % K_ROUND == 0
HDR_WORDS = 16
_H_NB, _H_COMMIT, _H_DONE, _H_STARTED = 0, 1, 2, 3
STATUS_OK, STATUS_GAP, STATUS_SLOT, STATUS_SYNC, STATUS_NODES, STATUS_SET = 0, 1, 2, 3, 4, 5
_H_SET = 4                              # boosted blocks: the slot's phrase set + 1 (0: not boosted)
_H_CUTS = 5                             # sessions with cuts (STREAM_BEAM_EP_RULES): the cuts done so far
MAX_SETS = 8                            # phrase sets of one session (the kernel takes them as arguments)
NODE_LIMIT = (1 << 31) - 1

STREAM_BEAM_RULES = """Frames.  A step makes the frames [lo, hi) of qasr.stream's rule final (STREAM_RULES: lo = the stream block's
frames_done, hi from the window's encoded length, `received` and END); they are GLOBAL frames t, and the candidates of
frame t are row t - first_frame of the window's top-N (k_topn / topn_host over the window's log-probabilities).

State of a slot: 16 + 20 W 32-bit words, then a ring of F rows x W entries of (parent node, label), two words each.
Word 0: nb, the live entries; 1: commit_len; 2: frames_done; 3: 1 once the slot has been stepped (a zeroed block is a fresh
stream: the single empty entry); 4-15: zero.  Then, W entries each, 64-bit: pb, pnb, score, prefix hash, parent hash, own
(the term of the entry's creation), lm_tot, word hash; 32-bit: length (labels since the stream began), last label, node,
context node.  Entries at and behind nb are zero.  Without a model own, lm_tot, word hash and context stay zero.

Per frame: the step of qasr.beam._search_one (_search_one_lm with a model) on every byte - lae, tie order, hashes, dead
candidates.  The one difference: a new prefix that lands in rank r at global frame t is node t * W + r (int32), stored in
row t mod F of the ring, entry r.  A step whose hi * W would pass 2^31 - 1 reports status 4.

Commit round.  After frame t with (t + 1) % K == 0 (K = K_ROUND), with h = t - Lg (Lg: the lag in frames); nothing happens
while h < 0 or when the beam is dead.  old(e) of an entry e is the sequence of its labels whose node was created at a
frame <= h; creation frames rise strictly along a chain (a prefix is created from an entry that was in the beam before that
frame), so old(e) is a prefix of e.  The committed text becomes old(entry 0), the best entry's; an entry survives iff
old(e) == old(entry 0) as LABEL sequences (a prefix that left the beam and came back owns a second node, so node ids are not
compared); survivors keep their order.  commit_len = len(old(0)).  commit_len never shrinks and committed labels never
change: entry 0 survived every earlier round, so its old() extends what was committed.  Chain walks stop at depth commit_len.

END.  After the last final frame, word-mode models add the unfinished-word term and re-order (LM_RULES).  No horizon: the
step's delta also carries everything of the best entry behind commit_len, and the first n_best entries are written as their
suffixes behind commit_len with score, lm_score, n_labels (of the suffix) and n_hyps; all of them start with the committed
text, which the host prepends.  The stored state is the beam after the step's frames (before the END re-ordering).

Per step out: the delta (labels and, per label, the creation frame of its node: a free emission time, NOT an alignment),
n_new_labels, commit_len (the delta included), the live entry count, status; the provisional tail = the best entry's
uncommitted labels, the first Ptail of them, with their true count (END rows: none).

Flags and status.  BEGIN resets the slot to the single empty entry first.  A beam that died (no live candidate) stays
dead: frames_done still advances, END gives n_hyps = 0, as offline.  Status 1: the stream rule's gap (lo < first_frame); 2: a
slot out of range; 3: the beam block's frames_done (0 on BEGIN) differs from the stream block's; 4: the node-id limit.  A
row with a non-zero status leaves its state alone (a BEGIN included) and writes the outputs of an empty step.

Consequences, the contract: `lagged_search_host`, the whole-stream statement, equals the concatenation of any sequence of
steps on every byte; with Lg >= the stream's length no round fires and the result is beam_search_host's on every byte."""


STREAM_BOOST_RULES = """Streaming phrase boosting: STREAM_BEAM_RULES with the search clause of qasr.boost.BOOST_RULES inside the frame
step (k_stream_beam_boost<LM> of csrc/qasr_stream_beam_boost.hip).  A session has G sets, 1 <= G <= 8 (MAX_SETS), each a
qasr.boost.PhraseSet of the same vocabulary; a slot uses one of them or none.

State of a slot: 16 + 24 W words, then the ring as in STREAM_BEAM_RULES.  The 64-bit arrays are the eight of
STREAM_BEAM_RULES, then boost_tot; the 32-bit arrays are its four, then bst (the automaton state), then one array of zeros
(the pad that keeps the 64-bit arrays of every slot 8-byte aligned for odd W).  Header word 4: the slot's set + 1, 0: not
boosted; words 5-15: zero.

Which set.  A BEGIN row stores boost_set[row] + 1 (boost_set -1: none) in header word 4; later rows of the stream read the
word and ignore the input.  A word outside 0 .. G reads as 0.  0 means no boosting: bst stays 0, every term is 0, boost_tot
stays 0.  A BEGIN row whose boost_set is outside -1 .. G - 1 gets status 5 (checked after the statuses 1 - 4) and, as every
status, leaves its state alone.

Start.  A fresh entry (BEGIN, or a zeroed block) starts in the start state of the slot's set: delta(root, space) with whole
words on, else the root; boost_tot 0.

Extending an entry (state s) by a label c != blank moves to s' = delta(s, c) with the term pot[s'] - pot[s] + bank[s'], added
where qasr.beam._search_one_boost adds it: to the score of the new prefix, into `own` (next to the model's term) and into
boost_tot, not into lm_tot.  Blank steps and the A path add nothing.

Commit round: unchanged.  It compares label sequences only; bst and boost_tot travel with the surviving entries.  The
provisional pot of a match that has begun inside a committed stretch is NOT settled at the commit: it stays in the entry's
score and boost_tot and is settled where BOOST_RULES settles it, at END.

END is BOOST_RULES' pass, written to the outputs only (the stored state stays the beam before it): for every live entry
of a boosted slot the virtual space step (whole words), then - pot[state], both into score and boost_tot; with a word-mode
model the unfinished-word term in the same pass; then ONE re-ordering by score, ties by previous rank.  END rows also
write end_boost_score (boost_tot of each reported entry).

Consequences, the contract: (1) any slicing of a stream into steps equals `lagged_search_host(..., boost=)` on every byte;
(2) with Lg >= the stream's length the END result equals beam_search_host(..., boost=) on every byte - labels, score, lm_tot,
boost_tot; (3) with set 0, or with every weight 0, every byte that this layout shares with STREAM_BEAM_RULES' is equal to
it; (4) for every final hypothesis boost_tot is exactly the brute-force sum of g over the phrase occurrences in its WHOLE
text (committed text plus remainder), however much of it was committed early."""


STREAM_BEAM_EP_RULES = """Streaming beam endpointing: STREAM_BEAM_RULES (STREAM_BOOST_RULES on a boosted plan) for a stream that qasr.stream_ep
cuts into utterances - at every cut the beam is finalised as at END and reset (k_stream_beam_ep<LM, BOOST> of
csrc/qasr_stream_beam_ep.hip).  The slot's block is the plan's: 16 + 20 W words, boosted 16 + 24 W, then the ring.

Order in a step.  window -> forward with log-probabilities -> top-N -> emit (STREAM_RULES) -> endpoint (EP_RULES) -> this
step, which therefore runs AFTER emit and endpoint of the same rows.  lo = the beam block's own frames_done (0 on BEGIN);
hi = the stream block's frames_done as emit left it; the step reads the row's records / n_records / status of the endpoint
step and nothing else of it: no tokens, no frame scores.  Cuts are decided by the greedy arg-max, not by the beam.

Frame loop.  For t = lo .. hi - 1, in this order: (a) the frame step of the rules, skipped while the beam is dead (the
walk goes on: it has to reach the cuts); (b) the commit round if (t + 1) % K == 0, unchanged (nothing while h < 0 or the
beam is dead); (c) while the next unread record has end == t + 1: a CUT.  Behind the loop every unread record is a cut too
(they have end == hi: the END record of a row without frames, a BEGIN|END row).  Records with the same end give one cut
each, the later ones on a fresh beam.

Cut k of the step (k counts the step's records from 0).  First the END pass of the rules, on the outputs only: the
unfinished-word term (word mode), the boost END pass (a boosted slot), ONE re-ordering by score, ties by previous rank.
cut_n_hyps[k] = min(live entries, n_best); for each of these entries its suffix behind commit_len, the suffix' length,
score, lm_score (with a model) and boost_score (boosted plan).  Then the best entry's uncommitted labels and their creation
frames are appended to the step's delta, and cut_delta_end[k] = the delta's length after that: the delta between two
cut_delta_end values is one utterance's remainder, and everything the step committed before it belongs to the same
utterance.  Then the beam is RESET to the single fresh entry: commit_len 0, length 0, hashes 0, last -1, node -1, the LM
context at the model's start, the boost state at the start state of the slot's set (header word 4 survives the cut),
boost_tot 0.  A beam that had died is alive again; one that is dead because the model blob is invalid (the kernel's check)
stays dead.  A cut of a dead beam has cut_n_hyps 0 and adds nothing to the delta.

Nodes stay t * W + r in ring row t % F; frames and the phase of the rounds stay GLOBAL - a cut moves neither - so the
bytes do not depend on how the stream is sliced into steps.  A fresh entry has node -1 and length 0, and chain walks stop at
depth length - commit_len: no walk of a later utterance reaches a node of an earlier one.

Header word 5 counts the cuts done (0 on BEGIN).  Per step out: STREAM_BEAM_RULES' delta, n_new_labels, n_live, status; commit_len
and the tail are those of the beam the step leaves behind (behind a cut at hi: 0 and none); n_cuts and the cut outputs.
There are no END rows: the END record is a cut like any other.

Status.  1, 2, 4, 5 as in the rules (1: lo < first_frame or first_frame < 0; 5 on boosted plans).  3, checked after 2 and 1
and before 4: lo > hi; lo < hi with hi > first_frame + e (e: the row's encoded length clamped to 0 .. Tw); n_records
outside 0 .. E; a record whose end is below the one before it (ends may repeat), outside lo .. hi, or equal to lo while
lo < hi; a first record whose index differs from header word 5 (0 on BEGIN); a non-zero endpoint status of the row.  Every
status leaves the state alone and writes an empty step.

Consequences, the contract: (1) any slicing of a stream into steps equals `lagged_search_ep_host`, the whole-stream
statement, on every byte - delta, cut outputs, state block and ring; (2) with Lg at or beyond the longest utterance every
cut's rows equal beam_search_host over the utterance's own candidates cand[first:end] - labels, score, lm_tot, boost_tot;
(3) a stream without a record equals step_batch_host on every byte the two share; (4) boost_tot of every cut hypothesis is
the brute-force sum over the phrase occurrences in that utterance's text alone."""


@dataclass
class StreamBeam:
    """What EncDecCTCModel.stream(beam=) takes.  width, n_best, cutoff_top_n, lm, alpha, beta: as decode(beam_width=, ...).
    lag_s: the commit lag in seconds (rounded to frames); the default of 4.0 s is untried on speech.  boost: phrase
    boosting across steps (STREAM_BOOST_RULES) - a list of phrases as decode(boost=) takes it, a qasr.boost.PhraseSet, or a
    dict of at most MAX_SETS named sets of which sess.open(boost=name) picks one; boost_weight: the default weight of
    phrases given without one.  endpoint: a qasr.stream_ep.Endpointing - the stream is cut into utterances and the beam is
    finalised and reset at every cut (STREAM_BEAM_EP_RULES); sess.take_utterances() then delivers per-utterance n-best.
    `endpoint` is the last constructor argument (positional or keyword) and an attribute, but NOT a dataclass field - the
    field list stays boost, boost_weight at its end.  repr() and == include it.  dataclasses.replace() rebuilds from the
    fields alone: replace(beam, lag_s=...) DROPS the endpointing and gives a session that never cuts - pass it along,
    replace(beam, lag_s=..., endpoint=beam.endpoint)."""
    width: int = 16
    n_best: int = 1
    cutoff_top_n: int = 40
    lm: object = None
    alpha: float = 0.0
    beta: float = 0.0
    lag_s: float = 4.0
    boost: object = None
    boost_weight: float = 1.0


def _stream_beam_init(fields_init, n_fields):
    """StreamBeam.__init__ with `endpoint` behind the dataclass fields, as the last positional or a keyword argument.  It is an
    attribute and not a dataclass field: the list of fields is pinned to end in boost, boost_weight, so repr and == do not see
    it, and dataclasses.replace keeps it only when it is passed (replace(beam, ..., endpoint=beam.endpoint))."""
    def __init__(self, *args, endpoint=None, **kw):
        if len(args) > n_fields + 1:
            raise TypeError(f'StreamBeam takes at most {n_fields + 1} positional arguments, got {len(args)}')
        if len(args) == n_fields + 1:
            if endpoint is not None:
                raise TypeError("StreamBeam got multiple values for argument 'endpoint'")
            args, endpoint = args[:n_fields], args[n_fields]
        fields_init(self, *args, **kw)
        self.endpoint = endpoint
    return __init__


def _stream_beam_repr(fields_repr):
    def __repr__(self):
        return fields_repr(self)[:-1] + f', endpoint={self.endpoint!r})'
    return __repr__


def _stream_beam_eq(fields_eq):
    def __eq__(self, other):
        r = fields_eq(self, other)
        return r if r is NotImplemented or not r else self.endpoint == other.endpoint
    return __eq__


StreamBeam.__init__ = _stream_beam_init(StreamBeam.__init__, len(StreamBeam.__dataclass_fields__))
StreamBeam.__repr__ = _stream_beam_repr(StreamBeam.__repr__)
StreamBeam.__eq__ = _stream_beam_eq(StreamBeam.__eq__)


class StreamBeamPlan:
    """W, N, n_best, the lag Lg and the round period K in frames, and the sizes that follow from STREAM_BEAM_RULES.

    Ring.  A round at frame t commits every label of the survivors created at a frame <= h = t - Lg, so afterwards every
    live node - every node a chain walk down to commit_len can reach - was created in (t - Lg, t].  The next round runs
    at t + K; until it has run, live nodes were created in (t - Lg, t + K]: Lg + K frames.  Before the first round (the
    first t >= Lg with (t + 1) % K == 0, so t < Lg + K) they were created in [0, t]: at most Lg + K frames again.  Frame
    t + K lands in the row of frame t - Lg, which died at the round before: F = Lg + K rows suffice, and no smaller ring
    does when every frame creates a node.
    Labels.  Creation frames rise strictly along a chain, so an entry has at most one uncommitted label per live frame:
    at most F.  A round commits labels created in (h - K, h] (the first round: in [0, h], h < K): at most K.
    Pitches.  end_pitch = tail_pitch = F (a suffix behind commit_len).  Every label a step commits was uncommitted before
    the step (<= F) or created in it (<= its final frames, one per frame along one chain): delta_pitch = F +
    max_final_frames, END steps included.
    Cuts (STREAM_BEAM_EP_RULES).  A cut at frame c resets the beam to an entry of length 0 and node -1: every chain of the
    utterance that follows holds nodes created at frames >= c only, every chain of the one before it nodes created below c.
    Chains of different utterances cover disjoint frames.  Ring: live nodes are still created in (t - Lg, t + K] of the
    last round t (a cut only kills nodes), so F = Lg + K rows suffice.  Labels: an entry still has at most one uncommitted
    label per live frame, so Pend = F holds for every cut.  Delta: a step's delta is, utterance by utterance, what rounds
    committed and what cuts appended; each of those labels was uncommitted before the step (only in the first utterance
    the step touches: <= F) or was created at a frame of the step, at most one per frame along one chain, and the chains
    of the step's utterances cover disjoint frames: delta_pitch = F + max_final_frames still holds.
    `walk_ep` steps through a protocol of frames with cuts and asserts all of it on the twin.
    boost: the slots carry bst and boost_tot (STREAM_BOOST_RULES' layout)."""

    def __init__(self, width=16, n_best=1, cutoff_top_n=40, lag_frames=200, max_final_frames=1, K=K_ROUND, boost=False):
        W, N, nb, Lg, K = int(width), int(cutoff_top_n), int(n_best), int(lag_frames), int(K)
        if not 1 <= W <= MAX_W:
            raise ValueError(f'StreamBeamPlan: width must be 1 .. {MAX_W}, got {W}')
        if not 1 <= N <= MAX_N:
            raise ValueError(f'StreamBeamPlan: cutoff_top_n must be 1 .. {MAX_N}, got {N}')
        if not 1 <= nb <= W:
            raise ValueError(f'StreamBeamPlan: n_best must be 1 .. width, got {nb}')
        if Lg < 0 or K < 1 or Lg + K > MAX_RING:
            raise ValueError(f'StreamBeamPlan: lag {Lg} frames must lie in 0 .. {MAX_RING} - K, K {K} >= 1')
        if int(max_final_frames) < 1:
            raise ValueError(f'StreamBeamPlan: max_final_frames {max_final_frames} < 1')
        self.W, self.N, self.n_best, self.Lg, self.K = W, N, nb, Lg, K
        self.F = Lg + K
        self.max_final_frames = int(max_final_frames)
        self.end_pitch = self.tail_pitch = self.F
        self.delta_pitch = self.F + self.max_final_frames
        self.boost = bool(boost)
        self.ent_words = (24 if self.boost else 20) * W
        self.slot_words = slot_words(W, self.F, self.boost)

    @classmethod
    def for_stream(cls, plan: qs.StreamPlan, beam: StreamBeam, K=K_ROUND):
        lag = float(beam.lag_s)
        if not np.isfinite(lag) or lag < 0:
            raise ValueError(f'StreamBeam: lag_s {beam.lag_s} must be finite and not negative')
        return cls(beam.width, beam.n_best, beam.cutoff_top_n, int(round(lag / plan.seconds_per_frame())),
                   max(plan.max_final_frames, 1), K, getattr(beam, 'boost', None) is not None)


MAX_RING = 1 << 20                      # rows of a ring (F); the C ABI refuses more


def slot_words(W, F, boost=False):
    return HDR_WORDS + (24 if boost else 20) * int(W) + 2 * int(F) * int(W)


def state_bytes(S, W, F, boost=False):
    """qasr_stream_beam_state_bytes(S, W, F); boost: qasr_stream_beam_boost_state_bytes(S, W, F)"""
    return 4 * int(S) * slot_words(W, F, boost)


def as_sets(boost):
    """boost= of the twins: None, one qasr.boost.PhraseSet, or a sequence of 1 .. MAX_SETS of them -> a list (None: none)"""
    if boost is None:
        return None
    sets = list(boost) if isinstance(boost, (list, tuple)) else [boost]
    if not 1 <= len(sets) <= MAX_SETS:
        raise ValueError(f'stream_beam: boost must be 1 .. {MAX_SETS} phrase sets, got {len(sets)}')
    return sets


class _Entries:
    """the live entries of one slot as arrays of nb elements"""
    names64 = ('pb', 'pnb', 'sc', 'hsh', 'phs', 'own', 'lmt', 'wh')
    names32 = ('ln', 'last', 'node', 'ctx')
    unsigned = ('hsh', 'phs', 'wh')

    @classmethod
    def fresh(cls, lm, boosted=False, bs=None):
        e = cls()
        if boosted:
            e.bst, e.btot = np.array([bs.start if bs is not None else 0], np.int32), np.zeros(1, np.int64)
        i64 = np.int64
        e.pb, e.pnb, e.sc = np.array([0], i64), np.array([NEG], i64), np.array([0], i64)
        e.hsh, e.phs, e.wh = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        e.own, e.lmt = np.zeros(1, i64), np.zeros(1, i64)
        e.ln, e.last, e.node = np.zeros(1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
        e.ctx = np.array([lm.start if lm is not None else 0], np.int32)
        return e

    def __len__(self):
        return len(self.sc)

    def take(self, idx):
        o = _Entries()
        for n in self.names64 + self.names32 + (('btot', 'bst') if hasattr(self, 'bst') else ()):
            setattr(o, n, getattr(self, n)[idx])
        return o


class StreamBeamState:
    """S slots as the device holds them: block int32 [S][slot_words].  row_frame, h_dead and trail are the twin's own
    bookkeeping for its assertions (which frame a ring row holds, the last round's horizon, every node ever made with the
    committed labels) and are no part of the state."""

    def __init__(self, S, plan: StreamBeamPlan, check=True):
        self.S, self.plan, self.check = int(S), plan, bool(check)
        self.block = np.zeros((self.S, plan.slot_words), dtype=np.int32)
        self.row_frame = np.full((self.S, plan.F), -1, dtype=np.int64)
        self.h_dead = np.full(self.S, -1, dtype=np.int64)
        self.trail = [dict(nodes={}, committed=[]) for _ in range(self.S)]

    def ring(self, slot):
        W, F = self.plan.W, self.plan.F
        return self.block[slot, HDR_WORDS + self.plan.ent_words:].reshape(F, W, 2)

    def header(self, slot):
        b = self.block[slot]
        return int(b[_H_NB]), int(b[_H_COMMIT]), int(b[_H_DONE]), int(b[_H_STARTED])

    def _arrays(self, slot):
        W = self.plan.W
        b = self.block[slot]
        n64, n32 = (9, 6) if self.plan.boost else (8, 4)
        a64 = b[HDR_WORDS:HDR_WORDS + 2 * n64 * W].view(np.int64).reshape(n64, W)
        a32 = b[HDR_WORDS + 2 * n64 * W:HDR_WORDS + (2 * n64 + n32) * W].reshape(n32, W)
        return a64, a32

    def boost_set(self, slot, n_sets):
        """header word 4 of a boosted block: the slot's set + 1; a word outside 0 .. n_sets reads as 0"""
        g = int(self.block[slot, _H_SET]) if self.plan.boost else 0
        return g if 0 <= g <= int(n_sets) else 0

    def load(self, slot, lm, bs=None):
        nb, commit, done, started = self.header(slot)
        if not started:
            return _Entries.fresh(lm, self.plan.boost, bs), 0, 0
        a64, a32 = self._arrays(slot)
        e = _Entries()
        for k, n in enumerate(_Entries.names64):
            v = a64[k, :nb].copy()
            setattr(e, n, v.view(np.uint64) if n in _Entries.unsigned else v)
        for k, n in enumerate(_Entries.names32):
            setattr(e, n, a32[k, :nb].copy())
        if self.plan.boost:
            e.btot, e.bst = a64[8, :nb].copy(), a32[4, :nb].copy()
        return e, commit, done

    def store(self, slot, e, commit, done, gset=0):
        a64, a32 = self._arrays(slot)
        nb = len(e)
        a64[:], a32[:] = 0, 0
        for k, n in enumerate(_Entries.names64):
            a64[k, :nb] = np.asarray(getattr(e, n)).view(np.int64) if n in _Entries.unsigned else getattr(e, n)
        for k, n in enumerate(_Entries.names32):
            a32[k, :nb] = getattr(e, n)
        if self.plan.boost:
            a64[8, :nb], a32[4, :nb] = e.btot, e.bst
        b = self.block[slot]
        b[:HDR_WORDS] = 0
        b[_H_NB], b[_H_COMMIT], b[_H_DONE], b[_H_STARTED] = nb, commit, done, 1
        if self.plan.boost:
            b[_H_SET] = gset


def _frame(e, c32, q32, t, W, blank, tab, lm, alpha_q, beta_q, bs=None):
    """one frame of qasr.beam._search_one / _search_one_lm on the entries e (nb >= 1); returns (next entries or None when
    no candidate lives, [(slot, parent node, label)] of the new nodes).  Entries that carry bst / btot (a boosted plan)
    keep them; bs: the slot's PhraseSet, and the frame is _search_one_boost's (None: every boost term is 0)."""
    N = len(c32)
    i64 = np.int64
    pb, pnb, sc, hsh, phs, ln, last, node = e.pb, e.pnb, e.sc, e.hsh, e.phs, e.ln, e.last, e.node
    ctx, wh, own, lmt = e.ctx, e.wh, e.own, e.lmt
    nb = len(sc)
    has_lm = lm is not None
    word_mode = has_lm and lm.word_mode
    half = 1 << (FRAC - 1)
    c, q = c32.astype(np.int64), q32.astype(i64)
    valid = c >= 0
    isb = valid & (c == blank)
    match = (last[:, None] == c[None, :]) & valid[None, :]
    has, nl = match.any(1), match.argmax(1)
    pm = (phs[:, None] == hsh[None, :]) & (ln[:, None] == ln[None, :] + 1)
    hasp, ps = pm.any(1), pm.argmax(1)
    q_l = q[nl]
    pb_n = sc + q[isb.argmax()] if isb.any() else np.full(nb, NEG, i64)
    ownp = has & (pnb != NEG)
    a = np.where(ownp, q_l + np.where(ownp, pnb, 0), NEG)
    pbase = np.where(last[ps] == last, pb[ps], sc[ps])
    ext = has & hasp & (pbase != NEG)
    ee = np.where(ext, q_l + np.where(ext, pbase, 0) + own, NEG)
    pnb_n = lae(a, ee, tab)
    sc_n = lae(pb_n, pnb_n, tab)
    child = np.zeros((nb, N), dtype=bool)
    sel = has & hasp
    child[ps[sel], nl[sel]] = True
    base = np.where(c[None, :] == last[:, None], pb[:, None], sc[:, None])
    ok = (valid & ~isb)[None, :] & ~child & (base != NEG)
    scored, raws = np.zeros((nb, N), dtype=bool), np.zeros((nb, N), i64)
    if word_mode:
        space = lm.space
        inword = (last >= 0) & (last != space)
        for n in np.flatnonzero(valid & (c == space)):
            for i in np.flatnonzero(ok[:, n] & inword):
                raws[i, n], scored[i, n] = lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[0], True
    elif has_lm:
        nlab, l2w = lm.n_labels, lm.label_to_word
        wids = np.where(valid & (c < nlab), l2w[np.clip(c, 0, nlab - 1)], -1)
        for i, n in zip(*np.nonzero(ok)):
            raws[i, n] = lm.raw(int(ctx[i]), int(wids[n]))[0]
        scored = ok
    tm = np.where(scored, ((raws * alpha_q + half) >> FRAC) + beta_q, 0)
    boosted = hasattr(e, 'bst')
    if boosted:
        btm, bnx = np.zeros((nb, N), i64), np.zeros((nb, N), i64)
        if bs is not None:
            for i, n in zip(*np.nonzero(ok)):
                btm[i, n], bnx[i, n] = bs.term(int(e.bst[i]), int(c[n]))
        own_new = tm + btm
    else:
        btm, own_new = 0, tm
    v = np.where(ok, np.where(ok, base, 0) + q[None, :] + tm + btm, NEG)
    allc = np.concatenate([sc_n[:, None], v], axis=1).ravel()
    n_live = int((allc != NEG).sum())
    if n_live == 0:
        return None, []
    order = np.argsort(-allc, kind='stable')[:min(W, n_live)]
    src, k = order // (N + 1), order % (N + 1)
    kept = k == 0
    kn = np.maximum(k - 1, 0)
    cn = c[kn]
    o = _Entries()
    o.pb = np.where(kept, pb_n[src], NEG)
    o.pnb = np.where(kept, pnb_n[src], allc[order])
    o.sc = allc[order]
    o.hsh = np.where(kept, hsh[src], _hmix(hsh[src], cn))
    o.phs = np.where(kept, phs[src], hsh[src])
    o.ln = np.where(kept, ln[src], ln[src] + 1).astype(np.int32)
    o.last = np.where(kept, last[src], cn).astype(np.int32)
    o.node = np.where(kept, node[src], t * W + np.arange(len(order))).astype(np.int32)
    o.own = np.where(kept, own[src], own_new[src, kn])
    if boosted:
        o.btot = np.where(kept, e.btot[src], e.btot[src] + btm[src, kn])
        o.bst = np.where(kept, e.bst[src], bnx[src, kn]).astype(np.int32)
    o.lmt = np.where(kept, lmt[src], lmt[src] + tm[src, kn])
    o.ctx, o.wh = ctx[src].copy(), wh[src].copy()
    new = []
    for s in np.flatnonzero(~kept):
        i, n = int(src[s]), int(kn[s])
        if has_lm:
            if word_mode and cn[s] != lm.space:
                o.wh[s] = _hmix(wh[i:i + 1], cn[s:s + 1])[0]
            else:
                o.wh[s] = 0
                if not word_mode:
                    o.ctx[s] = lm.raw(int(ctx[i]), int(wids[n]))[1]
                elif scored[i, n]:
                    o.ctx[s] = lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[1]
        new.append((int(s), int(node[i]), int(cn[s])))
    return o, new


@dataclass
class BeamStepRow:
    """What one step gives for one row.  labels / frames: the delta; tail: the best entry's uncommitted labels (all of
    them); end: on END rows the list of (suffix labels, score, lm_tot), best first, cut to n_best."""
    labels: List[int] = field(default_factory=list)
    frames: List[int] = field(default_factory=list)
    commit_len: int = 0
    n_live: int = 0
    status: int = 0
    tail: List[int] = field(default_factory=list)
    end: Optional[list] = None          # boosted plans: (suffix labels, score, lm_tot, boost_tot)


def _walk(state: StreamBeamState, slot, nd, depth):
    """`depth` (label, creation frame) pairs of the chain that ends in node nd, newest first"""
    W, F = state.plan.W, state.plan.F
    ring = state.ring(slot)
    out = []
    assert 0 <= depth <= F, (depth, F)                       # the plan's bound on uncommitted labels
    for _ in range(depth):
        assert nd >= 0, 'a chain ended above commit_len'
        f, r = divmod(int(nd), W)
        assert state.row_frame[slot, f % F] == f, ('a live node was overwritten', f, int(state.row_frame[slot, f % F]))
        assert not out or f < out[-1][1], 'creation frames must rise along a chain'
        nd, lab = int(ring[f % F, r, 0]), int(ring[f % F, r, 1])
        out.append((lab, f))
    return out


def _full_labels(trail, nd):
    out = []
    while nd >= 0:
        nd, lab = trail['nodes'][nd]
        out.append(lab)
    return out[::-1]


def advance_host(state: StreamBeamState, slot, cand_id, cand_q, first, lo, hi, begin, end, blank, lm=None, alpha_q=0,
                 beta_q=0, boost=None, boost_set=-1) -> BeamStepRow:
    """One row of one step under STREAM_BEAM_RULES with the status checks already passed: cand_id / cand_q int32 [Tw][N]
    of the window whose local frame 0 is global frame `first`; frames [lo, hi) become final.  boost: the session's phrase
    sets (a boosted plan: STREAM_BOOST_RULES), boost_set: the set a BEGIN row gives the slot (-1: none)."""
    plan = state.plan
    W, F, K, Lg = plan.W, plan.F, plan.K, plan.Lg
    tab = lae_table()
    cid, cq = np.asarray(cand_id, dtype=np.int32), np.asarray(cand_q, dtype=np.int32)
    assert cid.ndim == 2 and cid.shape == cq.shape and cid.shape[1] == plan.N, (cid.shape, cq.shape, plan.N)
    sets = as_sets(boost)
    assert (sets is not None) == plan.boost, 'advance_host: boost= goes with a plan built with boost=True'
    gset = 0
    if sets is not None:
        gset = int(boost_set) + 1 if begin else state.boost_set(slot, len(sets))
        assert 0 <= gset <= len(sets), (gset, len(sets))
    bs = sets[gset - 1] if gset else None
    if begin:
        e, commit = _Entries.fresh(lm, plan.boost, bs), 0
        state.row_frame[slot], state.h_dead[slot] = -1, -1
        state.trail[slot] = dict(nodes={}, committed=[])
    else:
        e, commit, done = state.load(slot, lm, bs)
        assert done == lo, (done, lo)
    trail = state.trail[slot]
    ring = state.ring(slot)
    out = BeamStepRow()
    for t in range(lo, hi):
        if len(e) == 0:
            break
        nxt, new = _frame(e, cid[t - first], cq[t - first], t, W, int(blank), tab, lm, alpha_q, beta_q, bs)
        if nxt is None:
            e = e.take(np.zeros(0, dtype=np.int64))
            break
        e = nxt
        if new:
            prev = int(state.row_frame[slot, t % F])
            assert prev in (-1, t) or prev <= state.h_dead[slot], ('a ring row is overwritten while it may be live', prev, t)
            state.row_frame[slot, t % F] = t
        for s, parent, lab in new:
            ring[t % F, s] = (parent, lab)
            if state.check:
                trail['nodes'][t * W + s] = (parent, lab)
        if (t + 1) % K == 0 and t - Lg >= 0:
            h = t - Lg
            olds = []
            for i in range(len(e)):
                ch = _walk(state, slot, int(e.node[i]), int(e.ln[i]) - commit)
                olds.append([(lab, f) for lab, f in ch if f <= h])
            assert len(olds[0]) <= K, (len(olds[0]), K)
            lab0 = [x[0] for x in olds[0]]
            keep = np.array([[x[0] for x in o] == lab0 for o in olds], dtype=bool)
            assert keep[0]
            out.labels += lab0[::-1]
            out.frames += [x[1] for x in olds[0]][::-1]
            commit += len(lab0)                                 # never shrinks: len(old(0)) >= 0 is added
            trail['committed'] += lab0[::-1]
            e = e.take(np.flatnonzero(keep))
            state.h_dead[slot] = h
            if state.check:                                     # committed labels never change: every survivor starts with them
                for i in range(len(e)):
                    assert _full_labels(trail, int(e.node[i]))[:commit] == trail['committed'], 'a committed label changed'
    state.store(slot, e, commit, hi, gset)
    out.n_live = len(e)
    if end:
        sc, lmt = e.sc.copy(), e.lmt.copy()
        btot = e.btot.copy() if plan.boost else None
        word_mode = lm is not None and lm.word_mode
        if (word_mode or bs is not None) and len(e):
            half = 1 << (FRAC - 1)
            if word_mode:
                for i in np.flatnonzero((e.last >= 0) & (e.last != lm.space)):
                    tv = ((lm.raw(int(e.ctx[i]), lm.lookup_word(e.wh[i]))[0] * alpha_q + half) >> FRAC) + beta_q
                    sc[i] += tv
                    lmt[i] += tv
            if bs is not None:
                for i in range(len(e)):
                    fin = bs.finish(int(e.bst[i]))
                    sc[i] += fin
                    btot[i] += fin
            rank = np.argsort(-sc, kind='stable')
        else:
            rank = np.arange(len(e))
        out.end = []
        for i in rank[:plan.n_best]:
            ch = _walk(state, slot, int(e.node[i]), int(e.ln[i]) - commit)[::-1]
            out.end.append(([x[0] for x in ch], int(sc[i]), int(lmt[i]), [x[1] for x in ch]) +
                           ((int(btot[i]),) if plan.boost else ()))
        if out.end:
            out.labels += out.end[0][0]
            out.frames += out.end[0][3]
            commit += len(out.end[0][0])
        out.end = [x[:3] + x[4:] for x in out.end]
    elif len(e):
        out.tail = [x[0] for x in _walk(state, slot, int(e.node[0]), int(e.ln[0]) - commit)[::-1]]
    out.commit_len = commit
    assert len(out.labels) <= plan.delta_pitch or hi - lo > plan.max_final_frames, (len(out.labels), plan.delta_pitch)
    return out


@dataclass
class BeamStepBatch:
    """k_stream_beam's outputs: labels / frames [B][P]; n_new_labels, commit_len, n_live, status [B]; tail_labels
    [B][Ptail], tail_n [B] (the true count); end_labels [B][n_best][Pend], end_n_labels [B][n_best], end_score int64
    [B][n_best], end_lm_score int64 [B][n_best] (None without a model), n_hyps [B]; k_stream_beam_boost's also
    end_boost_score int64 [B][n_best] (None without boost)."""
    labels: object
    frames: object
    n_new_labels: object
    commit_len: object
    n_live: object
    status: object
    tail_labels: object
    tail_n: object
    end_labels: object
    end_n_labels: object
    end_score: object
    end_lm_score: object
    n_hyps: object
    end_boost_score: object = None


def batch_buffers(B, plan: StreamBeamPlan, blank, with_lm, P=None, Ptail=None, Pend=None, with_boost=False) -> BeamStepBatch:
    """the outputs of an empty step"""
    P = plan.delta_pitch if P is None else int(P)
    Ptail = plan.tail_pitch if Ptail is None else int(Ptail)
    Pend = plan.end_pitch if Pend is None else int(Pend)
    i = lambda *s: np.zeros(s, np.int32)
    return BeamStepBatch(np.full((B, P), blank, np.int32), i(B, P), i(B), i(B), i(B), i(B), np.full((B, Ptail), blank, np.int32),
                         i(B), np.full((B, plan.n_best, Pend), blank, np.int32), i(B, plan.n_best),
                         np.full((B, plan.n_best), NEG, np.int64), np.zeros((B, plan.n_best), np.int64) if with_lm else None, i(B),
                         np.zeros((B, plan.n_best), np.int64) if with_boost else None)


def _weights(lm, alpha, beta, blank):
    if lm is None:
        return 0, 0
    from .ngram import fixed_weights
    if lm.n_labels != int(blank):
        raise ValueError(f'stream_beam: the model was loaded for {lm.n_labels} labels, blank is {blank}')
    return fixed_weights(alpha, beta)


def step_batch_host(bstate: StreamBeamState, sstate: qs.StreamState, slots, flags, cand_id, cand_q, enc_lens, first_frame,
                    blank, lm=None, alpha=0.0, beta=0.0, P=None, Ptail=None, Pend=None, boost=None, boost_set=None) -> BeamStepBatch:
    """The twin of one k_stream_beam launch: cand_id / cand_q int32 [B][Tw][N]; slots / flags (BEGIN, END) / enc_lens /
    first_frame int [B].  Reads sstate (the stream blocks, BEFORE emit_batch_host advances them), updates bstate.
    boost: the session's phrase sets (one PhraseSet or a sequence of at most MAX_SETS) on a boosted plan - the twin of
    k_stream_beam_boost; boost_set int [B]: the set of each BEGIN row (-1: none; None: -1 everywhere)."""
    plan, splan = bstate.plan, sstate.plan
    sets = as_sets(boost)
    if (sets is not None) != plan.boost:
        raise ValueError('stream_beam: boost= goes with a plan built with boost=True')
    for bs in sets or []:
        if bs.n_labels != int(blank):
            raise ValueError(f'stream_beam: the phrase set was compiled for {bs.n_labels} labels, blank is {blank}')
    alpha_q, beta_q = _weights(lm, alpha, beta, blank)
    cid, cq = np.asarray(cand_id), np.asarray(cand_q)
    B, Tw = cid.shape[0], cid.shape[1]
    o = batch_buffers(B, plan, blank, lm is not None, P, Ptail, Pend, sets is not None)
    bset = np.full(B, -1, np.int64) if boost_set is None else np.asarray(boost_set, dtype=np.int64)
    P, Ptail, Pend = o.labels.shape[1], o.tail_labels.shape[1], o.end_labels.shape[2]
    for b in range(B):
        slot = int(slots[b])
        if not (0 <= slot < bstate.S and slot < sstate.S):
            o.status[b] = STATUS_SLOT
            continue
        first = int(first_frame[b])
        e = max(0, min(int(enc_lens[b]), Tw))
        end, begin = bool(int(flags[b]) & qs.END), bool(int(flags[b]) & qs.BEGIN)
        r = max(sstate.received(slot), 0)
        lo, hi = splan.final_range(r, sstate.frames_done(slot), first, e, end)
        if lo < first or first < 0:
            o.status[b] = STATUS_GAP
            continue
        if (0 if begin else bstate.header(slot)[2]) != lo:
            o.status[b] = STATUS_SYNC
            continue
        if hi * plan.W > NODE_LIMIT:
            o.status[b] = STATUS_NODES
            continue
        if sets is not None and begin and not -1 <= int(bset[b]) < len(sets):
            o.status[b] = STATUS_SET
            continue
        row = advance_host(bstate, slot, cid[b], cq[b], first, lo, hi, begin, end, blank, lm, alpha_q, beta_q, sets,
                           int(bset[b]))
        n = min(len(row.labels), P)
        o.labels[b, :n], o.frames[b, :n], o.n_new_labels[b] = row.labels[:n], row.frames[:n], n
        o.commit_len[b], o.n_live[b] = row.commit_len, row.n_live
        nt = min(len(row.tail), Ptail)
        o.tail_labels[b, :nt], o.tail_n[b] = row.tail[:nt], len(row.tail)
        if row.end is not None:
            o.n_hyps[b] = len(row.end)
            for h, ent in enumerate(row.end):
                labs, sc, lmt = ent[:3]
                if sets is not None:
                    o.end_boost_score[b, h] = ent[3]
                m = min(len(labs), Pend)
                o.end_labels[b, h, :m], o.end_n_labels[b, h], o.end_score[b, h] = labs[:m], len(labs), sc
                if o.end_lm_score is not None:
                    o.end_lm_score[b, h] = lmt
    return o


@dataclass
class LaggedResult:
    """lagged_search_host's outputs: committed labels and their creation frames in commit order (the END step's
    included), and the final hypotheses best first as (labels - the committed text prepended -, score, lm_tot), with
    boost= (labels, score, lm_tot, boost_tot)."""
    labels: List[int]
    frames: List[int]
    hyps: list
    commit_len_before_end: int = 0


def lagged_search_host(cand_id, cand_q, lim, blank, beam_width=16, n_best=None, lm=None, alpha=0.0, beta=0.0, lag=200,
                       K=K_ROUND, cuts=None, check=True, boost=None) -> LaggedResult:
    """The whole-stream statement: cand_id / cand_q int32 [T][N] of ONE stream, its first `lim` frames searched under
    STREAM_BEAM_RULES with a lag of `lag` frames, ended after the last.  cuts: frame indices at which the stream is cut
    into steps (None: one step); the result does not depend on them.  boost: a qasr.boost.PhraseSet, and the rule is
    STREAM_BOOST_RULES."""
    cid, cq = np.asarray(cand_id, dtype=np.int32), np.asarray(cand_q, dtype=np.int32)
    lim = int(min(max(int(lim), 0), cid.shape[0]))
    W = int(beam_width)
    plan = StreamBeamPlan(W, W if n_best is None else n_best, cid.shape[1], lag, max(lim, 1), K, boost is not None)
    if boost is not None and boost.n_labels != int(blank):
        raise ValueError(f'lagged_search_host: the phrase set was compiled for {boost.n_labels} labels, blank is {blank}')
    alpha_q, beta_q = _weights(lm, alpha, beta, blank)
    if lim * W > NODE_LIMIT:
        raise ValueError(f'lagged_search_host: {lim} frames x width {W} pass the node-id limit')
    st = StreamBeamState(1, plan, check)
    edges = [0] + sorted(int(c) for c in (cuts or []) if 0 < int(c) < lim) + [lim]
    labels, frames, before, row = [], [], 0, None
    for i in range(len(edges) - 1):
        last = i == len(edges) - 2
        row = advance_host(st, 0, cid, cq, 0, edges[i], edges[i + 1], i == 0, last, blank, lm, alpha_q, beta_q, boost,
                           0 if boost is not None else -1)
        if last:
            before = row.commit_len - (len(row.end[0][0]) if row.end else 0)
        labels += row.labels
        frames += row.frames
    head = labels[:before]
    return LaggedResult(labels, frames, [(head + x[0],) + tuple(x[1:]) for x in row.end], before)


# ------------------------------------------------------------------------------------- cuts: STREAM_BEAM_EP_RULES
@dataclass
class BeamEpStepRow:
    """What one step with cuts gives for one row.  labels / frames: the delta; commit_len, n_live, tail: of the beam the step
    leaves behind; cuts: per cut the list of (suffix labels, score, lm_tot[, boost_tot]), best first, cut to n_best;
    cut_delta_end: the delta's length after each cut."""
    labels: List[int] = field(default_factory=list)
    frames: List[int] = field(default_factory=list)
    commit_len: int = 0
    n_live: int = 0
    tail: List[int] = field(default_factory=list)
    cuts: list = field(default_factory=list)
    cut_delta_end: List[int] = field(default_factory=list)


def _end_pass(state, slot, e, commit, lm, alpha_q, beta_q, bs):
    """the END pass of the rules on the entries e: [(suffix labels, score, lm_tot, creation frames[, boost_tot])], best first,
    cut to n_best"""
    plan = state.plan
    sc, lmt = e.sc.copy(), e.lmt.copy()
    btot = e.btot.copy() if plan.boost else None
    word_mode = lm is not None and lm.word_mode
    if (word_mode or bs is not None) and len(e):
        half = 1 << (FRAC - 1)
        if word_mode:
            for i in np.flatnonzero((e.last >= 0) & (e.last != lm.space)):
                tv = ((lm.raw(int(e.ctx[i]), lm.lookup_word(e.wh[i]))[0] * alpha_q + half) >> FRAC) + beta_q
                sc[i] += tv
                lmt[i] += tv
        if bs is not None:
            for i in range(len(e)):
                fin = bs.finish(int(e.bst[i]))
                sc[i] += fin
                btot[i] += fin
        rank = np.argsort(-sc, kind='stable')
    else:
        rank = np.arange(len(e))
    out = []
    for i in rank[:plan.n_best]:
        ch = _walk(state, slot, int(e.node[i]), int(e.ln[i]) - commit)[::-1]
        out.append(([x[0] for x in ch], int(sc[i]), int(lmt[i]), [x[1] for x in ch]) + ((int(btot[i]),) if plan.boost else ()))
    return out


def advance_ep_host(state: StreamBeamState, slot, cand_id, cand_q, first, lo, hi, begin, rec_ends, blank, lm=None, alpha_q=0,
                    beta_q=0, boost=None, boost_set=-1) -> BeamEpStepRow:
    """One row of one step under STREAM_BEAM_EP_RULES with the status checks already passed: advance_host's arguments, and
    rec_ends: the `end` of each of the step's records, in order."""
    plan = state.plan
    W, F, K, Lg = plan.W, plan.F, plan.K, plan.Lg
    tab = lae_table()
    cid, cq = np.asarray(cand_id, dtype=np.int32), np.asarray(cand_q, dtype=np.int32)
    assert cid.ndim == 2 and cid.shape == cq.shape and cid.shape[1] == plan.N, (cid.shape, cq.shape, plan.N)
    sets = as_sets(boost)
    assert (sets is not None) == plan.boost, 'advance_ep_host: boost= goes with a plan built with boost=True'
    gset = 0
    if sets is not None:
        gset = int(boost_set) + 1 if begin else state.boost_set(slot, len(sets))
        assert 0 <= gset <= len(sets), (gset, len(sets))
    bs = sets[gset - 1] if gset else None
    if begin:
        e, commit, cuts0 = _Entries.fresh(lm, plan.boost, bs), 0, 0
        state.row_frame[slot], state.h_dead[slot] = -1, -1
        state.trail[slot] = dict(nodes={}, committed=[])
    else:
        e, commit, done = state.load(slot, lm, bs)
        cuts0 = int(state.block[slot, _H_CUTS])
        assert done == lo, (done, lo)
    trail = state.trail[slot]
    ring = state.ring(slot)
    out = BeamEpStepRow()
    ends = [int(x) for x in rec_ends]
    rk = 0

    def cut(t_end):
        nonlocal e, commit
        hyps = _end_pass(state, slot, e, commit, lm, alpha_q, beta_q, bs)
        if hyps:
            out.labels += hyps[0][0]
            out.frames += hyps[0][3]
        out.cuts.append([x[:3] + x[4:] for x in hyps])
        out.cut_delta_end.append(len(out.labels))
        e, commit = _Entries.fresh(lm, plan.boost, bs), 0
        trail['committed'] = []
        state.h_dead[slot] = max(int(state.h_dead[slot]), t_end - 1)      # every node made before the cut is dead

    for t in range(lo, hi):
        if len(e):
            nxt, new = _frame(e, cid[t - first], cq[t - first], t, W, int(blank), tab, lm, alpha_q, beta_q, bs)
            if nxt is None:
                e = e.take(np.zeros(0, dtype=np.int64))
                new = []
            else:
                e = nxt
            if new:
                prev = int(state.row_frame[slot, t % F])
                assert prev in (-1, t) or prev <= state.h_dead[slot], ('a ring row is overwritten while it may be live', prev, t)
                state.row_frame[slot, t % F] = t
            for s, parent, lab in new:
                ring[t % F, s] = (parent, lab)
                if state.check:
                    trail['nodes'][t * W + s] = (parent, lab)
        if (t + 1) % K == 0 and t - Lg >= 0 and len(e):
            h = t - Lg
            olds = []
            for i in range(len(e)):
                ch = _walk(state, slot, int(e.node[i]), int(e.ln[i]) - commit)
                olds.append([(lab, f) for lab, f in ch if f <= h])
            assert len(olds[0]) <= K, (len(olds[0]), K)
            lab0 = [x[0] for x in olds[0]]
            keep = np.array([[x[0] for x in o] == lab0 for o in olds], dtype=bool)
            assert keep[0]
            out.labels += lab0[::-1]
            out.frames += [x[1] for x in olds[0]][::-1]
            commit += len(lab0)
            trail['committed'] += lab0[::-1]
            e = e.take(np.flatnonzero(keep))
            state.h_dead[slot] = max(int(state.h_dead[slot]), h)
            if state.check:
                for i in range(len(e)):
                    assert _full_labels(trail, int(e.node[i]))[:commit] == trail['committed'], 'a committed label changed'
        while rk < len(ends) and ends[rk] == t + 1:
            cut(t + 1)
            rk += 1
    while rk < len(ends):
        assert ends[rk] == hi, (ends, lo, hi)
        cut(hi)
        rk += 1
    state.store(slot, e, commit, hi, gset)
    state.block[slot, _H_CUTS] = cuts0 + len(ends)
    out.n_live, out.commit_len = len(e), commit
    if len(e):
        out.tail = [x[0] for x in _walk(state, slot, int(e.node[0]), int(e.ln[0]) - commit)[::-1]]
    assert len(out.labels) <= plan.delta_pitch or hi - lo > plan.max_final_frames, (len(out.labels), plan.delta_pitch)
    assert all(len(x[0]) <= plan.end_pitch for c in out.cuts for x in c)
    return out


@dataclass
class BeamEpStepBatch:
    """k_stream_beam_ep's outputs: labels / frames [B][P]; n_new_labels, commit_len, n_live, status [B]; tail_labels
    [B][Ptail], tail_n [B]; n_cuts [B]; cut_n_hyps, cut_delta_end [B][E]; cut_labels [B][E][n_best][Pend], cut_n_labels
    [B][E][n_best], cut_score int64 [B][E][n_best], cut_lm_score (None without a model), cut_boost_score (None without boost)."""
    labels: object
    frames: object
    n_new_labels: object
    commit_len: object
    n_live: object
    status: object
    tail_labels: object
    tail_n: object
    n_cuts: object
    cut_n_hyps: object
    cut_delta_end: object
    cut_labels: object
    cut_n_labels: object
    cut_score: object
    cut_lm_score: object = None
    cut_boost_score: object = None


def ep_batch_buffers(B, plan: StreamBeamPlan, E, blank, with_lm, P=None, Ptail=None, Pend=None) -> BeamEpStepBatch:
    """the outputs of an empty step"""
    P = plan.delta_pitch if P is None else int(P)
    Ptail = plan.tail_pitch if Ptail is None else int(Ptail)
    Pend = plan.end_pitch if Pend is None else int(Pend)
    E, nb = int(E), plan.n_best
    i = lambda *s: np.zeros(s, np.int32)
    return BeamEpStepBatch(np.full((B, P), blank, np.int32), i(B, P), i(B), i(B), i(B), i(B), np.full((B, Ptail), blank, np.int32),
                           i(B), i(B), i(B, E), i(B, E), np.full((B, E, nb, Pend), blank, np.int32), i(B, E, nb),
                           np.full((B, E, nb), NEG, np.int64), np.zeros((B, E, nb), np.int64) if with_lm else None,
                           np.zeros((B, E, nb), np.int64) if plan.boost else None)


def step_batch_ep_host(bstate: StreamBeamState, sstate: qs.StreamState, slots, flags, cand_id, cand_q, enc_lens, first_frame,
                       records, n_records, ep_status, blank, lm=None, alpha=0.0, beta=0.0, P=None, Ptail=None, Pend=None,
                       boost=None, boost_set=None) -> BeamEpStepBatch:
    """The twin of one k_stream_beam_ep launch, AFTER emit_batch_host and endpoint_batch_host of the same rows: step_batch_host's
    arguments, and records int32 [B][E][10], n_records, ep_status int [B] as qasr.stream_ep.endpoint_batch_host gave them."""
    from .stream_ep import R_END, R_INDEX
    plan = bstate.plan
    sets = as_sets(boost)
    if (sets is not None) != plan.boost:
        raise ValueError('stream_beam: boost= goes with a plan built with boost=True')
    for bs in sets or []:
        if bs.n_labels != int(blank):
            raise ValueError(f'stream_beam: the phrase set was compiled for {bs.n_labels} labels, blank is {blank}')
    alpha_q, beta_q = _weights(lm, alpha, beta, blank)
    cid, cq, rec = np.asarray(cand_id), np.asarray(cand_q), np.asarray(records)
    B, Tw, E = cid.shape[0], cid.shape[1], rec.shape[1]
    o = ep_batch_buffers(B, plan, E, blank, lm is not None, P, Ptail, Pend)
    bset = np.full(B, -1, np.int64) if boost_set is None else np.asarray(boost_set, dtype=np.int64)
    P, Ptail, Pend = o.labels.shape[1], o.tail_labels.shape[1], o.cut_labels.shape[3]
    for b in range(B):
        slot = int(slots[b])
        if not (0 <= slot < bstate.S and slot < sstate.S):
            o.status[b] = STATUS_SLOT
            continue
        first = int(first_frame[b])
        e = max(0, min(int(enc_lens[b]), Tw))
        begin = bool(int(flags[b]) & qs.BEGIN)
        lo, hi = (0 if begin else bstate.header(slot)[2]), sstate.frames_done(slot)
        if lo < first or first < 0:
            o.status[b] = STATUS_GAP
            continue
        n = int(n_records[b])
        bad = lo > hi or (lo < hi and hi > first + e) or not 0 <= n <= E or int(ep_status[b]) != 0
        if not bad and n:
            bad = int(rec[b, 0, R_INDEX]) != (0 if begin else int(bstate.block[slot, _H_CUTS]))
            prev = lo
            for k in range(n):
                en = int(rec[b, k, R_END])
                bad = bad or en < prev or en > hi or (en == lo and lo < hi)
                prev = en
        if bad:
            o.status[b] = STATUS_SYNC
            continue
        if hi * plan.W > NODE_LIMIT:
            o.status[b] = STATUS_NODES
            continue
        if sets is not None and begin and not -1 <= int(bset[b]) < len(sets):
            o.status[b] = STATUS_SET
            continue
        row = advance_ep_host(bstate, slot, cid[b], cq[b], first, lo, hi, begin, rec[b, :n, R_END], blank, lm, alpha_q, beta_q,
                              sets, int(bset[b]))
        m = min(len(row.labels), P)
        o.labels[b, :m], o.frames[b, :m], o.n_new_labels[b] = row.labels[:m], row.frames[:m], m
        o.commit_len[b], o.n_live[b] = row.commit_len, row.n_live
        nt = min(len(row.tail), Ptail)
        o.tail_labels[b, :nt], o.tail_n[b] = row.tail[:nt], len(row.tail)
        o.n_cuts[b] = n
        for k, hyps in enumerate(row.cuts):
            o.cut_n_hyps[b, k], o.cut_delta_end[b, k] = len(hyps), min(row.cut_delta_end[k], P)
            for h, ent in enumerate(hyps):
                labs, sc, lmt = ent[:3]
                mm = min(len(labs), Pend)
                o.cut_labels[b, k, h, :mm], o.cut_n_labels[b, k, h], o.cut_score[b, k, h] = labs[:mm], len(labs), sc
                if o.cut_lm_score is not None:
                    o.cut_lm_score[b, k, h] = lmt
                if sets is not None:
                    o.cut_boost_score[b, k, h] = ent[3]
    return o


def step_ep_host(bstate: StreamBeamState, sstate: qs.StreamState, slot, flag, cand_id, cand_q, enc_len, first, records, n_records,
                 ep_status, blank, **kw) -> BeamEpStepBatch:
    """step_batch_ep_host for one row: cand_id / cand_q [Tw][N], records [E][10]"""
    return step_batch_ep_host(bstate, sstate, [slot], [flag], np.asarray(cand_id)[None], np.asarray(cand_q)[None], [enc_len], [first],
                              np.asarray(records)[None], [n_records], [ep_status], blank, **kw)


@dataclass
class LaggedEpResult:
    """lagged_search_ep_host's outputs: the whole delta (labels, creation frames), per cut the delta's length after it
    (cut_delta_end), the cut's hypotheses best first as (suffix labels, score, lm_tot[, boost_tot]) (cuts), and per cut
    the utterance's best text - what was committed since the cut before plus the best suffix - with its frames (utts);
    block: the state block (ring included) the search leaves behind."""
    labels: List[int]
    frames: List[int]
    cut_delta_end: List[int]
    cuts: list
    utts: list
    block: object = None

    def __eq__(self, o):
        return (self.labels, self.frames, self.cut_delta_end, self.cuts, self.utts) == \
            (o.labels, o.frames, o.cut_delta_end, o.cuts, o.utts) and self.block.tobytes() == o.block.tobytes()


def lagged_search_ep_host(cand_id, cand_q, lim, cut_ends, blank, beam_width=16, n_best=None, lm=None, alpha=0.0, beta=0.0, lag=200,
                          K=K_ROUND, steps=None, check=True, boost=None) -> LaggedEpResult:
    """The whole-stream statement with cuts: cand_id / cand_q int32 [T][N] of ONE stream, its first `lim` frames searched
    under STREAM_BEAM_EP_RULES with a lag of `lag` frames; cut_ends: the `end` frame of every record of the stream in
    order (rising, repeats allowed, each in 0 .. lim; the END record's is lim).  steps: frame indices at which the stream
    is sliced into steps (None: one step); the result does not depend on them.  boost: a qasr.boost.PhraseSet."""
    cid, cq = np.asarray(cand_id, dtype=np.int32), np.asarray(cand_q, dtype=np.int32)
    lim = int(min(max(int(lim), 0), cid.shape[0]))
    W = int(beam_width)
    ends = [int(c) for c in cut_ends]
    if ends != sorted(ends) or any(not 0 <= c <= lim for c in ends) or (lim > 0 and 0 in ends):
        raise ValueError(f'lagged_search_ep_host: cut ends {ends} must rise inside 1 .. {lim}')
    plan = StreamBeamPlan(W, W if n_best is None else n_best, cid.shape[1], lag, max(lim, 1), K, boost is not None)
    if boost is not None and boost.n_labels != int(blank):
        raise ValueError(f'lagged_search_ep_host: the phrase set was compiled for {boost.n_labels} labels, blank is {blank}')
    alpha_q, beta_q = _weights(lm, alpha, beta, blank)
    if lim * W > NODE_LIMIT:
        raise ValueError(f'lagged_search_ep_host: {lim} frames x width {W} pass the node-id limit')
    st = StreamBeamState(1, plan, check)
    edges = [0] + sorted(int(c) for c in (steps or []) if 0 < int(c) < lim) + [lim]
    labels, frames, cde, cuts = [], [], [], []
    for i in range(len(edges) - 1):
        lo, hi = edges[i], edges[i + 1]
        mine = [c for c in ends if (lo < c <= hi) or (lo == hi == c)]
        row = advance_ep_host(st, 0, cid, cq, 0, lo, hi, i == 0, mine, blank, lm, alpha_q, beta_q, boost,
                              0 if boost is not None else -1)
        cde += [len(labels) + x for x in row.cut_delta_end]
        cuts += row.cuts
        labels += row.labels
        frames += row.frames
    utts = [(labels[a:b], frames[a:b]) for a, b in zip([0] + cde[:-1], cde)]
    return LaggedEpResult(labels, frames, cde, cuts, utts, st.block.copy())


def walk_ep(plan: StreamBeamPlan, cand_id, cand_q, step_edges, cut_ends, blank, lm=None, alpha=0.0, beta=0.0, boost=None):
    """Steps the twin through a protocol of frames that contains cuts - step_edges: the frame at which each step ends, in
    order; cut_ends: as lagged_search_ep_host takes them - and asserts the plan's sizes on every step: no live ring row is
    overwritten and chain walks stay within F (asserted inside the twin), every delta fits delta_pitch for steps of at
    most max_final_frames, every cut suffix and every tail fits F, creation frames rise inside every utterance and the
    utterances' frames are disjoint and in order.  Returns the number of cuts walked."""
    cid, cq = np.asarray(cand_id, dtype=np.int32), np.asarray(cand_q, dtype=np.int32)
    alpha_q, beta_q = _weights(lm, alpha, beta, blank)
    st = StreamBeamState(1, plan, check=True)
    ends = [int(c) for c in cut_ends]
    lo, n_cuts, last_frame = 0, 0, -1
    for i, hi in enumerate(step_edges):
        hi = int(hi)
        assert lo <= hi <= cid.shape[0] and hi - lo <= plan.max_final_frames, (lo, hi, plan.max_final_frames)
        mine = [c for c in ends if (lo < c <= hi) or (lo == hi == c and i == len(step_edges) - 1)]
        row = advance_ep_host(st, 0, cid, cq, 0, lo, hi, i == 0, mine, blank, lm, alpha_q, beta_q, boost, 0 if boost is not None else -1)
        assert len(row.labels) <= plan.delta_pitch and len(row.tail) <= plan.tail_pitch
        assert all(len(x[0]) <= plan.end_pitch for c in row.cuts for x in c)
        assert row.cut_delta_end == sorted(row.cut_delta_end) and all(x <= len(row.labels) for x in row.cut_delta_end)
        for f in row.frames:                          # one chain per utterance, utterances over disjoint frames, in order
            assert f > last_frame and f < hi, (f, last_frame, hi)
            last_frame = f
        n_cuts += len(mine)
        assert int(st.block[0, _H_CUTS]) == n_cuts
        lo = hi
    return n_cuts
