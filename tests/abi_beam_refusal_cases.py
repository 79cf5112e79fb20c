"""The refusals of the six beam entry points (qasr_ctc_beam, _lm, _boost, qasr_stream_beam, _boost, _ep), case by case: which
check fires and what qasr_last_error says.  Host code only: ctypes structs of qasr.engine filled by hand, one 16-byte-aligned
host buffer standing for every pointer, stream NULL.  Every argument block is a base that passes all checks with mutations
on top; the base alone is never passed, so nothing is ever launched.

An entry is a list of checks in the order of the source; a check is a list of mutations that reach its `fail(` line.  How the
entries become cases - (a) every mutation on its own, (b) each two neighbouring checks broken at once - and the runner are
abi_refusal_driver's, shared with abi_lattice_refusal_cases.

tests/golden/gen_golden_abi_beam_refusals.py records (entry, case, rc, text); test_abi_beam_refusals_cpu.py compares."""
import ctypes as C

import abi_refusal_driver as driver
from abi_refusal_driver import PTR, null as _null

S, B, W, N, NB, BLANK, SPACE = 3, 2, 16, 20, 2, 28, 27
T = 5                                                   # frames of the offline calls
SPF, WL, CH, RR, TW, MFF = 160, 4800, 1600, 1600, 30, 10  # samples per frame, window, chunk and right context in samples; frames
LG, K, F, P, PTAIL, PEND, E = 2, 7, 9, 24, 4, 12, 3     # P and Pend with room for F + 1
LAE = 16384
MAXW = 16 << 16                                         # QASR_LM_MAX_WEIGHT


# ---- the offline calls
BEAM_PTRS = ('cand_id', 'cand_q', 'lae_table', 'workspace', 'labels', 'n_labels', 'score', 'n_hyps')


def _offline_base(lib, engine, cls):
    a = cls()
    a.struct_size = C.sizeof(cls)
    a.B, a.T, a.N, a.beam_width, a.n_best, a.blank, a.lae_entries = B, T, N, W, NB, BLANK, LAE
    for n in BEAM_PTRS + ('lens',):
        setattr(a, n, PTR)
    a.workspace_bytes = lib.qasr_ctc_beam_workspace_bytes(B, T, W)
    assert a.workspace_bytes > 0
    if cls is not engine.BeamArgs:
        a.lm, a.lm_bytes, a.alpha_q, a.beta_q, a.space, a.lm_score = PTR, 4096, 1 << 15, 1 << 15, SPACE, PTR
    if cls is engine.BeamBoostArgs:
        a.boost, a.boost_bytes, a.boost_score, a.whole_words = PTR, 4096, PTR, 1
    return a


def _offline_common(lib, more_ptrs):
    need = lib.qasr_ctc_beam_workspace_bytes(B, T, W)
    return [
        ('struct_size', [('8', dict(struct_size=8))]),
        ('pointers', _null(BEAM_PTRS) + more_ptrs),
        ('shape', [('T=0', dict(T=0)), ('B=0', dict(B=0)), ('T=65537', dict(T=65537)), ('W=0', dict(beam_width=0)),
                   ('W=129', dict(beam_width=129)), ('B*T=2^31', dict(B=65536, T=32768))]),
        ('N', [('0', dict(N=0)), ('65', dict(N=65))]),
        ('n_best', [('0', dict(n_best=0)), ('W+1', dict(n_best=W + 1)), ('blank=-1', dict(blank=-1))]),
        ('lae_entries', [('16383', dict(lae_entries=LAE - 1))]),
        ('workspace', [('need-1', dict(workspace_bytes=need - 1)), ('0', dict(workspace_bytes=0))]),
    ]


def _model(field='lm'):
    return (field, [('misaligned', {field: PTR + 4}), ('64', {field + '_bytes': 64}), ('127', {field + '_bytes': 127}),
                    ('2^31', {field + '_bytes': 1 << 31})])


_WEIGHTS = ('weights', [('alpha=-1', dict(alpha_q=-1)), ('alpha>max', dict(alpha_q=MAXW + 1)), ('beta<-max', dict(beta_q=-MAXW - 1)),
                        ('beta>max', dict(beta_q=MAXW + 1))])
_SPACE = ('space', [('-2', dict(space=-2)), ('blank', dict(space=BLANK))])


def _offline_entries(lib, engine):
    lm_ptrs = _null(('lm', 'lm_score'))
    boost_ptrs = _null(('boost', 'boost_score', 'lm_score'))
    return [
        ('ctc_beam', lib.qasr_ctc_beam, lambda: _offline_base(lib, engine, engine.BeamArgs), _offline_common(lib, [])),
        ('ctc_beam_lm', lib.qasr_ctc_beam_lm, lambda: _offline_base(lib, engine, engine.BeamLmArgs),
         _offline_common(lib, lm_ptrs) + [_model(), _WEIGHTS, _SPACE]),
        ('ctc_beam_boost', lib.qasr_ctc_beam_boost, lambda: _offline_base(lib, engine, engine.BeamBoostArgs),
         _offline_common(lib, boost_ptrs) + [_model(), _WEIGHTS, _model('boost'), _SPACE,
                                             ('whole_words', [('no space', dict(whole_words=1, space=-1)),
                                                              ('no space, no lm', dict(whole_words=1, space=-1, lm=None))])]),
    ]


# ---- the streaming calls: the checks of the embedded qasr_stream_beam_args, its fields behind `pre`
STEP_PTRS = ('state', 'beam_state', 'slots', 'flags', 'cand_id', 'cand_q', 'enc_lens', 'first_frame', 'lae_table', 'labels', 'frames',
             'n_new_labels', 'commit_len', 'n_live', 'status', 'tail_labels', 'tail_n')
END_PTRS = ('end_labels', 'end_n_labels', 'end_score', 'n_hyps')
CUT_PTRS = ('records', 'n_records', 'ep_status', 'n_cuts', 'cut_n_hyps', 'cut_delta_end', 'cut_labels', 'cut_n_labels', 'cut_score')


def _fill_step(lib, a, engine, boosted):
    a.struct_size = C.sizeof(engine.StreamBeamArgs)
    a.S, a.B, a.Wl, a.C, a.Rr, a.samples_per_frame, a.Tw = S, B, WL, CH, RR, SPF, TW
    a.N, a.beam_width, a.n_best, a.blank = N, W, NB, BLANK
    a.Lg, a.K, a.F, a.max_final_frames, a.P, a.Ptail, a.Pend, a.lae_entries = LG, K, F, MFF, P, PTAIL, PEND, LAE
    a.state_bytes = lib.qasr_stream_state_bytes(S, WL, CH)
    a.beam_state_bytes = (lib.qasr_stream_beam_boost_state_bytes if boosted else lib.qasr_stream_beam_state_bytes)(S, W, F)
    assert a.state_bytes > 0 and a.beam_state_bytes > 0
    for n in STEP_PTRS + END_PTRS + ('lm', 'end_lm_score'):
        setattr(a, n, PTR)
    a.lm_bytes, a.alpha_q, a.beta_q, a.space = 4096, 1 << 15, 1 << 15, SPACE


def _fill_sets(q, engine):
    q.struct_size, q.n_sets = C.sizeof(engine.StreamBeamBoostArgs), 2
    for g in range(2):
        q.sets[g], q.set_bytes[g], q.whole_words[g] = PTR, 4096, g       # the second set holds whole words
    q.boost_set = q.end_boost_score = PTR


def _pre(pre, checks):
    return [(name, [(m, {pre + k: v for k, v in kw.items()}) for m, kw in muts]) for name, muts in checks]


def _geometry(lib):
    return [
        ('B', [('0', dict(B=0)), ('S+1', dict(B=S + 1)), ('S=0', dict(S=0)), ('65536', dict(S=70000, B=65536))]),
        ('at least 1', [('C=0', dict(C=0)), ('Wl=0', dict(Wl=0)), ('spf=0', dict(samples_per_frame=0))]),
        ('multiples', [('Wl+1', dict(Wl=WL + 1)), ('C-1', dict(C=CH - 1)), ('Rr+1', dict(Rr=RR + 1))]),
        ('Rr', [('Wl', dict(Rr=WL)), ('-spf', dict(Rr=-SPF)), ('Wl-C+spf', dict(Rr=WL - CH + SPF))]),
        ('state_bytes', [('16', dict(state_bytes=16)), ('need-4', dict(state_bytes=lib.qasr_stream_state_bytes(S, WL, CH) - 4))]),
    ]


def _ranges():
    return [
        ('Tw', [('0', dict(Tw=0)), ('65537', dict(Tw=65537))]),
        ('beam_width', [('0', dict(beam_width=0)), ('129', dict(beam_width=129))]),
        ('N', [('0', dict(N=0)), ('65', dict(N=65))]),
        ('n_best', [('0', dict(n_best=0)), ('W+1', dict(n_best=W + 1)), ('blank=-1', dict(blank=-1))]),
        ('lae_entries', [('16383', dict(lae_entries=LAE - 1))]),
        ('Lg, K', [('Lg=-1', dict(Lg=-1)), ('K=0', dict(K=0)), ('K=33', dict(K=33))]),
        ('F', [('Lg+K-1', dict(F=LG + K - 1)), ('2^20+1', dict(F=(1 << 20) + 1))]),
    ]


def _beam_state(need, unboosted=None):
    return ('beam_state_bytes', [('16', dict(beam_state_bytes=16)), ('need-4', dict(beam_state_bytes=need - 4)), ('F+1', dict(F=F + 1))] +
            ([('unboosted size', dict(beam_state_bytes=unboosted))] if unboosted else []))


def _tail():
    return [
        ('alignment', [('state', dict(state=PTR + 4)), ('beam_state', dict(beam_state=PTR + 8))]),
        ('max_final_frames', [('0', dict(max_final_frames=0)), ('Tw+1', dict(max_final_frames=TW + 1))]),
        ('pitches', [('Ptail=0', dict(Ptail=0)), ('P', dict(P=F + MFF - 1)), ('Pend', dict(Pend=F - 1))]),
    ]


def _stream_entries(lib, engine):
    need = lib.qasr_stream_beam_state_bytes(S, W, F)
    need_b = lib.qasr_stream_beam_boost_state_bytes(S, W, F)
    assert need_b > need
    lm_score = lambda name: ('lm score', [('NULL', {name: None})])
    no_lm = dict(lm=None)

    def plain():
        a = engine.StreamBeamArgs()
        _fill_step(lib, a, engine, False)
        return a

    def boost():
        q = engine.StreamBeamBoostArgs()
        _fill_step(lib, q.beam, engine, True)
        _fill_sets(q, engine)
        return q

    def ep(boosted):
        def make():
            x = engine.StreamBeamEpArgs()
            x.struct_size, x.E = C.sizeof(engine.StreamBeamEpArgs), E
            _fill_step(lib, x.boost.beam, engine, boosted)
            if boosted:
                _fill_sets(x.boost, engine)
            else:
                x.boost.struct_size = C.sizeof(engine.StreamBeamBoostArgs)
            for n in CUT_PTRS + ('cut_lm_score', 'cut_boost_score'):
                setattr(x, n, PTR)
            return x
        return make

    def sets_loop(pre, b):
        # `b`: the embedded step's fields; without the model the second set's whole words meet space -1
        return [('set', [('NULL', {pre + 'sets[0]': None}), ('second NULL', {pre + 'sets[1]': None}), ('misaligned', {pre + 'sets[0]': PTR + 8}),
                         ('64', {pre + 'set_bytes[1]': 64}), ('2^31', {pre + 'set_bytes[0]': 1 << 31})]),
                ('whole words', [('no space', {b + 'space': -1, b + 'lm': None})])]

    step = lambda b, ends: _pre(b, [('pointers', _null(STEP_PTRS + (END_PTRS if ends else ())))] + _geometry(lib) + _ranges())
    model = lambda b: _pre(b, [_model(), _WEIGHTS])
    entries = [('stream_beam', lib.qasr_stream_beam, plain,
                [('struct_size', [('8', dict(struct_size=8))])] + step('', True) + [_beam_state(need)] + _tail() +
                [lm_score('end_lm_score')] + model('') + [_SPACE])]
    b = 'beam.'
    entries.append(('stream_beam_boost', lib.qasr_stream_beam_boost, boost,
                    [('struct_size', [('8', dict(struct_size=8))])] +
                    _pre(b, [('beam_width first', [('0', dict(beam_width=0)), ('129', dict(beam_width=129))]),
                             ('beam.struct_size', [('8', dict(struct_size=8))])]) +
                    [c for c in step(b, True) if c[0] != 'beam_width'] +      # (refused earlier: that line is never reached)
                    _pre(b, [_beam_state(need_b, need)] + _tail() + [lm_score('end_lm_score')]) + model(b) + _pre(b, [_SPACE]) +
                    [('n_sets', [('0', dict(n_sets=0)), ('9', dict(n_sets=9)), ('-1', dict(n_sets=-1))]),
                     ('set pointers', _null(('boost_set', 'end_boost_score')))] +
                    _pre(b, [('space again', [('-2', dict(space=-2, **no_lm)), ('blank', dict(space=BLANK, **no_lm))])]) +
                    sets_loop('', b)))
    b, m = 'boost.beam.', 'boost.'
    for boosted in (True, False):
        n_sets = ('n_sets', [('9', {m + 'n_sets': 9}), ('-1', {m + 'n_sets': -1})])
        checks = ([('struct_size', [('8', dict(struct_size=8))]),
                   ('nested struct_size', [('boost', {m + 'struct_size': 8}), ('beam', {b + 'struct_size': 8})])] +
                  step(b, False) + [n_sets] + _pre(b, [_beam_state(need_b if boosted else need, need if boosted else None)] + _tail()) +
                  [lm_score('cut_lm_score')] + model(b) + _pre(b, [_SPACE]))
        if boosted:
            checks[-1][1].append(('-2, no lm', {b + 'space': -2, b + 'lm': None}))       # the space check is the sets' as well
            checks += [('set pointers', [('boost_set', {m + 'boost_set': None}), ('cut_boost_score', dict(cut_boost_score=None))])] + sets_loop(m, b)
        checks += [('E', [('0', dict(E=0)), ('-1', dict(E=-1)), ('2^30', dict(E=1 << 30)), ('n_best * Pend = 2^31', {b + 'Pend': 1 << 30}),
                          ('B * E * n_best * Pend >= 2^31', dict(E=1 << 26))]),
                   ('cut pointers', _null(CUT_PTRS))]
        entries.append(('stream_beam_ep' if boosted else 'stream_beam_ep (no sets)', lib.qasr_stream_beam_ep, ep(boosted), checks))
    return entries


def entries(lib, engine):
    """[(entry, function, base, checks)]; base() gives a fresh argument block that would pass"""
    return _offline_entries(lib, engine) + _stream_entries(lib, engine)


def cases(lib, engine):
    return driver.cases(entries(lib, engine))


def run(lib, engine):
    return driver.run(lib, entries(lib, engine))
