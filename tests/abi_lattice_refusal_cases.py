"""The refusals of the seven CTC lattice entry points (qasr_ctc_align, _post, _align_band, _post_band, _star, _spot and
qasr_stream_spot), case by case: which check fires and what qasr_last_error says.  Host code only: ctypes structs of qasr.engine
filled by hand, one 16-byte-aligned host buffer standing for every pointer, stream NULL.  Every argument block is a base that
passes all checks with mutations on top; the base alone is never passed, so nothing is ever launched.

An entry is a list of checks in the order of the source, one per `fail(` line that the entry reaches (its helpers' lines and
stream_geometry's five as stream_spot reaches them included); a check is a list of mutations that reach that line.  How the
entries become cases and the runner are abi_refusal_driver's.  The last check of ctc_star is its launch refusal: launch_star
counts the work-groups of B * T frames on the host and returns before it launches when they are more than INT_MAX.  Its NaN
penalty is a check of its own only because `%g` prints "nan" where the other two cases print a number: it is the same line.

ctc_align and ctc_align_band take their struct in two sizes.  A few later mutations are repeated with struct_size set to the
shorter (V1) size, inside the same check, so the same text must come back; a size that is neither is refused.  That the V1 size
ignores the two star fields is NOT shown here: the star check is the last one before the launch, so no refused call can tell the
difference; test_gpu_star.py shows it with real launches.

tests/golden/gen_golden_abi_lattice_refusals.py records (entry, case, rc, text); test_abi_lattice_refusals_cpu.py compares."""
import ctypes as C

import abi_refusal_driver as driver
from abi_beam_refusal_cases import CH, RR, S, SPF, TW, WL, _geometry        # the session of the streaming beam cases (B is 2 there too)
from abi_refusal_driver import PTR, null

B, T, CN, K, ML = 2, 6, 5, 2, 3
P, BLANK = B * K, CN - 1
LAE = 16384                                             # QASR_BEAM_TABLE_ENTRIES
BEAM_T, BAND_T = 65536, 1 << 22                         # QASR_BEAM_MAX_FRAMES, QASR_BAND_MAX_FRAMES
ALIGN_ML, BAND_ML, SPOT_ML = 2048, 1 << 20, 127         # QASR_ALIGN_ / BAND_ / SPOT_MAX_LABELS
MIN_THR, MAX_SPAN = -(16 << 16), 65536                  # QASR_SPOT_MIN_THRESHOLD_Q, QASR_SPOT_MAX_SPAN
PH, MFF = 4, 10
BIG = (1 << 31) - 1

FIVE = ('log_probs', 'targets', 'target_lens', 'workspace', 'ok')
_SIZE = ('struct_size', [('8', dict(struct_size=8))])
_BLANK = lambda c='C': ('blank', [('-1', dict(blank=-1)), (c, dict(blank=CN))])
_PITCH = lambda t=T: ('pitch', [('pitch_frame=C-1', dict(pitch_frame=CN - 1)), ('pitch_utt=T*pitch_frame-1', dict(pitch_utt=t * CN - 1))])
_STAR = lambda t=T: ('star_pitch', [('T-1', dict(star_pitch=t - 1))])
_LABELS = lambda cap: ('max_labels', [('0', dict(max_labels=0)), ('cap+1', dict(max_labels=cap + 1))])


def _base(cls, ptrs, **fields):
    def make():
        a = cls()
        a.struct_size = C.sizeof(cls)
        a.pitch_utt, a.pitch_frame = fields.get('Tw', T) * CN, CN
        for n in ptrs:
            setattr(a, n, PTR)
        for n, v in fields.items():
            setattr(a, n, v)
        return a
    return make


def _v1(cls, checks, names):
    """the first mutation of the named checks once more under the shorter struct's size"""
    v1 = getattr(cls, 'star_logp').offset
    for name, muts in checks:
        if name in names:
            muts.append((muts[0][0] + ', V1 size', dict(muts[0][1], struct_size=v1)))
    return checks


def _two_sizes(cls):
    v1 = getattr(cls, 'star_logp').offset
    assert C.sizeof(cls) == v1 + 16
    return ('struct_size', [('8', dict(struct_size=8)), ('V1+8', dict(struct_size=v1 + 8)), ('full+8', dict(struct_size=v1 + 24))])


def _shape(cap, k=True):
    muts = [('B=0', dict(B=0)), ('T=0', dict(T=0)), ('T=cap+1', dict(T=cap + 1)), ('C=0', dict(C=0))]
    return ('shape', muts + ([('K=0', dict(K=0))] if k else []))


def _post_tail(need):
    return [('lae', [('no table', dict(lae_table=None)), ('16383', dict(lae_entries=LAE - 1))]),
            ('post_pitch', [('T-1', dict(post_pitch=T - 1))]),
            ('workspace alignment', [('by 4', dict(workspace=PTR + 4))]),
            ('workspace', [('need-1', dict(workspace_bytes=need - 1))])]


def _spot_ranges():
    return [('threshold_q', [('1', dict(threshold_q=1)), ('min-1', dict(threshold_q=MIN_THR - 1))]),
            ('max_span', [('0', dict(max_span=0)), ('cap+1', dict(max_span=MAX_SPAN + 1))])]


def entries(lib, engine):
    """[(entry, function, base, checks)]; base() gives a fresh argument block that would pass"""
    out = []

    need = lib.qasr_ctc_align_workspace_bytes(P, T, ML)
    assert need > 0
    cls = engine.AlignArgs
    base = _base(cls, FIVE + ('lens', 'lae_table', 'start', 'nframes', 'score', 'path_score', 'total', 'star_logp'),
                 B=B, T=T, C=CN, P=P, K=K, blank=BLANK, max_labels=ML, lae_entries=LAE, workspace_bytes=need, star_pitch=T)
    out.append(('ctc_align', lib.qasr_ctc_align, base, _v1(cls, [
        _two_sizes(cls), ('pointers', null(FIVE)), _shape(BEAM_T), ('P', [('B*K+1', dict(P=P + 1))]), _LABELS(ALIGN_ML), _BLANK(), _PITCH(),
        ('total', [('no table', dict(lae_table=None))]), ('lae_entries', [('16383', dict(lae_entries=LAE - 1))]),
        ('workspace', [('need-1', dict(workspace_bytes=need - 1))]), _STAR()], ('pointers', 'P', 'blank', 'total', 'workspace'))))

    need = lib.qasr_ctc_post_workspace_bytes(P, T)
    assert need > 0
    more = ('start', 'nframes', 'frame_post', 'label_post')
    base = _base(engine.PostArgs, FIVE + more + ('lens', 'lae_table', 'ok_in', 'total', 'star_logp'),
                 B=B, T=T, C=CN, P=P, K=K, blank=BLANK, max_labels=ML, lae_entries=LAE, workspace_bytes=need, post_pitch=T, star_pitch=T)
    out.append(('ctc_post', lib.qasr_ctc_post, base,
                [_SIZE, ('pointers', null(FIVE)), ('more pointers', null(more)), _shape(BEAM_T), ('P', [('B*K+1', dict(P=P + 1))]),
                 _LABELS(ALIGN_ML), _BLANK(), _PITCH()] + _post_tail(need) + [_STAR()]))

    need = lib.qasr_ctc_align_band_workspace_bytes(B, T, 256)
    assert need > 0
    cls = engine.AlignBandArgs
    base = _base(cls, FIVE + ('lens', 'start', 'nframes', 'score', 'path_score', 'frame_logp', 'band_base', 'star_logp'),
                 B=B, T=T, C=CN, blank=BLANK, max_labels=ML, band_states=256, workspace_bytes=need, star_pitch=T)
    band = lambda: ('band_states', [('512', dict(band_states=512))])         # (fresh: _v1 appends to its list)
    out.append(('ctc_align_band', lib.qasr_ctc_align_band, base, _v1(cls, [
        _two_sizes(cls), ('pointers', null(FIVE)), band(), _shape(BAND_T, k=False), _LABELS(BAND_ML), _BLANK(), _PITCH(),
        ('workspace alignment', [('by 2', dict(workspace=PTR + 2))]), ('workspace', [('need-1', dict(workspace_bytes=need - 1))]), _STAR()],
        ('pointers', 'band_states', 'max_labels', 'workspace alignment', 'workspace'))))

    need = lib.qasr_ctc_post_band_workspace_bytes(B, T)
    assert need > 0
    more = ('start', 'nframes', 'band_base', 'frame_post', 'label_post')
    base = _base(engine.PostBandArgs, FIVE + more + ('lens', 'lae_table', 'ok_in', 'total', 'star_logp'),
                 B=B, T=T, C=CN, blank=BLANK, max_labels=ML, band_states=256, lae_entries=LAE, workspace_bytes=need, post_pitch=T,
                 star_pitch=T)
    out.append(('ctc_post_band', lib.qasr_ctc_post_band, base,
                [_SIZE, ('pointers', null(FIVE)), ('more pointers', null(more)), band(), _shape(BAND_T, k=False), _LABELS(BAND_ML), _BLANK(),
                 _PITCH()] + _post_tail(need) + [_STAR()]))

    base = _base(engine.StarArgs, ('log_probs', 'lens', 'star'), B=B, T=T, C=CN, penalty=0.5, star_pitch=T)
    out.append(('ctc_star', lib.qasr_ctc_star, base,
                [_SIZE, ('pointers', null(('log_probs', 'star'))), ('shape', [('B=0', dict(B=0)), ('T=0', dict(T=0)), ('C=0', dict(C=0))]),
                 _PITCH(), _STAR(), ('penalty', [('-0.5', dict(penalty=-0.5)), ('16.5', dict(penalty=16.5))]),
                 ('penalty NaN', [('nan', dict(penalty=float('nan')))]),
                 ('launch', [('B=T=2^31-1', dict(B=BIG, T=BIG, C=1, pitch_frame=1, pitch_utt=BIG, star_pitch=BIG))])]))

    ins = ('log_probs', 'star_logp', 'targets', 'target_lens')
    outs = ('hit_start', 'hit_end', 'hit_score', 'n_hits', 'ok')
    base = _base(engine.SpotArgs, ins + outs + ('lens', 'trace_score', 'trace_start'), B=B, T=T, C=CN, K=K, max_labels=ML, blank=BLANK,
                 threshold_q=-(1 << 16), max_span=T, max_hits=4, star_pitch=T, trace_pitch=T)
    out.append(('ctc_spot', lib.qasr_ctc_spot, base,
                [_SIZE, ('pointers', null(ins)), ('output pointers', null(outs)), _shape(BAND_T),
                 ('B*K', [('2^31', dict(B=65536, K=32768))]), _LABELS(SPOT_ML), _BLANK(), _STAR(), _PITCH()] + _spot_ranges() +
                [('max_hits', [('0', dict(max_hits=0))]),
                 ('trace pair', [('no trace_start', dict(trace_start=None)), ('no trace_score', dict(trace_score=None))]),
                 ('trace_pitch', [('T-1', dict(trace_pitch=T - 1))])]))

    ins = ('state', 'spot_state', 'slots', 'flags', 'log_probs', 'star_logp', 'enc_lens', 'first_frame', 'emit_status', 'targets',
           'target_lens')
    outs = ('hit_start', 'hit_end', 'hit_detect', 'hit_score', 'n_new_hits', 'n_hits_total', 'open_start', 'open_end', 'open_score',
            'ok', 'status')
    need = lib.qasr_stream_spot_state_bytes(S, K, ML)
    assert need > 0 and lib.qasr_stream_state_bytes(S, WL, CH) > 0
    base = _base(engine.StreamSpotArgs, ins + outs, S=S, B=B, Wl=WL, C=CH, Rr=RR, samples_per_frame=SPF, Tw=TW, n_classes=CN, K=K,
                 max_labels=ML, blank=BLANK, threshold_q=-(1 << 16), max_span=TW, PH=PH, max_final_frames=MFF, star_pitch=TW,
                 state_bytes=lib.qasr_stream_state_bytes(S, WL, CH), spot_state_bytes=need)
    out.append(('stream_spot', lib.qasr_stream_spot, base,
                [_SIZE, ('pointers', null(ins)), ('output pointers', null(outs))] + _geometry(lib) +
                [('Tw, n_classes, K', [('Tw=0', dict(Tw=0)), ('n_classes=0', dict(n_classes=0)), ('K=0', dict(K=0))]),
                 ('B*K', [('2^31', dict(K=1 << 30))]), _LABELS(SPOT_ML), _BLANK('n_classes'), _STAR(TW), _PITCH(TW)] + _spot_ranges() +
                [('PH', [('0', dict(PH=0))]),
                 ('max_final_frames', [('0', dict(max_final_frames=0)), ('Tw+1', dict(max_final_frames=TW + 1))]),
                 ('spot_state_bytes', [('need-1', dict(spot_state_bytes=need - 1)), ('16', dict(spot_state_bytes=16))]),
                 ('alignment', [('state', dict(state=PTR + 4)), ('spot_state', dict(spot_state=PTR + 8))])]))
    return out


def cases(lib, engine):
    return driver.cases(entries(lib, engine))


def run(lib, engine):
    return driver.run(lib, entries(lib, engine))
