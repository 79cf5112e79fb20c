"""The wrong values of a qasr_stream_beam_args that qasr_stream_beam, _boost and _ep all refuse (QASR_ERR_ARG, nothing launched):
one list for the three GPU refusal tests, as a function of the plans and the buffers.  Each entry is a dict of fields to set on
an otherwise good struct."""

STEP_POINTERS = ('state', 'beam_state', 'slots', 'flags', 'cand_id', 'cand_q', 'enc_lens', 'first_frame', 'lae_table', 'labels', 'frames',
                 'n_new_labels', 'commit_len', 'n_live', 'status', 'tail_labels', 'tail_n')
END_POINTERS = ('end_labels', 'end_n_labels', 'end_score', 'n_hyps')


def step_mutations(splan, bplan, S, state, bstate, lm_ptr, blank, ends):
    """splan / bplan: the StreamPlan and StreamBeamPlan of the call, state / bstate: its cuda state tensors (int32), lm_ptr: the
    model's device address, ends: the call writes the END outputs (stream_beam_ep does not: it neither requires them nor
    end_lm_score)"""
    W, nb, nbb = bplan.W, state.numel() * 4, bstate.numel() * 4
    return [dict(struct_size=8), dict(B=0), dict(B=S + 1), dict(Wl=0), dict(C=0), dict(samples_per_frame=0), dict(Wl=splan.Wl + 1),
            dict(C=splan.C - 1), dict(Rr=splan.Rr + 1), dict(Rr=splan.Wl), dict(state_bytes=nb - 4), dict(Tw=0), dict(Tw=65537),
            dict(N=0), dict(N=65), dict(beam_width=0), dict(beam_width=129), dict(n_best=0), dict(n_best=W + 1), dict(blank=-1),
            dict(lae_entries=16383), dict(Lg=-1), dict(K=0), dict(K=33), dict(F=bplan.F - 1), dict(F=(1 << 20) + 1),
            dict(beam_state_bytes=nbb - 4), dict(F=bplan.F + 1), dict(state=state.data_ptr() + 4), dict(beam_state=bstate.data_ptr() + 8),
            dict(max_final_frames=0), dict(max_final_frames=splan.Tw + 1), dict(P=bplan.delta_pitch - 1), dict(Ptail=0),
            dict(Pend=bplan.F - 1)] + ([dict(end_lm_score=None)] if ends else []) + \
        [dict(lm_bytes=64), dict(lm=lm_ptr + 4), dict(alpha_q=-1), dict(alpha_q=(16 << 16) + 1), dict(beta_q=-(16 << 16) - 1),
         dict(space=-2), dict(space=blank)] + [{n: None} for n in STEP_POINTERS + (END_POINTERS if ends else ())]
