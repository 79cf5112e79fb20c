"""Which check of the seven CTC lattice entry points refuses a wrong argument block, and in which words: every case of
abi_lattice_refusal_cases against tests/golden/abi_lattice_refusals.json, recorded before the checks were shared.  Host code
only; it runs where no GPU is, because a check that went missing would let a call through to a launch on host memory."""
import json
import os

import pytest

import abi_lattice_refusal_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(os.path.exists('/dev/kfd'), reason='never next to a GPU: an argument block that slips through would launch on host memory')
def test_lattice_refusals_match_the_recorded_ones():
    from qasr import engine
    lib = engine.load_library()
    with open(os.path.join(HERE, 'golden', 'abi_lattice_refusals.json')) as f:
        want = json.load(f)['cases']
    got = cases.run(lib, engine)                             # stops at the first call that is not refused
    assert [c[:2] for c in got] == [c[:2] for c in want], 'the fixture is of another list of cases: run gen_golden_abi_lattice_refusals.py on the PARENT library'
    for g, w in zip(got, want):
        assert g[2] == w[2] and g[3].encode() == w[3].encode(), (g, w)
    # (a) every check is reached by a case of its own; (b) every pair of neighbours answers with the earlier one's text
    for entry, _, _, checks in cases.entries(lib, engine):
        text = {c[1]: c[3] for c in got if c[0] == entry}
        firsts = [text[f'{name}/{muts[0][0]}'] for name, muts in checks]
        words = lambda t: ''.join(ch for ch in t if not ch.isdigit() and ch != '-')
        for (n0, _), (n1, _), t0 in zip(checks, checks[1:], firsts):
            assert words(text[f'{n0}+{n1}']) == words(t0), (entry, n0, n1)
        for (name, muts), t0 in zip(checks, firsts):
            assert all(words(text[f'{name}/{m}']) == words(t0) for m, _ in muts), (entry, name)  # one check, one message (numbers apart)
