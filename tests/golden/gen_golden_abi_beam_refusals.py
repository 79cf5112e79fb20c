#!/usr/bin/env python3
"""Golden fixture of the beam entry points' refusals: for every case of abi_beam_refusal_cases the return code and the text of
qasr_last_error, recorded from the library BEFORE its host checks are touched (QASR_LIB names it; default: the one in the
tree), so that a later library answers each wrong argument block with the same refusal, byte for byte.  Host only: no
call gets as far as a launch.  The texts hold counts and sizes, never an address: two runs must agree.

    python tests/golden/gen_golden_abi_beam_refusals.py      # -> abi_beam_refusals.json"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'q-asr_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import abi_beam_refusal_cases as cases  # noqa: E402
from qasr import engine  # noqa: E402


def main(cases=cases, name='abi_beam_refusals'):
    """(gen_golden_abi_lattice_refusals.py calls this with its own list of cases)"""
    lib = engine.load_library()
    got = cases.run(lib, engine)
    assert got == cases.run(lib, engine), 'the texts differ between two runs'
    with open(os.path.join(HERE, name + '.json'), 'w') as f:
        f.write('{"library": %s, "cases": [\n%s\n]}\n' % (json.dumps(lib.qasr_version().decode()), ',\n'.join(json.dumps(c) for c in got)))
    print(len(got), 'cases,', len({(e.split(' (')[0], t) for e, _, _, t in got}), 'distinct (entry, message) pairs')


if __name__ == '__main__':
    main()
