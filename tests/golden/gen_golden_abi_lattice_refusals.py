#!/usr/bin/env python3
"""Golden fixture of the CTC lattice entry points' refusals: for every case of abi_lattice_refusal_cases the return code and the
text of qasr_last_error, recorded from the library BEFORE its host checks are touched (QASR_LIB names it; default: the one in the
tree), exactly as gen_golden_abi_beam_refusals.py records the beam entries' (its main, with this list of cases).  Host only:
nothing is launched (ctc_star's last case is refused inside launch_star, before its launch).

    python tests/golden/gen_golden_abi_lattice_refusals.py      # -> abi_lattice_refusals.json"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden_abi_beam_refusals as gen  # noqa: E402  (puts the package and tests/ on the path)
import abi_lattice_refusal_cases  # noqa: E402

if __name__ == '__main__':
    gen.main(abi_lattice_refusal_cases, 'abi_lattice_refusals')
