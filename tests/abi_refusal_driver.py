"""What the refusal case lists of the entry points share (abi_beam_refusal_cases, abi_lattice_refusal_cases): the host buffer that
stands for every pointer, how a mutation is written into a ctypes struct, how a list of entries becomes a list of cases, and the
runner.  Host code only.

An entry is (name, function, base, checks): base() gives a fresh argument block that passes every check; checks is a list, in
the order of the source, of (check, [(mutation, {field: value})]), the mutations being the ones that reach that check's `fail(`
line.  The cases of an entry are (a) every mutation on its own, named `check/mutation`, and (b) for each two checks that follow
one another the first mutation of both at once, named `check+next`: the message must be the earlier check's.  A field that both
mutations set takes the earlier one's value.  The base alone is never passed, so nothing is ever launched."""
import ctypes as C

import numpy as np

_buf = np.zeros(64 + 4, dtype=np.int32)
PTR = (_buf.ctypes.data + 15) & ~15                     # stands for every pointer: a refused call reads none of them


def put(a, path, v):
    """a.path = v; path: dotted fields, the last one possibly indexed ('boost.sets[1]')"""
    *head, last = path.split('.')
    for h in head:
        a = getattr(a, h)
    if last.endswith(']'):
        name, i = last[:-1].split('[')
        getattr(a, name)[int(i)] = v
    else:
        setattr(a, last, v)


def null(names):
    return [(n, {n: None}) for n in names]


def cases(entries):
    """[(entry, case, function, base, mutation)], NULL args first"""
    out = []
    for entry, fn, base, checks in entries:
        out.append((entry, 'args NULL', fn, None, {}))
        for name, muts in checks:
            out += [(entry, f'{name}/{m}', fn, base, kw) for m, kw in muts]
        for (n0, m0), (n1, m1) in zip(checks, checks[1:]):
            out.append((entry, f'{n0}+{n1}', fn, base, {**m1[0][1], **m0[0][1]}))
    return out


def run(lib, entries):
    """Every case's (entry, case, rc, text).  Stops at the first rc that is not 1 (QASR_ERR_ARG): a call that is not refused
    would go on to launch."""
    got = []
    for entry, case, fn, base, kw in cases(entries):
        assert kw or base is None, (entry, case)                   # the base alone is never passed
        if base is None:
            rc = fn(None, None)
        else:
            a = base()
            for path, v in kw.items():
                put(a, path, v)
            rc = fn(None, C.byref(a))
        text = lib.qasr_last_error().decode()
        assert rc == 1, f'{entry}: {case}: rc {rc} ({text!r} is the last error)'
        got.append([entry, case, rc, text])
    return got
