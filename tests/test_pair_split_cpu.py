"""qasr_engine_opts.pair_split and the `pair` argument of qasr_sep_layer, as far as they go without a GPU: the option's default
and place in the struct, and the shapes the operator entry refuses before any HIP call."""
import ctypes as C

import pytest


@pytest.fixture(scope='module')
def lib():
    from qasr import build
    lib = C.CDLL(build.build_native())
    lib.qasr_last_error.restype = C.c_char_p
    return lib


def test_default_opts_carry_pair_split(lib):
    from qasr import engine
    o = engine.EngineOpts()
    lib.qasr_engine_default_opts(C.byref(o))
    assert o.pair_split == -1 and o.mask_skip == -1
    assert o.struct_size == C.sizeof(engine.EngineOpts) == 64           # the field took the reserved word: same size
    assert engine.EngineOpts.pair_split.offset == 60


def _args(engine, keep, K=75, cin=512, cout=512, Tp=256, tile=128, gen=2):
    a = engine.SepLayerArgs()
    a.B, a.T, a.Tp, a.cin, a.cout, a.K, a.dilation, a.tile, a.gen = 2, Tp - 6, Tp, cin, cout, K, 1, tile, gen
    buf = C.create_string_buffer(4096)                        # never dereferenced: the entry refuses before any launch
    keep.append(buf)
    p = C.addressof(buf)
    for n in ('x', 'wdw', 'wdw2', 'bias_dw', 'm_dw', 'w', 'bias', 'lens'):
        setattr(a, n, p)
    a.n_outs = 1
    a.outs[0].ptr, a.outs[0].mtab, a.outs[0].mode, a.outs[0].lo, a.outs[0].hi = p, p, 1, 0, 255
    a.dw_lo, a.dw_hi = -128, 127
    a.pair = 1
    return a


@pytest.mark.parametrize('change', [dict(K=33, cin=256, cout=256), dict(K=51, cin=256), dict(tile=64), dict(tile=32), dict(Tp=192),
                                    dict(gen=1), dict(gen=3), dict(K=0), 'hooks', 'dilation2', 'resadd'])
def test_operator_entry_refuses_pair_without_a_paired_form(lib, change):
    from qasr import engine
    keep = []
    a = _args(engine, keep, **(change if isinstance(change, dict) else {}))
    p = C.addressof(keep[0])
    if change == 'hooks':
        a.acc = p
    elif change == 'dilation2':
        a.K, a.dilation = 87, 2
    elif change == 'resadd':
        a.flags = 16                                           # QASR_F_RESADD with its operands
        for n in ('rx', 'rw', 'rbias', 'rm', 'm_main'):
            setattr(a, n, p)
        a.rcin = 512
    lib.qasr_sep_layer.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    assert lib.qasr_sep_layer(None, C.byref(a), None, 0) == 4, lib.qasr_last_error()      # QASR_ERR_UNSUPPORTED
    assert b'paired' in lib.qasr_last_error()


def test_pair_workspace_sizes(lib):
    lib.qasr_sep_pair_workspace_bytes.restype = C.c_size_t
    lib.qasr_sep_pair_timeout_offset.restype = C.c_size_t
    assert lib.qasr_sep_pair_workspace_bytes(32, 256) == 512 + 256 + 32 * 2 * 65536     # flags, time-out word, 64 KiB per tile
    assert lib.qasr_sep_pair_timeout_offset(32, 256) == 512
    assert lib.qasr_sep_pair_workspace_bytes(3, 192) == 0 and lib.qasr_sep_pair_workspace_bytes(0, 256) == 0
