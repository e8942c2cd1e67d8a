"""CPU checks of the C-ABI boundary: the library loads, exports every symbol include/dsnt_hip.h
declares, and its argument validation returns error codes without touching a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, 'include', 'dsnt_hip.h')]          # the product ABI
# the calibration probes and the debug switch the library once carried beside the ABI: gone, and not to come back unnoticed
RETIRED_PROBES = ['dsnt_debug_mfma_peak', 'dsnt_debug_coexec', 'dsnt_debug_bf16_peak', 'dsnt_debug_starve',
                  'dsnt_debug_grid_barrier', 'dsnt_debug_grid_barrier2', 'dsnt_debug_empty', 'dsnt_debug_force_gemm6']
# the list-fusing entry points of the persistent low-resolution stage (measured slower, profiles/r06_stage_ab.txt): removed in 132
RETIRED_STAGE = ['dsnt_list_fuse_bytes', 'dsnt_list_fuse', 'dsnt_list_fuse_plan', 'dsnt_list_stages', 'dsnt_list_stage_errors']


def _declared(headers=HEADERS):
    names = set()
    for h in headers:
        text = open(h).read()
        text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
        names |= set(re.findall(r'\b(dsnt_[a-z0-9_]+)\s*\(', text))
    return sorted(names)


def test_library_exports_every_declared_symbol():
    from dsnt import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), 'libdsnt_hip.so does not export ' + n
    bound = set(_lib.SIGNATURES) | set(_lib.PLAIN)
    assert bound == set(names), (sorted(bound - set(names)), sorted(set(names) - bound))
    assert lib.dsnt_version() >= 100
    # the product header declares no diagnostics, and nothing in the product package binds one at import time
    assert not [n for n in _declared(HEADERS[:1]) if n.startswith('dsnt_debug')]
    for n in RETIRED_PROBES:
        assert not hasattr(lib, n), 'libdsnt_hip.so still exports ' + n


def test_retired_stage_symbols_are_neither_exported_nor_bound():
    from dsnt import _lib
    lib = _lib.load()
    assert lib.dsnt_version() >= 132
    for n in RETIRED_STAGE:
        assert not hasattr(lib, n), 'libdsnt_hip.so still exports ' + n
        assert n not in _lib.SIGNATURES and n not in _lib.PLAIN, 'dsnt._lib still binds ' + n
        assert n not in _declared(), 'include/dsnt_hip.h still declares ' + n


def _prototypes(headers=HEADERS):
    """name -> (return type, [argument types]) of every prototype, as C type strings without the parameter names."""
    protos = {}
    for h in headers:
        text = re.sub(r'/\*.*?\*/', '', open(h).read(), flags=re.S)
        text = re.sub(r'//[^\n]*', '', text)
        text = re.sub(r'^\s*#[^\n]*', '', text, flags=re.M)
        for ret, name, args in re.findall(r'([A-Za-z_][\w\s]*?[\s\*]+)(dsnt_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text):
            types = []
            for a in args.split(','):
                a = ' '.join(a.split())
                if a in ('', 'void'):
                    continue
                types.append(re.sub(r'\s*\b[A-Za-z_]\w*$', '', a).replace(' *', '*'))    # drop the parameter's name
            assert name not in protos, name + ' declared twice'
            protos[name] = (' '.join(ret.split()).replace(' *', '*'), types)
    return protos


def _ctypes_ok(ctype, bound, _lib):
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'float': C.c_float, 'double': C.c_double,
               'uint64_t': C.c_uint64, 'uint32_t': C.c_uint32}
    structs = {'const dsnt_conv_geom*': _lib.GP, 'dsnt_bn_bwd_epilogue*': _lib.BP, 'dsnt_bn_prologue*': _lib.PP,
               'dsnt_out_bounds*': _lib.TP, 'dsnt_bn_bwd_apply*': _lib.AP}
    if ctype in scalars:
        return bound is scalars[ctype]
    for k, v in structs.items():
        if ctype in (k, 'const ' + k):
            return bound is v
    if ctype.endswith('*'):
        return bound in (C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p))
    return False


def test_ctypes_tables_match_the_header_argument_by_argument():
    """A ctypes row of the wrong width or length is silent undefined behaviour: every prototype of include/dsnt_hip.h is parsed
    and held against _lib.SIGNATURES (status return, trailing `void* stream` included) / _lib.PLAIN (return type too)."""
    from dsnt import _lib
    protos = _prototypes()
    bound = set(_lib.SIGNATURES) | set(_lib.PLAIN)
    assert len(protos) == len(bound), (sorted(bound - set(protos)), sorted(set(protos) - bound))    # nothing the regex cannot read
    assert set(protos) == bound
    returns = {'int': C.c_int, 'int64_t': C.c_int64, 'const char*': C.c_char_p, 'void': None}
    for name, (ret, types) in sorted(protos.items()):
        if name in _lib.SIGNATURES:
            assert ret == 'int', (name, ret)
            args = _lib.SIGNATURES[name]
        else:
            res, args = _lib.PLAIN[name]
            want = returns[ret] if ret in returns else C.c_void_p
            assert ret in returns or ret.endswith('*'), (name, ret)
            assert res is want, (name, ret, res)
        assert len(args) == len(types), (name, types, args)
        for i, (t, b) in enumerate(zip(types, args)):
            assert _ctypes_ok(t, b, _lib), '%s: argument %d is `%s` in the header, %r in dsnt._lib' % (name, i, t, b)


def test_argument_validation_without_gpu():
    from dsnt import _lib
    lib = _lib.load()
    g = _lib.ConvGeom(1, 8, 8, 6, 8, 8, 8, 1, 1, 1, 0, 1)       # Cin % 4 != 0
    rc = lib.dsnt_conv_fwd(None, None, None, None, None, None, 0, None, None, None, C.byref(g), None)
    assert rc == 2 and b'multiple of 4' in lib.dsnt_last_error()
    g = _lib.ConvGeom(1, 8, 8, 8, 7, 8, 8, 3, 3, 1, 1, 1)       # inconsistent output size
    rc = lib.dsnt_conv_fwd(None, None, None, None, None, None, 0, None, None, None, C.byref(g), None)
    assert rc == 1 and b'inconsistent' in lib.dsnt_last_error()
    g = _lib.ConvGeom(1, 8, 8, 8, 8, 8, 8, 3, 3, 1, 1, 1)
    rc = lib.dsnt_conv_fwd(None, None, None, None, None, None, 0, None, None, None, C.byref(g), None)
    assert rc == 3 and b'null' in lib.dsnt_last_error()
    # the split-precision entry point checks its arguments through the same helper, in the same order
    fwd6 = lambda g: lib.dsnt_conv_fwd_bf16x6(None, None, 0, None, None, None, None, 0, None, None, None, C.byref(g), None)
    rc = fwd6(_lib.ConvGeom(1, 8, 8, 6, 8, 8, 8, 1, 1, 1, 0, 1))            # Cin % 4 != 0
    assert rc == 2 and b'dsnt_conv_fwd_bf16x6: Cin=6 must be a multiple of 4' in lib.dsnt_last_error()
    rc = fwd6(_lib.ConvGeom(1, 8, 8, 16, 7, 8, 8, 3, 3, 1, 1, 1))           # inconsistent output size
    assert rc == 1 and b'dsnt_conv_fwd_bf16x6: output 7x8 inconsistent' in lib.dsnt_last_error()
    rc = fwd6(_lib.ConvGeom(1, 8, 8, 16, 8, 8, 8, 3, 3, 1, 1, 1))           # a geometry the kernels take, null tensors
    assert rc == 3 and b'dsnt_conv_fwd_bf16x6: null tensor' in lib.dsnt_last_error()
    assert lib.dsnt_head_fwd(None, None, None, 4, 8, 8, None) == 3
    assert lib.dsnt_reg_fwd(None, None, None, 4, 8, 8, 0.1, 9, None) == 3
    assert lib.dsnt_maxpool2_fwd(C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1, 7, 8, 4, None) == 1
    assert lib.dsnt_conv_wgrad_ws_floats(C.byref(g)) > 0
    assert lib.dsnt_conv_fwd_bm(C.byref(g)) in (32, 128)


def _head_refusals():
    """(entry point, arguments without the stream, return code, dsnt_last_error()) of calls the DSNT head's wrappers refuse
    before they touch a device; X is a non-null pointer that is never followed."""
    X, N, big = C.c_void_p(4096), None, 4096            # big x big = 2^24 pixels
    perm3 = C.cast((C.c_int * 3)(0, 2, 1), C.c_void_p)
    twice = C.cast((C.c_int * 3)(0, 0, 1), C.c_void_p)
    perm33 = C.cast((C.c_int * 33)(*range(33)), C.c_void_p)
    rows = []

    def add(name, args, rc, text):
        rows.append((name, args, rc, (name + ': ' + text).encode()))

    def shapes(name, ptrs, tail=(), first=False):
        """rows = 0 and h * w = 2^24 through check_rows; hw-only entry points (first=True) see the map as 1 x hw"""
        hw_ok, hw_big = ((64,), (1 << 24,)) if first else ((8, 8), (big, big))
        add(name, ptrs + (0,) + hw_ok + tail, 1, 'rows=0 out of range')
        add(name, ptrs + (4,) + hw_big + tail, 1, 'bad map size %dx%d' % ((1, 1 << 24) if first else (big, big)))

    add('dsnt_preact_fwd', (N, X, 4, 64, 0, 0., 1e-6), 3, 'null tensor')
    add('dsnt_preact_fwd', (X, X, 4, 64, 5, 0., 1e-6), 3, 'unknown mode 5')
    shapes('dsnt_preact_fwd', (X, X), (0, 0., 1e-6), first=True)
    add('dsnt_preact_bwd', (X, N, X, X, 4, 64, 0, 0., 1e-6), 3, 'null tensor')
    add('dsnt_preact_bwd', (N, X, X, X, 4, 64, 2, 0., 1e-6), 3, 'null tensor')       # modes 2..4 read x
    add('dsnt_preact_bwd', (X, X, X, X, 4, 64, 5, 0., 1e-6), 3, 'unknown mode 5')
    shapes('dsnt_preact_bwd', (N, X, X, X), (0, 0., 1e-6), first=True)
    for name, n in (('dsnt_expect_fwd', 2), ('dsnt_expect_bwd', 2), ('dsnt_head_fwd', 3)):
        add(name, (X,) * (n - 1) + (N, 4, 8, 8), 3, 'null tensor')
        shapes(name, (X,) * n)
    add('dsnt_heatmap_stats', (X, 4, 8, 8, X, N), 3, 'null tensor')
    add('dsnt_heatmap_stats', (X, 0, 8, 8, X, X), 1, 'rows=0 out of range')
    add('dsnt_heatmap_stats', (X, 4, big, big, X, X), 1, 'bad map size 4096x4096')
    for name, n in (('dsnt_make_gauss', 2), ('dsnt_make_gauss_bwd', 3)):
        add(name, (N,) + (X,) * (n - 1) + (4, 8, 8, 1.), 3, 'null tensor')
        add(name, (X,) * n + (4, 8, 8, 0.), 3, 'sigma must be positive')
        shapes(name, (X,) * n, (1.,))
    for name, n in (('dsnt_reg_fwd', 3), ('dsnt_reg_bwd', 4), ('dsnt_reg_bwd_mu', 4)):
        add(name, (X, N) + (X,) * (n - 2) + (4, 8, 8, 1., 0), 3, 'null tensor')          # kinds 0..2 read the target
        shapes(name, (X,) * n, (1., 0))
    add('dsnt_reg_fwd', (X, X, X, 4, 8, 8, 1., 4), 3, 'unknown kind 4')
    add('dsnt_reg_bwd', (X, X, X, X, 4, 8, 8, 1., 4), 3, 'unknown kind 4')
    add('dsnt_reg_bwd_mu', (X, X, X, X, 4, 8, 8, 1., 3), 3, 'kind 3 has no target Gaussian')
    for name, n, tail in (('dsnt_head_loss_rows', 5, (1., 0)), ('dsnt_head_bwd', 7, (1., 0)),
                          ('dsnt_head_loss_grad', 8, (1., 0, 1.))):
        add(name, (N,) + (X,) * (n - 1) + (4, 8, 8) + tail, 3, 'null tensor')
        add(name, (X,) * n + (4, 8, 8, 1., 4) + tail[2:], 3, 'unknown regulariser 4')
        shapes(name, (X,) * n, tail)
    add('dsnt_head_loss_grad', (X,) * 8 + (4, 1, 4097, 1., 0, 1.), 1,
        'heat-maps of up to 4096 pixels (got 1x4097); use dsnt_head_loss_rows + dsnt_head_bwd for larger ones')
    for name, ptrs, tail in (('dsnt_euclid_fwd', 3, (2,)), ('dsnt_euclid_bwd', 5, (2,)), ('dsnt_masked_avg_fwd', 3, ()),
                             ('dsnt_masked_avg_bwd', 4, ()), ('dsnt_fc2_fwd', 4, (64,)), ('dsnt_fc2_bwd', 6, (64,)),
                             ('dsnt_mask_denom', 2, ())):
        add(name, (X,) * ptrs + (0,) + tail, 3, 'bad argument')                          # n = 0 / rows = 0
    add('dsnt_euclid_fwd', (X, X, N, 4, 2), 3, 'bad argument')
    add('dsnt_euclid_bwd', (X, X, X, X, N, 4, 2), 3, 'bad argument')
    add('dsnt_masked_avg_fwd', (N, X, X, 4), 3, 'bad argument')
    add('dsnt_masked_avg_bwd', (N, X, X, X, 4), 3, 'bad argument')
    add('dsnt_fc2_fwd', (X, N, X, X, 4, 64), 3, 'bad argument')
    add('dsnt_fc2_bwd', (X, X, X, X, N, X, 4, 64), 3, 'bad argument')
    add('dsnt_mask_denom', (X, N, 4), 3, 'bad argument')
    add('dsnt_head_loss_reduce', (X, X, X, N, 1., X, X, 4), 3, 'bad argument')
    add('dsnt_head_loss_reduce', (X, X, X, X, 1., X, X, 0), 3, 'bad argument')
    add('dsnt_scale_by_scalar', (X, N, 4), 3, 'null pointer or n <= 0')
    add('dsnt_scale_by_scalar', (X, X, 0), 3, 'null pointer or n <= 0')
    for name, extra in (('dsnt_flip_merge_head', ()), ('dsnt_flip_merge_head_stats', (X, X, X))):
        def flip(B=2, J=3, h=8, w=8, perm=perm3, strategy=0, preact=0, logits=X, extra=extra):
            return (logits, B, J, h, w, perm, strategy, preact, 0., 1e-6, X, X, X, X, X) + extra
        add(name, flip(logits=N), 3, 'null pointer')
        add(name, flip(strategy=2), 3, 'unknown strategy 2')
        add(name, flip(preact=5), 3, 'unknown preact mode 5')
        add(name, flip(J=33, perm=perm33), 1, 'J=33 outside 1..32')
        add(name, flip(B=0), 1, 'B=0 out of range')
        add(name, flip(h=big, w=big), 1, 'bad map size 4096x4096')
        add(name, flip(perm=twice), 3, 'perm is not a permutation of 0..2 (perm[1] = 0)')
    add('dsnt_flip_merge_head_stats', flip(extra=(X, N, X)), 3, 'null pointer')
    return rows


def test_head_wrappers_refuse_bad_arguments_without_gpu():
    """Return code and exact dsnt_last_error() of every DSNT head entry point (head_ops.hip, head_loss.hip, head_fwd.hip) on
    arguments it refuses: null tensors, rows = 0, h * w = 2^24, unknown modes, kinds, regularisers and strategies,
    sigma = 0, rows too long for the fused loss, J = 33 and a non-permutation.  Nothing here reaches a device."""
    from dsnt import _lib
    lib = _lib.load()
    table = _head_refusals()
    moved = [n for n in _lib.SIGNATURES if re.match(
        r'dsnt_(preact|expect|make_gauss|euclid|masked_avg|fc2|reg|head|mask_denom|scale_by_scalar|flip_merge_head|heatmap_stats)', n)]
    assert len(moved) == 25 and set(moved) == {row[0] for row in table}
    for name, args, rc, text in table:
        got = getattr(lib, name)(*args, None)
        assert (got, lib.dsnt_last_error()) == (rc, text), (name, args)


def test_ops_refuse_cpu_tensors():
    import torch
    import dsnt.nn as dn
    from dsnt.model import build_mpii_pose_model
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dn.dsnt(torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dn.euclidean_loss(torch.zeros(2, 3, 2), torch.zeros(2, 3, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dn.js_reg_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 2), 0.1)
    m = build_mpii_pose_model(base='hg1', output_strat='dsnt')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(1, 3, 64, 64))


def test_missing_library_is_loud(monkeypatch):
    from dsnt import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libdsnt_hip.so')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _lib.load()


def test_launch_list_records_instead_of_launching():
    """dsnt_list_*: between begin and end the entry points validate as usual and launch nothing; errors do not record."""
    from dsnt import _lib
    lib = _lib.load()
    h = lib.dsnt_list_create()
    assert h and lib.dsnt_list_size(h) == 0 and lib.dsnt_list_segments(h) == 1
    assert lib.dsnt_list_end() != 0 and b'not recording' in lib.dsnt_last_error()
    assert lib.dsnt_list_begin(h) == 0
    assert lib.dsnt_list_begin(h) != 0                         # one recording per thread
    g = _lib.ConvGeom(1, 8, 8, 6, 8, 8, 8, 1, 1, 1, 0, 1)     # invalid geometry: rejected, nothing recorded
    assert lib.dsnt_conv_fwd(None, None, None, None, None, None, 0, None, None, None, C.byref(g), None) == 2
    assert lib.dsnt_list_size(h) == 0
    # a valid call records one launch without touching a device (pointers are only captured); stream = lane 1
    assert lib.dsnt_axpy(C.c_void_p(4096), C.c_void_p(8192), 1.0, 0, 1024, C.c_void_p(1)) == 0
    assert lib.dsnt_list_size(h) == 1
    assert lib.dsnt_list_mark(h) == 1 and lib.dsnt_list_segments(h) == 2
    assert lib.dsnt_list_end() == 0
    assert lib.dsnt_list_replay(h, 5, None, 3) != 0            # bad arguments are refused before anything is enqueued
    lib.dsnt_list_destroy(h)


def test_no_packed_fp32_instruction_with_crossed_halves_on_its_own_destination():
    """The one instruction form that loses results on gfx950 (profiles/r03_slp_packed_add_hazard.txt: a v_pk_*_f32 whose
    destination pair is also a source pair read with crossed halves — what hipcc's SLP vectoriser makes of adjacent scalar
    sums) must not appear in the shipped library: every translation unit is built with -fno-slp-vectorize (build.py),
    and this disassembles the built code objects to hold it to that."""
    import importlib.util
    import shutil
    if not shutil.which('/opt/rocm/lib/llvm/bin/llvm-objdump'):
        pytest.skip('llvm-objdump not available')
    spec = importlib.util.spec_from_file_location('check_isa', os.path.join(ROOT, 'tools', 'check_isa_packed_f32.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from dsnt import _lib
    total, bad = mod.scan(_lib.LIB_PATH)
    assert not bad, bad[:5]
