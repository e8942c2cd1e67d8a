"""CPU checks of the weight-gradient dispatch (csrc/conv_wgrad.hip): what the dsnt_conv_wgrad* entry points refuse, with which
code and text, in which order; how many launches a valid call records on each of its four routes; and that every query about a
geometry — route, slab count, workspace size — describes the same plan, the one tests/plan_ref.py and tests/wgrad_group_ref.py
restate.  Nothing here reaches a device: the library assumes 256 CUs without one, pointers are fake and never followed."""
import ctypes as C
import itertools

import pytest

import plan_ref as P
import wgrad_group_ref as G

X, BAD, NUL = C.c_void_p(4096), C.c_void_p(4096 + 4), None
SHARE, NARROW = 2, 4                                # DSNT_WGRAD_SHARE_CHIP, DSNT_WGRAD_NARROW
FLAGS = (0, 1, SHARE, SHARE | NARROW)
# one geometry per route of dsnt_conv_wgrad_f16x3, as (N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil), under the value
# dsnt_conv_f16x3_route(g, 1) gives it: 1 the stem kernel, 2 the halo kernel, 3 the 1x1 kernel, 0 the implicit GEMM
ROUTES = {
    1: (1, 5, 33, 16, 4, 32, 64, 4, 4, 1, 1, 1),
    2: (2, 16, 16, 64, 16, 16, 64, 3, 3, 1, 1, 1),
    3: (1, 128, 128, 64, 128, 128, 64, 1, 1, 1, 0, 1),
    0: (1, 8, 8, 8, 8, 8, 8, 3, 3, 1, 1, 1),
}
FIELDS = ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'R', 'S', 'stride', 'pad', 'dil')


def _geom(t, **change):
    from dsnt._lib import ConvGeom
    d = dict(zip(FIELDS, t))
    d.update(change)
    return ConvGeom(*[d[f] for f in FIELDS])


def _wgrad_args(g, x=X, sc=NUL, sh=NUL, dy=X, ws=X, dw=X, db=NUL, acc=0):
    return (x, sc, sh, 1, dy, ws, dw, db, acc, None if g is None else C.byref(g))


def _f16x3_args(g, ab=X, gb=X, **kw):
    a = _wgrad_args(g, **kw)
    return a[:9] + (ab, gb) + a[9:]


def _wgrad_refusals():
    """(entry point, arguments without the stream, return code, dsnt_last_error()) of calls the weight-gradient entry points
    refuse, in the order of their checks.  The descriptor entry points return minus the code."""
    rows = []
    unsupported = 'geometry not supported (need Wo % 4 == 0, tensors < 2 GiB)'

    def add(name, args, rc, text, who=None):
        rows.append((name, args, rc, ((who or name) + ': ' + text).encode()))

    # dsnt_conv_wgrad_f16x3: dsnt_conv_wgrad_bf16x6_ok and the bounds before the route, then the checks of the route.  The
    # implicit GEMM reports as dsnt_conv_wgrad, and so does everything an inconsistent geometry falls through to
    name = 'dsnt_conv_wgrad_f16x3'
    for route, t in ROUTES.items():
        who = 'dsnt_conv_wgrad' if route == 0 else name
        g = _geom(t)
        add(name, _f16x3_args(_geom(t, W=t[2] + 1, Wo=t[5] + 1)), 1, unsupported)                  # Wo % 4 != 0
        add(name, _f16x3_args(_geom(t, W=t[2] + 1, Wo=t[5] + 1), ab=NUL), 1, unsupported)          # ... comes before the bounds
        add(name, _f16x3_args(g, ab=NUL), 3, 'both operand bounds are required')
        add(name, _f16x3_args(g, gb=NUL, x=NUL), 3, 'both operand bounds are required')            # ... before the tensors
        add(name, _f16x3_args(_geom(t, Cin=6)), 1, unsupported)                                    # Cin % 4 != 0
        add(name, _f16x3_args(_geom(t, Ho=t[4] + 4), x=NUL), 1,
            'output %dx%d inconsistent with input/filter (expected %dx%d)' % (t[4] + 4, t[5], t[4], t[5]), who='dsnt_conv_wgrad')
        for miss in ('x', 'dy', 'ws'):
            add(name, _f16x3_args(g, **{miss: NUL}), 3, 'null tensor', who=who)
        add(name, _f16x3_args(g, x=NUL, dw=NUL, db=X), 3, 'null tensor', who=who)                  # ... before dbias
        add(name, _f16x3_args(g, dw=NUL, db=X), 3, 'dbias without dw', who=who)
        add(name, _f16x3_args(g, dw=NUL, db=X, sc=X), 3, 'dbias without dw', who=who)              # ... before the prologue
        pair = 'the 4x4 / 16 -> 64 stem geometry takes a raw operand only' if route == 1 else 'in_scale/in_shift must be given together'
        add(name, _f16x3_args(g, sc=X), 3, pair, who=who)
        add(name, _f16x3_args(g, sh=X, x=BAD), 3, pair, who=who)                                   # ... before the alignment
        if route == 1:
            add(name, _f16x3_args(g, sc=X, sh=X), 3, pair, who=who)                                # a whole prologue on the stem
        for mis in ('x', 'dy', 'ws', 'dw'):
            add(name, _f16x3_args(g, **{mis: BAD}), 2, 'tensors must be 16-byte aligned', who=who)
    add(name, _f16x3_args(None), 1, unsupported)
    # (the 1x1 plan does not look at the dilation: the one geometry check that fails on a route of its own)
    add(name, _f16x3_args(_geom(ROUTES[3], dil=0)), 1, 'non-positive dimension')

    # dsnt_conv_wgrad and dsnt_conv_wgrad_bf16x6: always the implicit GEMM, both report as dsnt_conv_wgrad
    t = ROUTES[0]
    g = _geom(t)
    who = 'dsnt_conv_wgrad'
    add('dsnt_conv_wgrad', _wgrad_args(None), 3, 'null geometry')
    add('dsnt_conv_wgrad', _wgrad_args(_geom(t, N=0)), 1, 'non-positive dimension')
    add('dsnt_conv_wgrad', _wgrad_args(_geom(t, Cin=6)), 2, 'Cin=6 must be a multiple of 4')
    add('dsnt_conv_wgrad', _wgrad_args(_geom(t, Cout=6)), 2, 'Cout=6 must be a multiple of 4')
    add('dsnt_conv_wgrad', _wgrad_args(_geom(t, H=7, W=7, Ho=7, Wo=7), x=NUL), 3, 'null tensor')   # Wo % 4 != 0 is fine in fp32
    add('dsnt_conv_wgrad_bf16x6', _wgrad_args(None), 1, unsupported)
    add('dsnt_conv_wgrad_bf16x6', _wgrad_args(_geom(t, Cin=6)), 1, unsupported)
    add('dsnt_conv_wgrad_bf16x6', _wgrad_args(_geom(t, H=7, W=7, Ho=7, Wo=7)), 1, unsupported)
    add('dsnt_conv_wgrad_bf16x6', _wgrad_args(_geom(t, N=1 << 21, Cin=4)), 1, unsupported)         # 2^31 bytes of x
    for name in ('dsnt_conv_wgrad', 'dsnt_conv_wgrad_bf16x6'):
        add(name, _wgrad_args(_geom(t, Ho=12), x=NUL), 1, 'output 12x8 inconsistent with input/filter (expected 8x8)', who=who)
        for miss in ('x', 'dy', 'ws'):
            add(name, _wgrad_args(g, **{miss: NUL}), 3, 'null tensor', who=who)
        add(name, _wgrad_args(g, dw=NUL, db=X, sc=X), 3, 'dbias without dw', who=who)
        add(name, _wgrad_args(g, sc=X, x=BAD), 3, 'in_scale/in_shift must be given together', who=who)
        add(name, _wgrad_args(g, sh=X), 3, 'in_scale/in_shift must be given together', who=who)
        for mis in ('x', 'dy', 'ws', 'dw'):
            add(name, _wgrad_args(g, **{mis: BAD}), 2, 'tensors must be 16-byte aligned', who=who)

    # the descriptors of the grouped launch: the geometry check, then one text for everything else
    out = C.cast(C.create_string_buffer(256), C.c_void_p)
    for name, nb, needs in (('dsnt_conv_wgrad_desc', 0, 'in_scale/in_shift and a geometry'),
                            ('dsnt_conv_wgrad_desc_f16x3', 2, 'in_scale/in_shift, both operand bounds and a geometry')):
        text = 'needs x, dy, ws (16-byte aligned), %s dsnt_conv_wgrad_bf16x6_ok accepts' % needs

        def desc(g, x=X, sc=X, sh=X, dy=X, ws=X, ab=X, gb=X, out=out, nb=nb):
            return (x, sc, sh, 1, dy, ws) + (ab, gb)[:nb] + (None if g is None else C.byref(g), out)
        add(name, desc(None), -3, 'null geometry')
        add(name, desc(_geom(t, Cin=6), x=NUL), -2, 'Cin=6 must be a multiple of 4')
        add(name, desc(_geom(t, Ho=12)), -1, 'output 12x8 inconsistent with input/filter (expected 8x8)')
        for miss in ('x', 'dy', 'ws', 'sc', 'sh', 'out') + ('ab', 'gb')[:nb]:
            add(name, desc(g, **{miss: NUL}), -3, text)
        for mis in ('x', 'dy', 'ws'):
            add(name, desc(g, **{mis: BAD}), -3, text)
        add(name, desc(_geom(t, H=7, W=7, Ho=7, Wo=7)), -3, text)

    for name in ('dsnt_conv_wgrad_group', 'dsnt_wgrad_reduce_all'):
        for args in ((NUL, 1, 1), (X, 0, 1), (X, 65536, 1), (X, 1, 0)):
            add(name, args, 3, 'bad argument')
    return rows


def test_weight_gradient_entry_points_refuse_bad_arguments_without_gpu():
    """Return code and exact dsnt_last_error() of every refusal of dsnt_conv_wgrad, _bf16x6, _f16x3 (on each of its four routes),
    _desc, _desc_f16x3, _group and dsnt_wgrad_reduce_all; rows that break two rules at once hold the order of the checks."""
    from dsnt import _lib
    lib = _lib.load()
    for route, t in ROUTES.items():
        assert lib.dsnt_conv_f16x3_route(C.byref(_geom(t)), 1) == route
    table = _wgrad_refusals()
    assert {row[0] for row in table} == {'dsnt_conv_wgrad', 'dsnt_conv_wgrad_bf16x6', 'dsnt_conv_wgrad_f16x3', 'dsnt_conv_wgrad_desc',
                                         'dsnt_conv_wgrad_desc_f16x3', 'dsnt_conv_wgrad_group', 'dsnt_wgrad_reduce_all'}
    for name, args, rc, text in table:
        stream = () if 'desc' in name else (None,)
        got = getattr(lib, name)(*args, *stream)
        assert (got, lib.dsnt_last_error()) == (rc, text), (name, args)


def test_weight_gradient_calls_record_one_launch_or_two():
    """Between dsnt_list_begin and dsnt_list_end a valid call returns 0 and records the kernel of its route, and the slab
    reduction behind it where dw is given; a refused call records nothing; a descriptor is filled without a launch."""
    from dsnt import _lib
    lib = _lib.load()
    h = lib.dsnt_list_create()
    assert lib.dsnt_list_begin(h) == 0
    try:
        def recorded(rc_want, name, *args):
            before = lib.dsnt_list_size(h)
            rc = getattr(lib, name)(*args)
            assert (rc == 0) == (rc_want == 0), (name, rc, lib.dsnt_last_error())
            return lib.dsnt_list_size(h) - before

        for (route, t), acc in itertools.product(ROUTES.items(), FLAGS):
            g = _geom(t)
            assert recorded(0, 'dsnt_conv_wgrad_f16x3', *_f16x3_args(g, dw=NUL, acc=acc), None) == 1, (route, acc)
            assert recorded(0, 'dsnt_conv_wgrad_f16x3', *_f16x3_args(g, db=X, acc=acc), None) == 2, (route, acc)
            if route != 1:
                assert recorded(0, 'dsnt_conv_wgrad_f16x3', *_f16x3_args(g, sc=X, sh=X, acc=acc), None) == 2, (route, acc)
            assert recorded(3, 'dsnt_conv_wgrad_f16x3', *_f16x3_args(g, ws=NUL, acc=acc), None) == 0
            assert recorded(2, 'dsnt_conv_wgrad_f16x3', *_f16x3_args(g, dw=BAD, acc=acc), None) == 0
        g = _geom(ROUTES[0])
        for name, acc in itertools.product(('dsnt_conv_wgrad', 'dsnt_conv_wgrad_bf16x6'), FLAGS):
            assert recorded(0, name, *_wgrad_args(g, dw=NUL, acc=acc), None) == 1
            assert recorded(0, name, *_wgrad_args(g, sc=X, sh=X, db=X, acc=acc), None) == 2
            assert recorded(3, name, *_wgrad_args(g, dy=NUL, acc=acc), None) == 0
        nbytes = lib.dsnt_conv_wgrad_desc_bytes()
        out = C.create_string_buffer(nbytes)
        before = lib.dsnt_list_size(h)
        for t in ROUTES.values():
            g, blocks = _geom(t), G.plan(_case9(t))
            blocks = blocks[0] * blocks[1] * blocks[2]
            assert lib.dsnt_conv_wgrad_desc(X, X, X, 1, X, X, C.byref(g), out) == blocks
            assert lib.dsnt_conv_wgrad_desc_f16x3(X, X, X, 1, X, X, X, X, C.byref(g), out) == blocks
        assert lib.dsnt_list_size(h) == before
        assert recorded(0, 'dsnt_conv_wgrad_group', X, 4, 16, None) == 1
        assert recorded(0, 'dsnt_wgrad_reduce_all', X, 4, 16, None) == 1
        assert recorded(3, 'dsnt_conv_wgrad_group', X, 0, 16, None) == 0
        assert recorded(3, 'dsnt_wgrad_reduce_all', NUL, 4, 16, None) == 0
    finally:
        assert lib.dsnt_list_end() == 0
        lib.dsnt_list_destroy(h)


def _case9(t):
    """(N, H, W, Cin, Cout, k, stride, pad, dil) of tests/wgrad_group_ref.py from the twelve fields."""
    N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil = t
    assert R == S and G.out_hw((N, H, W, Cin, Cout, R, stride, pad, dil)) == (Ho, Wo)
    return N, H, W, Cin, Cout, R, stride, pad, dil


def _fields(N, H, W, Cin, Cout, k, stride):
    pad = k // 2
    Ho, Wo = G.out_hw((N, H, W, Cin, Cout, k, stride, pad, 1))
    return N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, 1


CHANNELS = [(8, 8), (64, 64), (96, 64), (64, 128), (128, 64), (128, 128), (256, 128), (128, 256)]
GRID = [_fields(N, HW, HW, Cin, Cout, k, stride)
        for N in (1, 2, 32) for HW in (4, 6, 8, 16, 32, 64, 128) for Cin, Cout in CHANNELS for k, stride in ((1, 1), (3, 1), (3, 2))]
GRID += [(N, Ho + 1, Wo + 1, 16, Ho, Wo, 64, 4, 4, 1, 1, 1) for N in (1, 32) for Ho, Wo in ((4, 32), (128, 128))]       # the stem
# a tensor of exactly 2^31 bytes: one byte past what 32-bit byte offsets address (x, then dy; 1x1 and 3x3)
GRID += [_fields(32, 128, 128, Cin, Cout, k, 1) for Cin, Cout in ((1024, 64), (64, 1024)) for k in (1, 3)]


def test_every_query_describes_the_plan_of_the_launch():
    """Over production and edge geometries and every value of the `accumulate` flags: the workspace of dsnt_conv_wgrad_f16x3 is its
    slabs, dsnt_conv_wgrad_ws_floats covers it and the fp32 / bf16x6 plan, the route is the one tests/plan_ref.py derives,
    dsnt_conv_wgrad_halo_ok names route 2, and the slab count is that of the restated plan of the route's kernel."""
    from dsnt import _lib
    lib = _lib.load()
    seen = set()
    for t in GRID:
        N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil = t
        g, K = _geom(t), R * S * Cin
        case5, case9 = (N, H, W, Cin, Cout), _case9(t)
        fits = N * H * W * Cin * 4 < P.LIMIT and N * Ho * Wo * Cout * 4 < P.LIMIT
        route = lib.dsnt_conv_f16x3_route(C.byref(g), 1)
        if not (fits and Wo % 4 == 0):          # dsnt_conv_wgrad_bf16x6_ok (Cin and Cout are multiples of 4 all over the grid)
            want = -1
        elif R == 4:
            want = P.route((N, Ho, Wo), 4, True, stem=True)
        else:
            want = P.route(case5, R, True) if stride == 1 else 0
        assert route == want, t
        if route >= 0:
            assert lib.dsnt_conv_wgrad_halo_ok(C.byref(g)) == (route == 2), t
        plain = lib.dsnt_conv_wgrad_splits(C.byref(g))
        assert plain == G.plan(case9)[2], t
        cover = lib.dsnt_conv_wgrad_ws_floats(C.byref(g))
        assert cover >= plain * Cout * (K + 1), t
        for acc in FLAGS:
            share = bool(acc & SHARE)
            splits = lib.dsnt_conv_wgrad_f16x3_splits(C.byref(g), acc)
            assert lib.dsnt_conv_wgrad_f16x3_ws_floats(C.byref(g), acc) == splits * Cout * (K + 1), (t, acc)
            assert cover >= splits * Cout * (K + 1), (t, acc)
            if route == 1:
                assert splits == P.stem4((N, Ho, Wo))['wgrad_grid'], (t, acc)
            elif route == 2:
                assert splits == P.wgrad3(case5, share=(2 if acc & NARROW else 1) if share else 0)['nslabs'], (t, acc)
            elif route == 3:
                assert splits == P.wgrad1(case5, share=share)['nsplits'], (t, acc)
            else:
                assert splits == plain, (t, acc)
        seen.add(route)
    assert seen == {-1, 0, 1, 2, 3}
