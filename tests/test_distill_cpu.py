"""Heat-map distillation without a GPU: the plain-torch definition against its closed forms, the fp32 run against the fp64
run (K_ref, which the GPU bounds of tests/test_distill_gpu.py are multiples of), and every refusal of the two entry points,
of `dsnt.nn.distill_loss` and of `forward_distill_loss`."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import distill_ref as dr


# ------------------------------------------------------------------ 1. the reference is right
@pytest.mark.parametrize('kind', dr.KINDS)
def test_autograd_gradient_equals_the_closed_form(kind):
    worst = 0.0
    for h, w in ((16, 16), (7, 7)):
        for (name, t, s, T), o64 in zip(dr.cases(h, w), dr.reference(h, w, kind)):
            g = dr.closed_form_grad(s.double(), t.double(), T, kind).numpy()
            worst = max(worst, float(np.abs(g - o64['g']).max()))
    assert worst <= 1e-12, worst


@pytest.mark.parametrize('kind', dr.KINDS)
def test_known_values(kind):
    g = torch.Generator().manual_seed(0)
    x = 3.0 * torch.randn(5, 49, generator=g, dtype=torch.float64)
    for T in dr.TEMPERATURES:
        assert float(dr.rows_loss(x, x.clone(), T, kind).abs().max()) <= 1e-13          # identical rows
        assert float(dr.rows_loss(x + 37.5, x, T, kind).abs().max()) <= 1e-12           # shift invariance
    # two disjoint one-hot-like rows, a logit gap of G between the hot pixel and the rest
    G = 60.0
    s, t = torch.zeros(1, 49, dtype=torch.float64), torch.zeros(1, 49, dtype=torch.float64)
    s[0, 3], t[0, 40] = G, G
    for T in dr.TEMPERATURES:
        L = float(dr.rows_loss(s, t, T, kind))
        if kind == 'js':
            assert L <= T * T * math.log(2.0) * (1 + 1e-12)
            if T == 1.0:
                assert abs(L - math.log(2.0)) <= 1e-9
        elif kind == 'kl':
            assert abs(L - T * T * (G / T)) <= 1e-4 * T * G       # p = 1 at the teacher's pixel, where lq = -G / T
        else:
            assert abs(L - 2.0 * T * T) <= 1e-6 * T * T if T == 1.0 else L <= 2.0 * T * T
    # js is bounded by T^2 ln 2 over the whole matrix
    if kind == 'js':
        for (name, t, s, T), o64 in zip(dr.cases(14, 14), dr.reference(14, 14, 'js')):
            assert o64['L'].min() >= -1e-12 and o64['L'].max() <= T * T * math.log(2.0) * (1 + 1e-12), name


# ------------------------------------------------------------------ 2. K_ref is pinned
@pytest.mark.parametrize('kind', dr.KINDS)
def test_fp32_reference_error_is_pinned(kind):
    """K_ref[kind]: the fp32 run's worst gradient ratio and value error against the fp64 run over the whole matrix (13
    pairs x 3 temperatures x 6 map sizes).  Measured on the builder's CPU: gradient js 4.2, kl 13.5, mse 7.5; value js 1.10,
    kl 0.78, mse 0.07 units.  The GPU bounds are 4 K_ref, so they can never grow past 128 * 2^-24 D_r and 16 units."""
    grad, value = dr.k_ref(kind)
    print('K_ref[%s]: gradient %.2f, value %.3f units' % (kind, grad, value))
    assert grad <= 32.0, grad
    assert value <= 4.0, value


def test_case_matrix_is_the_issues():
    assert len(dr.PAIRS) == 10 and len(dr.CONVERGED) == 4 and dr.ROWS == 32
    cs = dr.cases(7, 7)
    assert len(cs) == 14 * 3
    by = {(n, T): (t, s) for n, t, s, T in cs}
    t, s = by[('diffuse/diffuse', 1.0)]
    assert torch.equal(s, torch.roll(t, 7, 0))
    t, s = by[('bimodal/converged', 2.0)]
    assert torch.equal(s, t)
    t, s = by[('offset/converged', 4.0)]
    assert torch.equal(s, t + 37.5)
    t, s = by[('onehot/converged', 1.0)]
    assert 0 < float((s - t).abs().max()) < 1e-2
    m = dr.mask_of(7, 7)
    assert (m == 0).any() and (m == 1).any()


# ------------------------------------------------------------------ 3. refusals of the C ABI and of distill_loss
def _distill_refusals():
    """(entry point, arguments without the stream, return code, dsnt_last_error()); X is a non-null pointer that is never
    followed."""
    X, N, F = C.c_void_p(4096), None, C.c_float
    rows = []

    def add(name, args, rc, text):
        rows.append((name, args, rc, (name + ': ' + text).encode()))

    def both(ptrs_rows, ptrs_grad, tail, rc, text):
        add('dsnt_distill_rows', ptrs_rows + tail, rc, text)
        add('dsnt_distill_loss_grad', ptrs_grad + tail, rc, text)

    ok = (4, 2, 8, 8, F(1.0), 1)                        # rows, teacher_rows, h, w, temperature, kind
    R, G = (X, X, X), (X, X, X, X, X, X)
    for i in range(3):                                  # student, teacher, loss_row
        add('dsnt_distill_rows', tuple(N if j == i else X for j in range(3)) + ok, 3, 'null tensor')
    for i in (0, 1, 4, 5):                              # student, teacher, loss_row, g_logits
        add('dsnt_distill_loss_grad', tuple(N if j == i else X for j in range(6)) + ok, 3, 'null tensor')
    add('dsnt_distill_loss_grad', (X, X, X, N, X, X) + ok, 3, 'null tensor')         # a mask without its denominator
    both(R, G, (0, 1, 8, 8, F(1.0), 1), 1, 'rows=0 out of range')
    both(R, G, (1 << 31, 1, 8, 8, F(1.0), 1), 1, 'rows=2147483648 out of range')
    both(R, G, (4, 2, 4096, 4096, F(1.0), 1), 1, 'bad map size 4096x4096')
    both(R, G, (4, 2, 0, 8, F(1.0), 1), 1, 'bad map size 0x8')
    both(R, G, (4, 2, 8, -1, F(1.0), 1), 1, 'bad map size 8x-1')
    both(R, G, (4, 0, 8, 8, F(1.0), 1), 1, 'teacher_rows=0 does not divide rows=4')
    both(R, G, (4, -2, 8, 8, F(1.0), 1), 1, 'teacher_rows=-2 does not divide rows=4')
    both(R, G, (4, 3, 8, 8, F(1.0), 1), 1, 'teacher_rows=3 does not divide rows=4')
    both(R, G, (4, 8, 8, 8, F(1.0), 1), 1, 'teacher_rows=8 does not divide rows=4')
    for bad in (0.0, -1.0, float('nan'), float('-inf')):
        both(R, G, (4, 2, 8, 8, F(bad), 1), 3, 'temperature must be positive')
    both(R, G, (4, 2, 8, 8, F(1.0), 3), 3, 'unknown kind 3')
    both(R, G, (4, 2, 8, 8, F(1.0), -1), 3, 'unknown kind -1')
    return rows


def test_entry_points_refuse_bad_arguments_without_gpu():
    from dsnt import _lib
    lib = _lib.load()
    assert lib.dsnt_version() >= 133
    table = _distill_refusals()
    assert {row[0] for row in table} == {n for n in _lib.SIGNATURES if n.startswith('dsnt_distill')}
    for name, args, rc, text in table:
        got = getattr(lib, name)(*args, None)
        assert (got, lib.dsnt_last_error()) == (rc, text), (name, args)
    # a NULL mask needs no denominator: the call gets past the null check (and is refused for its kind)
    got = lib.dsnt_distill_loss_grad(C.c_void_p(4096), C.c_void_p(4096), None, None, C.c_void_p(4096), C.c_void_p(4096),
                                     4, 2, 8, 8, C.c_float(1.0), 7, None)
    assert (got, lib.dsnt_last_error()) == (3, b'dsnt_distill_loss_grad: unknown kind 7')


def test_distill_loss_refuses_cpu_tensors_and_bad_shapes():
    import dsnt.nn as dn
    s, t = torch.zeros(2, 3, 4, 8, 8), torch.zeros(3, 4, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dn.distill_loss(s, t)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dn.distill_loss(s.requires_grad_(), t, mask=torch.ones(3, 4), kind='js', temperature=2.0)
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(3, 4, 8, 4), torch.zeros(2, 2, 3, 4, 8, 8), torch.zeros(8, 8),
                torch.zeros(2, 3, 1, 8, 8)):
        with pytest.raises(ValueError) as e:
            dn.distill_loss(s, bad)
        assert str(tuple(bad.shape)) in str(e.value) and str(tuple(s.shape)) in str(e.value)
    with pytest.raises(ValueError, match='unknown kind'):
        dn.distill_loss(s, t, kind='var')
    assert dn.DISTILL_KINDS == {k: dn.REG_KINDS[k] for k in ('js', 'kl', 'mse')}


# ------------------------------------------------------------------ 4. refusals of forward_distill_loss
def _cpu_head(x4):
    """A stand-in for the device head, so that forward_part2 runs without one: (heat-maps, coordinates)."""
    hm = torch.softmax(x4.flatten(-2), -1).view_as(x4)
    return hm, torch.zeros(*x4.shape[:-2], 2)


def test_forward_distill_loss_refusals(monkeypatch):
    import dsnt.nn as dn
    from dsnt.model import build_mpii_pose_model
    monkeypatch.setattr(dn, 'head_forward', _cpu_head)
    teacher = torch.zeros(2, 16, 64, 64)
    for base in ('hg2', 'resnet18'):
        with pytest.raises(ValueError, match='gauss'):
            build_mpii_pose_model(base=base, output_strat='gauss').forward_distill_loss(teacher)
        with pytest.raises(ValueError, match='sigmoid'):
            build_mpii_pose_model(base=base, output_strat='dsnt', preact='sigmoid').forward_distill_loss(teacher)
        m = build_mpii_pose_model(base=base, output_strat='dsnt', reg='js')
        with pytest.raises(RuntimeError, match='no forward'):
            m.forward_distill_loss(teacher)
    # remembered in all three cases of the hourglass's forward_part2 and in the ResNet's; a size mismatch names both sizes
    from dsnt.hourglass import StackedOutputs
    hg = build_mpii_pose_model(base='hg2', output_strat='dsnt', reg='js')
    slab = torch.zeros(2, 2, 16, 32, 32)
    for outs, shapes in ((StackedOutputs(slab), [(2, 2, 16, 32, 32)]),                # the one-launch slab path
                         (list(slab.unbind(0)), [(2, 16, 32, 32)] * 2),               # the per-stack path
                         (slab[0], [(1, 16, 32, 32)] * 2)):                          # a bare tensor, iterated along dim 0
        hg.forward_part2(outs)
        assert [tuple(x.shape) for x in hg._distill_logits] == shapes
        with pytest.raises(ValueError, match='64x64.*32x32'):
            hg.forward_distill_loss(teacher)
        with pytest.raises(RuntimeError, match='no CPU fallback'):              # sizes agree: it reaches the device op
            hg.forward_distill_loss(torch.zeros(shapes[0][-4:]))
    rn = build_mpii_pose_model(base='resnet18', output_strat='dsnt')
    rn.forward_part2(torch.zeros(2, 16, 7, 7))
    with pytest.raises(ValueError, match='64x64.*7x7'):
        rn.forward_distill_loss(teacher)
    hg.forward_part2(StackedOutputs(slab))
    hg.output_strat = 'gauss'
    hg.forward_part2(list(slab.unbind(0)))
    hg.output_strat = 'dsnt'
    with pytest.raises(RuntimeError, match='no forward'):                       # a gauss forward leaves nothing behind
        hg.forward_distill_loss(teacher)


def test_teacher_logits_restores_every_training_flag():
    """Eval mode and no autograd inside, the last stack's logits as a contiguous fp32 copy, and every module's own
    `training` flag back afterwards: a frozen (eval) submodule of a training teacher stays frozen."""
    from torch import nn
    from dsnt.model import teacher_logits

    class Stub(nn.Module):
        def __init__(self):
            super().__init__()
            self.live, self.frozen = nn.BatchNorm2d(3), nn.BatchNorm2d(3)
            self.seen = None

        def forward_part1(self, x):
            self.seen = (self.training, self.live.training, self.frozen.training, torch.is_grad_enabled())
            y = self.frozen(self.live(x)).double()
            return [y, y.transpose(-1, -2) * 2]

    m = Stub().train()
    m.frozen.eval()
    x = torch.randn(2, 3, 4, 5)
    out = teacher_logits(m, x)
    assert m.seen == (False, False, False, False)
    assert (m.training, m.live.training, m.frozen.training) == (True, True, False)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (2, 3, 5, 4) and not out.requires_grad
    assert int(m.live.num_batches_tracked) == 0                                  # running statistics untouched
    m.eval()
    teacher_logits(m, x)
    assert (m.training, m.live.training, m.frozen.training) == (False, False, False)
