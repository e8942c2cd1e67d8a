"""Heat-map distillation on the GPU (csrc/distill.hip, dsnt.nn.distill_loss, forward_distill_loss) against the fp64
definition of tests/distill_ref.py.

The matrix: 10 teacher/student regime pairs and 4 converged pairs x T in {1, 2, 4}, 32 teacher rows, at the smallest map
size that reaches each variant of the kernel (distill_ref.GPU_SIZES), once through `distill_loss(...).backward()` with a
mask that has both kinds of row and once through the C ABI with mask = NULL.  Every row of every case is checked: per-row
values, the scalar and the logit gradient, with the yardstick of distill_ref (gradient error over 2^-24 T (max p + max q),
values in units of 1e-5 max(1, |L64|)).  The bounds are FACTOR = 4 times K_ref[kind], the fp32 torch run's own worst
figures over the same matrix, computed at run time (the factor 4 of test_head_regimes_gpu.py and of the convolution tests).

Measured on an MI355X: worst figure / bound (4 K_ref) per kind over the whole matrix at the five sizes, both paths, the
walking grid and the unaligned calls.

    kind   gradient ratio      value, units
    js      3.63 / 16.7        0.041 / 4.40
    kl      5.14 / 53.9        0.349 / 3.12
    mse     3.97 / 29.9        0.044 / 0.27

Model level (hg2 student + 0.5 x the term against an hg1 teacher, smooth network): loss 31.8579102 vs 31.8579086 (kl, T = 2)
and 3.6726832 vs 3.6726830 (js, T = 1); worst parameter gradient rel-L2 1.0e-4 (hg.conv1.bias), cosine 1 - 3e-11.
"""
import numpy as np
import pytest
import torch

import distill_ref as dr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
KIND_NO = {'js': 0, 'kl': 1, 'mse': 2}


def _bounds(kind):
    kg, kv = dr.k_ref(kind, dr.GPU_SIZES)
    return FACTOR * kg, FACTOR * kv


def _abi(student, teacher, T, kind, mask=None, grad=True, out=None):
    """dsnt_distill_loss_grad / dsnt_distill_rows on device tensors [R, n] / [Rt, n] (h, w in `out`): (loss_row, g_logits)."""
    from dsnt import _lib
    import dsnt.nn as dn
    h, w = out
    rows, trows = student.shape[0], teacher.shape[0]
    loss_row = torch.full((rows,), float('nan'), device=DEV)
    if not grad:
        _lib.call('dsnt_distill_rows', _lib.ptr(student), _lib.ptr(teacher), _lib.ptr(loss_row), rows, trows, h, w, T,
                  KIND_NO[kind])
        return loss_row, None
    g = torch.full_like(student, float('nan'))
    denom2 = None if mask is None else dn.mask_denominator(mask, rows, student.device)
    _lib.call('dsnt_distill_loss_grad', _lib.ptr(student), _lib.ptr(teacher), _lib.ptr(mask), _lib.ptr(denom2),
              _lib.ptr(loss_row), _lib.ptr(g), rows, trows, h, w, T, KIND_NO[kind])
    return loss_row, g


class _Worst:
    def __init__(self, kind):
        self.kind, self.bg, self.bv = kind, *_bounds(kind)
        self.g = self.v = 0.0
        self.at_g = self.at_v = None

    def grad(self, ratio, where):
        r = float(np.max(ratio))
        if r > self.g:
            self.g, self.at_g = r, where

    def value(self, units, where):
        u = float(np.max(units))
        if u > self.v:
            self.v, self.at_v = u, where

    def check(self, what):
        print('%s %s: gradient %.2f / %.1f at %s, value %.3f / %.2f units at %s'
              % (what, self.kind, self.g, self.bg, self.at_g, self.v, self.bv, self.at_v))
        assert self.g <= self.bg, (what, self.kind, self.g, self.bg, self.at_g)
        assert self.v <= self.bv, (what, self.kind, self.v, self.bv, self.at_v)


@pytest.mark.parametrize('kind', dr.KINDS)
@pytest.mark.parametrize('size', dr.GPU_SIZES, ids=lambda s: '%dx%d' % s)
def test_matrix_against_fp64(size, kind):
    import dsnt.nn as dn
    h, w = size
    worst = _Worst(kind)
    mask = dr.mask_of(h, w)
    assert (mask == 0).any() and (mask == 1).any()
    wm = dr.weights(mask, dr.ROWS).numpy()
    for (name, t, s, T), o64 in zip(dr.cases(h, w), dr.reference(h, w, kind)):
        where = (h, w, name, T)
        td = t.to(DEV)
        # through autograd, masked
        sd = s.to(DEV).view(dr.ROWS, 1, h, w).requires_grad_()
        loss = dn.distill_loss(sd, td.view(dr.ROWS, 1, h, w), mask.to(DEV).view(dr.ROWS, 1), kind, T)
        loss.backward()
        g = sd.grad.view(dr.ROWS, -1).cpu().numpy()
        assert (g[mask.numpy() == 0] == 0).all(), where                   # exactly 0, and (below) not in the scalar
        worst.grad(dr.ratio_rows(g, o64, T, wm), where + ('masked',))
        worst.value(dr.value_units(loss.item(), float((wm * o64['L']).sum())), where + ('masked scalar',))
        # through the C ABI, mask = NULL
        loss_row, g = _abi(s.to(DEV), td, T, kind, out=size)
        worst.grad(dr.ratio_rows(g.cpu().numpy(), o64, T, np.full(dr.ROWS, 1.0 / dr.ROWS)), where + ('abi',))
        worst.value(dr.value_units(loss_row.cpu().numpy(), o64['L']), where + ('abi rows',))
        plain = dn.distill_loss(s.to(DEV).view(dr.ROWS, 1, h, w), td.view(dr.ROWS, 1, h, w), None, kind, T)
        worst.value(dr.value_units(plain.item(), o64['scalar']), where + ('scalar',))
    worst.check('matrix %dx%d' % size)


@pytest.mark.parametrize('kind', dr.KINDS)
@pytest.mark.parametrize('size', [(64, 64), (7, 7)], ids=lambda s: '%dx%d' % s)
def test_teacher_broadcast_is_bit_exact(size, kind):
    """Student [3, 32, 1, h, w] against teacher [32, 1, h, w]: the same bits as with the teacher expanded in memory."""
    import dsnt.nn as dn
    h, w = size
    cs = {n: (t, s) for n, t, s, T in dr.cases(h, w) if T == 2.0}
    t = cs['bimodal/peaked'][0]
    s = torch.stack([cs['bimodal/peaked'][1], cs['peaked/edge'][1], t + 0.25]).view(3, dr.ROWS, 1, h, w)
    t = t.view(dr.ROWS, 1, h, w)
    mask = dr.mask_of(h, w).view(dr.ROWS, 1)
    got = []
    for teacher in (t, t.expand(3, *t.shape).contiguous()):
        sd = s.to(DEV).requires_grad_()
        loss = dn.distill_loss(sd, teacher.to(DEV), mask.to(DEV), kind, 2.0)
        loss.backward()
        got.append((loss.detach().clone(), sd.grad.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert torch.isfinite(got[0][1]).all() and got[0][1].abs().max() > 0


@pytest.mark.parametrize('kind', dr.KINDS)
@pytest.mark.parametrize('size', [(64, 64), (7, 7)], ids=lambda s: '%dx%d' % s)
def test_walking_grid(size, kind, monkeypatch):
    """Teacher rows well past the threshold (twice the device's compute units, csrc/distill.hip `walk`; here four times
    them) and two student rows each: one workgroup per teacher row walks its student rows.  Held to the fp64 run, and
    to the bits of the one-workgroup-per-student-row launch of the same call (DSNT_OFF=distill_walk)."""
    h, w = size
    T = 2.0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = -(-4 * cus // dr.ROWS)                                           # cases of 32 rows: 32 on a 256-CU device
    cs = [(t, s) for _, t, s, T_ in dr.cases(h, w) if T_ == T]
    cs = [cs[i % len(cs)] for i in range(n)]
    t = torch.cat([c[0] for c in cs])
    s = torch.cat([torch.cat([c[1] for c in cs]), t])                    # the second slab has converged exactly
    trows, rows = t.shape[0], s.shape[0]
    assert trows >= 4 * cus and rows == 2 * trows                        # the walking form, by a factor of two
    o64 = dr.run(s, t, T, kind)
    sd, td = s.to(DEV), t.to(DEV)
    loss_row, g = _abi(sd, td, T, kind, out=size)
    worst = _Worst(kind)
    worst.grad(dr.ratio_rows(g.cpu().numpy(), o64, T, np.full(rows, 1.0 / rows)), size)
    worst.value(dr.value_units(loss_row.cpu().numpy(), o64['L']), size)
    worst.check('walking %dx%d' % size)
    monkeypatch.setenv('DSNT_OFF', 'distill_walk')
    loss_row1, g1 = _abi(sd, td, T, kind, out=size)
    assert torch.equal(loss_row, loss_row1) and torch.equal(g, g1)
    only, _ = _abi(sd, td, T, kind, grad=False, out=size)
    monkeypatch.delenv('DSNT_OFF')
    only2, _ = _abi(sd, td, T, kind, grad=False, out=size)
    assert torch.equal(loss_row, only) and torch.equal(loss_row, only2)


def _off_by_one(x):
    """A copy of x one float past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 8, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize('kind', dr.KINDS)
@pytest.mark.parametrize('size', [(64, 64), (14, 14)], ids=lambda s: '%dx%d' % s)
def test_unaligned_pointers_take_the_scalar_path(size, kind):
    """Student, teacher and gradient each one float off a 16-byte boundary, one at a time and all together, to the same
    bounds; the aligned call is the control."""
    from dsnt import _lib
    h, w = size
    worst, control = _Worst(kind), _Worst(kind)
    wr = np.full(dr.ROWS, 1.0 / dr.ROWS)
    for (name, t, s, T), o64 in zip(dr.cases(h, w), dr.reference(h, w, kind)):
        sd, td = s.to(DEV), t.to(DEV)
        loss_row, g = _abi(sd, td, T, kind, out=size)
        control.grad(dr.ratio_rows(g.cpu().numpy(), o64, T, wr), name)
        control.value(dr.value_units(loss_row.cpu().numpy(), o64['L']), name)
        first = None
        for off_s, off_t, off_g in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            s_, t_ = (_off_by_one(sd) if off_s else sd), (_off_by_one(td) if off_t else td)
            g_ = _off_by_one(torch.full_like(sd, float('nan'))) if off_g else torch.full_like(sd, float('nan'))
            lr_ = torch.full((dr.ROWS,), float('nan'), device=DEV)
            _lib.call('dsnt_distill_loss_grad', _lib.ptr(s_), _lib.ptr(t_), None, None, _lib.ptr(lr_), _lib.ptr(g_),
                      dr.ROWS, dr.ROWS, h, w, T, KIND_NO[kind])
            worst.grad(dr.ratio_rows(g_.cpu().numpy(), o64, T, wr), (name, T, off_s, off_t, off_g))
            worst.value(dr.value_units(lr_.cpu().numpy(), o64['L']), (name, T, off_s, off_t, off_g))
            # whichever pointer is off, the same variant runs: the same bits
            if first is None:
                first = (lr_.clone(), g_.clone())
            assert torch.equal(first[0], lr_) and torch.equal(first[1], g_), (name, T, off_s, off_t, off_g)
    control.check('aligned %dx%d' % size)
    worst.check('unaligned %dx%d' % size)


@pytest.mark.parametrize('kind', dr.KINDS)
@pytest.mark.parametrize('size', dr.GPU_SIZES, ids=lambda s: '%dx%d' % s)
def test_consistency(size, kind):
    import dsnt.nn as dn
    h, w = size
    cs = {n: (t, s) for n, t, s, T in dr.cases(h, w) if T == 2.0}
    t, s = cs['straddle/bimodal']
    sd, td = s.to(DEV), t.to(DEV)
    mask = dr.mask_of(h, w).to(DEV)
    runs = [_abi(sd, td, 2.0, kind, mask=mask, out=size) for _ in range(3)]
    for lr, g in runs[1:]:
        assert torch.equal(lr, runs[0][0]) and torch.equal(g, runs[0][1])
    only, _ = _abi(sd, td, 2.0, kind, grad=False, out=size)
    assert torch.equal(only, runs[0][0])                                       # the two entry points: the same loss_row
    assert torch.isfinite(only).all()
    # an upstream gradient of 3: exactly 3 x the gradient, up to its one rounding
    grads = []
    for scale in (1.0, 3.0):
        x = sd.view(dr.ROWS, 1, h, w).clone().requires_grad_()
        (scale * dn.distill_loss(x, td.view(dr.ROWS, 1, h, w), mask.view(dr.ROWS, 1), kind, 2.0)).backward()
        grads.append(x.grad.double())
    assert torch.equal(grads[0].float(), runs[0][1].view_as(grads[0]))
    assert ((grads[1] - 3.0 * grads[0]).abs() <= 2.0 ** -23 * (3.0 * grads[0]).abs() + 2.0 ** -126).all()   # + the smallest normal number
    # no gradient wanted: dsnt_distill_rows, the same scalar
    with torch.no_grad():
        a = dn.distill_loss(sd.view(dr.ROWS, 1, h, w), td.view(dr.ROWS, 1, h, w), mask.view(dr.ROWS, 1), kind, 2.0)
    x = sd.view(dr.ROWS, 1, h, w).clone().requires_grad_()
    b = dn.distill_loss(x, td.view(dr.ROWS, 1, h, w), mask.view(dr.ROWS, 1), kind, 2.0)
    assert torch.equal(a, b.detach())
    # the teacher is a constant
    tt = td.view(dr.ROWS, 1, h, w).clone().requires_grad_()
    dn.distill_loss(x, tt, None, kind, 2.0).backward()
    assert tt.grad is None


# ------------------------------------------------------------------ model level
def _rel_l2(got, want, floor=0.0):
    return (got.double() - want.double()).norm().item() / max(want.double().norm().item(), floor, 1e-30)


def _grads_close(m, o, tol, what):
    """Every parameter gradient: relative L2 error <= tol (floor = 1e-3 of the largest gradient norm: conv biases that
    feed a batch-norm have an exactly-zero true gradient, only noise).  As tests/test_model_gpu.py's."""
    floor = 1e-3 * max(q.grad.double().norm().item() for q in o.parameters() if q.grad is not None)
    worst = (0.0, None)
    for (n, p), (_, q) in zip(m.named_parameters(), o.named_parameters()):
        assert p.grad is not None and p.grad.shape == q.grad.shape, n
        e = _rel_l2(p.grad.cpu(), q.grad, floor)
        worst = max(worst, (e, n))
        assert e <= tol, (what, n, e)
    return worst


class _NoRelu:
    """Context: run BOTH implementations without ReLU, so that no pre-activation within 1e-7 of zero lands on opposite
    sides of the kink in the two of them (tests/test_model_gpu.py's, where the bars below are known to hold)."""

    def __enter__(self):
        import os
        import torch.nn.functional as F
        from dsnt_oracle import hourglass as ohg
        os.environ['DSNT_DEBUG_NO_RELU'] = '1'
        self.ohg, self.saved = ohg, ohg.F

        class Shim:
            relu = staticmethod(lambda t: t)
            max_pool2d = staticmethod(F.max_pool2d)
            interpolate = staticmethod(F.interpolate)
        ohg.F = Shim
        return self

    def __exit__(self, *a):
        import os
        os.environ.pop('DSNT_DEBUG_NO_RELU', None)
        self.ohg.F = self.saved

    @staticmethod
    def strip(oracle_model):
        import torch.nn as nn
        for seq in oracle_model.hg.fc:
            seq[2] = nn.Identity()


@pytest.fixture(scope='module')
def pair():
    """The student (hg2 + dsnt + js, smooth network, seed 3) on the GPU, the fp64 oracle of it on the CPU with its forward
    done once, the batch (4 x 128 px) and an hg1 teacher's logits (seed 5) from the GPU."""
    import os
    from dsnt import synthetic
    from dsnt.model import build_mpii_pose_model, teacher_logits
    from dsnt_oracle import model as omodel
    saved = os.environ.get('DSNT_MFMA')
    os.environ['DSNT_MFMA'] = 'f32'
    with _NoRelu():
        m = build_mpii_pose_model(base='hg2', output_strat='dsnt', reg='js')
        o = omodel.build_mpii_pose_model(base='hg2', output_strat='dsnt', reg='js')
        _NoRelu.strip(o)
        synthetic.fill_state_dict(m, seed=3)
        synthetic.fill_state_dict(o, seed=3)
        m.cuda().train()
        o.double().train()
        teacher = build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
        synthetic.fill_state_dict(teacher, seed=5)
        teacher.cuda().train()
        x, target, mask = synthetic.batch(4, size=128, seed=2, mask_p=0.8)
        t_hm = teacher_logits(teacher, x.to(DEV))
        assert teacher.training and t_hm.shape == (4, 16, 32, 32) and t_hm.is_contiguous() and t_hm.dtype == torch.float32
        assert not t_hm.requires_grad
        logits_o = o.forward_part1(x.double())
        outs_o = o.forward_part2(logits_o)
        task_o = o.forward_loss(outs_o, target.double(), mask.double())
        yield dict(m=m, o=o, x=x, target=target, mask=mask, t_hm=t_hm, logits_o=logits_o, task_o=task_o)
    if saved is None:
        os.environ.pop('DSNT_MFMA', None)
    else:
        os.environ['DSNT_MFMA'] = saved


@pytest.mark.parametrize('kind,T,use_mask', [('kl', 2.0, True), ('js', 1.0, False)])
def test_hg2_task_plus_distillation_vs_oracle(pair, kind, T, use_mask):
    m, o, x, target, mask, t_hm = (pair[k] for k in ('m', 'o', 'x', 'target', 'mask', 't_hm'))
    m.zero_grad()
    outs = m(x.to(DEV))
    dmask = mask.to(DEV) if use_mask else None
    loss = m.forward_loss(outs, target.to(DEV), mask.to(DEV)) + 0.5 * m.forward_distill_loss(t_hm, dmask, kind, T)
    loss.backward()
    # the oracle: the same task loss, plus the definition on its per-stack logits, summed over the stacks
    o.zero_grad()
    t64 = t_hm.cpu().double().reshape(64, -1)
    wr = dr.weights(mask if use_mask else None, 64)
    term = sum((dr.rows_loss(lo.reshape(64, -1), t64, T, kind) * wr).sum() for lo in pair['logits_o'])
    loss_o = pair['task_o'] + 0.5 * term
    loss_o.backward(retain_graph=True)
    print('loss %.7f vs %.7f (distillation term %.6f)' % (loss.item(), loss_o.item(), term.item()))
    assert term.item() > 1e-3
    assert abs(loss.item() - loss_o.item()) <= 1e-4 * max(1.0, abs(loss_o.item()))
    pm, po = dict(m.named_parameters()), dict(o.named_parameters())
    assert list(pm) == list(po) and len(pm) == 396
    worst = _grads_close(m, o, 1e-3, 'hg2 + ' + kind)
    flat_m = torch.cat([p.grad.cpu().reshape(-1) for p in pm.values()]).double()
    flat_o = torch.cat([p.grad.reshape(-1) for p in po.values()]).double()
    cos = (flat_m @ flat_o / (flat_m.norm() * flat_o.norm())).item()
    print('worst gradient rel-L2 %.2e (%s), cosine 1 - %.1e' % (worst[0], worst[1], 1 - cos))
    assert cos >= 1 - 1e-7, (cos, worst)


def test_hg2_distillation_alone_backpropagates(pair):
    """No forward_loss call and no labels: every parameter gets a gradient, and the logits slab receives exactly the
    g_logits of a direct distill_loss call on the same logits."""
    import dsnt.nn as dn
    m, x, t_hm = pair['m'], pair['x'], pair['t_hm']
    m.zero_grad()
    m(x.to(DEV))
    (slab,) = m._distill_logits
    assert slab.shape == (2, 4, 16, 32, 32)
    seen = []
    slab.register_hook(lambda g: seen.append(g.clone()))
    m.forward_distill_loss(t_hm, None, 'kl', 2.0).backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert sum(1 for p in m.parameters() if p.grad.abs().max() > 0) >= 300
    direct = slab.detach().clone().requires_grad_()
    (2 * dn.distill_loss(direct, t_hm, None, 'kl', 2.0)).backward()
    assert len(seen) == 1 and torch.equal(seen[0], direct.grad)
