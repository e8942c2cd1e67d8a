"""What the four evaluators of `dsnt.evaluator` share, without a GPU: the batch preparation `_batch_args`, the joint
count that the three table classes check before anything else, and that no class takes its methods from an unrelated one.

`score_ref.awkward` is also the feed of tests/test_evaluator_shared_gpu.py."""
import inspect

import numpy as np
import pytest
import torch

import score_ref
from dsnt import evaluator


def test_batch_args_round_awkward_inputs_to_what_the_kernels_take():
    B, J = 5, 3
    pred, target, m, b, mask, head, _ = score_ref.case(B, J, seed=1)
    # fp64 coordinates that no fp32 holds, so that the rounding shows
    pred, target = pred.astype(np.float64) + 1e-9, target.astype(np.float64) * (1 + 1e-10)
    assert not np.array_equal(pred, pred.astype(np.float32)) and not np.array_equal(head, head.astype(np.float32))
    args = score_ref.awkward(pred, target, m, b, mask, head)
    assert [a.dtype for a in args] == [torch.float64, torch.float64, torch.float64, torch.float32, torch.float64,
                                       torch.float32] and args[5].shape == (B, 1, 2)
    out = evaluator._batch_args(*args)
    want = (pred.astype(np.float32), target.astype(np.float32), m, b.astype(np.float32).astype(np.float64),
            mask.astype(np.float32), head.astype(np.float32).astype(np.float64))
    names = ('pred', 'target', 'm', 'b', 'mask', 'head')
    dtypes = (torch.float32, torch.float32, torch.float64, torch.float64, torch.float32, torch.float64)
    shapes = ((B, J, 2), (B, J, 2), (B, 2, 2), (B, 2), (B, J), (B,))
    assert len(out) == 6
    for name, got, dtype, shape, ref in zip(names, out, dtypes, shapes, want):
        assert got.dtype == dtype and tuple(got.shape) == shape and got.is_contiguous(), name
        assert got.device == args[0].device and not got.requires_grad, name
        assert np.array_equal(got.numpy(), ref) and got.numpy().dtype == ref.dtype, name


def test_table_classes_refuse_a_wrong_joint_count_first(monkeypatch):
    def touched(*a):
        raise AssertionError('the library was called: %r' % (a[0],))
    monkeypatch.setattr(evaluator, 'call', touched)
    monkeypatch.setattr(evaluator, 'ptr', touched)
    args = score_ref.awkward(*score_ref.case(5, 3, seed=1)[:6])
    score = torch.zeros(5, 3)
    for ev, extra in ((evaluator.PCKhCurve(n_joints=4), ()), (evaluator.ErrorField(n_joints=4), ()),
                      (evaluator.Reliability([0.5], n_joints=4), (score,))):
        with pytest.raises(ValueError, match='3 joints, the tables? ha(s|ve) 4'):
            ev.add_normalized(*args, *extra)
        assert not ev._tables and not ev._identity


def test_no_class_borrows_a_method_of_another():
    """A function in a class's own namespace was defined there: what a class shares with another it inherits."""
    classes = [c for _, c in inspect.getmembers(evaluator, inspect.isclass) if c.__module__ == evaluator.__name__]
    assert {'PCKhEvaluator', 'PCKhCurve', 'ErrorField', 'Reliability', 'ScoreCalibration'} <= {c.__name__ for c in classes}
    for cls in classes:
        for name, value in vars(cls).items():
            f = getattr(value, '__func__', value)               # (a staticmethod or classmethod holds its function)
            if inspect.isfunction(f):
                assert f.__qualname__ == '%s.%s' % (cls.__qualname__, name), (cls.__name__, name, f.__qualname__)
    for cls in (evaluator.PCKhCurve, evaluator.ErrorField, evaluator.Reliability):
        for name in ('_rows', '_names', 'merge', 'all_reduce', 'reset'):       # one definition, in a base of all three
            assert name not in vars(cls) and any(name in vars(b) for b in cls.__mro__[1:]), (cls.__name__, name)
