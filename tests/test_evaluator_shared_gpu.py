"""One batch through all four evaluators of `dsnt.evaluator`: `PCKhEvaluator`, `PCKhCurve`, `Reliability` and `ErrorField`
count the same joints and the same hits at PCKh@0.5, for every joint and for 'all', fed clean tensors or the awkward views
and dtypes of tests/test_evaluator_shared_cpu.py, in one batch or in two; and all of them count what `score_ref.restate`
counts on the host.

The inputs are `score_ref.case(37, 16, seed=3716)` with the head lengths and `transform_b` rounded to fp32 values, which is
what an f32 `head` and an f32 `transform_b` can hold: so both feeds, and the restatement, see the same numbers."""
import numpy as np
import pytest
import torch

import score_ref
from score_ref import EDGES20, THR1

pytestmark = pytest.mark.gpu

B, J = 37, 16


def _case():
    pred, target, m, b, mask, head, score = score_ref.case(B, J, seed=3716)
    args = (pred, target, m, score_ref.f32(b), mask, score_ref.f32(head), score)
    assert score_ref.case_is_clear(args, THR1)
    # every valid joint lies inside ErrorField's frame, so its totals are the valid joints
    assert (np.abs(target.astype(np.float64)) < 0.9).all() and (mask == 1).sum() > B * J // 3
    return args


def _clean(pred, target, m, b, mask, head):
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in (pred, target, mask, head, m, b)]
    assert [a.dtype for a in t] == [torch.float32, torch.float32, torch.float32, torch.float64, torch.float64, torch.float64]
    return t


def _run(batches, score):
    """The state of the four evaluators after `batches` (lists of the six `add_normalized` arguments) with
    the scores `score` cut the same way: per name (hits, count) of the meters, then the three tables."""
    from dsnt.evaluator import ErrorField, PCKhCurve, PCKhEvaluator, Reliability
    meters, curve, rel, field = PCKhEvaluator(0.5), PCKhCurve([0.5]), Reliability(EDGES20, [0.5]), ErrorField(threshold=0.5)
    at = 0
    for args in batches:
        args = [a.cuda() for a in args]
        n = args[0].shape[0]
        meters.add_normalized(*args)
        curve.add_normalized(*args)
        rel.add_normalized(*args, torch.from_numpy(score[at:at + n]).cuda())
        field.add_normalized(*args)
        at += n
    assert at == B
    names = PCKhEvaluator.JOINT_NAMES + ['all']
    return ({n: (float(meters.meters[n].hits), float(meters.meters[n].count)) for n in names}, curve.counts(),
            rel.counts(), field.tables(), (curve, rel, field))


def test_one_batch_through_all_four_evaluators():
    args = _case()
    six, score = args[:6], args[6]
    want = score_ref.restate(*args, EDGES20, THR1).sum(1)        # [J, 2]: within 0.5, beyond
    assert want.shape == (J, 2) and want[:, 0].min() > 0 and want[:, 1].min() > 0       # hits and misses on every joint
    clean = _run([_clean(*six)], score)
    views = _run([score_ref.awkward(*six, device='cuda')], score)
    split = _run([[a[:20] for a in _clean(*six)], [a[20:] for a in score_ref.awkward(*six, device='cuda')]], score)
    for other in (views, split):
        assert other[0] == clean[0]
        assert torch.equal(other[1], clean[1]) and torch.equal(other[2], clean[2])
        assert all(torch.equal(a, b) for a, b in zip(other[3], clean[3]))      # the fp64 sums too, bit for bit
    meters, _, _, _, (curve, rel, field) = clean
    for name in list(range(J)) + ['all']:
        key = curve.joint_names[name] if name != 'all' else name
        rows = curve._rows(name)
        hits, count = int(want[rows, 0].sum()), int(want[rows].sum())
        assert meters[key] == (hits, count), name
        table = curve.counts()[rows].sum(0)
        assert (int(table[0]), int(table.sum())) == (hits, count), name
        marginal = rel.counts()[rows].sum((0, 1))
        assert torch.equal(marginal, table), name
        totals, misses = field.totals(name), field.misses(name)
        assert (int((totals - misses).sum()), int(totals.sum())) == (hits, count), name
