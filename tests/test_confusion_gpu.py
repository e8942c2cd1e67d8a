"""Joint confusion on the device (`joint_confusion_kernel`, csrc/pckh.hip, through `dsnt_joint_confusion`) and
`dsnt.evaluator.JointConfusion` against the numpy restatement of tests/confusion_ref.py.

Both tables must equal the restatement exactly.  The only expression that may round differently on the device is the
distance (FMA contraction), and tests/test_confusion_cpu.py holds every seeded case 1e-9 relative clear of the threshold
and of ties; the hand-built cases sit exactly on both, in integers that any order of operations computes exactly.

Shapes are chosen around DSNT_CONFUSION_BLOCK = 256 and DSNT_CONFUSION_MAX_BLOCKS = 64 (include/dsnt_hip.h): a pass of a
workgroup takes 256 // J persons, so B runs just below, at and above one pass for J = 1, 3, 16, 17 (one idle thread) and
64, and past 64 passes (the grid strides) at J = 16 and J = 64.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import confusion_ref as ref
from dsnt._lib import call, ptr

pytestmark = pytest.mark.gpu

SENTINEL = -7
THR = ref.THR


@functools.lru_cache(maxsize=None)
def reference(B, J):
    """(args, mirror, table, mutual) of a seeded shape: restated once, shared by the tests, never written to."""
    args, mirror = ref.shape_case(B, J), ref.mirror_of(J)
    return (args, mirror) + ref.restate(*args, mirror)


def new_tables(J, table=0, mutual=0):
    """Device tables pre-filled with `table` and `mutual`, each with 8 sentinel guard cells behind it."""
    t = torch.full((J * (J + 1) + 8,), SENTINEL, dtype=torch.int64, device='cuda')
    u = torch.full((J + 8,), SENTINEL, dtype=torch.int64, device='cuda')
    t[:J * (J + 1)] = table
    u[:J] = mutual
    return t, u


def upload(args):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    assert dev[0].dtype == dev[1].dtype == dev[4].dtype == torch.float32 and dev[2].dtype == dev[5].dtype == torch.float64
    return dev


def launch(args, mirror, tables, thr=THR):
    """One `dsnt_joint_confusion` call on numpy (pred, target, m, b, mask, head) into `tables`."""
    B, J = args[4].shape
    call('dsnt_joint_confusion', *[ptr(t) for t in upload(args)], thr, (C.c_int * J)(*mirror), ptr(tables[0]),
         ptr(tables[1]), B, J)


def read(tables, J):
    """(table [J, J + 1], mutual [J]) as numpy; the guard cells must be intact."""
    t, u = tables[0].cpu(), tables[1].cpu()
    assert (t[J * (J + 1):] == SENTINEL).all().item() and (u[J:] == SENTINEL).all().item()
    return t[:J * (J + 1)].view(J, J + 1).numpy(), u[:J].numpy()


def on_device(args, mirror, table=0, mutual=0):
    tables = new_tables(args[4].shape[1], table, mutual)
    launch(args, mirror, tables)
    return read(tables, args[4].shape[1])


@pytest.mark.parametrize('B,J', ref.SHAPES, ids=['%dx%d' % s for s in ref.SHAPES])
def test_tables_match_restatement(B, J):
    """Into tables that hold 5 and 3 in every cell: the kernel adds and never stores.  Then what must hold whatever the
    input: the diagonal is `dsnt_pckh`'s hits of the same input on the device, the row sums its valid joints, and
    `mutual` is the same for a joint and its mirror."""
    args, mirror, table, mutual = reference(B, J)
    kinds = ref.kinds(table, mutual, mirror)
    print('B=%d J=%d: %s' % (B, J, kinds))
    got = on_device(args, mirror, table=5, mutual=3)
    assert got[0].dtype == table.dtype and np.array_equal(got[0], table + 5), (B, J)
    assert np.array_equal(got[1], mutual + 3), (B, J)
    dev = upload(args)
    hits, valid = torch.empty(B, J, device='cuda'), torch.empty(B, J, device='cuda')
    call('dsnt_pckh', *[ptr(t) for t in dev], THR, ptr(hits), ptr(valid), B, J)
    got = on_device(args, mirror)
    assert np.array_equal(np.diagonal(got[0]), hits.sum(0).cpu().numpy().astype(np.int64))
    assert np.array_equal(got[0].sum(1), valid.sum(0).cpu().numpy().astype(np.int64))
    assert all(got[1][j] == got[1][mirror[j]] for j in range(J)) and all(got[1][j] == 0 for j in range(J) if mirror[j] == j)


def test_hand_built_cases():
    """The exact threshold, the exact tie both ways round, the unannotated and the NaN target, the NaN predictions, the
    exchange, the collapse and the exchange with a masked partner: each alone, and all as one batch."""
    names = sorted(ref.HAND)
    for name in names:
        got = on_device(ref.hand([ref.HAND[name][0]]), ref.HAND_MIRROR)
        want = ref.hand_tables(name)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, got)
    got = on_device(ref.hand([ref.HAND[n][0] for n in names]), ref.HAND_MIRROR)
    assert np.array_equal(got[0], sum(ref.hand_tables(n)[0] for n in names))
    assert np.array_equal(got[1], sum(ref.hand_tables(n)[1] for n in names))
    # one ulp less head length and the joint at the threshold landed nowhere
    args = list(ref.hand([ref.HAND['at_threshold'][0]]))
    args[5] = np.array([np.nextafter(10.0, 0.0)])
    assert on_device(args, ref.HAND_MIRROR)[0][0].tolist() == [0, 0, 0, 1]
    # a head length of 0: inf and NaN distances, every counted joint lands nowhere
    args = list(ref.hand([ref.HAND['exchange'][0]], heads=0.0))
    got = on_device(args, ref.HAND_MIRROR)
    assert got[0][:, 3].tolist() == [1, 1, 1] and got[0].sum() == 3 and not got[1].any()
    # without a mirror the exchange is two confusions and no exchange
    got = on_device(ref.hand([ref.HAND['exchange'][0]]), [0, 1, 2])
    assert np.array_equal(got[0], ref.hand_tables('exchange')[0]) and not got[1].any()


@pytest.mark.parametrize('B,J,cut', [(1025, 16, 333), (86, 3, 1), (5, 64, 3)])
def test_a_batch_cut_in_two_gives_the_same_tables(B, J, cut):
    args, mirror, table, mutual = reference(B, J)
    tables = new_tables(J)
    for lo, hi in ((0, cut), (cut, B)):
        launch(tuple(a[lo:hi] for a in args), mirror, tables)
    got = read(tables, J)
    assert np.array_equal(got[0], table) and np.array_equal(got[1], mutual)
    again = on_device(args, mirror)                            # and two runs of the whole agree
    assert np.array_equal(again[0], table) and np.array_equal(again[1], mutual)


def _feed(ev, args):
    pred, target, m, b, mask, head = [torch.from_numpy(a).cuda() for a in args]
    return ev.add_normalized(pred, target, mask, head, m, b)


def test_class_over_two_batches():
    from dsnt.evaluator import JointConfusion, PCKhEvaluator
    a, b = reference(15, 16), reference(17, 16)
    ev, meter = JointConfusion(), PCKhEvaluator(THR)
    assert ev.mirror == a[1]
    for args in (a[0], b[0]):
        assert _feed(ev, args) is None
        _feed(meter, args)
    table, mutual = a[2] + b[2], a[3] + b[3]
    assert ev.counts().dtype == torch.int64 and not ev.counts().is_cuda
    assert np.array_equal(ev.counts().numpy(), table) and np.array_equal(ev.mutual().numpy(), mutual)
    kinds = ref.kinds(table, mutual, ev.mirror)
    rates = ev.rates('all')
    assert ev.valid('all') == table.sum() and all(rates[k] == kinds[k] / table.sum() for k in kinds)
    for name in PCKhEvaluator.JOINT_NAMES + list(PCKhEvaluator.JOINT_GROUPS):        # PCKhEvaluator's figure
        count, hits = int(meter.meters[name].count), int(meter.meters[name].hits)
        assert ev.valid(name) == count and ev.pckh(name) == hits / count, name
    # the state loads into an object that never sees a GPU, and answers the same; merge adds to it
    cpu = JointConfusion()
    cpu.load_state_dict(ev.state_dict())
    assert cpu.rates('ubody') == ev.rates('ubody') and cpu.top(5) == ev.top(5) and len(ev.top(5)) == 5
    cpu.merge(ev)
    assert np.array_equal(cpu.counts().numpy(), 2 * table) and np.array_equal(cpu.mutual().numpy(), 2 * mutual)
    ev.reset()
    assert not ev.counts().any() and not ev.mutual().any()
    _feed(ev, b[0])
    assert np.array_equal(ev.counts().numpy(), b[2]) and np.array_equal(ev.mutual().numpy(), b[3])
    with pytest.raises(ValueError, match='16 joints, the tables have 7'):
        _feed(JointConfusion(n_joints=7), a[0])


def test_class_add_in_image_space_and_seventeen_unnamed_joints():
    from dsnt.evaluator import JointConfusion
    names = sorted(ref.HAND)
    pred, target, m, b, mask, head = ref.hand([ref.HAND[n][0] for n in names])
    ev = JointConfusion(n_joints=3, mirror=ref.HAND_MIRROR)
    ev.add(*[torch.from_numpy(a).cuda() for a in (pred, target, mask, head)])
    assert np.array_equal(ev.counts().numpy(), sum(ref.hand_tables(n)[0] for n in names))
    assert np.array_equal(ev.mutual().numpy(), sum(ref.hand_tables(n)[1] for n in names))
    assert ev.mutual().tolist() == [0, 1, 1] and ev.rates(2)['mutual'] == 1 / ev.valid(2)
    args, mirror, table, mutual = reference(16, 17)
    ev = JointConfusion(n_joints=17, mirror=mirror)
    _feed(ev, args)
    assert np.array_equal(ev.counts().numpy(), table) and np.array_equal(ev.mutual().numpy(), mutual)
    assert ev.matrix().shape == (17, 18) and ev.top(3)[0][2] == max(table[j, k] for j in range(17) for k in range(17) if j != k)
    with pytest.raises(KeyError):
        ev.rates('total_mpii')


def test_add_without_host_sync():
    """After the first call has allocated the tables, `add_normalized` enqueues and returns."""
    from dsnt.evaluator import JointConfusion
    a, b = reference(15, 16), reference(17, 16)
    dev = [[torch.from_numpy(x).cuda() for x in args] for args in (a[0], b[0])]
    ev = JointConfusion()

    def step(k):
        pred, target, m, b_, mask, head = dev[k]
        ev.add_normalized(pred, target, mask, head, m, b_)
    step(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                    # any synchronising call raises
    try:
        step(1)
        step(1)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert np.array_equal(ev.counts().numpy(), a[2] + 2 * b[2]) and np.array_equal(ev.mutual().numpy(), a[3] + 2 * b[3])
