"""The Poisson bootstrap of PCKh without a GPU: the weight rule of `dsnt_pckh_boot` as tests/boot_ref.py restates it (its
constants, its statistics, its domain), the host mathematics of `dsnt.evaluator.PCKhBootstrap` on tables made by the
restatement and loaded through `load_state_dict`, and the refusals of the entry point and of `add_normalized`, none of which
touches a device."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import boot_ref
import loader_ref
import score_ref
from dsnt import _lib, evaluator

MACROS = boot_ref.header_macros()
SEEDS = (0, 1, 0x123456789ABCDEF)
ALL16 = list(range(16))


# ---------------------------------------------------------------------------------------------------- the weight rule
def _e_inverse_bounds(terms=40):
    """Exact rationals lo < e^-1 < hi from the alternating series sum (-1)^i / i!, whose error is below its next term."""
    s, f = Fraction(0), 1
    for i in range(terms):
        f = f * i if i else 1
        s += Fraction((-1) ** i, f)
    step = Fraction(1, f * terms)
    return s - step, s + step


def test_cdf_constants_rederived_exactly():
    """c_k = floor(2^32 e^-1 sum_{i<=k} 1/i!) in exact rational arithmetic: e^-1 is bracketed so tightly (40 terms: 1e-47)
    that both ends of the bracket floor to the same integer, which must be the header's and the restatement's."""
    lo, hi = _e_inverse_bounds()
    assert 0 < hi - lo < Fraction(1, 10 ** 45)
    want, partial, f = [], Fraction(0), 1
    for k in range(12):
        f = f * k if k else 1
        partial += Fraction(1, f)
        a, b = math.floor(2 ** 32 * lo * partial), math.floor(2 ** 32 * hi * partial)
        assert a == b, k
        want.append(a)
    assert want == MACROS['CDF'] == [int(c) for c in boot_ref.CDF]
    assert want[0] == 1580030168 and want[-1] == 4294967292 < 2 ** 32
    assert MACROS['DOMAIN'] == boot_ref.DOMAIN == 0x424F4F54
    # the weights 0..12 have probabilities diff(c) / 2^32: mean and variance of Poisson(1) to 32 bits
    p = np.diff(np.array([0] + want + [2 ** 32], dtype=np.float64)) / 2.0 ** 32
    mean = (p * np.arange(13)).sum()
    assert abs(mean - 1) < 1e-8 and abs((p * np.arange(13) ** 2).sum() - mean ** 2 - 1) < 1e-7
    # the bound on B: a u32 cell takes at most 12 from each example
    assert MACROS['MAX_B'] == (2 ** 32 - 1) // 12


def test_weight_by_hand_and_shape():
    """One weight by a plain loop over the constants, and the layout: column 0 is 1, four replicates share a Philox call."""
    ids = np.array([5, -3, (7 << 32) + 11], np.int64)
    seed, R = 0xABCDEF0123456789, 10
    w = boot_ref.weights(ids, R, seed)
    assert w.shape == (3, R + 1) and w.dtype == np.int64 and (w[:, 0] == 1).all() and w.min() >= 0 and w.max() <= 12
    for n, i in enumerate(ids):
        bits = int(i) & (2 ** 64 - 1)
        for r in range(1, R + 1):
            words = loader_ref.philox4x32_10(bits & 0xFFFFFFFF, bits >> 32, (r - 1) >> 2, 0x424F4F54, seed)
            u = int(words[(r - 1) & 3])
            assert w[n, r] == sum(1 for c in MACROS['CDF'] if u >= c), (n, r)
    # a weight depends on (id, r, seed) alone: not on R, nor on which other ids come with it
    assert np.array_equal(boot_ref.weights(ids[1:], 7, seed), w[1:, :8])


@pytest.mark.parametrize('seed', SEEDS)
def test_weight_statistics(seed):
    """ids 0..4095, R = 64: the mean within 0.01 of 1 (5 sigma of 1 / sqrt(4096 * 64)), adjacent replicates uncorrelated to
    |rho| < 0.08 (5 sigma of 1 / sqrt(4096))."""
    w = boot_ref.weights(np.arange(4096), 64, seed)[:, 1:].astype(np.float64)
    mean = w.mean()
    rho = [np.corrcoef(w[:, r], w[:, r + 1])[0, 1] for r in range(63)]
    print('seed %#x: mean %.4f, worst |rho| %.4f' % (seed, mean, np.abs(rho).max()))
    assert abs(mean - 1) < 0.01
    assert np.abs(rho).max() < 0.08


def test_domain_separation():
    """The bootstrap's uniforms differ from the same call at the augmentation draw's domains and the epoch order's."""
    ids = np.arange(64)
    mine = boot_ref.uniforms(ids, 8, 3)
    for other in (0, 1, 2, loader_ref.DOMAIN):
        theirs = boot_ref.uniforms(ids, 8, 3, domain=other)
        assert (mine != theirs).mean() > 0.99, other
    assert boot_ref.DOMAIN not in (0, 1, 2) and not loader_ref.DOMAIN <= boot_ref.DOMAIN < loader_ref.DOMAIN + 256


# ---------------------------------------------------------------------------------------------------- host mathematics
R, SEED = 50, 9


def _feed(n=120, seed=4, J=16, thr=score_ref.THR3, spread=None):
    """(columns [n, J], valid [n, J], ids [n]) of a `score_ref.case`: the columns are the restatement's."""
    pred, target, m, b, mask, head, _ = score_ref.case(n, J, seed)
    if spread is not None:
        pred = (target + np.random.default_rng(seed + 1).normal(0, spread, target.shape)).astype(np.float32)
    k = score_ref.column(score_ref.distance(pred, target, m, b, head), thr)
    ids = np.random.default_rng(seed).permutation(10 * n)[:n].astype(np.int64) - 3 * n      # shuffled, some negative
    return k, mask == 1, ids


def _loaded(tab, thr=score_ref.THR3, seed=SEED, **kw):
    ev = evaluator.PCKhBootstrap(replicates=tab.shape[0] - 1, thresholds=thr, seed=seed, n_joints=tab.shape[1], **kw)
    ev.load_state_dict({'thresholds': torch.tensor(thr, dtype=torch.float64), 'seed': seed,
                        'replicates': tab.shape[0] - 1, 'table': torch.from_numpy(tab)})
    return ev


@pytest.fixture(scope='module')
def fed():
    k, valid, ids = _feed()
    return k, valid, ids, boot_ref.table(k, valid, ids, R, SEED, 16, 3)


def test_defaults_and_slice_zero(fed):
    ev = evaluator.PCKhBootstrap()
    assert (ev.R, ev.seed, ev.T, ev.n_joints) == (1000, 0, 1, 16) and ev.thresholds.tolist() == [0.5]
    assert ev.counts().shape == (1001, 16, 2) and ev.counts().dtype == torch.int64 and not ev.counts().any()
    assert math.isnan(ev.pckh()) and np.isnan(ev.replicates()).all() and math.isnan(ev.stderr())
    assert evaluator.PCKhBootstrap(seed=-1).seed == 2 ** 64 - 1
    with pytest.raises(ValueError):
        evaluator.PCKhBootstrap(replicates=0)
    k, valid, ids, tab = fed
    one_hot = np.zeros((16, 4), np.int64)
    np.add.at(one_hot, (np.broadcast_to(np.arange(16), k.shape)[valid], k[valid]), 1)
    assert np.array_equal(tab[0], one_hot) and tab[0].sum() == valid.sum()
    # every copy puts an example's whole weight on each of its valid joints
    w = boot_ref.weights(ids, R, SEED)
    assert np.array_equal(tab.sum(2), np.einsum('nr,nj->rj', w, valid.astype(np.int64)))


def test_readers_equal_the_numpy_readers(fed):
    k, valid, ids, tab = fed
    ev = _loaded(tab)
    curve = evaluator.PCKhCurve(thresholds=score_ref.THR3)
    curve.load_state_dict({'thresholds': torch.tensor(score_ref.THR3), 'table': torch.from_numpy(tab[0].copy())})
    assert torch.equal(ev.counts(), torch.from_numpy(tab))
    for name, rows in (('total_mpii', ev.groups['total_mpii']), ('rwrist', [10]), (3, [3]), ('all', ALL16)):
        for t, thr in enumerate((0.1, 0.2, 0.5)):
            assert ev.pckh(thr, name) == curve.pckh(thr, name) == boot_ref.pckh(tab, t, rows)
            reps = ev.replicates(thr, name)
            assert reps.dtype == np.float64 and reps.shape == (R,)
            assert np.array_equal(reps, boot_ref.replicates(tab, t, rows))
            assert ev.stderr(thr, name) == boot_ref.stderr(tab, t, rows) > 0
            for level in (0.95, 0.5):
                lo, hi = ev.interval(thr, name, level)
                assert (lo, hi) == boot_ref.interval(tab, t, rows, level) and lo <= hi
    lo, hi = ev.interval(0.5)
    assert lo < ev.pckh(0.5) < hi                                   # (true of this feed; not a theorem)
    with pytest.raises(KeyError):
        ev.pckh(0.3)
    with pytest.raises(KeyError):
        ev.replicates(0.5, 'nose')


def test_replicate_without_valid_joints_is_nan_and_left_out():
    """Three examples: most replicates draw weight 0 for all of them at least once in 200."""
    k, valid, ids = _feed(n=3, J=1, thr=score_ref.THR1)
    valid[:] = True
    tab = boot_ref.table(k, valid, ids, 200, SEED, 1, 1)
    ev = _loaded(tab, thr=score_ref.THR1)
    reps = ev.replicates(0.5, 0)
    empty = tab[1:].sum((1, 2)) == 0
    assert empty.any() and not empty.all() and np.array_equal(np.isnan(reps), empty)
    assert ev.stderr(0.5, 0) == float(np.std(reps[~empty], ddof=1))
    assert ev.interval(0.5, 0) == boot_ref.interval(tab, 0, [0])


def test_compare(fed):
    k, valid, ids, tab = fed
    k2, _, _ = _feed(spread=0.12)                                   # a better model on the same examples
    tab2 = boot_ref.table(k2, valid, ids, R, SEED, 16, 3)
    a, b = _loaded(tab2), _loaded(tab)
    got, want = a.compare(b, 0.5), boot_ref.compare(tab2, tab, 2, a.groups['total_mpii'])
    assert got == want and set(got) == {'diff', 'interval', 'stderr', 'p_greater'}
    assert got['diff'] == a.pckh(0.5) - b.pckh(0.5) > 0 and got['p_greater'] > 0.9
    assert got['interval'][0] <= got['diff'] <= got['interval'][1] and got['stderr'] > 0
    back = b.compare(a, 0.5)
    assert back['diff'] == -got['diff'] and abs(back['p_greater'] + got['p_greater'] - 1) < 1e-12
    assert a.compare(b, 0.1, 'rwrist', level=0.5) == boot_ref.compare(tab2, tab, 0, [10], 0.5)
    same = a.compare(a)
    assert same['diff'] == 0 and same['p_greater'] == 0.5 and same['interval'] == (0.0, 0.0)
    # another seed, another R, other thresholds, another joint count
    with pytest.raises(ValueError, match='seed'):
        a.compare(_loaded(boot_ref.table(k, valid, ids, R, SEED + 1, 16, 3), seed=SEED + 1))
    with pytest.raises(ValueError, match='replicates'):
        a.compare(_loaded(boot_ref.table(k, valid, ids, R - 1, SEED, 16, 3)))
    with pytest.raises(ValueError):
        a.compare(_loaded(boot_ref.table(k, valid, ids, R, SEED, 16, 3), thr=score_ref.f32([0.1, 0.2, 0.4])))
    with pytest.raises(ValueError):
        a.compare(_loaded(boot_ref.table(k[:, :5], valid[:, :5], ids, R, SEED, 5, 3)))
    # one example missing on one side, and the same number of examples under other ids
    with pytest.raises(ValueError, match='same examples'):
        a.compare(_loaded(boot_ref.table(k[1:], valid[1:], ids[1:], R, SEED, 16, 3)))
    with pytest.raises(ValueError, match='same examples'):
        a.compare(_loaded(boot_ref.table(k, valid, ids + 1, R, SEED, 16, 3)))


def test_merge_state_dict_and_reset(fed):
    k, valid, ids, tab = fed
    halves = [boot_ref.table(k[s], valid[s], ids[s], R, SEED, 16, 3) for s in (slice(0, 47), slice(47, None))]
    a, b = _loaded(halves[0]), _loaded(halves[1])
    a.merge(b)
    assert torch.equal(a.counts(), torch.from_numpy(tab))
    for other in (_loaded(tab, seed=SEED + 1), _loaded(tab[:-1]), _loaded(tab, thr=score_ref.f32([0.1, 0.2, 0.4])),
                  _loaded(tab[:, :5])):
        with pytest.raises(ValueError):
            a.merge(other)
    state = a.state_dict()
    assert set(state) == {'thresholds', 'seed', 'replicates', 'table'} and state['seed'] == SEED and state['replicates'] == R
    c = evaluator.PCKhBootstrap(replicates=R, seed=SEED)            # one threshold: the state brings its own
    c.load_state_dict(state)
    assert torch.equal(c.counts(), a.counts()) and torch.equal(c.thresholds, a.thresholds) and c.T == 3
    assert c.interval(0.2) == a.interval(0.2)
    state['table'][0, 0, 0] += 1
    assert not torch.equal(c.counts(), state['table'])             # the state was copied
    for wrong in (dict(state, seed=SEED + 1), dict(state, replicates=R + 1), dict(state, table=state['table'][1:]),
                  dict(state, table=state['table'][:, :5]), dict(state, table=state['table'][:, :, :3])):
        with pytest.raises(ValueError):
            evaluator.PCKhBootstrap(replicates=R, seed=SEED).load_state_dict(wrong)
    c.reset()
    assert not c.counts().any()


@pytest.mark.parametrize('seed', range(5))
def test_standard_error_is_plausible(seed):
    """2000 Bernoulli(0.8) examples of one joint, R = 400: the bootstrap's standard error within 15 % of the binomial
    sqrt(p (1 - p) / N), about 4 sigma of the estimator's own 1 / sqrt(2 R) = 3.5 % spread."""
    n = 2000
    hit = np.random.default_rng(100 + seed).random(n) < 0.8
    tab = boot_ref.table(np.where(hit, 0, 1)[:, None], np.ones((n, 1), bool), np.arange(n), 400, seed, 1, 1)
    ev = _loaded(tab, thr=score_ref.THR1, seed=seed)
    p = ev.pckh(0.5, 0)
    ratio = ev.stderr(0.5, 0) / math.sqrt(p * (1 - p) / n)
    print('seed %d: p %.4f, stderr ratio %.3f' % (seed, p, ratio))
    assert p == hit.mean() and abs(ratio - 1) < 0.15
    lo, hi = ev.interval(0.5, 0)
    assert lo < p < hi and 3 < (hi - lo) / ev.stderr(0.5, 0) < 5    # a 95 % interval is about 3.9 standard errors wide


# ---------------------------------------------------------------------------------------------------- refusals
def test_entry_point_refuses_bad_arguments_without_gpu():
    """Return code and exact message of every refusal of `dsnt_pckh_boot`; the pointers are never followed."""
    lib = _lib.load()
    fn = _lib.fn('dsnt_pckh_boot')
    assert lib.dsnt_version() >= 127
    p = C.c_void_p(4096)

    def rc(thr=(0.5,), T=None, B=4, J=3, R=5, ptrs=(p,) * 7, table=p, thr_ptr=True):
        arr = (C.c_double * max(len(thr), 1))(*thr) if thr_ptr else None
        code = fn(*ptrs, arr, len(thr) if T is None else T, 7, R, table, B, J, None)
        return code, lib.dsnt_last_error()

    bad = (3, b'dsnt_pckh_boot: bad argument')
    for slot in range(7):                                           # pred, target, m, b, mask, head, ids
        assert rc(ptrs=(p,) * slot + (None,) + (p,) * (6 - slot)) == bad, slot
    assert rc(table=None) == bad and rc(thr_ptr=False) == bad
    assert rc(B=0) == bad and rc(J=0) == bad and rc(R=0) == bad and rc(B=-1) == bad and rc(R=-1) == bad
    assert rc(T=0) == (3, b'dsnt_pckh_boot: T=0 outside 1..64')
    assert rc([0.01 * k for k in range(65)]) == (3, b'dsnt_pckh_boot: T=65 outside 1..64')
    nan, inf = float('nan'), float('inf')
    assert rc([0.2, 0.1]) == (3, b'dsnt_pckh_boot: thresholds must be strictly ascending (index 1)')
    assert rc([0.1, 0.2, 0.2]) == (3, b'dsnt_pckh_boot: thresholds must be strictly ascending (index 2)')
    assert rc([0.1, nan]) == (3, b'dsnt_pckh_boot: threshold 1 is not finite')
    assert rc([inf]) == (3, b'dsnt_pckh_boot: threshold 0 is not finite')
    fit = (3, b'dsnt_pckh_boot: (R + 1) * J * (T + 1) does not fit an int')
    assert rc(R=2 ** 29, J=2) == fit                                # (2^29 + 1) * 2 * 2 = 2^31 + 4
    assert rc(J=2 ** 30) == fit and rc(R=2 ** 31 - 1, J=1) == fit
    assert rc(R=2 ** 29 - 1, J=2) == fit                            # 2^31 exactly
    assert rc(R=2 ** 29 - 2, J=2, thr=[inf])[1].endswith(b'threshold 0 is not finite')    # 2^31 - 4 fits: refused further on
    most = MACROS['MAX_B']
    assert rc(B=most + 1) == (3, b'dsnt_pckh_boot: B=%d above %d' % (most + 1, most))
    assert rc(B=most, thr=[0.2, 0.1])[1].endswith(b"(index 1)")                   # B at the bound passes that check


def test_add_normalized_refuses_before_the_library(monkeypatch):
    def touched(*a):
        raise AssertionError('the library was called: %r' % (a[0],))
    monkeypatch.setattr(evaluator, 'call', touched)
    monkeypatch.setattr(evaluator, 'ptr', touched)
    args = score_ref.awkward(*score_ref.case(5, 3, seed=1)[:6])
    index = torch.arange(5)
    ev = evaluator.PCKhBootstrap(replicates=4, n_joints=4)
    with pytest.raises(ValueError, match='3 joints, the tables? ha(s|ve) 4'):
        ev.add_normalized(*args, index)
    with pytest.raises(ValueError, match='3 joints, the tables? ha(s|ve) 4'):
        ev.add(args[0], args[1], args[2], args[3], index)
    ev = evaluator.PCKhBootstrap(replicates=4, n_joints=3)
    for bad in (torch.arange(4), torch.arange(6), torch.arange(5).reshape(5, 1), torch.tensor(3), torch.arange(5.0),
                torch.arange(5, dtype=torch.float64), torch.ones(5, dtype=torch.bool), np.arange(5.0)):
        with pytest.raises(ValueError, match='index'):
            ev.add_normalized(*args, bad)
    assert not ev._tables and not ev._identity
    with pytest.raises(AssertionError, match='the library was called'):        # a good batch does reach the library
        ev.add_normalized(*args, index.to(torch.int32))
