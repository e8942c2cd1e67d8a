"""CPU checks of the synthetic occlusion (dsnt.data.Occlude; csrc/occlude.hip): the numpy restatement
(tests/occlude_ref.py) has the properties the construction promises, the Philox domain words lie apart from every other
stream of the project, the entry point is exported, declared, bound and validates its arguments without a GPU, and the
host side of `Occlude` and of the loaders' `occlude=` refuses what it should."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import occlude_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020            # the draw is deterministic: the seed was picked once and the bounds below hold for it


def _coords(B, J, seed=0, spread=1.3):
    r = np.random.default_rng(seed)
    return r.uniform(-spread, spread, (B, J, 2)).astype(np.float32), (r.random((B, J)) < 0.7).astype(np.float32)


@pytest.mark.parametrize('centre', ['uniform', 'joint'])
def test_drawn_rectangles_are_non_empty_inside_the_image_and_of_the_asked_sides(centre):
    B, S, K, lo, hi = 300, 37, 8, 3, 15
    coords, mask = _coords(B, 16, 1)
    rects, donor, sides = ref.draw(B, S, K, lo, hi, ref.p24_of(0.7), SEED, 5, 0, centre, coords, mask, unclipped=True)
    used = sides[..., 0] > 0
    counts = used.sum(1)
    assert used.any() and (~used).any()
    assert all(used[b, :counts[b]].all() for b in range(B))              # the used rows come first
    r = rects[used].astype(np.int64)
    assert (r[:, 0] < r[:, 2]).all() and (r[:, 1] < r[:, 3]).all()         # non-empty
    assert r.min() >= 0 and r.max() <= S
    s = sides[used]
    assert s.min() >= lo and s.max() <= hi and set(np.unique(s)) == set(range(lo, hi + 1))
    assert ((r[:, 2] - r[:, 0]) <= s[:, 0]).all() and ((r[:, 3] - r[:, 1]) <= s[:, 1]).all()
    assert not rects[~used].any()                                          # unused rows are all zero
    assert (donor != np.arange(B)).all() and donor.min() >= 0 and donor.max() < B


def test_donor_is_another_sample_and_the_sample_itself_only_alone():
    for B in (2, 3, 7):
        seen = set()
        for step in range(40):
            donor = ref.draw(B, 8, 1, 1, 4, 1 << 24, SEED, step)[1]
            assert (donor != np.arange(B)).all() and donor.min() >= 0 and donor.max() < B
            seen |= set(zip(range(B), donor.tolist()))
        assert len(seen) == B * (B - 1)                                    # every other sample is reachable
    assert ref.draw(1, 8, 1, 1, 4, 1 << 24, SEED, 0)[1].tolist() == [0]


def test_probability_word():
    B, S, K = 4096, 16, 4
    never = ref.draw(B, S, K, 2, 5, 0, SEED, 1)[0]
    assert not never.any()
    always, _, sides = ref.draw(B, S, K, 2, 5, 1 << 24, SEED, 1, unclipped=True)
    counts = (sides[..., 0] > 0).sum(1)
    assert counts.min() == 1 and set(np.unique(counts)) == set(range(1, K + 1))     # the count histogram covers 1..K
    assert min(np.bincount(counts, minlength=K + 1)[1:]) > B / K / 2
    half = ref.draw(B, S, K, 2, 5, ref.p24_of(0.5), SEED, 1)[0]
    n = int(half.reshape(B, -1).any(1).sum())
    assert abs(n - 2048) <= 160, n                                        # 5 sigma of Binomial(4096, 0.5): sigma = 32
    assert ref.p24_of(0.5) == 1 << 23 and ref.p24_of(1.0) == 1 << 24 and ref.p24_of(0.0) == 0


def test_joint_centring_without_a_usable_joint_is_the_uniform_draw():
    B, S, K = 40, 21, 3
    coords, mask = _coords(B, 16, 2)
    uniform = ref.draw(B, S, K, 2, 9, 1 << 24, SEED, 3, 7)
    for c, m in ((coords, np.zeros_like(mask)),                           # all joints masked
                 (np.full_like(coords, 1.5), mask), (np.full_like(coords, np.nan), mask),   # no joint has a pixel
                 (np.zeros((B, 0, 2), np.float32), np.zeros((B, 0), np.float32))):           # no joints at all
        got = ref.draw(B, S, K, 2, 9, 1 << 24, SEED, 3, 7, 'joint', c, m)
        assert np.array_equal(got[0], uniform[0]) and np.array_equal(got[1], uniform[1])
    # with usable joints every rectangle holds the pixel of one of them
    rects, _ = ref.draw(B, S, K, 2, 9, 1 << 24, SEED, 3, 7, 'joint', coords, mask)
    px, py = ref.joint_pixels(coords, S)
    for b in range(B):
        ok = [(px[b, j], py[b, j]) for j in range(16) if px[b, j] >= 0 and mask[b, j] != 0]
        for x0, y0, x1, y1 in rects[b]:
            if ok and x1 > x0:
                assert any(x0 <= x < x1 and y0 <= y < y1 for x, y in ok)


def test_joint_pixels_and_covered_joints():
    S = 8
    c = np.array([[[-1.0, -1.0], [0.0, 0.0], [0.999, 0.999], [1.0, 0.0], [-1.0001, 0.0], [np.nan, 0.0], [0.0, np.inf],
                   [np.float32(1) - np.float32(2 ** -24), 0.0], [-0.25, 0.5]]], np.float32)
    px, py = ref.joint_pixels(c, S)
    assert px[0].tolist() == [0, 4, 7, -1, -1, -1, -1, -1, 3] and py[0].tolist() == [0, 4, 7, -1, -1, -1, -1, -1, 6]     # 1 - 2^-24 + 1 rounds to 2
    rects = np.array([[[3, 6, 5, 7], [4, 4, 4, 9], [0, 0, 1, 1]]], np.int32)        # the second one is empty
    assert ref.occluded_joints(rects, c, S)[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1]
    assert ref.occluded_joints(rects, np.zeros((1, 0, 2), np.float32), S).shape == (1, 0)


def test_the_draw_is_a_function_of_seed_step_and_sample_word_alone():
    a = ref.draw(6, 16, 2, 2, 6, 1 << 24, SEED, 9, 4)
    b = ref.draw(10, 16, 2, 2, 6, 1 << 24, SEED, 9, 0)
    assert np.array_equal(a[0], b[0][4:])                                  # sample word = draw_offset + b
    assert not np.array_equal(a[0], ref.draw(6, 16, 2, 2, 6, 1 << 24, SEED, 10, 4)[0])
    assert not np.array_equal(a[0], ref.draw(6, 16, 2, 2, 6, 1 << 24, SEED + 1, 9, 4)[0])
    assert not np.array_equal(a[0], ref.draw(6, 16, 2, 2, 6, 1 << 24, SEED, 9 + 2 ** 32, 4)[0])   # the step's high word counts


def test_fills_of_the_restatement():
    r = np.random.default_rng(3)
    x = r.standard_normal((2, 3, 8, 8)).astype(np.float32)
    x[0, 0, 0, 0], x[1, 2, 7, 7] = np.nan, -0.0
    rects = np.array([[[1, 2, 6, 5], [4, 3, 8, 8]], [[0, 0, 0, 0], [0, 0, 0, 0]]], np.int32)
    donor = np.array([1, 0], np.int32)
    inside = ref.cover(rects, 8)
    assert inside[0].sum() == 5 * 3 + 4 * 5 - 2 * 2 and not inside[1].any()
    bits = x.view(np.int32)
    for fill in ('value', 'noise', 'paste'):
        out = ref.apply(x, rects, donor, fill, SEED, 3, 0, (0.25, -1.0, 2.0), (0.4, 0.5, 0.6), (0.2, 0.3, 0.4))
        assert np.array_equal(out[1], bits[1])
        assert np.array_equal(out[0][:, ~inside[0]], bits[0][:, ~inside[0]])
        got = out[0].view(np.float32)[:, inside[0]]
        if fill == 'value':
            assert np.array_equal(got, np.broadcast_to(np.float32([0.25, -1.0, 2.0])[:, None], got.shape))
        elif fill == 'paste':
            assert np.array_equal(out[0][:, inside[0]], bits[1][:, inside[0]])
        else:
            u = got * np.float32([0.2, 0.3, 0.4])[:, None] + np.float32([0.4, 0.5, 0.6])[:, None]
            assert u.min() > -1e-6 and u.max() < 1 + 1e-6 and np.unique(got).size > got.size * 0.9
    n0, n1 = ref.noise(8, SEED, 3, 0, (0, 0, 0), (1, 1, 1)), ref.noise(8, SEED, 3, 1, (0, 0, 0), (1, 1, 1))
    assert n0.min() > 0 and n0.max() <= 1 and not np.array_equal(n0, n1)


def test_domain_words_collide_with_no_other_stream():
    text = open(os.path.join(ROOT, 'include', 'dsnt_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    macros = dict(re.findall(r'^#define (DSNT_[A-Z_]+) (\S.*)$', header, flags=re.M))
    D = int(macros['DSNT_OCCLUDE_DOMAIN'].rstrip('u'), 16)
    assert D == ref.DOMAIN == 0x4F43434C
    assert int(macros['DSNT_OCCLUDE_MAX_RECTS']) == ref.MAX_RECTS == 8
    assert int(macros['DSNT_OCCLUDE_MAX_JOINTS']) == ref.MAX_JOINTS == 256
    for name, code in ref.FILLS.items():
        assert int(macros['DSNT_OCCLUDE_FILL_' + name.upper()]) == code
    for name, code in ref.CENTRES.items():
        assert int(macros['DSNT_OCCLUDE_CENTRE_' + name.upper()]) == code
    boot = int(macros['DSNT_PCKH_BOOT_DOMAIN'].rstrip('u'), 16)
    sample = int(macros['DSNT_SAMPLE_DOMAIN'].rstrip('u'), 16)
    source = open(os.path.join(ROOT, 'dsnt-pose2d_amd', 'csrc', 'augment.hip')).read()
    order = int(re.search(r'ORDER_DOMAIN = (0x[0-9A-Fa-f]+)u', source).group(1), 16)
    rounds = int(re.search(r'ORDER_ROUNDS = (\d+)', source).group(1))
    others = {0, 1, 2, boot, sample} | {order + r for r in range(rounds)}
    assert order == 0x4F524400 and rounds == 8 and len(others) == 13
    mine = {D + k for k in range(11)}
    assert max(mine) < 2 ** 32 and not mine & others


def test_occlude_symbol_exported_declared_and_bound():
    from dsnt import _lib
    lib = _lib.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dsnt_hip.h')).read(), flags=re.S)
    assert hasattr(lib, 'dsnt_occlude') and 'dsnt_occlude' in _lib.SIGNATURES
    assert re.search(r'\bint\s+dsnt_occlude\s*\(', header)
    assert lib.dsnt_version() >= 131


def test_occlude_entry_point_validates_arguments_without_gpu():
    from dsnt import _lib
    lib = _lib.load()
    err = lambda: lib.dsnt_last_error().decode()
    X = lambda k: C.c_void_p(1 << 20 | k << 44)            # distinct non-null pointers, never followed, 16 TiB apart

    def call(inp=X(1), out=X(2), B=2, S=8, K=2, lo=1, hi=4, p24=1 << 23, fill=0, centre=0, fv=X(3), mean=X(4), std=X(5),
             coords=X(6), mask=X(7), J=16, rects=X(8), donor=X(9), occluded=X(10), draw=1):
        return lib.dsnt_occlude(inp, out, B, S, K, lo, hi, p24, fill, centre, fv, mean, std, coords, mask, J, rects, donor,
                                occluded, draw, 1, 2, 0, None)

    for name in ('inp', 'out', 'fv', 'mean', 'std', 'rects', 'donor'):
        assert call(**{name: None}) == 3 and err() == 'dsnt_occlude: null pointer', name
    for kw in (dict(S=0), dict(S=4097, hi=4), dict(S=-1), dict(B=0), dict(B=65536), dict(K=0), dict(K=9), dict(J=-1),
               dict(J=257)):
        a = dict(dict(B=2, S=8, K=2, J=16), **kw)
        assert call(**kw) == 1 and err() == 'dsnt_occlude: bad shape B=%d S=%d K=%d J=%d' % (a['B'], a['S'], a['K'], a['J']), kw
    for lo, hi in ((0, 4), (5, 4), (1, 9), (-2, -1), (9, 9)):
        assert call(lo=lo, hi=hi) == 1, (lo, hi)
        assert err() == 'dsnt_occlude: sides %d..%d outside 1 <= side_min <= side_max <= S=8' % (lo, hi)
    for fill in (-1, 3):
        assert call(fill=fill) == 3 and err() == 'dsnt_occlude: unknown fill %d' % fill
    for centre in (-1, 2):
        assert call(centre=centre) == 3 and err() == 'dsnt_occlude: unknown centre %d' % centre
    assert call(p24=(1 << 24) + 1) == 3 and err() == 'dsnt_occlude: p24=16777217 above 2^24'
    joints = 'dsnt_occlude: J=16 joints need coords and occluded, and joint centring a mask'
    assert call(coords=None) == 3 and err() == joints
    assert call(occluded=None) == 3 and err() == joints
    assert call(mask=None, centre=1) == 3 and err() == joints
    # in == out, and ranges that overlap from either side: B * 3 * S * S * 4 = 1536 bytes
    base = 1 << 20
    for inp, out in ((base, base), (base, base + 1535), (base + 1535, base), (base, base + 16)):
        assert call(inp=C.c_void_p(inp), out=C.c_void_p(out)) == 3, (inp, out)
        assert err().startswith('dsnt_occlude: in and out overlap')
    # valid arguments record a launch without touching a device, so nothing above got as far as one by luck
    h = lib.dsnt_list_create()
    assert lib.dsnt_list_begin(h) == 0
    try:
        n = 0
        for kw in (dict(), dict(inp=C.c_void_p(base), out=C.c_void_p(base + 1536)), dict(out=C.c_void_p(base), inp=C.c_void_p(base + 1536)),
                   dict(mask=None), dict(J=0, coords=None, mask=None, occluded=None), dict(J=0, centre=1, coords=None, mask=None, occluded=None),
                   dict(S=5, hi=5), dict(S=4096, hi=4096, B=65535, K=8, J=256), dict(p24=0), dict(p24=1 << 24),
                   dict(fill=2, centre=1, draw=0), dict(B=1, S=1, K=1, lo=1, hi=1, fill=1)):
            n += 1
            assert call(**kw) == 0 and lib.dsnt_list_size(h) == n, kw
    finally:
        assert lib.dsnt_list_end() == 0
        lib.dsnt_list_destroy(h)


def test_occlude_refuses_bad_arguments_on_the_host():
    from dsnt.data import DeviceAugment, ImageSpecs, Occlude
    for kw, text in ((dict(p=-0.1), '0 <= p <= 1'), (dict(p=1.5), '0 <= p <= 1'), (dict(p=float('nan')), '0 <= p <= 1'),
                     (dict(max_rects=0), 'max_rects'), (dict(max_rects=9), 'max_rects'), (dict(side=(0.0, 0.4)), 'side must'),
                     (dict(side=(0.5, 0.4)), 'side must'), (dict(side=(0.1, 1.2)), 'side must'), (dict(fill='blur'), 'fill must'),
                     (dict(centre='head'), 'centre must'), (dict(fill_value=(0, 0)), 'fill_value needs'),
                     (dict(mean=(0,) * 4), 'mean needs'), (dict(std=(1,)), 'std needs')):
        with pytest.raises(RuntimeError, match='dsnt: .*' + text):
            Occlude(**kw)
    occ = Occlude(side=(0.1, 0.4))
    assert occ.sides(256) == (26, 102) and occ.sides(5) == (1, 2) and Occlude(side=(0.001, 1.0)).sides(64) == (1, 64)
    aug = DeviceAugment(ImageSpecs(8, True, False), (0.4, 0.5, 0.6), (0.2, 0.3, 0.4), seed=11)
    like = Occlude.like(aug, fill='noise', p=1.0)
    assert like.mean == [0.4, 0.5, 0.6] and like.std == [1.0, 1.0, 1.0] and like.seed == 11 and like.fill == 'noise'
    assert Occlude.like(aug, seed=3).seed == 3
    with pytest.raises(RuntimeError, match='DeviceAugment'):
        Occlude.like(object())
    B, S, J = 2, 8, 16
    sample = {'input': torch.zeros(B, 3, S, S), 'part_coords': torch.zeros(B, J, 2), 'part_mask': torch.ones(B, J),
              'params': {}}
    with pytest.raises(RuntimeError, match='sample dict'):
        occ(torch.zeros(B, 3, S, S), 0)
    with pytest.raises(RuntimeError, match='input_pair'):
        occ(dict(sample, input_pair=torch.zeros(2 * B, 3, S, S)), 0)
    with pytest.raises(RuntimeError, match=r'input must be \[B, 3, S, S\]'):
        occ(dict(sample, input=torch.zeros(B, 3, S, S + 1)), 0)
    with pytest.raises(RuntimeError, match=r'input must be \[B, 3, S, S\]'):
        occ(dict(sample, input=torch.zeros(B, 1, S, S)), 0)
    with pytest.raises(RuntimeError, match='input must be torch.float32'):
        occ(dict(sample, input=torch.zeros(B, 3, S, S, dtype=torch.float64)), 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):              # a host tensor
        occ(sample, 0)
    for off in (-1, 2 ** 32):
        with pytest.raises(RuntimeError, match='draw_offset'):
            occ(sample, 0, draw_offset=off)


def _stand_in(N=6, R=8, J=16):
    """A DeviceDataset shell around CPU tensors, as in tests/test_loader_cpu.py: the checks are host logic."""
    from dsnt.data import DeviceDataset
    d = DeviceDataset.__new__(DeviceDataset)
    d.crops, d.keypoints, d.keypoint_mask = (torch.zeros(N, R, R, 3, dtype=torch.uint8),
                                             torch.zeros(N, J, 2, dtype=torch.float64), torch.ones(N, J))
    d.matrix, d.head_lengths = torch.eye(3, dtype=torch.float64).expand(N, 3, 3).contiguous(), torch.ones(N, dtype=torch.float64)
    return d


def test_loaders_take_an_occlude_and_refuse_anything_else():
    from dsnt.data import DeviceAugment, EpochLoader, ImageSpecs, Occlude, WeightedLoader
    aug = DeviceAugment(ImageSpecs(4, False, False), (0, 0, 0), (1, 1, 1))
    d, occ = _stand_in(), Occlude()
    ld = EpochLoader(d, 2, aug, occlude=occ)
    assert ld.occlude is occ and EpochLoader(d, 2, aug).occlude is None
    with pytest.raises(RuntimeError, match='occlude must be an Occlude'):
        EpochLoader(d, 2, aug, occlude=lambda s, step: s)
    with pytest.raises(RuntimeError, match='flip_pair'):
        EpochLoader(d, 2, aug, occlude=occ, flip_pair=True)
    with pytest.raises(RuntimeError, match='occlude must be an Occlude'):
        WeightedLoader(d, 2, aug, torch.ones(6), occlude=object())
    with pytest.raises(RuntimeError, match='no CPU fallback'):             # all host checks passed: the CDF build is next
        WeightedLoader(d, 2, aug, torch.ones(6), occlude=occ)
