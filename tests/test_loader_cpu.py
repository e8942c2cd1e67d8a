"""CPU checks of the device-resident training set (dsnt.data.DeviceDataset, EpochLoader; csrc/augment.hip): the new entry
points are exported, declared, bound and validate their arguments; the epoch order restated in numpy
(tests/loader_ref.py) is a bijection keyed by (seed, epoch); the loader and the dataset refuse bad arguments on the host,
before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import loader_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dsnt_epoch_indices', 'dsnt_augment_fwd_gather', 'dsnt_augment_fwd_pair_gather', 'dsnt_augment_keypoints_gather')
SIZES = (1, 2, 3, 7, 64, 65, 1000, 4097, 25000)


def test_loader_symbols_exported_declared_and_bound():
    from dsnt import _lib
    lib = _lib.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dsnt_hip.h')).read(), flags=re.S)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\bint\s+%s\s*\(' % n, header), n
    assert lib.dsnt_version() >= 118


def test_loader_entry_points_validate_arguments_without_gpu():
    from dsnt import _lib
    lib = _lib.load()
    v = C.c_void_p(4096)
    ok = lambda rc: rc == 0
    # dsnt_epoch_indices(n, seed, epoch, first, count, shuffle, out): the range must lie inside [0, n)
    assert lib.dsnt_epoch_indices(10, 0, 0, 0, 4, 1, None, None) == 3
    for n, first, count in ((0, 0, 1), (10, 0, 0), (10, -1, 4), (10, 8, 3), (10, 0, 11)):
        assert lib.dsnt_epoch_indices(n, 0, 0, first, count, 1, v, None) == 1, (n, first, count)
    g = lambda N, idx, B, R, S: lib.dsnt_augment_fwd_gather(v, N, idx, B, R, S, v, v, v, v, 1, 0, 0, 0, v, v, v, None)
    assert g(4, None, 2, 384, 256) == 3                                     # no index tensor
    assert g(0, v, 2, 384, 256) == 1 and g(4, v, 70000, 384, 256) == 1 and g(4, v, 2, 384, 0) == 1
    assert lib.dsnt_augment_fwd_pair_gather(None, 4, v, 2, 384, 256, v, v, v, v, 1, 0, 0, 0, v, v, v, None) == 3
    kg = lambda hl, N, B, J, norm: lib.dsnt_augment_keypoints_gather(v, v, v, hl, N, v, B, J, v, v, v, v, 1, v, v, v, v,
                                                                     norm, None)
    assert kg(None, 4, 2, 16, v) == 3 and kg(v, 4, 2, 16, None) == 3
    assert kg(v, 0, 2, 16, v) == 1 and kg(v, 4, 0, 16, v) == 1 and kg(v, 4, 2, 0, v) == 1
    assert not ok(lib.dsnt_augment_fwd_gather(v, -1, v, 2, 384, 256, v, v, v, v, 1, 0, 0, 0, v, v, v, None))


def test_philox_restatement_known_answers():
    """Random123's Philox4x32-10 known-answer vectors: the generator of augment.hip, restated."""
    assert [int(x) for x in loader_ref.philox4x32_10(0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    m = 0xFFFFFFFF
    assert [int(x) for x in loader_ref.philox4x32_10(m, m, m, m, 2 ** 64 - 1)] == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


@pytest.mark.parametrize('n', SIZES)
def test_order_is_a_bijection(n):
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        for epoch in (0, 1, 2 ** 33 + 5):
            o = loader_ref.order(n, seed, epoch)
            assert o.dtype == np.int64 and o.shape == (n,)
            assert np.array_equal(np.sort(o), np.arange(n)), (n, seed, epoch)


def test_order_depends_on_epoch_and_seed_and_shuffle_off_is_identity():
    for n in SIZES:
        assert np.array_equal(loader_ref.order(n, 3, 0, shuffle=False), np.arange(n))
        if n < 7:
            continue
        a, b, c = loader_ref.order(n, 3, 0), loader_ref.order(n, 3, 1), loader_ref.order(n, 4, 0)
        assert not np.array_equal(a, b) and not np.array_equal(a, c), n
        assert not np.array_equal(a, np.arange(n)), n
    # a shuffle, not a rotation: few fixed points, and sub-ranges are the matching slice of the full order
    o = loader_ref.order(25000, 0, 0)
    assert (o == np.arange(25000)).sum() < 25
    assert np.array_equal(loader_ref.order(25000, 0, 0, positions=np.arange(4096, 4196)), o[4096:4196])


def _tensors(N=6, R=8, J=16):
    return (torch.zeros(N, R, R, 3, dtype=torch.uint8), torch.zeros(N, J, 2, dtype=torch.float64),
            torch.ones(N, J, dtype=torch.float32), torch.eye(3, dtype=torch.float64).expand(N, 3, 3).contiguous(),
            torch.ones(N, dtype=torch.float64))


def test_device_dataset_refuses_bad_arguments():
    from dsnt.data import DeviceDataset
    crops, kp, km, m, hl = _tensors()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        DeviceDataset(crops, kp, km, m, hl)
    with pytest.raises(RuntimeError, match='uint8'):
        DeviceDataset(crops.float(), kp, km, m, hl)
    with pytest.raises(RuntimeError, match='float64'):
        DeviceDataset(crops, kp.float(), km, m, hl)
    with pytest.raises(RuntimeError, match='float32'):
        DeviceDataset(crops, kp, km.double(), m, hl)
    with pytest.raises(RuntimeError, match=r'\[N, R, R, 3\]'):
        DeviceDataset(crops[:, :, :6], kp, km, m, hl)
    with pytest.raises(RuntimeError, match='matrix must have shape'):
        DeviceDataset(crops, kp, km, m[:, :2], hl)
    with pytest.raises(RuntimeError, match='head_lengths must have shape'):
        DeviceDataset(crops, kp, km, m, hl[:5])
    with pytest.raises(RuntimeError, match='must be a tensor'):
        DeviceDataset(crops.numpy(), kp, km, m, hl)
    # from_arrays: host checks first, and never a CPU "device"
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        DeviceDataset.from_arrays(crops.numpy(), kp.numpy(), km.numpy(), m.numpy(), hl.numpy(), device='cpu')
    with pytest.raises(RuntimeError, match='crops must be uint8'):
        DeviceDataset.from_arrays(crops.numpy().astype(np.float32), kp, km, m, hl)
    with pytest.raises(RuntimeError, match='keypoints must be floating point'):
        DeviceDataset.from_arrays(crops, kp.long(), km, m, hl)
    with pytest.raises(RuntimeError, match='keypoint_mask must have shape'):
        DeviceDataset.from_arrays(crops, kp, km[:, :15], m, hl)


def _stand_in(N=6, J=16):
    """A DeviceDataset shell around CPU tensors (the constructor would refuse them): EpochLoader's argument checks are
    host logic and must refuse before touching the device."""
    from dsnt.data import DeviceDataset
    d = DeviceDataset.__new__(DeviceDataset)
    d.crops, d.keypoints, d.keypoint_mask, d.matrix, d.head_lengths = _tensors(N, J=J)
    return d


def test_epoch_loader_refuses_bad_arguments():
    from dsnt.data import DeviceAugment, EpochLoader, ImageSpecs
    aug = DeviceAugment(ImageSpecs(4, False, False), (0, 0, 0), (1, 1, 1))
    d = _stand_in(N=6)
    assert len(EpochLoader(d, 4, aug)) == 2 and len(EpochLoader(d, 4, aug, drop_last=True)) == 1
    assert len(EpochLoader(d, 3, aug, drop_last=True, rank=1, world_size=2)) == 1
    with pytest.raises(RuntimeError, match='drop_last'):
        EpochLoader(d, 2, aug, world_size=2, rank=0)
    with pytest.raises(RuntimeError, match='rank'):
        EpochLoader(d, 2, aug, world_size=2, rank=2, drop_last=True)
    with pytest.raises(RuntimeError, match='rank'):
        EpochLoader(d, 2, aug, rank=-1)
    with pytest.raises(RuntimeError, match='leaves no batch'):
        EpochLoader(d, 7, aug, drop_last=True)
    with pytest.raises(RuntimeError, match='leaves no batch'):
        EpochLoader(d, 4, aug, drop_last=True, world_size=2)
    with pytest.raises(RuntimeError, match='batch_size'):
        EpochLoader(d, 0, aug)
    with pytest.raises(RuntimeError, match='DeviceDataset'):
        EpochLoader(_tensors(), 2, aug)
    with pytest.raises(RuntimeError, match='DeviceAugment'):
        EpochLoader(d, 2, object())
    with pytest.raises(RuntimeError, match='HFLIP_INDICES'):
        EpochLoader(_stand_in(J=15), 2, aug)                      # drawn flips need the 16 MPII joints
    EpochLoader(_stand_in(J=15), 2, DeviceAugment(ImageSpecs(4, False, False), (0, 0, 0), (1, 1, 1), use_aug=False))


def test_epoch_loader_state_round_trip():
    from dsnt.data import DeviceAugment, EpochLoader, ImageSpecs
    ld = EpochLoader(_stand_in(N=6), 4, DeviceAugment(ImageSpecs(4, False, False), (0, 0, 0), (1, 1, 1)), seed=9)
    assert ld.state_dict() == {'epoch': 0, 'batch': 0, 'seed': 9}
    ld.load_state_dict({'epoch': 3, 'batch': 1, 'seed': 11})
    assert ld.state_dict() == {'epoch': 3, 'batch': 1, 'seed': 11}
    ld.set_epoch(5)
    assert ld.state_dict() == {'epoch': 5, 'batch': 0, 'seed': 11}
