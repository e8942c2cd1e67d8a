"""CPU checks of the batched flip-evaluation ABI: `dsnt_flip_merge_head` and `dsnt_augment_fwd_pair` are exported,
declared and bound, and `dsnt_flip_merge_head` refuses bad arguments with a status and a message before any launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dsnt_flip_merge_head', 'dsnt_augment_fwd_pair')


def test_new_symbols_exported_declared_and_bound():
    from dsnt import _lib
    lib = _lib.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dsnt_hip.h')).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name)
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert name in _lib.SIGNATURES
    assert lib.dsnt_version() >= 116
    assert re.search(r'#define DSNT_FLIP_DSNT 0\b', header) and re.search(r'#define DSNT_FLIP_GAUSS 1\b', header)


def _perm(values):
    return (C.c_int * len(values))(*values)


HFLIP = [5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 15, 14, 13, 12, 11, 10]
FAKE = C.c_void_p(1 << 20)      # never dereferenced: every case below is refused before a launch


def _call(**kw):
    from dsnt import _lib
    lib = _lib.load()
    a = dict(logits=FAKE, B=2, J=16, h=8, w=8, perm=_perm(HFLIP), strategy=0, preact=0, thr=0.0, eps=0.0,
             tm=FAKE, tb=FAKE, hm=None, coords=FAKE, img=FAKE)
    a.update(kw)
    rc = lib.dsnt_flip_merge_head(a['logits'], a['B'], a['J'], a['h'], a['w'], a['perm'], a['strategy'], a['preact'],
                                  a['thr'], a['eps'], a['tm'], a['tb'], a['hm'], a['coords'], a['img'], None)
    return rc, lib.dsnt_last_error().decode()


@pytest.mark.parametrize('name', ['logits', 'perm', 'tm', 'tb', 'coords', 'img'])
def test_null_pointers_are_refused(name):
    rc, msg = _call(**{name: None})
    assert rc == 3 and 'null' in msg and 'dsnt_flip_merge_head' in msg


@pytest.mark.parametrize('perm', [[0] * 16, HFLIP[:15] + [16], HFLIP[:15] + [-1], list(range(15)) + [14]])
def test_non_permutation_is_refused(perm):
    rc, msg = _call(perm=_perm(perm))
    assert rc == 3 and 'permutation' in msg


@pytest.mark.parametrize('kw', [dict(h=0), dict(w=-3), dict(h=4096, w=4096), dict(B=0), dict(B=-1),
                                dict(B=1 << 30), dict(J=0), dict(J=33, perm=_perm(list(range(33))))])
def test_bad_shapes_are_refused(kw):
    rc, msg = _call(**kw)
    assert rc == 1 and 'dsnt_flip_merge_head' in msg


@pytest.mark.parametrize('kw,what', [(dict(strategy=2), 'strategy'), (dict(strategy=-1), 'strategy'),
                                     (dict(preact=5), 'preact'), (dict(preact=-1), 'preact')])
def test_unknown_strategy_or_preact_is_refused(kw, what):
    rc, msg = _call(**kw)
    assert rc == 3 and what in msg


def test_python_surface_refuses_bad_input_without_gpu():
    import torch
    from dsnt import inference
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        inference.flip_merge_head(torch.zeros(2, 16, 4, 4), torch.zeros(1, 2, 2, dtype=torch.float64),
                                  torch.zeros(1, 1, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='strategies'):
        inference.flip_merge_head(torch.zeros(2, 16, 4, 4), None, None, strategy='fc')
    with pytest.raises(Exception, match='preactivation'):
        inference.flip_merge_head(torch.zeros(2, 16, 4, 4), None, None, preact='tanh')
    # the batch-1 contract of generate_predictions is unchanged
    with pytest.raises(AssertionError, match='batch_size=1'):
        inference.generate_predictions(None, [], use_flipped=True, batch_size=4)
