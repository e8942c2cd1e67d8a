"""conv3 + projection shortcut as one forward launch (dsnt_conv1x1_fwd_ds_f16x3) INSIDE a model.

In production the engine fuses the two sites of the stem from DSNT_X_DS_FUSE_ROWS = 65536 rows, which no oracle-sized model
reaches.  A child process (tests/shortcut_fused_child.py) lifts that threshold and those of the 1x1 kernels and runs the hg2_128
golden vectors and hg2's every-gradient checks (the functions and bars of tests/test_model_gpu.py); its train-mode tapes must hold
exactly the two fused forward launches, no stand-alone shortcut forward of those geometries, and the shortcuts' two stand-alone
backward launches (no skip tensor: they read conv3's dL/dy).  A second child with DSNT_OFF=dsfuse runs the same step on the
two-launch path: loss, coordinates and every gradient are equal bit for bit."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _child(tmp, name, cases, off=None):
    env = dict(os.environ)
    for k in [k for k in env if k.startswith('DSNT_X_') or k in ('DSNT_OFF', 'DSNT_X', 'DSNT_DEBUG_NO_RELU')]:
        env.pop(k)
    env.update(DSNT_MFMA='bf16x6', DSNT_SPLIT='f16x3', DSNT_BF16X6_MIN_ROWS='0', DSNT_X_DS_FUSE_ROWS='0',
               DSNT_X_BWD1_MIN_ROWS='0', DSNT_X_FWD1_MIN_ROWS='0')
    if off:
        env['DSNT_OFF'] = off
    out, dump = str(tmp / (name + '.json')), str(tmp / (name + '.pt'))
    r = subprocess.run([sys.executable, os.path.join(HERE, 'shortcut_fused_child.py'), cases, out, dump], env=env, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    with open(out) as f:
        return json.load(f), dump


@pytest.fixture(scope='module')
def fused(tmp_path_factory):
    return _child(tmp_path_factory.mktemp('dsfuse'), 'fused', 'golden,grads:smooth,grads:relu,dump')


@pytest.fixture(scope='module')
def unfused(tmp_path_factory):
    return _child(tmp_path_factory.mktemp('dsfuse_off'), 'unfused', 'dump', off='dsfuse')


@pytest.mark.parametrize('case', ['golden', 'grads:smooth', 'grads:relu'])
def test_goldens_and_gradients_with_the_shortcuts_inside_conv3s_launches(fused, case):
    rep = fused[0].get(case)
    assert rep is not None and rep['ok'], rep
    assert rep['census'], 'no train-mode tape'
    for c in rep['census']:
        assert c == dict(fwd_ds=2, ds_fwd=0, ds_bwd=2), rep['census']


def _same_step(a, b):
    a, b = torch.load(a), torch.load(b)
    assert torch.equal(a['loss'], b['loss'])
    for x, y in zip(a['coords'], b['coords']):
        assert torch.equal(x, y)
    differ = [n for n in a['grads'] if not torch.equal(a['grads'][n], b['grads'][n])]
    assert not differ, (len(differ), differ[:6])


def test_two_launch_path_gives_the_same_step_bit_for_bit(fused, unfused):
    for rep, want in ((fused[0], dict(fwd_ds=2, ds_fwd=0, ds_bwd=2)), (unfused[0], dict(fwd_ds=0, ds_fwd=2, ds_bwd=2))):
        assert rep.get('dump') and rep['dump']['ok'], rep.get('dump')
        assert rep['dump']['census'] == [want], rep['dump']['census']
    _same_step(fused[1], unfused[1])
