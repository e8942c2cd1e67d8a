"""Pin the oracle to the reference itself, through the reference's answers stored in
`tests/golden/oracle_vs_reference.npz` (made by `tests/golden/make_golden.py oracle_vs_reference`,
which builds every model the way these tests build the oracle's, loads its weights into the reference
and stores what the reference returns).  Runs anywhere, the GPU box included.
Checks forward, loss and EVERY parameter gradient, fp64 (tight) and fp32: small outputs whole,
gradients / buffers / large maps per tensor (max, L2, sum, seeded samples; golden_util.check_segments).

Weights and inputs come from `dsnt.synthetic` (numpy PCG64), never from torch's generators, whose
values depend on the CPU's vector ISA.  The hourglass cases run at 128x128: at 64x64 the innermost
level is 1x1, train-mode BatchNorm there normalises over two values, and the BLAS code path or thread
split of the machine alone moves the fp64 gradients by up to 6e-5 (relative), far past the 1e-10 bar;
at 128x128 that spread is 1e-12.
"""
import numpy as np
import pytest
import torch

import golden_util as gu
from dsnt import synthetic
from dsnt_oracle import nn as onn
from dsnt_oracle import model as omodel

G = gu.load('oracle_vs_reference')


def _max_err(t, key):
    return float(np.abs(t.detach().double().numpy() - G[key]).max())


@pytest.mark.parametrize('base,reg,dtype,tol', [
    ('hg1', 'none', torch.float64, 1e-10), ('hg2', 'js', torch.float64, 1e-10),
    ('hg2', 'js', torch.float32, 2e-4), ('hg2', 'var', torch.float64, 1e-10),
    ('hg2', 'kl', torch.float64, 1e-10), ('hg2', 'mse', torch.float64, 1e-10)])
def test_hourglass_model_forward_loss_grads(base, reg, dtype, tol):
    k = 'model.%s_%s_%s.' % (base, reg, str(dtype).split('.')[-1])
    mine = omodel.build_mpii_pose_model(base=base, output_strat='dsnt', reg=reg, reg_coeff=1.0)
    synthetic.fill_state_dict(mine, seed=0)
    mine.to(dtype)
    assert list(mine.state_dict().keys()) == list(G[k + 'keys'])
    x, target, mask = synthetic.batch(2, size=128, seed=1, mask_p=0.8, dtype=dtype)
    mine.train()
    out_m = mine(x)
    assert len(out_m) == len([f for f in G.files if f.startswith(k + 'out')])
    for i, b in enumerate(out_m):
        assert _max_err(b, k + 'out%d' % i) <= tol
    for i, h in enumerate(mine.heatmaps_array):
        gu.check_segments(G, k + 'hm%d' % i, [('hm', h)], tol, scaled=False)
    loss_m = mine.forward_loss(out_m, target, mask)
    loss_r = float(G[k + 'loss'])
    assert abs(loss_r - loss_m.item()) <= tol * max(1, abs(loss_r))
    loss_m.backward()
    gu.check_segments(G, k + 'grad', [(n, q.grad) for n, q in mine.named_parameters()], tol)
    gu.check_segments(G, k + 'buf', list(mine.named_buffers()), tol, scaled=False)
    assert _max_err(mine.compute_coords(out_m), k + 'coords') <= max(tol, 1e-6)
    assert mine.compute_coords(out_m).dtype == torch.float32
    gu.check_segments(G, k + 'heatmaps', [('hm', mine.heatmaps)], tol, scaled=False)


def test_mask_none_and_tensor_part2():
    mine = omodel.build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(mine, seed=0)
    mine.to(torch.float64)
    x, t, _ = synthetic.batch(2, size=128, seed=2, dtype=torch.float64)
    lm = mine.forward_loss(mine(x), t, None)
    assert abs(float(G['part2.loss']) - lm.item()) <= 1e-10
    # inference.py:47 hands forward_part2 a bare 4-D tensor of batch 1
    hm = synthetic.tensor('part2.hm', (1, 16, 8, 8), seed=2, dtype=torch.float64)
    b = mine.forward_part2(hm)
    assert int(G['part2.len']) == len(b) == 1 and _max_err(b[0], 'part2.out0') <= 1e-12


def test_builder_quirks():
    # hg builder defaults to the gauss strategy; resnet-style kwargs are filtered out
    m = omodel.build_mpii_pose_model(base='hg', dilate=2, truncate=1)
    assert m.output_strat == str(G['quirks.output_strat']) == 'gauss'
    assert m.hg.num_stacks == int(G['quirks.num_stacks']) == 2
    assert omodel.build_mpii_pose_model(base='hg8').hg.num_stacks == 8
    for bad in ('vgg', 'hgx'):
        with pytest.raises(Exception, match='unsupported base model type'):
            omodel.build_mpii_pose_model(base=bad)
        assert 'unsupported base model type' in str(G['quirks.error_' + bad])
    assert m.image_specs.size == int(G['quirks.image_size']) == 256
    assert m.heatmap_size == int(G['quirks.heatmap_size']) == 64


@pytest.mark.parametrize('dilate,truncate,hm', [(0, 1, 14), (2, 0, 28), (0, 0, 7), (1, 1, 14)])
def test_resnet_wrapper_matches_reference_wrapper(dilate, truncate, hm):
    """The reference's ResNetHumanPoseModel driven with the oracle's ResNet (torchvision is absent:
    SURVEY.md §8c) vs the oracle's wrapper; shapes follow tests/test_model.py:11-37."""
    import copy
    from dsnt_oracle import resnet as oresnet
    k = 'resnet.d%d_t%d.' % (dilate, truncate)
    torch.manual_seed(0)
    base = oresnet.resnet18().double()
    mine = omodel.ResNetHumanPoseModel(copy.deepcopy(base), n_chans=16, dilate=dilate,
                                       truncate=truncate, reg='js')
    synthetic.fill_state_dict(mine, seed=0)
    mine.double()
    x = synthetic.tensor('resnet.x', (2, 3, 224, 224), seed=4, dtype=torch.float64)
    t = synthetic.tensor('resnet.t', (2, 16, 2), seed=4, dtype=torch.float64, kind='uniform')
    b = mine(x)
    assert G[k + 'out'].shape == (2, 16, 2) and tuple(G[k + 'hm_shape']) == (2, 16, hm, hm)
    assert mine.heatmaps.shape == (2, 16, hm, hm)
    assert _max_err(b, k + 'out') <= 1e-10
    lb = mine.forward_loss(b, t, None)
    assert abs(float(G[k + 'loss']) - lb.item()) <= 1e-10
    lb.backward()
    gu.check_segments(G, k + 'grad', [(n, q.grad) for n, q in mine.named_parameters()], 1e-9)


@pytest.mark.parametrize('preact', ['softmax', 'thresholded_softmax', 'abs', 'relu', 'sigmoid'])
def test_preact_variants(preact):
    x = synthetic.tensor('preact.x', (3, 16, 8, 8), seed=6, dtype=torch.float64)
    m = omodel.hm_preact(x, preact)
    assert _max_err(m, 'preact.' + preact) <= 1e-14


def test_nn_functions_random():
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-6)):
        k = 'nnf.%s.' % str(dtype).split('.')[-1]
        hm = torch.softmax(synthetic.tensor(k + 'hm', (4, 16, 64 * 64), seed=3).to(dtype) * 3, -1)
        hm = hm.view(4, 16, 64, 64).requires_grad_()
        mu = synthetic.tensor(k + 'mu', (4, 16, 2), seed=3, kind='uniform').to(dtype)
        mask = (synthetic.tensor(k + 'mask', (4, 16), seed=3, kind='uniform') < 0.4).to(dtype)   # p = 0.7
        for name in ('kl_reg_loss', 'js_reg_loss', 'mse_reg_loss', 'variance_reg_loss'):
            a = float(G[k + name])
            b = getattr(onn, name)(hm, mu, 1 / 32, mask)
            assert abs(a - b.item()) <= tol * max(1, abs(a)), name
            gb, = torch.autograd.grad(b, hm)
            gu.check_segments(G, k + name + '.grad', [('grad', gb)], tol)
        assert _max_err(onn.dsnt(hm), k + 'dsnt') <= tol
        gu.check_segments(G, k + 'make_gauss', [('g', onn.make_gauss(mu, 64, 64, 1 / 32))], tol, scaled=False)
        gu.check_segments(G, k + 'softmax_2d', [('s', onn.softmax_2d(hm))], tol, scaled=False)
        b = onn.thresholded_softmax(hm.flatten(-2), -0.5)
        gu.check_segments(G, k + 'thresholded_softmax', [('s', b)], tol, scaled=False)


def test_inference_flip_restatement_matches_reference_pieces():
    """The reference's `inference.py` imports absent packages (progressbar, tele, torchdata), so its
    `generate_predictions` cannot run; the pieces the oracle restates are pinned instead: `reverse_tensor`
    (util.py:207-210) and the flip-average steps (inference.py:33-57) run by hand on a reference model."""
    from dsnt_oracle import inference as oinf
    t = torch.arange(24.).view(2, 3, 4)
    assert torch.equal(oinf.reverse_tensor(t, -1), torch.from_numpy(G['flip.reverse']))
    om = omodel.build_mpii_pose_model(base='hg1', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(om, seed=0)
    om.double()                           # fp64: an untrained eval-mode net is too ill-conditioned for a stored fp32 pin
    x, _, _ = synthetic.batch(1, size=64, seed=3, mask_p=1.0, dtype=torch.float64)
    data = [{'input': x[0], 'transform_m': torch.eye(2, dtype=torch.float64) * 50,
             'transform_b': torch.ones(1, 2, dtype=torch.float64)}]
    got = oinf.generate_predictions(om, data, use_flipped=True, batch_size=1)
    assert _max_err(got, 'flip.want') <= 1e-9


# (x, y, sigma, normalize, clip_size): the draw_gaussian cases (tests/golden/make_golden.py HMU_DRAWS, same order)
HMU_DRAWS = [(4, 4, 1, False, None), (0, 4, 1, False, 7), (-3, 2, 1.5, False, 7), (-4, 2, 1, False, 7),
             (18, 3, 1, False, 7), (19, 3, 1, False, 7), (7, 15, 2, True, 7), (3.7, 2.2, 1, True, None)]


# Drawn Gaussians are exp() in fp32: bit equality holds only within one math library code path (the
# tails differ in the last bits between the AVX2 and AVX-512 ones); 1e-7 is 2 ulp at the peak value 1.
DRAW_TOL = 1e-7


def test_heatmap_util_matches_reference():
    """`gauss` strategy helpers (util.py:70-198).  The reference's encode_heatmaps calls Python round() on a
    tensor element, which today's PyTorch rejects (TypeError: an API drift, not a denial), so encoding is
    pinned through the reference's own draw_gaussian at the documented rounded pixel + its known answers."""
    from dsnt_oracle import util as outil
    hm = synthetic.tensor('hmu.hm', (3, 5, 16, 16), seed=3)
    hm[0, 0].zero_()                      # maximum not positive -> (0, 0) pixel
    hm[0, 1, 0, 7] = 9.0                  # border pixel: no neighbour offset
    hm[0, 2, 5, 5] = 9.0; hm[0, 2, 5, 4] = hm[0, 2, 5, 6] = 1.0   # equal neighbours: sign 0
    for nb in (True, False):
        assert torch.equal(torch.from_numpy(G['hmu.decode_nb%d' % nb]),
                           outil.decode_heatmaps(hm, use_neighbours=nb))
    assert torch.equal(torch.from_numpy(G['hmu.get_preds']), outil.get_preds(hm))
    for i, (x, y, sigma, norm, clip) in enumerate(HMU_DRAWS):
        b = torch.zeros(16, 16)
        outil.draw_gaussian(b, x, y, sigma, normalize=norm, clip_size=clip)
        assert np.abs(G['hmu.draws'][i] - b.numpy()).max() <= DRAW_TOL, (x, y, sigma, norm, clip)
    coords = synthetic.tensor('hmu.coords', (4, 6, 2), seed=3, scale=1.2, kind='uniform')   # some joints off the map
    enc = outil.encode_heatmaps(coords, 16, 16, 1.25)
    assert enc.dtype == torch.float32 and np.abs(G['hmu.encode'] - enc.numpy()).max() <= DRAW_TOL


def test_gauss_strategy_model_matches_reference_pieces():
    """HourglassHumanPoseModel with output_strat='gauss' (model.py:247-258, 268-269): the reference path
    itself needs a CUDA device (`.cuda()` at :253) and the drifted round(); check the oracle's loss against
    mse_loss over reference-drawn targets and the decode against the reference's decode_heatmaps."""
    import torch.nn.functional as F
    from dsnt_oracle import util as outil
    m = omodel.build_mpii_pose_model(base='hg2')                    # builder default: gauss
    assert m.output_strat == 'gauss'
    synthetic.fill_state_dict(m, seed=0)
    m.train()
    x, target, _ = synthetic.batch(2, size=64, seed=5)
    out = m(x)
    assert isinstance(out, list) and len(out) == 2 and out[0].shape == (2, 16, 16, 16)
    loss = m.forward_loss(out, target, None)
    tgt = outil.encode_heatmaps(target, 16, 16, 1.0)
    want = sum(F.mse_loss(o, tgt) for o in out)
    assert abs(loss.item() - want.item()) <= 1e-7
    loss.backward()
    assert all(p.grad is not None for p in m.parameters())
    assert torch.equal(m.compute_coords(out), torch.from_numpy(G['gauss.decode']))
