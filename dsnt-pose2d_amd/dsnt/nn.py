"""DSNT operator library on MI355X — same surface as the reference's `dsnt.nn`.

Every public name, positional/keyword argument and default of
`/root/reference/src/dsnt/nn.py` is kept (`dsnt`, `euclidean_loss`, `thresholded_softmax`,
`make_gauss`, `kl_reg_loss`, `js_reg_loss`, `mse_reg_loss`, `variance_reg_loss`, ...), so
`train.py` / `infer.py` style callers import it unchanged.  Underneath, each op is a
`torch.autograd.Function` that enqueues hand-written HIP kernels from libdsnt_hip.so on the
current stream (csrc/head_ops.hip, head_loss.hip, head_fwd.hip).  Tensors must be fp32 and
resident on the HIP device: there is no CPU fallback, by design.
"""
import math

import numpy as np
import torch
from torch.autograd import Function

from . import _lib
from ._lib import ptr, f32, call

PREACT_MODES = {'softmax': 0, 'thresholded_softmax': 1, 'abs': 2, 'relu': 3, 'sigmoid': 4}
REG_KINDS = {'js': 0, 'kl': 1, 'mse': 2, 'var': 3}


def _rows(t, trailing):
    n = 1
    for s in t.shape[:t.dim() - trailing]:
        n *= s
    return n


# ------------------------------------------------------------------ meshgrids (nn.py:25-63)
def generate_xy(inp):
    """X and Y meshgrids expanded to `inp`'s shape (reference nn.py:25-46).

    Compatibility helper only — the kernels evaluate x_w = (2w-(W-1))/W in registers and never
    read a materialised meshgrid.
    """
    h, w = inp.shape[-2], inp.shape[-1]
    lead = [1] * (inp.dim() - 2)
    xs = torch.linspace(-(w - 1) / w, (w - 1) / w, w, device=inp.device).view(*lead, 1, w)
    ys = torch.linspace(-(h - 1) / h, (h - 1) / h, h, device=inp.device).view(*lead, h, 1)
    return xs.expand_as(inp).to(inp.dtype), ys.expand_as(inp).to(inp.dtype)


def expectation_2d(values, probabilities):
    """sum(values * probabilities) over the last two dims (reference nn.py:49-63)."""
    return (values * probabilities).flatten(-2).sum(-1)


# ------------------------------------------------------------------ dsnt (nn.py:66-78)
class _Dsnt(Function):
    @staticmethod
    def forward(ctx, heatmaps):
        hm = f32(heatmaps).contiguous()
        h, w = hm.shape[-2], hm.shape[-1]
        rows = _rows(hm, 2)
        coords = torch.empty(*hm.shape[:-2], 2, device=hm.device, dtype=hm.dtype)
        call('dsnt_expect_fwd', ptr(hm), ptr(coords), rows, h, w)
        ctx.shape = hm.shape
        return coords

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        ghm = torch.empty(ctx.shape, device=g.device, dtype=g.dtype)
        call('dsnt_expect_bwd', ptr(g), ptr(ghm), _rows(ghm, 2), ctx.shape[-2], ctx.shape[-1])
        return ghm


def dsnt(heatmaps):
    """Differentiable spatial to numerical transform: [..., H, W] -> [..., 2] as (x, y)."""
    return _Dsnt.apply(heatmaps)


# ------------------------------------------------------------------ per-joint statistics of heat-maps
def _stats_dict(stats, index, lead):
    """The packed kernel outputs (`stats` f32 [rows, 7], `index` int32 [rows]) as the public dict of views."""
    st = stats.view(*lead, 7)
    return {'peak': st[..., 0], 'peak_index': index.view(*lead), 'mass': st[..., 1], 'mean': st[..., 2:4],
            'cov': st[..., 4:7]}


def heatmap_stats(heatmaps):
    """Per-joint statistics of post-activation heat-maps `[..., H, W]` (`dsnt_heatmap_stats`, one read of the maps).

    A dict of device tensors over the leading dimensions `[...]`, all views of two buffers:
      * `peak` f32 `[...]`: the largest pixel, and `peak_index` int32 `[...]`: the first flat index `y * W + x` holding it;
      * `mass` f32 `[...]`: the sum of the map (1 for softmax, not for the other preactivations or raw maps);
      * `mean` f32 `[..., 2]`: `(sum X p, sum Y p)` on the DSNT grid, bit for bit what `dsnt(heatmaps)` returns;
      * `cov` f32 `[..., 3]`: `(vxx, vyy, vxy)`, the second central moments about that mean in normalised units.
    Nothing is calibrated: `peak` (confidence) and the spread `sqrt(vxx + vyy)` are the two quantities to threshold on.
    Forward only: the result carries no gradient, whatever `heatmaps` requires.  Device tensors only."""
    hm = f32(heatmaps.detach()).contiguous()
    if hm.dim() < 2:
        raise RuntimeError('dsnt: heatmap_stats needs [..., H, W], got %s' % (tuple(hm.shape),))
    h, w = hm.shape[-2], hm.shape[-1]
    rows = _rows(hm, 2)
    stats = torch.empty(rows, 7, device=hm.device, dtype=torch.float32)
    index = torch.empty(rows, device=hm.device, dtype=torch.int32)
    call('dsnt_heatmap_stats', ptr(hm), rows, h, w, ptr(stats), ptr(index))
    return _stats_dict(stats, index, hm.shape[:-2])


# ------------------------------------------------------------------ mode-seeking read-out of heat-maps
MODES_MAX_RADIUS, MODES_MAX_COUNT = 8, 4      # DSNT_MODES_MAX_RADIUS, DSNT_MODES_MAX_K of include/dsnt_hip.h


def heatmap_modes(heatmaps, radius=3, count=2, transform_m=None, transform_b=None):
    """The `count` dominant modes of heat-maps `[..., J, H, W]` as window centroids (`dsnt_map_modes`, one launch, DESIGN.md
    §22): where a bimodal map's expectation lands between its modes, mode 0 is the heavier one and mode 1 the runner-up.

    The window score of a pixel is the sum of the map over the `(2 radius + 1)^2` window about it, clipped to the map.
    Mode 0 is the first pixel (row-major) with the largest score, mode k the same among the pixels further than
    `2 radius` (Chebyshev) from every earlier mode, so the windows are disjoint.  The maps are used as given.  A dict of
    device tensors:
      * `coords` f32 `[..., J, K, 2]`: the centroid `(x, y)` of the map over the mode's window, on the DSNT grid;
      * `mass` f32 `[..., J, K]`: the sum of the map over the window (a share of 1 for softmax maps);
      * `index` int32 `[..., J, K]`: the window's centre `y * W + x`, -1 when there is no such mode (then `mass` and
        `coords` are NaN; `coords` are also NaN when the window's sum is not positive);
      * `image` f64 `[..., J, K, 2]` when `transform_m` `[B, 2, 2]` and `transform_b` `[B, 1, 2]` are given (both or
        neither; `B` the product of the leading dimensions): `transform_b + coords @ transform_m`, as `predict` does.
    `radius` 0..8, `count` 1..4, `H * W <= 8192`.  `radius=0` makes mode 0 the peak pixel of `heatmap_stats`; a radius
    that covers the map makes it the global mean, with no mode 1.  Forward only.  Device tensors only."""
    hm = f32(heatmaps.detach()).contiguous()
    if hm.dim() < 3:
        raise RuntimeError('dsnt: heatmap_modes needs [..., J, H, W], got %s' % (tuple(hm.shape),))
    if (transform_m is None) != (transform_b is None):
        raise ValueError('dsnt: heatmap_modes needs transform_m and transform_b together')
    if not 0 <= int(radius) <= MODES_MAX_RADIUS:
        raise ValueError('dsnt: heatmap_modes: radius=%r outside 0..%d' % (radius, MODES_MAX_RADIUS))
    if not 1 <= int(count) <= MODES_MAX_COUNT:
        raise ValueError('dsnt: heatmap_modes: count=%r outside 1..%d' % (count, MODES_MAX_COUNT))
    J, h, w = hm.shape[-3:]
    rows, K, lead = _rows(hm, 2), int(count), tuple(hm.shape[:-2])
    coords = torch.empty(*lead, K, 2, device=hm.device, dtype=torch.float32)
    mass = torch.empty(*lead, K, device=hm.device, dtype=torch.float32)
    index = torch.empty(*lead, K, device=hm.device, dtype=torch.int32)
    tm = tb = image = None
    if transform_m is not None:
        B = rows // max(J, 1)
        tm = transform_m.to(device=hm.device, dtype=torch.float64).contiguous()
        tb = transform_b.to(device=hm.device, dtype=torch.float64).contiguous()
        if tm.numel() != 4 * B or tb.numel() != 2 * B:
            raise RuntimeError('dsnt: heatmap_modes: transform_m %s / transform_b %s for %d samples'
                               % (tuple(tm.shape), tuple(tb.shape), B))
        image = torch.empty(*lead, K, 2, device=hm.device, dtype=torch.float64)
    call('dsnt_map_modes', ptr(hm), rows, J, h, w, int(radius), K, ptr(tm), ptr(tb), ptr(coords), ptr(mass), ptr(index),
         ptr(image))
    out = {'coords': coords, 'mass': mass, 'index': index}
    if image is not None:
        out['image'] = image
    return out


# ------------------------------------------------------------------ 'fc' output strategy (model.py:222-223, 293-303)
class _Fc2(Function):
    @staticmethod
    def forward(ctx, heatmaps, weight, bias):
        hm = f32(heatmaps).contiguous()
        hw = hm.shape[-2] * hm.shape[-1]
        rows = _rows(hm, 2)
        if tuple(weight.shape) != (2, hw):
            raise RuntimeError('dsnt.nn.fc_coords: weight must be [2, %d], got %s' % (hw, tuple(weight.shape)))
        w = f32(weight).contiguous()
        b = None if bias is None else f32(bias).contiguous()
        out = torch.empty(*hm.shape[:-2], 2, device=hm.device, dtype=hm.dtype)
        call('dsnt_fc2_fwd', ptr(hm), ptr(w), ptr(b), ptr(out), rows, hw)
        ctx.save_for_backward(hm, w)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        hm, w = ctx.saved_tensors
        g = g.contiguous()
        hw = w.shape[1]
        ghm = torch.empty_like(hm) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w)
        gb = torch.empty(2, device=w.device, dtype=w.dtype) if ctx.has_bias else None
        call('dsnt_fc2_bwd', ptr(g), ptr(hm), ptr(w), ptr(ghm), ptr(gw), ptr(gb), _rows(hm, 2), hw)
        return ghm, gw, gb


def fc_coords(heatmaps, weight, bias=None):
    """`out_fc(hm.view(-1, H*W)).view(..., 2)`: the reference's fully-connected output strategy."""
    return _Fc2.apply(heatmaps, weight, bias)


# ------------------------------------------------------------------ masked average (nn.py:81-94)
class _MaskedAverage(Function):
    @staticmethod
    def forward(ctx, losses, mask):
        l = f32(losses).contiguous()
        m = None if mask is None else f32(mask).contiguous()
        if m is not None and m.shape != l.shape:
            m = m.expand_as(l).contiguous()
        out2 = torch.empty(2, device=l.device, dtype=l.dtype)
        call('dsnt_masked_avg_fwd', ptr(l), ptr(m), ptr(out2), l.numel())
        ctx.save_for_backward(out2, m)
        ctx.shape = l.shape
        return out2[0].clone()

    @staticmethod
    def backward(ctx, g):
        out2, m = ctx.saved_tensors
        gl = torch.empty(ctx.shape, device=g.device, dtype=g.dtype)
        call('dsnt_masked_avg_bwd', ptr(g.contiguous().view(1)), ptr(m), ptr(out2), ptr(gl),
             gl.numel())
        return gl, None


def masked_average(losses, mask=None):
    """sum(l*m)/clamp(sum m, 1); plain mean (numel clamped to >= 1) without a mask."""
    return _MaskedAverage.apply(losses, mask)


# ------------------------------------------------------------------ euclidean loss (nn.py:97-116)
class _EuclidDist(Function):
    @staticmethod
    def forward(ctx, actual, target):
        a = f32(actual).contiguous()
        t = f32(target).expand_as(a).contiguous()
        d = a.shape[-1]
        n = a.numel() // d
        dist = torch.empty(a.shape[:-1], device=a.device, dtype=a.dtype)
        call('dsnt_euclid_fwd', ptr(a), ptr(t), ptr(dist), n, d)
        ctx.save_for_backward(a, t, dist)
        return dist

    @staticmethod
    def backward(ctx, g):
        a, t, dist = ctx.saved_tensors
        ga = torch.empty_like(a)
        call('dsnt_euclid_bwd', ptr(a), ptr(t), ptr(dist), ptr(g.contiguous()), ptr(ga),
             dist.numel(), a.shape[-1])
        gt = -ga if ctx.needs_input_grad[1] else None
        return ga, gt


def euclidean_loss(actual, target, mask=None):
    """Average Euclidean distance between predicted and target points.

    actual, target: ([batches x] n x d); mask: ([batches x] n) or None.
    """
    return masked_average(_EuclidDist.apply(actual, target), mask)


# ------------------------------------------------------------------ heat-map normalisation
class _Preact(Function):
    """model.py:24-45 normalisations; mode 1 is nn.py:119-139."""

    @staticmethod
    def forward(ctx, inp, mode, threshold, eps):
        x = f32(inp).contiguous()
        hw = x.shape[-1]
        y = torch.empty_like(x)
        call('dsnt_preact_fwd', ptr(x), ptr(y), x.numel() // hw, hw, mode, threshold, eps)
        ctx.mode, ctx.threshold, ctx.eps = mode, threshold, eps
        ctx.save_for_backward(x if mode >= 2 else None, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gx = torch.empty_like(y)
        hw = y.shape[-1]
        call('dsnt_preact_bwd', ptr(x), ptr(y), ptr(g.contiguous()), ptr(gx), y.numel() // hw, hw,
             ctx.mode, ctx.threshold, ctx.eps)
        return gx, None, None, None


class ThresholdedSoftmax(Function):
    """Same call convention as the reference's Function (nn.py:119-139)."""

    @staticmethod
    def forward(ctx, inp, threshold=-np.inf, eps=1e-12):
        x = f32(inp).contiguous()
        hw = x.shape[-1]
        y = torch.empty_like(x)
        call('dsnt_preact_fwd', ptr(x), ptr(y), x.numel() // hw, hw, 1, float(threshold), float(eps))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        (y,) = ctx.saved_tensors
        gx = torch.empty_like(y)
        hw = y.shape[-1]
        call('dsnt_preact_bwd', None, ptr(y), ptr(grad_output.contiguous()), ptr(gx),
             y.numel() // hw, hw, 1, 0.0, 0.0)
        return gx, None, None


def thresholded_softmax(inp, threshold=-np.inf, eps=1e-12):
    """Softmax over the last dim with inputs below `threshold` forced to exactly zero."""
    return ThresholdedSoftmax.apply(inp, threshold, eps)


def softmax_2d(inp):
    """Softmax with the last two tensor dimensions combined (reference nn.py:160-165)."""
    size = inp.size()
    flat = inp.reshape(-1, size[-1] * size[-2])
    return _Preact.apply(flat, 0, 0.0, 0.0).view(*size)


def hm_preact(x, preact):
    """`HumanPoseModel._hm_preact` (model.py:24-45): [..., J, H, W] -> [-1, J, H, W]."""
    if preact not in PREACT_MODES:
        raise Exception('unrecognised heatmap preactivation function: {}'.format(preact))
    n_chans, h, w = x.size(-3), x.size(-2), x.size(-1)
    flat = x.reshape(-1, h * w)
    mode = PREACT_MODES[preact]
    thr = -0.5 if mode == 1 else 0.0
    eps = 0.0 if mode == 0 else 1e-12
    return _Preact.apply(flat, mode, thr, eps).view(-1, n_chans, h, w)


# ------------------------------------------------------------------ make_gauss (nn.py:168-205)
class _MakeGauss(Function):
    @staticmethod
    def forward(ctx, coords, width, height, sigma):
        c = f32(coords).contiguous()
        out = torch.empty(*c.shape[:-1], height, width, device=c.device, dtype=c.dtype)
        call('dsnt_make_gauss', ptr(c), ptr(out), c.numel() // 2, height, width, float(sigma))
        ctx.save_for_backward(c)
        ctx.hw, ctx.sigma = (height, width), float(sigma)
        return out

    @staticmethod
    def backward(ctx, g):
        (c,) = ctx.saved_tensors
        gc = torch.empty_like(c)
        call('dsnt_make_gauss_bwd', ptr(c), ptr(f32(g).contiguous()), ptr(gc), c.numel() // 2, ctx.hw[0], ctx.hw[1],
             ctx.sigma)
        return gc, None, None, None


def make_gauss(coords, width, height, sigma):
    """Normalised 2-D Gaussians with means `coords` (normalised units) and std `sigma`."""
    return _MakeGauss.apply(coords, width, height, sigma)


def _kl_2d(p, q, eps=1e-24):
    """Compatibility helper (nn.py:208-211); the reg-loss functions below use fused kernels."""
    return (p * ((p + eps).log() - (q + eps).log())).sum(-1).sum(-1)


def _js_2d(p, q, eps=1e-24):
    """Compatibility helper (nn.py:214-216)."""
    m = 0.5 * (p + q)
    return 0.5 * _kl_2d(p, m, eps) + 0.5 * _kl_2d(q, m, eps)


# ------------------------------------------------------------------ regularisers (nn.py:219-298)
class _RegRows(Function):
    """Per-heat-map divergence from the target Gaussian (or variance error), fused."""

    @staticmethod
    def forward(ctx, heatmaps, mu_t, sigma_t, kind):
        hm = f32(heatmaps).contiguous()
        h, w = hm.shape[-2], hm.shape[-1]
        rows = _rows(hm, 2)
        mu = None
        if kind != 3:
            mu = f32(mu_t).expand(*hm.shape[:-2], 2).contiguous()
        out = torch.empty(hm.shape[:-2], device=hm.device, dtype=hm.dtype)
        call('dsnt_reg_fwd', ptr(hm), ptr(mu), ptr(out), rows, h, w, float(sigma_t), kind)
        ctx.save_for_backward(hm, mu)
        ctx.sigma, ctx.kind = float(sigma_t), kind
        ctx.mu_shape = tuple(mu_t.shape) if torch.is_tensor(mu_t) else None
        return out

    @staticmethod
    def backward(ctx, g):
        hm, mu = ctx.saved_tensors
        g = f32(g).contiguous()
        rows, h, w = _rows(hm, 2), hm.shape[-2], hm.shape[-1]
        ghm = gmu = None
        if ctx.needs_input_grad[0]:
            ghm = torch.empty_like(hm)
            call('dsnt_reg_bwd', ptr(hm), ptr(mu), ptr(g), ptr(ghm), rows, h, w, ctx.sigma, ctx.kind)
        if ctx.needs_input_grad[1]:
            # the reference's target is make_gauss(mu_t) inside autograd (nn.py:219-271): differentiable in mu_t
            if ctx.kind == 3:                       # the variance regulariser never reads mu_t
                gmu = torch.zeros(ctx.mu_shape, device=hm.device, dtype=hm.dtype)
            else:
                gmu = torch.empty_like(mu)
                call('dsnt_reg_bwd_mu', ptr(hm), ptr(mu), ptr(g), ptr(gmu), rows, h, w, ctx.sigma, ctx.kind)
                gmu = gmu.sum_to_size(ctx.mu_shape)  # mu_t may have been broadcast over leading dimensions
        return ghm, gmu, None, None


def kl_reg_loss(heatmaps, mu_t, sigma_t, mask=None):
    """Average KL(heatmap || target Gaussian)."""
    return masked_average(_RegRows.apply(heatmaps, mu_t, sigma_t, 1), mask)


def js_reg_loss(heatmaps, mu_t, sigma_t, mask=None):
    """Average Jensen-Shannon divergence between heatmaps and target Gaussians."""
    return masked_average(_RegRows.apply(heatmaps, mu_t, sigma_t, 0), mask)


def mse_reg_loss(heatmaps, mu_t, sigma_t, mask=None):
    """Average summed squared error between heatmaps and target Gaussians."""
    return masked_average(_RegRows.apply(heatmaps, mu_t, sigma_t, 2), mask)


def variance_reg_loss(heatmaps, mu_t, sigma_t, mask=None):
    """Mean squared error between heatmap variances and sigma_t^2 (mu_t unused)."""
    return masked_average(_RegRows.apply(heatmaps, mu_t, sigma_t, 3), mask)


# ------------------------------------------------------------------ fused head (model.py:233-307)
class _HeadForward(Function):
    """softmax preact + dsnt in one pass: logits [B,J,H,W] -> (heatmaps, coords [B,J,2])."""

    @staticmethod
    def forward(ctx, logits):
        x = f32(logits).contiguous()
        h, w = x.shape[-2], x.shape[-1]
        rows = _rows(x, 2)
        hm = torch.empty_like(x)
        coords = torch.empty(*x.shape[:-2], 2, device=x.device, dtype=x.dtype)
        call('dsnt_head_fwd', ptr(x), ptr(hm), ptr(coords), rows, h, w)
        ctx.save_for_backward(hm)
        return hm, coords

    @staticmethod
    def backward(ctx, g_hm, g_coords):
        (hm,) = ctx.saved_tensors
        h, w = hm.shape[-2], hm.shape[-1]
        rows = _rows(hm, 2)
        g = None
        if g_coords is not None:
            g = torch.empty_like(hm)
            call('dsnt_expect_bwd', ptr(g_coords.contiguous()), ptr(g), rows, h, w)
        if g_hm is not None:
            g = g_hm.contiguous() if g is None else g + g_hm
        gx = torch.empty_like(hm)
        call('dsnt_preact_bwd', None, ptr(hm), ptr(g), ptr(gx), rows, h * w, 0, 0.0, 0.0)
        return gx


def head_forward(logits):
    return _HeadForward.apply(logits)


class _HeadLoss(Function):
    """euclidean_loss + reg_coeff * reg_loss for one stack, straight from the logits' saved heat-maps.

    Train step (gradients wanted, heat-maps of <= 4096 pixels): ONE kernel reads the heat-maps and leaves both the
    per-row loss terms and d loss / d logits for an upstream gradient of 1 (`dsnt_head_loss_grad`); backward only
    rescales it when the upstream gradient is not 1 — the heat-maps are read once, not twice (SURVEY.md Appendix A:
    4 HBM passes per stack).  Otherwise: loss rows now, `dsnt_head_bwd` in backward."""

    @staticmethod
    def forward(ctx, logits, hm, coords, target, mask, kind, sigma, reg_coeff, denom2):
        h, w = hm.shape[-2], hm.shape[-1]
        rows = _rows(hm, 2)
        t = f32(target).expand_as(coords).contiguous()
        m = None if mask is None else f32(mask).expand(coords.shape[:-1]).contiguous()
        dist = torch.empty(rows, device=hm.device, dtype=hm.dtype)
        reg = torch.empty(rows, device=hm.device, dtype=hm.dtype) if kind >= 0 else None
        if denom2 is None:
            denom2 = mask_denominator(m, rows, hm.device)
        ctx.g0 = None
        if ctx.needs_input_grad[0] and h * w <= 4096:
            g0 = torch.empty_like(hm)
            call('dsnt_head_loss_grad', ptr(hm), ptr(coords), ptr(t), ptr(m), ptr(denom2), ptr(dist), ptr(reg), ptr(g0),
                 rows, h, w, sigma, kind, reg_coeff)
            ctx.g0 = g0
        else:
            call('dsnt_head_loss_rows', ptr(hm), ptr(coords), ptr(t), ptr(dist), ptr(reg), rows, h, w,
                 sigma, kind)
        out = torch.empty(3, device=hm.device, dtype=hm.dtype)      # [loss, e2[0], e2[1]]
        e2 = out[1:]
        call('dsnt_head_loss_reduce', ptr(dist), ptr(reg), ptr(m), ptr(denom2), reg_coeff, ptr(out), ptr(e2), rows)
        ctx.save_for_backward(hm, coords, t, m, dist, e2)
        ctx.kind, ctx.sigma, ctx.reg_coeff = kind, sigma, reg_coeff
        return out[0]

    @staticmethod
    def backward(ctx, g):
        hm, coords, t, m, dist, e2 = ctx.saved_tensors
        h, w = hm.shape[-2], hm.shape[-1]
        rows = _rows(hm, 2)
        g1 = f32(g).contiguous().view(1)
        if ctx.g0 is not None:                 # first backward through the fused kernel's gradient: rescale in place
            g_logits, ctx.g0 = ctx.g0, None
            call('dsnt_scale_by_scalar', ptr(g_logits), ptr(g1), g_logits.numel())
            return g_logits, None, None, None, None, None, None, None, None
        g_dist = torch.empty(rows, device=hm.device, dtype=hm.dtype)
        call('dsnt_masked_avg_bwd', ptr(g1), ptr(m), ptr(e2), ptr(g_dist), rows)
        g_reg = (g_dist * ctx.reg_coeff) if ctx.kind >= 0 else None   # same mask and denominator
        g_logits = torch.empty_like(hm)
        call('dsnt_head_bwd', ptr(hm), ptr(coords), ptr(t), ptr(dist), ptr(g_dist), ptr(g_reg),
             ptr(g_logits), rows, h, w, ctx.sigma, ctx.kind)
        return g_logits, None, None, None, None, None, None, None, None


def mask_denominator(mask, rows, device):
    """{sum(mask), clamp(sum(mask), 1)} as two device floats (`masked_average`'s denominator, nn.py:81-94; mask None:
    `rows`): computed once per `forward_loss` call and shared by every stack's head_loss."""
    m = None if mask is None else f32(mask).contiguous()
    out = torch.empty(2, device=device, dtype=torch.float32)
    call('dsnt_mask_denom', ptr(m), ptr(out), rows)
    return out


def head_loss(logits, hm, coords, target, mask, reg, sigma, reg_coeff, denom2=None):
    kind = REG_KINDS.get(reg, -1)
    return _HeadLoss.apply(logits, hm, coords, target, mask, kind, float(sigma), float(reg_coeff), denom2)


# ------------------------------------------------------------------ heat-map distillation (csrc/distill.hip)
DISTILL_KINDS = {'js': 0, 'kl': 1, 'mse': 2}      # the numbers of REG_KINDS


class _DistillLoss(Function):
    """masked_average of the per-row distillation loss, straight from the two logit tensors (follows `_HeadLoss`).

    Gradients wanted: ONE kernel reads both maps and leaves the per-row values and d loss / d student logits for an
    upstream gradient of 1 (`dsnt_distill_loss_grad`); backward only rescales it when the upstream gradient is not 1.
    Otherwise: `dsnt_distill_rows`.  The teacher is a constant: its gradient is None."""

    @staticmethod
    def forward(ctx, student, teacher, mask, kind, temperature):
        s, t = f32(student).contiguous(), f32(teacher).contiguous()
        h, w = s.shape[-2], s.shape[-1]
        rows, teacher_rows = _rows(s, 2), _rows(t, 2)
        m = None if mask is None else mask.to(torch.float32).expand(s.shape[:-2]).contiguous()
        loss_row = torch.empty(rows, device=s.device, dtype=s.dtype)
        ctx.g0 = None
        if ctx.needs_input_grad[0]:
            denom2 = None if m is None else mask_denominator(m, rows, s.device)      # no mask: the kernel's 1 / rows
            g0 = torch.empty_like(s)
            call('dsnt_distill_loss_grad', ptr(s), ptr(t), ptr(m), ptr(denom2), ptr(loss_row), ptr(g0), rows,
                 teacher_rows, h, w, temperature, kind)
            ctx.g0 = g0
        else:
            call('dsnt_distill_rows', ptr(s), ptr(t), ptr(loss_row), rows, teacher_rows, h, w, temperature, kind)
        out2 = torch.empty(2, device=s.device, dtype=s.dtype)
        call('dsnt_masked_avg_fwd', ptr(loss_row), ptr(m), ptr(out2), rows)
        return out2[0].clone()

    @staticmethod
    def backward(ctx, g):
        g_logits, ctx.g0 = ctx.g0, None
        if g_logits is None:
            raise RuntimeError('dsnt: distill_loss keeps its gradient for one backward pass')
        call('dsnt_scale_by_scalar', ptr(g_logits), ptr(f32(g).contiguous().view(1)), g_logits.numel())
        return g_logits, None, None, None, None


def distill_loss(student_logits, teacher_logits, mask=None, kind='kl', temperature=1.0):
    """Average distillation loss between a student's and a teacher's heat-map LOGITS (`[..., J, H, W]`, before any softmax).

    Per `(…, joint)` row, with `lq = log_softmax(student / T)`, `lp = log_softmax(teacher / T)` over the `H * W` pixels,
    `q = exp(lq)`, `p = exp(lp)` and `T = temperature > 0`:
      * `kind='kl'`:  `T^2 sum p (lp - lq)`, KL(teacher || student), the usual distillation term.  Mind the order: it is the
        opposite of `kl_reg_loss`, which is KL(heat-map || target);
      * `kind='js'`:  `T^2` times the Jensen-Shannon divergence of p and q;
      * `kind='mse'`: `T^2 sum (q - p)^2`.
    Everything is formed in the log domain from the logits: there is no `eps`, and a pixel whose probability underflows
    contributes 0.  `teacher_logits` has the student's shape, or the shape of its trailing dimensions, which the student's
    leading dimensions then repeat (student `[S, B, J, H, W]` against teacher `[B, J, H, W]`: nothing is expanded in
    memory); anything else raises `ValueError`.  `mask` broadcasts to the student's `[..., J]`; the result is
    `masked_average(rows, mask)` over all student rows.  The teacher is treated as a constant: it gets no gradient,
    whatever it requires.  Device tensors only."""
    if kind not in DISTILL_KINDS:
        raise ValueError('dsnt: distill_loss: unknown kind %r (one of %s)' % (kind, ', '.join(sorted(DISTILL_KINDS))))
    ss, ts = tuple(student_logits.shape), tuple(teacher_logits.shape)
    if len(ss) < 3 or len(ts) < 3 or len(ts) > len(ss) or ss[len(ss) - len(ts):] != ts:
        raise ValueError('dsnt: distill_loss: teacher logits %s do not match student logits %s ([..., J, H, W]: the same '
                         'shape, or that of its trailing dimensions)' % (ts, ss))
    return _DistillLoss.apply(student_logits, teacher_logits.detach(), mask, DISTILL_KINDS[kind], float(temperature))
