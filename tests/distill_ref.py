"""The heat-map distillation loss in plain torch, its case matrix and its yardstick (no GPU, no fixture).

Used by tests/test_distill_cpu.py (the definition against its closed forms, fp32 against fp64) and
tests/test_distill_gpu.py (HIP against the fp64 run).  Three parts:

* `rows_loss(s, t, T, kind)`: the definition of DESIGN.md §26 per row, in the dtype of its arguments, and `run(...)`:
  values, the masked-average scalar and the gradient with respect to the student's logits by autograd.
* `cases(h, w)`: the teacher/student pairs, built from tests/head_regimes.py's `make(regime, h, w, 32)` logits.
* `ratio_rows` / `value_units`: the yardstick (below), and `k_ref(kind, sizes)`: the fp32 run's worst figures against the
  fp64 run over the whole matrix.

The yardstick.  The gradient of a row is T (q - p) for `kl` and T q (v - sum q v) for `js` and `mse`, where v is itself a
difference (lq - lm, q - p) that vanishes as the student converges: the scale of head_regimes.scale_rows, built from v,
then goes to 0 while fp32's error does not.  The error is measured against the size of the distributions instead,

    D_r = T (max_i p_i + max_i q_i),        ratio_r = max_j |g_j - g64_j| / (2^-24 D_r),

with p and q from the fp64 run.  D_r is never 0, so no row is left out.  Values are measured in the suite's unit
1e-5 max(1, |L64|), per row and for the scalar.
"""
import functools
import math

import numpy as np
import torch

import head_regimes as hr

KINDS = ('js', 'kl', 'mse')                     # kind numbers 0, 1, 2 as dsnt_reg_*
TEMPERATURES = (1.0, 2.0, 4.0)
ROWS = 32
EPS24 = 2.0 ** -24
# (teacher regime, student regime); a pair of equal regimes rolls the student's rows by 7
PAIRS = (('peaked', 'diffuse'), ('peaked', 'edge'), ('bimodal', 'peaked'), ('onehot', 'peaked'), ('peaked', 'onehot'),
         ('onehot', 'onehot'), ('edge', 'offset'), ('offset', 'straddle'), ('straddle', 'bimodal'), ('diffuse', 'diffuse'))
CONVERGED = ('peaked', 'onehot', 'bimodal', 'offset')
# map size -> the variant of csrc/distill.hip it reaches
GPU_SIZES = ((64, 64),      # cached, 16-byte accesses
             (64, 48),      # non-square
             (14, 14),      # hw % 4 == 0 but w % 4 != 0
             (7, 7),        # one float at a time
             (96, 96))      # streamed: more than 4096 pixels
SIZES = GPU_SIZES[:2] + ((16, 16),) + GPU_SIZES[2:]


# ------------------------------------------------------------------ the definition
def rows_loss(s, t, T, kind):
    """L per row of student logits `s` [R, n] against teacher logits `t` [R, n] at temperature T, in their dtype."""
    lq, lp = torch.log_softmax(s / T, -1), torch.log_softmax(t / T, -1)
    q, p = lq.exp(), lp.exp()
    if kind == 'kl':
        L = (p * (lp - lq)).sum(-1)
    elif kind == 'js':
        lm = torch.logaddexp(lp, lq) - math.log(2.0)
        L = 0.5 * (p * (lp - lm)).sum(-1) + 0.5 * (q * (lq - lm)).sum(-1)
    elif kind == 'mse':
        L = ((q - p) ** 2).sum(-1)
    else:
        raise ValueError('unknown kind %r' % (kind,))
    return T * T * L


def closed_form_grad(s, t, T, kind):
    """dL_r / ds by the closed forms of DESIGN.md §26 (teacher constant)."""
    lq, lp = torch.log_softmax(s / T, -1), torch.log_softmax(t / T, -1)
    q, p = lq.exp(), lp.exp()
    if kind == 'kl':
        return T * (q - p)
    if kind == 'js':
        v = 0.5 * (lq - (torch.logaddexp(lp, lq) - math.log(2.0)))
    else:
        v = 2.0 * (q - p)
    return T * q * (v - (q * v).sum(-1, keepdim=True))


def weights(mask, rows, dtype=torch.float64):
    """w_r of masked_average: mask_r / clamp(sum mask, 1), or 1 / rows without a mask."""
    if mask is None:
        return torch.full((rows,), 1.0 / rows, dtype=dtype)
    m = mask.reshape(-1).to(dtype)
    return m / m.sum().clamp(min=1.0)


def run(student, teacher, T, kind, mask=None, dtype=torch.float64):
    """The definition on the CPU in `dtype`.  student [R, n]; teacher [Rt, n] with R % Rt == 0 (student row r pairs with
    teacher row r % Rt).  Returns float64 numpy arrays: L [R], g = dL_r/ds [R, n] (unweighted: the gradient of sum_r L_r),
    pmax, qmax [R] (the rows' largest probabilities), and the scalar sum_r w_r L_r."""
    s = student.detach().clone().to(dtype).requires_grad_()
    t = teacher.detach().to(dtype)
    t = t.repeat(s.shape[0] // t.shape[0], 1)
    L = rows_loss(s, t, T, kind)
    L.sum().backward()
    with torch.no_grad():
        q, p = torch.softmax(s / T, -1), torch.softmax(t / T, -1)
        scalar = (L * weights(mask, L.numel(), dtype)).sum()
    f = lambda a: a.detach().double().numpy()
    return dict(L=f(L), g=f(s.grad), pmax=f(p.max(-1)[0]), qmax=f(q.max(-1)[0]), scalar=float(scalar))


# ------------------------------------------------------------------ the case matrix
@functools.lru_cache(maxsize=None)
def _pairs(h, w):
    out = []
    logits = lambda regime: hr.make(regime, h, w, ROWS)[0].reshape(ROWS, h * w)
    for tr, sr in PAIRS:
        t, s = logits(tr), logits(sr)
        if tr == sr:
            s = torch.roll(s, 7, 0)
        out.append(('%s/%s' % (tr, sr), t, s))
    gen = torch.Generator().manual_seed(h * 1000 + w)
    for regime in CONVERGED:
        t = logits(regime)
        if regime == 'bimodal':
            s = t.clone()
        elif regime == 'offset':
            s = t + 37.5                       # shift invariance: the true value is 0
        else:
            s = t + 1e-3 * torch.randn(t.shape, generator=gen)
        out.append(('%s/converged' % regime, t, s))
    return tuple(out)


def cases(h, w):
    """[(name, teacher [32, hw], student [32, hw], T)]: every pair at every temperature, fp32 CPU tensors."""
    return [(name, t.clone(), s.clone(), T) for name, t, s in _pairs(h, w) for T in TEMPERATURES]


def mask_of(h, w):
    """A mask [32] with both kinds of row (head_regimes' own)."""
    return hr.make('peaked', h, w, ROWS)[2].reshape(ROWS)


@functools.lru_cache(maxsize=None)
def reference(h, w, kind):
    """The fp64 run(...) of every case of cases(h, w), computed once and shared: treat as read-only."""
    return tuple(run(s, t, T, kind) for _, t, s, T in cases(h, w))


# ------------------------------------------------------------------ the yardstick
def scale_rows(o64, T):
    return T * (o64['pmax'] + o64['qmax'])


def ratio_rows(g, o64, T, w=None):
    """max_j |g_j - w_r g64_j| / (2^-24 w_r D_r) per row.  `w`: the row weights g carries (None: unweighted); a row of
    weight 0 gives 0 for an exact 0 and inf otherwise.  A non-finite g gives inf."""
    g = np.asarray(g, dtype=np.float64)
    w = np.ones(g.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    err = np.abs(g - w[:, None] * o64['g']).max(-1)
    err = np.where(np.isfinite(err), err, np.inf)
    S = EPS24 * w * scale_rows(o64, T)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = err / S
    return np.where(S > 0, r, np.where(err == 0, 0.0, np.inf))


def value_units(got, want):
    """|got - want| / (1e-5 max(1, |want|)), elementwise; non-finite gives inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    u = np.abs(got - want) / (1e-5 * np.maximum(1.0, np.abs(want)))
    return np.where(np.isfinite(u), u, np.inf)


@functools.lru_cache(maxsize=None)
def k_ref_table(kind, sizes=SIZES):
    """{(h, w, case name, T): (gradient ratio, value units)} of the fp32 run against the fp64 run."""
    out = {}
    for h, w in sizes:
        for (name, t, s, T), o64 in zip(cases(h, w), reference(h, w, kind)):
            o32 = run(s, t, T, kind, None, torch.float32)
            grad = float(ratio_rows(o32['g'], o64, T).max())
            val = max(float(value_units(o32['L'], o64['L']).max()), float(value_units(o32['scalar'], o64['scalar'])))
            out[(h, w, name, T)] = (grad, val)
    return out


def k_ref(kind, sizes=SIZES):
    """(gradient K_ref, value K_ref): the fp32 run's worst figures over the whole matrix of `sizes`."""
    tab = k_ref_table(kind, tuple(sizes))
    return max(v[0] for v in tab.values()), max(v[1] for v in tab.values())
