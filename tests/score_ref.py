"""numpy restatement of dsnt_score_hist and dsnt_score_lookup (csrc/pckh.hip; rules in DESIGN.md section 19), and the
inputs of tests/test_reliability_cpu.py and tests/test_reliability_gpu.py.

The table is `[J][S + 2][T + 1]`: the score row of a joint against `dsnt_pckh_hist`'s distance column.  Row r is the number
of score edges <= the score (fp32 widened to fp64), so a score on an edge belongs to the row above it; NaN scores go to
row S + 1.  Everything here is fp64 numpy on the host.
"""
import numpy as np


def f32(values):
    """Edges and thresholds as the evaluators hold them: the fp64 values of their fp32 roundings."""
    return np.asarray(values, np.float64).astype(np.float32).astype(np.float64)


EDGES20 = f32(2.0 ** (-10 + np.arange(20) / 2))               # 2^-10 .. 2^-0.5, half an octave apart
THR3, THR1, THR15 = f32([0.1, 0.2, 0.5]), f32([0.5]), f32(np.arange(1, 16) / 30)


def distance(pred, target, m, b, head):
    """`pckh_distance`: bmm(x, m) + b on row vectors in fp64, the distance over the head length."""
    with np.errstate(all='ignore'):
        p = np.einsum('bji,bik->bjk', pred.astype(np.float64), m) + b[:, None, :]
        t = np.einsum('bji,bik->bjk', target.astype(np.float64), m) + b[:, None, :]
        return np.sqrt((p[..., 0] - t[..., 0]) ** 2 + (p[..., 1] - t[..., 1]) ** 2) / head[:, None]


def column(d, thr):
    """`dsnt_pckh_hist`'s bin: the first threshold d does not exceed; T for NaN, inf and anything beyond the last."""
    k = np.searchsorted(thr, np.where(np.isfinite(d), d, 0.0), side='left')
    k[~np.isfinite(d)] = len(thr)
    return k


def row(score, edges):
    """The number of edges <= the score; S + 1 for a NaN.  (searchsorted's side='right' counts the edges <= s.)"""
    s = np.asarray(score, np.float32).astype(np.float64)
    r = np.searchsorted(edges, np.where(np.isnan(s), 0.0, s), side='right')
    r[np.isnan(s)] = len(edges) + 1
    return r


def restate(pred, target, m, b, mask, head, score, edges, thr):
    """The table int64 [J, S + 2, T + 1] of one batch."""
    B, J = mask.shape
    k, r = column(distance(pred, target, m, b, head), thr), row(score, edges)
    valid = mask == 1
    table = np.zeros((J, len(edges) + 2, len(thr) + 1), np.int64)
    jj = np.broadcast_to(np.arange(J), (B, J))
    np.add.at(table, (jj[valid], r[valid], k[valid]), 1)
    return table


def restate_loop(pred, target, m, b, mask, head, score, edges, thr):
    """The same table by a plain double loop over samples and joints, comparison by comparison."""
    B, J = mask.shape
    S, T = len(edges), len(thr)
    table = np.zeros((J, S + 2, T + 1), np.int64)
    for n in range(B):
        for j in range(J):
            if mask[n, j] != 1:
                continue
            with np.errstate(all='ignore'):
                p = pred[n, j].astype(np.float64) @ m[n] + b[n]
                t = target[n, j].astype(np.float64) @ m[n] + b[n]
                d = np.sqrt(((p - t) ** 2).sum()) / head[n]
            k = T
            for q in range(T - 1, -1, -1):
                if d <= thr[q]:
                    k = q
            s = float(score[n, j])
            r = S + 1 if s != s else sum(1 for e in edges if e <= s)
            table[j, r, k] += 1
    return table


def lookup(score, edges, values, per_joint):
    """`dsnt_score_lookup`: values[joint][row(score)] for a score array [..., J]."""
    r = row(score, edges)
    J = score.shape[-1]
    j = np.broadcast_to(np.arange(J), score.shape) if per_joint else np.zeros(score.shape, np.int64)
    return values[j, r]


def case(B, J, seed):
    """`_case` of tests/test_pckh_curve_gpu.py (about half the predictions within 0.5 head lengths, a non-symmetric
    transform per image, masks of 0, 1, 0.5 and 2), then a score drawn after the other arrays that tracks the error:
    0.5 * exp(-2 d + N(0, 0.35)) in f32.  Returns (pred, target, m, b, mask, head, score)."""
    r = np.random.default_rng(seed)
    target = r.uniform(-0.9, 0.9, (B, J, 2)).astype(np.float32)
    pred = (target + r.normal(0, 0.2, (B, J, 2))).astype(np.float32)
    m = np.array([[150.0, 90.0], [-20.0, 60.0]]) + r.uniform(-10, 10, (B, 2, 2))
    b = r.uniform(0, 400, (B, 2))
    head = r.uniform(40, 120, B)
    mask = r.choice(np.array([0, 1, 1, 1, 0.5, 2], np.float32), (B, J))
    d = distance(pred, target, m, b, head)
    score = (0.5 * np.exp(-2.0 * d + r.normal(0, 0.35, (B, J)))).astype(np.float32)
    return pred, target, m, b, mask, head, score


def awkward(pred, target, m, b, mask, head, device='cpu'):
    """The first six arrays of `case` as tensors on `device` in the argument order of `add_normalized`, in forms the kernels
    cannot take: `pred` a strided fp64 view, `target` and `mask` fp64, `head` f32, `transform_m` a transposed view and
    `transform_b` f32 `[B, 1, 2]` (tests/test_evaluator_shared_cpu.py, tests/test_evaluator_shared_gpu.py)."""
    import torch
    wide = torch.zeros(pred.shape[:2] + (4,), dtype=torch.float64, device=device)
    wide[..., ::2] = torch.from_numpy(pred).to(device)
    m_t = torch.from_numpy(m).to(device).transpose(1, 2).contiguous().transpose(1, 2)
    out = (wide[..., ::2], torch.from_numpy(target).double().to(device), torch.from_numpy(mask).double().to(device),
           torch.from_numpy(head).float().to(device), m_t,
           torch.from_numpy(b).float().reshape(pred.shape[0], 1, 2).to(device))
    assert not out[0].is_contiguous() and not out[4].is_contiguous()
    return out


def clear_of_thresholds(d, thr):
    """No distance within 1e-9 relative of a threshold, so that an fp64 contraction difference moves no joint across a
    bin edge.  (Score rows need no margin: fp32 scores against fp32-valued edges compare exactly.)"""
    return bool((np.abs(d[..., None] - thr) > 1e-9 * thr).all())


def case_is_clear(args, thr):
    return clear_of_thresholds(distance(args[0], args[1], args[2], args[3], args[5]), thr)
