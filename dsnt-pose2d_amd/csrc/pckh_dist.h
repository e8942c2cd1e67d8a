// The PCKh distance (evaluator.py:66, train.py:243-258): the one fp64 expression behind every evaluator of pckh.hip and
// the per-example scores of sampler.hip.  Contraction is pinned to the compiler's default for device code inside these
// functions, so a unit built with -ffp-contract=off (sampler.hip) holds the very instructions pckh.hip holds.
#pragma once

// Distance of joint i (of image n) between the back-projected prediction and target, in head lengths: one expression for
// pckh_kernel, joint_table_kernel and error_field_kernel, so that the curve at a threshold holds the very hits of the
// single-threshold kernel and the field's misses are exactly its non-hits.
__device__ __forceinline__ double pckh_distance(const float* __restrict__ pred, const float* __restrict__ target,
                                                const double* __restrict__ m, const double* __restrict__ b,
                                                const double* __restrict__ head, long i, long n) {
#pragma clang fp contract(fast)
    const double* mm = m + (size_t)n * 4;
    const double* bb = b + (size_t)n * 2;
    const double px = pred[2 * i], py = pred[2 * i + 1], tx = target[2 * i], ty = target[2 * i + 1];
    // row-vector times matrix plus offset (train.py:243-258: bmm(norm, transform_m) + transform_b)
    const double ox = px * mm[0] + py * mm[2] + bb[0], oy = px * mm[1] + py * mm[3] + bb[1];
    const double gx = tx * mm[0] + ty * mm[2] + bb[0], gy = tx * mm[1] + ty * mm[3] + bb[1];
    return sqrt((ox - gx) * (ox - gx) + (oy - gy) * (oy - gy)) / head[n];
}
// The two-index form of that expression, for the kernels that hold one point against many: prediction j against the
// target of every joint k of its person (joint_confusion_kernel), the centre of every pixel against a target
// (target_mass_kernel).  It comes in the expression's two halves, so that a point is back-projected once and not once
// per pair: pckh_distance(i, n) is pckh_between(pckh_project(pred i), pckh_project(target i), head[n]), operation for
// operation and in the same order.
struct pckh_point { double x, y; };
__device__ __forceinline__ pckh_point pckh_project(double x, double y, const double* __restrict__ mm,
                                                   const double* __restrict__ bb) {
#pragma clang fp contract(fast)
    return {x * mm[0] + y * mm[2] + bb[0], x * mm[1] + y * mm[3] + bb[1]};
}
__device__ __forceinline__ double pckh_between(const pckh_point o, const pckh_point g, double head) {
#pragma clang fp contract(fast)
    return sqrt((o.x - g.x) * (o.x - g.x) + (o.y - g.y) * (o.y - g.y)) / head;
}
