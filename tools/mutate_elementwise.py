"""Sensitivity of tests/test_elementwise_edges_gpu.py: build libdsnt_hip.so from a scratch copy of csrc/ that carries ONE
change in resample.hip (a, c), optim.hip (e, f), bn.hip (d, g) or ew_bodies.h (b), outside the tree, and print its path.  The module run against it must FAIL:

    python3 tools/mutate_elementwise.py a|b|c|d|e|f|g <empty scratch directory>          # build (no GPU needed)
    DSNT_HIP_LIB=<printed path> python3 -m pytest -m gpu tests/test_elementwise_edges_gpu.py

     what changes                                                                  which tests fail (nothing else does)
  a  maxpool2_fwd_kernel: `V.x > m.x` -> `>=` (the LAST of equal maxima wins)       test_maxpool2_on_ties (all five)
  b  the same in tile_op_stats_body<0> only (dsnt_maxpool2_fwd_stats)               test_maxpool2_on_ties (all five: fused vs plain bytes)
  c  maxpool3s2_fwd_kernel: `v.x > m.x` -> `>=`                                     test_maxpool3s2_on_ties (all twelve)
  d  FIXED apply: the second element in flight computed with relu = 0              test_apply_fixed_two_in_flight_loop_and_tail,
                                                                                   test_apply_pro_two_in_flight_at_the_capped_grid (both)
  e  rmsprop_kernel loses its weight-decay fma                                     test_rmsprop_three_steps (the two weight_decay = 1e-4
                                                                                   settings), test_guarded_steps_...[rmsprop]
  f  sgd_kernel: `momentum * buf[i] + gi` -> `momentum * gi + buf[i]`               test_sgd_three_steps (the four momentum = 0.9 settings),
                                                                                   test_guarded_steps_...[sgd]
  g  tile_reduce_kernel: the final combine loop stops at `rpar - 1`                test_tile_reductions and test_fused_producers_equal_bn_stats
                                                                                   (seven of the eight shapes each — dsnt_bn_stats is their
                                                                                   yardstick; with one row in all, the dropped partial is zero)

Values and skipped work only: no mutation touches an address, a bound or a loop limit in a way that could read or write outside a
tensor (g reads one lane partial FEWER).  The header mutation (b) rebuilds every source that includes ew_bodies.h.  Nothing here
changes the product."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dsnt-pose2d_amd', 'csrc')
MUTATIONS = {
    'a': ('resample.hip', 'if (V.x > m.x || V.x != V.x) { m.x = V.x; k.x = P; }', 'if (V.x >= m.x || V.x != V.x) { m.x = V.x; k.x = P; }'),
    'b': ('ew_bodies.h', 'if (V.x > v.x || V.x != V.x) { v.x = V.x; k.x = P; }', 'if (V.x >= v.x || V.x != V.x) { v.x = V.x; k.x = P; }'),
    'c': ('resample.hip', 'if (v.x > m.x || v.x != v.x) { m.x = v.x; k.x = p; }', 'if (v.x >= m.x || v.x != v.x) { m.x = v.x; k.x = p; }'),
    'd': ('bn.hip', 'o1 = bn_apply_one(g1, x1, v, relu);', 'o1 = bn_apply_one(g1, x1, v, 0);'),
    'e': ('optim.hip', '        if (wd != 0.f) gi = fmaf(wd, pi, gi);\n        const float s = alpha * sq[i]', '        const float s = alpha * sq[i]'),
    'f': ('optim.hip', 'momentum * buf[i] + gi', 'momentum * gi + buf[i]'),
    'g': ('bn.hip', 'for (int j = 0; j < rpar; ++j)', 'for (int j = 0; j < rpar - 1; ++j)'),
}


def main(which, out):
    name, old, new = MUTATIONS[which]
    os.makedirs(out, exist_ok=True)
    assert os.path.realpath(out) != os.path.realpath(CSRC) and not os.listdir(out), 'need an empty directory outside csrc/'
    src = os.path.join(out, 'dsnt-pose2d_amd', 'csrc')
    shutil.copytree(os.path.join(ROOT, 'include'), os.path.join(out, 'include'))
    # csrc/build/ (the objects of the in-tree build) is copied with its file times, so build.py compiles only what the change
    # reaches; the build_<name>/ directories of experiment libraries and the libraries themselves stay behind
    shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns('build_*', '*.so'))
    shutil.copy(os.path.join(ROOT, 'dsnt-pose2d_amd', 'build.py'), os.path.join(out, 'dsnt-pose2d_amd', 'build.py'))
    path = os.path.join(src, name)
    text = open(path).read()
    assert text.count(old) == 1, 'mutation %s: pattern found %d times' % (which, text.count(old))
    open(path, 'w').write(text.replace(old, new))
    subprocess.check_call([sys.executable, os.path.join(out, 'dsnt-pose2d_amd', 'build.py')], stdout=subprocess.DEVNULL)
    print(os.path.join(src, 'libdsnt_hip.so'))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
