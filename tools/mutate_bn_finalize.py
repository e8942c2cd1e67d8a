"""Sensitivity of tests/test_bn_finalize_gpu.py: build libdsnt_hip.so from a scratch copy of csrc/ that carries ONE change to the
BatchNorm finalise step in bn.hip (a, b) or bn_pro.h (b, c), outside the tree, and print its path.  The module run against it
must FAIL:

    python3 tools/mutate_bn_finalize.py a|b|c <empty scratch directory>          # build (no GPU needed)
    DSNT_HIP_LIB=<printed path> python3 -m pytest -m gpu tests/test_bn_finalize_gpu.py

     what changes                                                              which tests fail (measured on an MI355X; the rest pass)
  a  bn_finalize_kernel: the lane stride `t += FIN_P` -> `FIN_P + 1` (tiles         test_bn_finalize and test_bn_bwd_finalize: all ten cases of 65 tiles
     dropped from the second trip on)                                             or more each; test_bn_bwd_finalize_bound: the three of 65 or more
  b  the combine's accumulators are `float` (bn_finalize_kernel's a0 / a1 and      test_bn_finalize 14 of 15, test_bn_bwd_finalize 13 of 15, test_bn_bwd_
     bn_pro_sums' lane sum)                                                       finalize_bound 5 of 5, test_conv_prologue_finalises_... 18 of 30,
                                                                                 test_apply_prologue_finalises_... 19 of 30: every cancelling case and
                                                                                 most producer ones of many tiles (one tile has nothing to combine)
  c  bn_pro_forward: every workgroup moves the running statistics               test_conv_prologue_moves_the_running_statistics_once_at_a_full_grid,
                                                                                 both kernels.  (NOT the launches of three or four workgroups in
                                                                                 test_conv_prologue_finalises_...: they start together, read the old
                                                                                 pair together and store the same value — why the full-grid test exists.)

Values and skipped work only: no mutation touches an address or a bound in a way that could read or write outside a tensor (a reads
FEWER tiles; c writes the elements workgroup 0 writes anyway).  A header mutation rebuilds every source that includes it.  Nothing
here changes the product."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dsnt-pose2d_amd', 'csrc')
MUTATIONS = {
    'a': [('bn.hip', 'for (int t = part; t < ntiles; t += FIN_P) {', 'for (int t = part; t < ntiles; t += FIN_P + 1) {')],
    'b': [('bn.hip', '    double a0[VP], a1[VP];\n', '    float a0[VP], a1[VP];\n'),
          ('bn_pro.h', '        double a = 0.0;\n        if (lane < L) {', '        float a = 0.f;\n        if (lane < L) {')],
    'c': [('bn_pro.h', '__device__ __forceinline__ void bn_pro_forward(const BnProP& q, double* sh, bool writer) {\n',
           '__device__ __forceinline__ void bn_pro_forward(const BnProP& q, double* sh, bool writer) {\n    writer = true;\n')],
}


def main(which, out):
    os.makedirs(out, exist_ok=True)
    assert os.path.realpath(out) != os.path.realpath(CSRC) and not os.listdir(out), 'need an empty directory outside csrc/'
    src = os.path.join(out, 'dsnt-pose2d_amd', 'csrc')
    shutil.copytree(os.path.join(ROOT, 'include'), os.path.join(out, 'include'))
    # csrc/build/ (the objects of the in-tree build) is copied with its file times, so build.py compiles only what the change
    # reaches; the build_<name>/ directories of experiment libraries and the libraries themselves stay behind
    shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns('build_*', '*.so'))
    shutil.copy(os.path.join(ROOT, 'dsnt-pose2d_amd', 'build.py'), os.path.join(out, 'dsnt-pose2d_amd', 'build.py'))
    for name, old, new in MUTATIONS[which]:
        path = os.path.join(src, name)
        text = open(path).read()
        assert text.count(old) == 1, 'mutation %s: pattern found %d times in %s' % (which, text.count(old), name)
        open(path, 'w').write(text.replace(old, new))
    subprocess.check_call([sys.executable, os.path.join(out, 'dsnt-pose2d_amd', 'build.py')], stdout=subprocess.DEVNULL)
    print(os.path.join(src, 'libdsnt_hip.so'))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
