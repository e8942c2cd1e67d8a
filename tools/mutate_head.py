"""Sensitivity of tests/test_head_regimes_gpu.py: build libdsnt_hip.so from a scratch copy of csrc/ whose head_loss.hip
carries ONE arithmetic change in head_loss_grad_kernel, outside the tree, and print its path.  The regime tests run
against it must FAIL:

    python3 tools/mutate_head.py a|b|c <empty scratch directory>          # build (no GPU needed)
    DSNT_HIP_LIB=<printed path> python3 -m pytest -m gpu tests/test_head_regimes_gpu.py

  a  the `far` threshold of the JS shortcut 1e-30f -> 1e-12f (the target Gaussian treated as underflowed where it is not)
  b  `elem` (the general JS path) loses its `- m * rcp(m + REG_EPS)` term
  c  x and y exchanged where head_loss_grad_kernel has no position table (tab == false: w + h > HEAD_SEP_MAX)

Arithmetic only: no mutation touches an index, an address or a bound.  Nothing here changes the product."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dsnt-pose2d_amd', 'csrc')
MUTATIONS = {
    'a': ('far = qmax < 1e-30f;', 'far = qmax < 1e-12f;'),
    'b': ('0.5f * (fmaf(LN2, dp, p * __builtin_amdgcn_rcpf(p + REG_EPS)) - m * __builtin_amdgcn_rcpf(m + REG_EPS)));',
          '0.5f * (fmaf(LN2, dp, p * __builtin_amdgcn_rcpf(p + REG_EPS))));'),
    'c': ('                float x, y; g.xy(i, x, y);\n                one(slot, p, x, y);',
          '                float x, y; g.xy(i, x, y);\n                one(slot, p, tab ? x : y, tab ? y : x);'),
}


def main(which, out):
    old, new = MUTATIONS[which]
    os.makedirs(out, exist_ok=True)
    assert os.path.realpath(out) != os.path.realpath(CSRC) and not os.listdir(out), 'need an empty directory outside csrc/'
    inc = os.path.join(out, 'include')
    src = os.path.join(out, 'dsnt-pose2d_amd', 'csrc')
    shutil.copytree(os.path.join(ROOT, 'include'), inc)
    # csrc/build/ (the objects of the in-tree build) is copied with its file times, so build.py compiles head_loss.hip alone;
    # only the build_<name>/ directories of experiment libraries and the libraries themselves stay behind
    shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns('build_*', '*.so'))
    shutil.copy(os.path.join(ROOT, 'dsnt-pose2d_amd', 'build.py'), os.path.join(out, 'dsnt-pose2d_amd', 'build.py'))
    path = os.path.join(src, 'head_loss.hip')
    text = open(path).read()
    assert text.count(old) == 1, 'mutation %s: pattern found %d times' % (which, text.count(old))
    open(path, 'w').write(text.replace(old, new))
    subprocess.check_call([sys.executable, os.path.join(out, 'dsnt-pose2d_amd', 'build.py')], stdout=subprocess.DEVNULL)
    print(os.path.join(src, 'libdsnt_hip.so'))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
