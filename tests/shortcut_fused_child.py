"""Child process of tests/test_shortcut_fused_inmodel_gpu.py (not collected by pytest: no test_ prefix).

The library reads its row thresholds once per process, and the engine reads DSNT_X_DS_FUSE_ROWS / DSNT_OFF when a tape is
created, so putting conv3 + projection shortcut of the stem on the fused forward launch (csrc/fwd1.hip DS) in the oracle-sized
models needs a process of its own.  Runs the cases it is given, each the very function
of tests/test_model_gpu.py where there is one, and reports per case: ok / the failure, and the launch census of the train-mode
tapes the case built.

usage: python tests/shortcut_fused_child.py <case,case,...> <result.json> [<dump.pt>]
  golden       the hg2_128 golden vectors
  grads:smooth / grads:relu   hg2's every-gradient check against the oracle
  dump         loss, coordinates and every gradient of one hg2 step (batch 4, 128 px) -> <dump.pt>
"""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, 'dsnt-pose2d_amd'), os.path.join(ROOT, 'oracle')]

DS_GEOMS = {(128, 64), (256, 128)}       # (Cout, Cin) of the two projection shortcuts of the stem


def census(models):
    """Per train-mode tape: fused forward launches, and stand-alone shortcut launches (forward; backward) of the stem's two
    geometries."""
    out = []
    for m in models:
        root = m.hg if hasattr(m, 'hg') else m
        for prog in root._runner().programs.values():
            if not (prog.record and prog.training):
                continue
            rep = dict(fwd_ds=0, ds_fwd=0, ds_bwd=0)
            for e in prog.tape.fwd:
                if e[0] is None:
                    continue
                if e[2] == 'dsnt_conv1x1_fwd_ds_f16x3':
                    rep['fwd_ds'] += 1
                elif e[2] == 'dsnt_conv1x1_fwd_f16x3':
                    g = e[1][-2]._obj
                    if (g.Cout, g.Cin) in DS_GEOMS and e[1][7] is None:         # a raw operand: the shortcut
                        rep['ds_fwd'] += 1
            for e in prog.tape.bwd:
                if e[0] is None:
                    continue
                if e[2] == 'dsnt_conv1x1_bwd_f16x3':
                    g = e[1][-1]._obj
                    if (g.Cout, g.Cin) in DS_GEOMS and not e[1][0]._obj.scale:
                        rep['ds_bwd'] += 1
            out.append(rep)
    return out


def dump(path):
    import torch
    from dsnt import synthetic
    from dsnt.model import build_mpii_pose_model
    m = build_mpii_pose_model(base='hg2', output_strat='dsnt', reg='js')
    synthetic.fill_state_dict(m, seed=3)
    m.cuda().train()
    x, target, mask = synthetic.batch(4, size=128, seed=2, mask_p=0.8)
    outs = m(x.cuda())
    loss = m.forward_loss(outs, target.cuda(), mask.cuda())
    loss.backward()
    torch.cuda.synchronize()
    torch.save(dict(loss=loss.detach().cpu(), coords=[o.detach().cpu() for o in outs],
                    grads={n: p.grad.detach().cpu() for n, p in m.named_parameters()}), path)


def main(cases, out_path, dump_path=None):
    import dsnt.model as dmodel
    built = []
    real = dmodel.build_mpii_pose_model

    def recording(*a, **k):
        m = real(*a, **k)
        built.append(m)
        return m
    dmodel.build_mpii_pose_model = recording
    import test_model_gpu as tm
    report = {}
    for case in cases.split(','):
        del built[:]
        try:
            if case == 'golden':
                tm.test_end_to_end_vs_golden('hg2', 128, 'js', 'hg2_128', 'f16x3')
            elif case == 'grads:smooth':
                tm.test_hg2_every_gradient_vs_oracle(True)
            elif case == 'grads:relu':
                tm.test_hg2_every_gradient_vs_oracle(False)
            elif case == 'dump':
                dump(dump_path)
            else:
                raise SystemExit('unknown case ' + case)
            report[case] = dict(ok=True, census=census(built))
        except Exception:
            report[case] = dict(ok=False, error=traceback.format_exc()[-3000:], census=[])
            if not isinstance(sys.exc_info()[1], AssertionError):
                break               # (not a failed check: nothing more is started on the device)
    with open(out_path, 'w') as f:
        json.dump(report, f)


if __name__ == '__main__':
    main(*sys.argv[1:4])
