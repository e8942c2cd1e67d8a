"""How far from centred are the inputs of the BatchNorms?  The largest |mean| * invstd (channel mean against channel spread, fp64,
biased variance + eps) that any BatchNorm input of an oracle model shows, at synthetic.fill_state_dict initialisation and after ten
oracle optimiser steps (RMSprop, lr 2.5e-4, a fresh synthetic batch per step).  CPU only, forward hooks on the oracle's
nn.BatchNorm2d modules.  The number to read beside DESIGN.md's table of what the one-pass tile sums cost in invstd.

    python3 tools/bn_offset_survey.py [--bases hg2,resnet34] [--batch 4] [--size 128] [--steps 10]"""
import argparse
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dsnt-pose2d_amd'), os.path.join(ROOT, 'oracle')):
    sys.path.insert(0, p)
from dsnt import synthetic                      # noqa: E402
from dsnt_oracle import model as omodel         # noqa: E402


def survey(base, batch, size, steps):
    kw = dict(output_strat='dsnt', reg='js') if base.startswith('hg') else dict(output_strat='dsnt')
    m = omodel.build_mpii_pose_model(base=base, **kw)
    synthetic.fill_state_dict(m, seed=0)
    m.train()
    seen = {}

    def hook(mod, inp):
        x = inp[0].detach().double()
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        r = mean.abs() / torch.sqrt(var + mod.eps)
        k = int(r.argmax())
        if float(r[k]) > seen.get('ratio', -1.0):
            seen.update(ratio=float(r[k]), name=names[mod], channel=k, rows=x.numel() // x.shape[1])
    names = {mod: n for n, mod in m.named_modules() if isinstance(mod, nn.BatchNorm2d)}
    for mod in names:
        mod.register_forward_pre_hook(hook)
    opt = torch.optim.RMSprop(m.parameters(), lr=2.5e-4)
    out = []
    for step in range(steps + 1):
        seen.clear()
        x, t, k = synthetic.batch(batch, size=size, seed=1 + step, mask_p=0.9)
        loss = m.forward_loss(m(x), t, k)
        out.append(dict(seen))
        if step < steps:
            opt.zero_grad()
            loss.backward()
            opt.step()
    return len(names), out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--bases', default='hg2,resnet34')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--steps', type=int, default=10)
    a = ap.parse_args()
    torch.manual_seed(0)
    for base in a.bases.split(','):
        n, out = survey(base, a.batch, a.size, a.steps)
        for tag, s in (('initialisation', out[0]), ('after %d steps' % a.steps, out[-1]), ('largest on the way', max(out, key=lambda d: d['ratio']))):
            print('%-9s %3d BatchNorms  %-18s max |mean| invstd = %7.3f   (%s, channel %d, %d rows)' % (
                base, n, tag, s['ratio'], s['name'], s['channel'], s['rows']))
