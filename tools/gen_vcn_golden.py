#!/usr/bin/env python3
"""Generate tests/golden/vcn/ by IMPORTING the reference's VCN (third_party/ext_nnutils/VCNplus.py) and running it on the CPU.

    python tools/gen_vcn_golden.py --reference PATH_TO_REFERENCE_CHECKOUT

The model is filled with tests/vcn_restated.py's vcn_test_weights (so no weight file is committed) and run on its
input_pair(), 320x384, in eval mode, with flow_reg / WarpModule rebuilt for that size as auto_gen.py:109-116 does.  kornia and
cv2 are imported by VCNplus.py / submodule.py but not used on the inference path; they are stubbed.  Written:
  state_dict.json  [[name, shape], ...] of the reference's state_dict
  final.npz        flow [1,2,320,384], occ [80,96]
  levels.npz       flow<l> [1,2,h,w] of every level l = 0..4; flowh<l>, enth<l> of levels 0-2
Only this generator reads the reference; no test does.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import vcn_restated as R                           # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'vcn')


def import_reference(ref):
    for name in ('kornia', 'cv2'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, os.path.join(ref, 'third_party'))
    from ext_nnutils import VCNplus
    return VCNplus


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference checkout (holds third_party/ext_nnutils)')
    args = ap.parse_args()
    V = import_reference(args.reference)
    torch.manual_seed(0)
    H, W = R.PAIR_SHAPE
    model = V.VCN([1, 256, 256], md=[4, 4, 4, 4, 4], fac=1.)
    names = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    R.fill_state_dict(model)
    for i in range(len(model.reg_modules)):                 # auto_gen.py:109-116
        old = getattr(model, 'flow_reg%d' % 2 ** (6 - i))
        model.reg_modules[i] = V.flow_reg([1, W // 2 ** (6 - i), H // 2 ** (6 - i)], ent=old.ent, maxdisp=old.md, fac=old.fac)
    for i in range(len(model.warp_modules)):
        model.warp_modules[i] = V.WarpModule([1, W // 2 ** (6 - i), H // 2 ** (6 - i)])
    model.eval()

    rec = {}
    orig = model.cost_matching

    def cost_matching(up_flow, c1, c2, flowh, enth, level):
        out = orig(up_flow, c1, c2, flowh, enth, level)
        rec['flow%d' % level] = out[0].numpy()
        if level <= 2:
            rec['flowh%d' % level] = out[1].numpy()
            rec['enth%d' % level] = out[2].numpy()
        return out
    model.cost_matching = cost_matching

    im = R.pair_input(*R.input_pair())
    with torch.no_grad():
        flow, occ = model(im)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'state_dict.json'), 'w') as fh:
        json.dump(names, fh, separators=(',', ':'))
    np.savez_compressed(os.path.join(OUT, 'final.npz'), flow=flow.numpy(), occ=occ.numpy())
    np.savez_compressed(os.path.join(OUT, 'levels.npz'), **rec)
    for n in sorted(os.listdir(OUT)):
        print(n, os.path.getsize(os.path.join(OUT, n)))
    print('entries %d, parameters %d' % (len(names), sum(p.numel() for p in model.parameters())))


if __name__ == '__main__':
    main()
