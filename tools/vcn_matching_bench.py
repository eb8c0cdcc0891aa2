#!/usr/bin/env python3
"""Time and memory of VCN's matching stage on the GPU, fused kernels against the reference-shaped torch path.

    python tools/vcn_matching_bench.py [--height 1088 --width 1920] [--reps 5] [--json out.json]

For one padded pair (random weights, as auto_gen.py's dry run) it records the ms of a whole flow_inference-sized forward; then,
per level, on that forward's own features, the ms and the peak torch.cuda.max_memory_allocated of
  fused:     vcn.corr_proj (+ ReLU) and vcn.flow_reg (csrc/vcn.hip)
  reference: tests/vcn_restated.py's corr_proj_reference_shaped and flow_reg_reference_shaped (the dense cost volume)
each measured from a clean allocator peak.  Run it under rocprofv3 --kernel-trace --stats for per-kernel times.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import vcn_restated as R                           # noqa: E402
from lasr_amd.ext_nnutils import vcn               # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return sorted(t)[len(t) // 2]


def peak(fn, base):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=1088)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip_reference', action='store_true')
    ap.add_argument('--json', default='')
    a = ap.parse_args()
    dev = 'cuda'
    torch.manual_seed(0)
    model = R.fill_state_dict(vcn.VCN()).eval().to(dev)
    im = torch.randn(2, 3, a.height, a.width, device=dev)
    rec = {'size': [a.height, a.width]}
    with torch.no_grad():
        t0 = time.time()
        model(im)
        torch.cuda.synchronize()
        rec['first_forward_ms'] = (time.time() - t0) * 1e3
        rec['forward_ms'] = timed(lambda: model(im), a.reps)
        torch.cuda.reset_peak_memory_stats()
        model(im)
        torch.cuda.synchronize()
        rec['forward_peak_mib'] = torch.cuda.max_memory_allocated() / 2 ** 20
        feats = model.pspnet(im)
        _, _, levels = model(im, return_levels=True)
        rows = []
        for lvl, c in enumerate(feats):
            c1, c2 = c[:1].contiguous(), c[1:].contiguous()
            h, w = c1.shape[2:]
            up = None if lvl == 0 else F.interpolate(levels[lvl - 1][0], [h, w], mode='bilinear', align_corners=False) * 2
            bf = getattr(model, 'f' + model.LEVELS[lvl])
            W, sc, sh = bf.projection()
            W, sc, sh = W.detach().contiguous(), sc.detach().contiguous(), sh.detach().contiguous()
            md, mdv = model.md[lvl], model.mdv(lvl)
            cost = getattr(model, 'p' + model.LEVELS[lvl])(bf(F.relu(vcn.corr_proj(c1, c2, up, W, sc, sh, md, mdv))))
            base = torch.cuda.memory_allocated()
            row = {'level': lvl, 'h': h, 'w': w, 'C': c1.shape[1], 'F': W.shape[0]}
            row['fused_corr_ms'] = timed(lambda: F.relu_(vcn.corr_proj(c1, c2, up, W, sc, sh, md, mdv)), a.reps)
            row['fused_reg_ms'] = timed(lambda: vcn.flow_reg(cost, up, md, mdv), a.reps)
            row['fused_corr_peak_mib'] = peak(lambda: F.relu_(vcn.corr_proj(c1, c2, up, W, sc, sh, md, mdv)), base)
            row['fused_reg_peak_mib'] = peak(lambda: vcn.flow_reg(cost, up, md, mdv), base)
            if not a.skip_reference:
                row['ref_corr_ms'] = timed(lambda: F.relu_(R.corr_proj_reference_shaped(c1, c2, up, W, sc, sh, md, mdv)), a.reps)
                row['ref_reg_ms'] = timed(lambda: R.flow_reg_reference_shaped(cost, up, md, mdv), a.reps)
                row['ref_corr_peak_mib'] = peak(lambda: F.relu_(R.corr_proj_reference_shaped(c1, c2, up, W, sc, sh, md, mdv)),
                                                base)
                row['ref_reg_peak_mib'] = peak(lambda: R.flow_reg_reference_shaped(cost, up, md, mdv), base)
                rf = R.corr_proj_reference_shaped(c1, c2, up, W, sc, sh, md, mdv)
                row['corr_max_rel_diff'] = float((vcn.corr_proj(c1, c2, up, W, sc, sh, md, mdv) - rf).abs().max() /
                                                 rf.abs().max())
                del rf
            rows.append(row)
            print(json.dumps(row), flush=True)
        rec['levels'] = rows
    print(json.dumps({k: v for k, v in rec.items() if k != 'levels'}), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
