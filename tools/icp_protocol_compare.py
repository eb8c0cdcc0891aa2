#!/usr/bin/env python3
"""Chamfer distance of scripts/reconstruct_demo.py's meshes under eval_mesh.py --icp fast and --icp reference.

    python tools/icp_protocol_compare.py [--json out.json] [reconstruct_demo.py arguments, e.g. --nframes 8 --deterministic]

Runs the demo unchanged and scores every pair it scores a second time with icp='reference' (same seed, so the same samples), and
records both distances with the iteration count the reference protocol reached."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default='')
    args, rest = ap.parse_known_args(argv)
    demo = _load('reconstruct_demo')
    rows = []
    load = demo._load

    def load_wrapped(name):
        mod = load(name)
        if name == 'eval_mesh':
            fast = mod.evaluate_pair

            def both(pred, gt, **kw):
                cd = fast(pred, gt, **kw)
                info = {}
                rows.append({'fast': cd, 'reference': fast(pred, gt, icp='reference', aligned=info, **kw),
                             'iterations': info['icp_iterations'], 'converged': info['icp_converged']})
                return cd
            mod.evaluate_pair = both
        return mod
    demo._load = load_wrapped
    out = demo.main(rest)
    n = len(rows) // 3                                              # the demo scores the template, stage 0 and stage 1, n frames each
    rec = {'demo': {k: out[k] for k in ('sequence', 'chamfer_unit_sphere_template')}, 'arguments': rest}
    for k, name in enumerate(('unit_sphere_template', 'stage0', 'stage1')):
        part = rows[k * n:(k + 1) * n]
        rec[name] = {'chamfer_fast': float(np.mean([r['fast'] for r in part])), 'chamfer_reference': float(np.mean([r['reference'] for r in part])),
                     'per_frame': part}
    print(json.dumps(rec))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(rec, fh, indent=1)
    return rec


if __name__ == '__main__':
    main()
