#!/usr/bin/env python3
"""What does the fold penalty of the optimiser cost per step?  (scripts/fold_penalty.py, csrc/foldpen.hip)

    python tools/foldpen_bench.py [--iters 20] [--repeats 3] [--json out.json]

N = 16 and 64 posed meshes on the geodesic sphere of frequency 8 (1280 faces, the stage-0 mesh) and of frequency 11 (2420 faces, the
M2 mesh), the seeded, jittered frames of tools/meshcheck_bench.py with the vertex of largest x of every frame pushed across its ring
as tests/meshnbr_restated.py's crease does, so that some entries are charged.  Per case the forward with rows (two launches:
entries, fold), the forward without rows (no gradient wanted) and the backward (one launch: the gather per vertex), each as the
median over --iters calls between two device events, repeated --repeats times (the medians' minimum and maximum are reported), the
three alternating repeat by repeat.  Nothing here is a gate, and no test asserts a time.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import fold_penalty as fp   # noqa: E402
from meshcheck_bench import frames_of   # noqa: E402
from meshnbr_bench import alternating   # noqa: E402


def folded(verts, faces):
    """Every frame with its vertex of largest x moved 1.5 ring radii towards its first ring neighbour and 5 % below the surface."""
    v, f = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy()
    for x in v:
        k = int(np.argmax(x[:, 0]))
        ring = np.array(sorted(set(f[(f == k).any(1)].reshape(-1).tolist()) - {k}))
        c = x[ring].mean(0)
        x[k] = c + 1.5 * (x[ring[0]] - c) - 0.05 * c
    return torch.from_numpy(v.astype(np.float32)).to(verts.device)


def run_case(nu, N, args, dev):
    verts, faces = frames_of(nu, N, 7, dev)
    verts = folded(verts, faces)
    pen = fp.FoldPenalty(faces, args.fold_deg, n_verts=verts.shape[1])
    up = torch.ones(N, 2, device=dev)
    loss, values, rows = pen.launch_forward(verts, True)
    fns = {
        'forward': lambda: pen.launch_forward(verts, True),
        'forward_no_rows': lambda: pen.launch_forward(verts, False),
        'backward': lambda: pen.launch_backward(rows, up, tuple(verts.shape)),
    }
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    vstart, inc = pen.index(verts.shape[1])
    res = {'nu': nu, 'N': N, 'V': verts.shape[1], 'F': faces.shape[0], 'list_entries': pen.keys.numel(), 'incidences': inc.numel(),
           'incidences_per_vertex': inc.numel() / verts.shape[1], 'entries_charged': int((values != 0).sum()),
           'rows_bytes': rows.numel() * 4, 'loss_mean': loss.mean(0).tolist()}
    res.update(alternating(fns, args.iters, args.repeats))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--fold_deg', type=float, default=fp.DEFAULT_FOLD_DEG)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('foldpen_bench.py: no HIP device: times are measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'repeats': args.repeats,
           'cases': [run_case(nu, N, args, dev) for nu in (8, 11) for N in (16, 64)]}
    print(json.dumps(res))
    if args.json:
        if os.path.dirname(args.json):
            os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
