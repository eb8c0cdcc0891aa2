#!/usr/bin/env python3
"""What does the intersection penalty of the optimiser cost per step?  (scripts/isect_penalty.py, csrc/isectpen.hip)

    python tools/isectpen_bench.py [--iters 20] [--repeats 3] [--json out.json]

N = 16 and 64 posed meshes on the geodesic sphere of frequency 8 (1280 faces, the stage-0 mesh) and of frequency 11 (2420 faces, the
M2 mesh), the seeded, jittered frames of tools/meshcheck_bench.py with the topmost vertex of every frame pushed through the opposite
side as tests/meshcheck_restated.py's pinch2 does, so that some pairs are charged.  Per case the penalty with its gradient (three
launches: zero, pairs, finalise), the penalty without (gunit NULL), and the yardstick: lasr_meshcheck_faces + lasr_meshcheck_pairs
on the same input in the same run, the same walk with detection only.  Each is the median over --iters calls between two device
events, repeated --repeats times (the medians' minimum and maximum are reported), the three alternating repeat by repeat.  Nothing
here is a gate, and no test asserts a time.
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
import isect_penalty as ip   # noqa: E402
from lasr_amd.nnutils import meshcheck   # noqa: E402
from meshcheck_bench import frames_of   # noqa: E402
from meshnbr_bench import alternating   # noqa: E402


def pinched(verts):
    """Every frame with its topmost vertex moved to -1.3 times its position: through the opposite side."""
    v = verts.cpu().numpy().astype(np.float64)
    for x in v:
        k = int(np.argmax(x[:, 2]))
        x[k] = -1.3 * x[k] + np.array([0.013, -0.021, 0.])
    return torch.from_numpy(v.astype(np.float32)).to(verts.device)


def run_case(nu, N, args, dev):
    verts, faces = frames_of(nu, N, 7, dev)
    verts = pinched(verts)
    V, F = verts.shape[1], faces.shape[0]
    pen = ip.IsectPenalty(faces, n_verts=V)

    def yardstick():
        ws, nbytes, _, _ = meshcheck._records(verts, faces, N, V, F)
        return meshcheck._pairs(ws, nbytes, N, F, 0, dev)[0]
    fns = {
        'penalty': lambda: pen.launch(verts, True),
        'penalty_no_grad': lambda: pen.launch(verts, False),
        'meshcheck_faces_and_pairs': yardstick,
    }
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    loss, gunit, n_pairs, n_dropped = pen.launch(verts, True)
    same = bool(torch.equal(n_pairs, yardstick()))
    res = {'nu': nu, 'N': N, 'V': V, 'F': F, 'tile_pairs': ((F + 255) // 256) * ((F + 255) // 256 + 1) // 2,
           'n_pairs_mean': float(n_pairs.double().mean()), 'n_pairs_as_meshcheck': same, 'n_dropped': int(n_dropped.sum()),
           'loss_mean': float(loss.mean()), 'scratch_bytes': int(ip._lib.lib().lasr_isectpen_scratch_bytes(N, V))}
    res.update(alternating(fns, args.iters, args.repeats))
    res['ratio'] = res['penalty']['median_ms'] / res['meshcheck_faces_and_pairs']['median_ms']
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('isectpen_bench.py: no HIP device: times are measured on the GPU or not at all')
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
