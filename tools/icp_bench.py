#!/usr/bin/env python3
"""Nearest-neighbour search and ICP at evaluation size.

    python tools/icp_bench.py [--points 10000] [--iters 64] [--reps 20] [--json out.json]

Two 10 000-point samples of an ellipsoid, one turned and shifted.  Records, from HIP events, the median ms of one
fused_ops.nearest_point call and of one chamfer3D.nn_tiled call at every split count of --splits, and the ms per iteration of
iterative_closest_point (thr = -1: --iters iterations, one chunk) against eval_mesh.py's icp() loop.  Run it under
rocprofv3 --kernel-trace --stats for the per-kernel times."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from lasr_amd.chamfer3D import dist_chamfer_3D as dc          # noqa: E402
from lasr_amd.nnutils import fused_ops                        # noqa: E402
from lasr_amd.nnutils.icp import iterative_closest_point      # noqa: E402


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


def clouds(n, dev):
    rng = np.random.default_rng(0)

    def sample():
        u = rng.standard_normal((n, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True) * [5., 3., 2.]
    c, s = np.cos(0.1), np.sin(0.1)
    x = sample() @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.]]) + [0.1, -0.05, 0.08]
    return torch.from_numpy(x.astype(np.float32)).to(dev)[None], torch.from_numpy(sample().astype(np.float32)).to(dev)[None]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=10000)
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--splits', default='0,1,5,10,20')
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    import eval_mesh
    dev = torch.device('cuda', 0)
    x, y = clouds(args.points, dev)
    out = {'points': args.points, 'nearest_point_ms': timed(lambda: fused_ops.nearest_point(x, y), args.reps), 'nn_tiled_ms': {}}
    for s in [int(v) for v in args.splits.split(',')]:
        out['nn_tiled_ms'][str(s)] = timed(lambda: dc.nn_tiled(x, y, splits=s), args.reps)
    d0, i0 = fused_ops.nearest_point(x, y)
    d1, i1 = dc.nn_tiled(x, y)
    out['bit_identical'] = bool(torch.equal(d0, d1) and torch.equal(i0, i1.long()))
    run = lambda: iterative_closest_point(x, y, max_iterations=args.iters, relative_rmse_thr=-1., chunk=args.iters)   # noqa: E731
    out['icp_device_ms_per_iteration'] = timed(run, 5) / args.iters
    out['icp_host_loop_ms_per_iteration'] = timed(lambda: eval_mesh.icp(x[0], y[0], iters=args.iters, tol=-1.), 3) / args.iters
    sol = iterative_closest_point(x, y, max_iterations=10000)
    out['icp_to_convergence'] = {'iterations': sol.iterations, 'converged': sol.converged, 'rmse': float(sol.rmse[0])}
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == '__main__':
    main()
