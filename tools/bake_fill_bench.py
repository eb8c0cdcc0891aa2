#!/usr/bin/env python3
"""What does completing an atlas cost?  (lasr_amd/nnutils/bake.py, csrc/bake_fill.hip; DESIGN.md 4.11, "Fill")

    python tools/bake_fill_bench.py [--nu 11] [--res 8] [--iters 20] [--json out.json]

The geodesic sphere of frequency --nu (11: mesh M2, 1212 vertices / 2420 faces) with --res x --res texels per face and the half
x < 0 unseen: one lasr_bake_mirror launch over the listed texels and one lasr_bake_blend iteration, warm-up excluded, each as the
median over --iters launches between two device events (as tools/maskprop_bench.py).  A cold path: no test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import _lib, synth   # noqa: E402
from lasr_amd.nnutils import bake   # noqa: E402


def timed(fn, iters):
    """Median / min / max milliseconds of fn over iters calls, each between two device events."""
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--nu', type=int, default=11)
    ap.add_argument('--res', type=int, default=8)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('bake_fill_bench.py: no HIP device: times are measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    v, f = synth.geodesic_sphere(args.nu)
    rest, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev).int()
    V, F, R = rest.shape[0], faces.shape[0], args.res
    g = torch.Generator(device='cpu').manual_seed(0)
    tex = torch.rand(F, R * R, 3, generator=g).to(dev)
    weight = (rest[faces.long()].mean(1)[:, :1] >= 0).float().expand(F, R * R).contiguous()     # the faces of the half x < 0 unseen
    texels = torch.nonzero(weight.reshape(-1) == 0).reshape(-1).int()
    M = int(texels.shape[0])
    out, src, d2 = tex.clone(), torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, device=dev)
    max_d2 = (0.05 * float((rest.max(0).values - rest.min(0).values).norm())) ** 2
    mirror = lambda: _lib.call('lasr_bake_mirror', rest, faces, texels, tex, weight, out, src, d2, V, F, R, M, 0, max_d2)   # noqa: E731
    nbr = bake.face_neighbours(faces, V)
    fixed = (weight > 0).to(torch.uint8)
    dst = torch.empty_like(tex)
    blend = lambda: _lib.call('lasr_bake_blend', tex, dst, fixed, nbr, F, R)   # noqa: E731
    for fn in (mirror, blend):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {'device': torch.cuda.get_device_name(0), 'V': V, 'F': F, 'R': R, 'listed': M, 'filled': int((src >= 0).sum()),
           'pairs': M * F, 'iters': args.iters, 'mirror': timed(mirror, args.iters), 'blend_one_iteration': timed(blend, args.iters)}
    res['mirror_gpairs_per_s'] = M * F / (res['mirror']['median_ms'] * 1e-3) / 1e9
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
