#!/usr/bin/env python3
"""What does the shape score cost?  (lasr_amd/nnutils/meshcheck.py, csrc/meshcheck.hip)

    python tools/meshcheck_bench.py [--iters 20] [--repeats 3] [--json out.json]

Two cases: `lasr`, the geodesic sphere of frequency 11 (mesh M2, 2420 faces) in 64 seeded, jittered frames, and `large`, the
sphere of frequency 64 (81 920 faces) in one frame.  Per case the per-face pass (lasr_meshcheck_faces: records, volume, area; two
launches) and the pair pass (lasr_meshcheck_pairs: three memsets and the tiled pair kernel), warm-up excluded, each as the median
over --iters calls between two device events, repeated --repeats times (the medians' minimum and maximum are reported, as
tools/varflow_bench.py does); the share of the face pairs that are candidates, that is reach the exact test, counted with torch;
and, from those counts and not from counters, in how many 64-lane batches the kernel tests them and what share of the batches'
lanes is live.  As context at 2420 faces, a broad phase composed from torch: the box overlap over all pairs of faces of every frame.
No test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import _lib, synth   # noqa: E402
from lasr_amd.nnutils import meshcheck   # noqa: E402


def timed(fn, iters, repeats):
    """fn timed between two device events: the median of iters calls, `repeats` times -> median of medians, their min and max (ms)."""
    meds = []
    for _ in range(repeats):
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        meds.append(statistics.median(ms))
    return {'median_ms': statistics.median(meds), 'min_ms': min(meds), 'max_ms': max(meds)}


def frames_of(nu, T, seed, dev):
    """T jittered frames of the geodesic sphere of frequency nu: 3 % of the radius and 2 % per coordinate, seeded."""
    v, f = synth.geodesic_sphere(nu)
    rng = np.random.default_rng(seed)
    scale = 0.03 if nu <= 16 else 0.03 * 16 / nu                                 # keep the jitter below the edge length
    verts = np.stack([v * (1 + scale * rng.uniform(-1, 1, (len(v), 1))) + scale * 2 / 3 * rng.uniform(-1, 1, v.shape) for _ in range(T)])
    return torch.from_numpy(verts.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev).int()


def box_overlap(verts, faces):
    """The torch broad phase of one frame: bool [F,F], closed box overlap of every pair of faces."""
    tri = verts[faces.long()]
    lo, hi = tri.amin(1), tri.amax(1)
    return ((lo[:, None] <= hi[None]) & (lo[None] <= hi[:, None])).all(-1)


def candidate_count(verts, faces, rows=256):
    """The candidate pairs of one frame (boxes overlap, no shared vertex, i < j), in chunks of `rows` faces, and the number of
    64-lane batches the pair kernel tests them in: a wave (64 faces of tile I) empties its queue whenever 64 candidates wait and
    once more at the end of its tile J, so c candidates of a (wave, tile J) take ceil(c / 64) batches."""
    tri = verts[faces.long()]
    lo, hi = tri.amin(1), tri.amax(1)
    F, total = faces.shape[0], 0
    NT = (F + 255) // 256
    per_queue = torch.zeros(((F + 63) // 64) * NT, dtype=torch.int64, device=verts.device)
    j = torch.arange(F, device=verts.device)
    for r in range(0, F, rows):
        s = slice(r, min(r + rows, F))
        over = ((lo[s, None] <= hi[None]) & (lo[None] <= hi[s, None])).all(-1)
        share = (faces[s, None, :, None] == faces[None, :, None, :]).flatten(2).any(-1)
        ci, cj = torch.nonzero(over & ~share & (j[None] > j[s, None]), as_tuple=True)
        total += int(ci.numel())
        per_queue += torch.bincount(((ci + r) // 64) * NT + cj // 256, minlength=per_queue.numel())
    return total, int(((per_queue + 63) // 64).sum())


def run_case(name, nu, T, args, dev):
    verts, faces = frames_of(nu, T, 7, dev)
    V, F = verts.shape[1], faces.shape[0]
    nbytes = _lib.lib().lasr_meshcheck_workspace_bytes(T, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    vol, area = torch.zeros(T, dtype=torch.float64, device=dev), torch.zeros(T, dtype=torch.float64, device=dev)
    n_pairs, count = torch.zeros(T, dtype=torch.int64, device=dev), torch.zeros(T, F, dtype=torch.int32, device=dev)
    cursor, pairs = torch.zeros(T, dtype=torch.int32, device=dev), torch.zeros(T, args.max_pairs, 2, dtype=torch.int32, device=dev)
    face_pass = lambda: _lib.call('lasr_meshcheck_faces', verts, faces, ws, nbytes, vol, area, T, V, F)   # noqa: E731
    pair_pass = lambda: _lib.call('lasr_meshcheck_pairs', ws, nbytes, count, n_pairs, cursor, pairs, T, F, args.max_pairs, on=dev)   # noqa: E731
    for fn in (face_pass, pair_pass):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    all_pairs = T * F * (F - 1) // 2
    counted = [candidate_count(verts[t], faces) for t in range(T)]
    cand, batches = sum(c for c, _ in counted), sum(b for _, b in counted)
    res = {'case': name, 'T': T, 'V': V, 'F': F, 'face_pairs': all_pairs, 'candidates': cand, 'candidate_share': cand / all_pairs,
           'exact_test_batches': batches, 'exact_test_live_lane_share_from_counts': cand / (64. * batches) if batches else None,
           'intersecting_pairs': int(n_pairs.sum()), 'workspace_bytes': nbytes,
           'face_pass': timed(face_pass, args.iters, args.repeats), 'pair_pass': timed(pair_pass, args.iters, args.repeats)}
    res['gpairs_per_s'] = all_pairs / (res['pair_pass']['median_ms'] * 1e-3) / 1e9
    if name == 'lasr':
        def torch_broad():
            for t in range(T):
                box_overlap(verts[t], faces)
        for _ in range(2):
            torch_broad()
        torch.cuda.synchronize()
        res['torch_box_overlap'] = timed(torch_broad, max(args.iters // 4, 3), args.repeats)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--max_pairs', type=int, default=meshcheck.DEFAULT_MAX_PAIRS)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('meshcheck_bench.py: no HIP device: times are measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'repeats': args.repeats,
           'cases': [run_case('lasr', 11, 64, args, dev), run_case('large', 64, 1, args, dev)]}
    print(json.dumps(res))
    if args.json:
        if os.path.dirname(args.json):
            os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
