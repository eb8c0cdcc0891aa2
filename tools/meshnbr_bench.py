#!/usr/bin/env python3
"""What does the neighbour pass of the shape score cost?  (scripts/shape_neighbours.py, csrc/meshnbr.hip)

    python tools/meshnbr_bench.py [--iters 20] [--repeats 3] [--json out.json]

The two cases of tools/meshcheck_bench.py, with its method: `lasr`, the geodesic sphere of frequency 11 (2420 faces) in 64 seeded,
jittered frames, and `large`, the sphere of frequency 64 (81 920 faces) in one frame.  Per case the list pass (lasr_meshnbr_list: a
memset and the tiled kernel over the index triples; once per topology), the test pass (lasr_meshnbr_test: four memsets, the test
kernel over (entries, frames), the decode) and, in the same process and alternating with it repeat by repeat, the pair pass
(lasr_meshcheck_pairs), each as the median over --iters calls between two device events, repeated --repeats times (the medians'
minimum and maximum are reported).  The sort of the list (torch.sort) is timed as a line of its own.  Nothing here is a gate, and
no test asserts a time.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import shape_neighbours as sn   # noqa: E402
from lasr_amd import _lib   # noqa: E402
from meshcheck_bench import frames_of, timed   # noqa: E402


def alternating(fns, iters, repeats):
    """name -> timed(): one repeat of each function in turn, `repeats` times, so that a drift of the clocks hits all alike."""
    per = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            per[name].append(timed(fn, iters, 1)['median_ms'])
    return {name: {'median_ms': sorted(ms)[len(ms) // 2], 'min_ms': min(ms), 'max_ms': max(ms)} for name, ms in per.items()}


def run_case(name, nu, T, args, dev):
    verts, faces = frames_of(nu, T, 7, dev)
    V, F = verts.shape[1], faces.shape[0]
    nbytes = _lib.lib().lasr_meshcheck_workspace_bytes(T, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    vol, area = torch.zeros(T, dtype=torch.float64, device=dev), torch.zeros(T, dtype=torch.float64, device=dev)
    _lib.call('lasr_meshcheck_faces', verts, faces, ws, nbytes, vol, area, T, V, F)
    n_pairs, count = torch.zeros(T, dtype=torch.int64, device=dev), torch.zeros(T, F, dtype=torch.int32, device=dev)
    cursor, pairs = torch.zeros(T, dtype=torch.int32, device=dev), torch.zeros(T, args.max_pairs, 2, dtype=torch.int32, device=dev)
    keys, counts = sn.neighbour_list(faces)
    n = keys.numel()
    capacity = sn.CAPACITY_PER_FACE * F
    raw, counters = torch.empty(capacity, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    totals, nbr = torch.zeros(T, 2, dtype=torch.int64, device=dev), torch.zeros(T, 2, F, dtype=torch.int32, device=dev)
    hits, min_cos = torch.zeros(T, args.max_pairs, 3, dtype=torch.int32, device=dev), torch.zeros(T, device=dev)
    k = sn.fold_k(args.fold_deg)
    fns = {
        'list_pass': lambda: _lib.call('lasr_meshnbr_list', faces, raw, counters, F, capacity, on=dev),
        'list_sort': lambda: torch.sort(raw[:n]),
        'test_pass': lambda: _lib.call('lasr_meshnbr_test', ws, nbytes, keys, n, k, nbr, totals, cursor, hits, min_cos, T, F, args.max_pairs,
                                       on=dev),
        'pair_pass': lambda: _lib.call('lasr_meshcheck_pairs', ws, nbytes, count, n_pairs, cursor, pairs, T, F, args.max_pairs, on=dev),
    }
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {'case': name, 'T': T, 'V': V, 'F': F, 'list_entries': n, 'topology': {c: int(x) for c, x in counts.items()},
           'entries_tested': n * T, 'face_pairs_walked': T * F * (F - 1) // 2, 'n_pierced': int(totals[:, 0].sum()),
           'n_creased': int(totals[:, 1].sum()), 'min_dihedral': float(sn.dihedral(min_cos.min().item())),
           'intersecting_pairs': int(n_pairs.sum())}
    res.update(alternating(fns, args.iters, args.repeats))
    res['test_over_pair'] = res['test_pass']['median_ms'] / res['pair_pass']['median_ms']
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--max_pairs', type=int, default=sn.DEFAULT_MAX_PAIRS)
    ap.add_argument('--fold_deg', type=float, default=sn.DEFAULT_FOLD_DEG)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('meshnbr_bench.py: no HIP device: times are measured on the GPU or not at all')
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
