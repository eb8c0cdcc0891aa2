#!/usr/bin/env python3
"""What does the large-displacement matching stage of the variational flow cost?  (preprocess/flow_match.py, csrc/flowmatch.hip;
DESIGN.md 4.16)

    python tools/flowmatch_bench.py [--sizes 480x854,1080x1920] [--match 24] [--patch 2] [--prop 16] [--iters 20] [--runs 3] [--json out.json]

On a seeded synthetic pair (the band-limited texture of tools/varflow_bench.py translated by (0.011 W, 0.004 H), with a block of
0.05 W x 0.05 H pasted over it that moves by (0.04 W, -0.03 H): a part that moves further than its own size) these are timed, warm-up
excluded, each as the median over --iters calls between device events, and the whole measurement --runs times, the variants
alternating inside a run:
  search        one lasr_flowmatch_search on the stage's level (-1: the finest with a longer side <= 512), A -> B
  select_prop   lasr_flowmatch_select and --prop lasr_flowmatch_propagate launches on the flow the plain estimate hands to that
                level, and the apply (fuse)
  pair_plain    varflow.flow_pair: both directions and their consistency maps, as the parent commit computes them
  pair_match    flow_match.flow_pair with --match: the same, plus two quantisations, two searches and a fuse per direction
Before anything is timed two searches are compared bit for bit, and the share of the block's pixels whose flow is within 1 px of
the block's motion is printed for both pairs.  The search's work is h w (2R+1)^2 (2r+1)^2 sums of absolute differences of one pixel
pair (one v_sad_u8 each); its rate is set against the vector unit's issue rate, 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12
lane-instructions per second (the FP32 vector peak of 157.3 TFLOPS counts two per fused multiply-add).  No test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from lasr_amd.nnutils import varflow   # noqa: E402
import flow_match                      # noqa: E402
from varflow_bench import make_pair, timed   # noqa: E402

VALU_LANE_RATE = 256 * 4 * 32 * 2.4e9


def make_dart_pair(H, W, dev):
    """make_pair's two frames with a block pasted into both: at (0.3 W, 0.5 H) in A, moved by (0.04 W, -0.03 H) in B.
    -> (A, B, the block's (x0, y0, w, h) in A, its motion (dx, dy))."""
    A, B, _ = make_pair(H, W, dev)
    g = torch.Generator(device='cpu').manual_seed(1)
    bw, bh = max(int(0.05 * W), 4), max(int(0.05 * H), 4)
    block = torch.randint(0, 256, (bh // 4 + 1, bw // 4 + 1, 3), generator=g, dtype=torch.uint8)
    block = block.repeat_interleave(4, 0).repeat_interleave(4, 1)[:bh, :bw].to(dev)
    x0, y0, dx, dy = int(0.3 * W), int(0.5 * H), int(round(0.04 * W)), -int(round(0.03 * H))
    A, B = A.clone(), B.clone()
    A[y0:y0 + bh, x0:x0 + bw] = block
    B[y0 + dy:y0 + dy + bh, x0 + dx:x0 + dx + bw] = block
    return A, B, (x0, y0, bw, bh), (dx, dy)


def block_hit(f, box, motion):
    """Share of the block's pixels whose flow [H,W,2] is within 1 px of its motion."""
    x0, y0, bw, bh = box
    part = f[y0:y0 + bh, x0:x0 + bw]
    want = torch.tensor([float(motion[0]), float(motion[1])], device=f.device)
    return float(((part - want).norm(dim=-1) <= 1).float().mean())


def bench_size(H, W, args, dev):
    R, r, N = args.match, args.patch, args.prop
    A, B, box, motion = make_dart_pair(H, W, dev)
    L, qA, qB, (d_ab, c_ab), (d_ba, c_ba) = flow_match.matches(A, B, R, r)
    h, w = int(qA.shape[0]), int(qA.shape[1])
    again = flow_match.search(qA, qB, R, r)
    assert torch.equal(again[0], d_ab) and torch.equal(again[1], c_ab), 'two searches differ'
    seen = []
    varflow.flow(A, B, init=lambda lev, uv: (seen.append(uv.clone()) if lev == L else None) or uv)
    uv_in = seen[0]                                                        # what the plain estimate hands to the stage's level
    plain, matched = varflow.flow_pair(A, B)[0], flow_match.flow_pair(A, B, R, patch=r, prop=N)[0]
    variants = {'search': lambda: flow_match.search(qA, qB, R, r),
                'select_prop': lambda: flow_match.fuse(qA, qB, d_ab, c_ab, d_ba, uv_in, R, r, 0.9, N),
                'pair_plain': lambda: varflow.flow_pair(A, B),
                'pair_match': lambda: flow_match.flow_pair(A, B, R, patch=r, prop=N)}
    torch.cuda.synchronize()
    sads = h * w * (2 * R + 1) ** 2 * (2 * r + 1) ** 2
    res = {'H': H, 'W': W, 'level': L, 'h': h, 'w': w, 'R': R, 'r': r, 'N': N, 'block': box, 'motion': motion,
           'motion_at_level': [m / 2 ** L for m in motion], 'block_hit_plain': block_hit(plain, box, motion),
           'block_hit_match': block_hit(matched, box, motion), 'search_sads': sads, 'runs': []}
    for fn in variants.values():                                           # warm-up: every shape of the timed window
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.runs):
        run = {name: timed(fn, args.iters) for name, fn in variants.items()}
        res['runs'].append(run)
        print(json.dumps(dict(run, H=H, W=W)), flush=True)
    for name in variants:
        med = [run[name]['median_ms'] for run in res['runs']]
        res[name] = {'median_ms': statistics.median(med), 'min_of_medians_ms': min(med), 'max_of_medians_ms': max(med)}
    res['search_sad_per_s'] = sads / (res['search']['median_ms'] * 1e-3)
    res['search_share_of_valu_issue'] = res['search_sad_per_s'] / VALU_LANE_RATE
    res['stage_adds_ms'] = res['pair_match']['median_ms'] - res['pair_plain']['median_ms']
    res['pair_match_over_plain'] = res['pair_match']['median_ms'] / res['pair_plain']['median_ms']
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='480x854,1080x1920')
    ap.add_argument('--match', type=int, default=24)
    ap.add_argument('--patch', type=int, default=2)
    ap.add_argument('--prop', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('flowmatch_bench.py: no HIP device: times are measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'sizes': []}
    for s in args.sizes.split(','):
        H, W = (int(v) for v in s.split('x'))
        out['sizes'].append(bench_size(H, W, args, dev))
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
