#!/usr/bin/env python3
"""A camel-sized run of the dense point tracks for a kernel trace (lasr_amd/nnutils/tracks.py, csrc/tracks.hip).

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o tracks -- python tools/tracks_bench.py [--frames 90] [--size 1080x1920] [--nu 11]

(OUT/tracks_kernel_trace.csv then lists every launch of track_project_kernel with its start and end.)

A seeded blob (synth.blobby_mesh, 20 nu^2 faces) turns once over --frames frames in front of a 1080p camera and fills about a
sixth of the frame; every covered pixel of frame 0 is a query.  track_points runs twice (the first run loads the code objects);
the script prints the problem's size and the byte floor of one lasr_track_project launch: the anchor records read once per frame
window, tracks and state written once.  The launch times come from the trace, not from this script; no test asserts a time.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import synth                   # noqa: E402
from lasr_amd.nnutils import tracks as tk    # noqa: E402


def scene(T, H, W, nu):
    v, f, _ = synth.blobby_mesh(nu)
    verts = []
    for t in range(T):
        w = v.astype(np.float64) * (1. + 0.05 * np.sin(4. * v[:, 1:2] + 2. * math.pi * t / T))
        verts.append(w @ synth.yaw_matrix(2. * math.pi * t / T).astype(np.float64).T + np.array([0., 0., 1.6]))
    focal = 0.9 * H
    K = np.tile(np.array([[focal, focal, W / 2. + 0.3, H / 2. - 0.2]], np.float32), (T, 1))
    return np.stack(verts).astype(np.float32), f, K


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--frames', default=90, type=int)
    p.add_argument('--size', default='1080x1920')
    p.add_argument('--nu', default=11, type=int, help='mesh frequency: 20 nu^2 faces')
    p.add_argument('--window', default=1, type=int)
    args = p.parse_args(argv)
    H, W = (int(x) for x in args.size.split('x'))
    dev = torch.device('cuda', 0)
    verts, faces, K = scene(args.frames, H, W, args.nu)
    tv, tf, tK = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(K).to(dev)
    with torch.no_grad():
        queries = tk.covered_queries(tk.frame_raster(tv, tf, tK, 0, H, W), 0, 1, H, W)
        for _ in range(2):
            tracks, state, anchors = tk.track_points(tv, tf, tK, queries, H, W, window=args.window)
            torch.cuda.synchronize()
    Q, T = state.shape
    n = min(tk.CHUNK_FRAMES, T)
    st = state.cpu().numpy()
    print(json.dumps({'frames': T, 'size': [H, W], 'faces': int(faces.shape[0]), 'queries': Q, 'frames_per_window': n,
                      'floor_bytes_per_full_window': Q * 16 + n * Q * (8 + 1),
                      'anchored': float((st != 0).any(1).mean()), 'visible': float((st == 1).mean()),
                      'hidden': float((st == 2).mean())}))


if __name__ == '__main__':
    main()
