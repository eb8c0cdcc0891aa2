#!/usr/bin/env python3
"""Time the reprojection scores on one chunk of 1080p frames against a torch composition of the same silhouette metric
(lasr_amd/nnutils/reproj.py, csrc/reproj.hip).

    python tools/reproj_bench.py [--frames 8] [--size 1080x1920] [--nu 11] [--bound_th 0.008] [--out reproj_bench.json]

The scene is the one of tools/tracks_bench.py (a seeded blob in front of a 1080p camera); the annotation is the raster of the same
mesh grown by 3 %.  Three things are timed with device events, in windows of at least --window seconds that alternate, seven
windows each: lasr_reproj_pixels on silhouettes alone and with the flow and colour groups, lasr_reproj_boundary, and
torch_silhouette below (boolean shifts and XORs for the boundary map, a conv2d with the disk for the dilation, sums for the
counts).  The rasters are made once, outside the windows.  The eight silhouette counts of the two must be equal, or the script
fails.  It prints, and with --out writes, one JSON line; no test asserts a time.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from lasr_amd import _lib                       # noqa: E402
from lasr_amd.nnutils import bake, reproj      # noqa: E402


def torch_silhouette(pred, gt, rho):
    """pred, gt bool [n,H,W] -> int64 [n,8]: inter, union, n_pred, n_gt, n_pb, n_gb, pm, gm as include/lasr_ops.h defines them."""
    def boundary(seg):
        e, s, se = torch.zeros_like(seg), torch.zeros_like(seg), torch.zeros_like(seg)
        e[:, :, :-1] = seg[:, :, 1:]
        s[:, :-1] = seg[:, 1:]
        se[:, :-1, :-1] = seg[:, 1:, 1:]
        b = (seg ^ e) | (seg ^ s) | (seg ^ se)
        b[:, -1] = seg[:, -1] ^ e[:, -1]
        b[:, :, -1] = seg[:, :, -1] ^ s[:, :, -1]
        b[:, -1, -1] = False
        return b

    y, x = torch.meshgrid(torch.arange(-rho, rho + 1, device=pred.device), torch.arange(-rho, rho + 1, device=pred.device), indexing='ij')
    disk = (x * x + y * y <= rho * rho).float()[None, None]

    def dilate(b):
        return torch.nn.functional.conv2d(b.float()[:, None], disk, padding=rho)[:, 0] > 0.5

    bp, bg = boundary(pred), boundary(gt)
    cols = [pred & gt, pred | gt, pred, gt, bp, bg, bp & dilate(bg), bg & dilate(bp)]
    return torch.stack([c.sum((1, 2)) for c in cols], 1)


def timed(fn, seconds, windows=1):
    """Median, min and max over `windows` windows of the time of one call of fn in microseconds (device events; every window
    repeats fn for at least `seconds`)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(5):
        fn()
    end.record()
    torch.cuda.synchronize()
    reps = max(5, int(seconds * 1e3 / max(start.elapsed_time(end) / 5, 1e-3)))
    out = []
    for _ in range(windows):
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end) * 1e3 / reps)
    return out, reps


def main(argv=None):
    import tracks_bench
    p = argparse.ArgumentParser()
    p.add_argument('--frames', default=8, type=int)
    p.add_argument('--size', default='1080x1920')
    p.add_argument('--nu', default=11, type=int, help='mesh frequency: 20 nu^2 faces')
    p.add_argument('--bound_th', default=0.008, type=float)
    p.add_argument('--window', default=0.3, type=float, help='seconds of work per timed window')
    p.add_argument('--out', default='')
    args = p.parse_args(argv)
    H, W = (int(x) for x in args.size.split('x'))
    n, IS, WW = args.frames, max(H, W), (W + 63) // 64
    dev = torch.device('cuda', 0)
    verts, faces, K = tracks_bench.scene(n + 1, H, W, args.nu)
    V, F = verts.shape[1], faces.shape[0]
    rho = reproj.radius_of(args.bound_th, H, W)
    rng = np.random.default_rng(0)
    tv, tf, tK = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).int().to(dev), torch.from_numpy(K).to(dev)
    with torch.no_grad():
        raster = bake.face_index_raster(tv[:n], tf, tK[:n], IS)
        centre = tv[:n].mean(1, keepdim=True)
        gt = (bake.face_index_raster((tv[:n] - centre) * 1.03 + centre, tf, tK[:n], IS)[:, 1, :H, :W] >= 0).to(torch.uint8).contiguous()
    flow = torch.from_numpy(rng.normal(0, 2, (n, H, W, 3)).astype(np.float32)).to(dev)
    flow[..., 2] = 1.
    occ = torch.zeros(n, H, W, device=dev)
    frames = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(dev)
    colors = torch.from_numpy(rng.integers(0, 256, (n, V, 3), dtype=np.uint8)).to(dev)
    bits = torch.zeros(n, 2, H, WW, dtype=torch.int64, device=dev)
    bbits = torch.zeros_like(bits)
    counts = torch.zeros(n, 12, dtype=torch.int64, device=dev)
    sums = torch.zeros(n, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(int(_lib.lib().lasr_reproj_workspace_bytes(n, H, W)) // 8, dtype=torch.float64, device=dev)
    v0, v1, k0, k1 = tv[:n].contiguous(), tv[1:n + 1].contiguous(), tK[:n].contiguous(), tK[1:n + 1].contiguous()

    def pixels_sil():
        _lib.call('lasr_reproj_pixels', v0, None, tf, k0, None, raster, gt, None, None, None, None, bits, counts, sums, ws, n, V, F, IS, H, W)

    def pixels_all():
        _lib.call('lasr_reproj_pixels', v0, v1, tf, k0, k1, raster, gt, flow, occ, frames, colors, bits, counts, sums, ws, n, V, F, IS, H, W)

    def boundary():
        _lib.call('lasr_reproj_boundary', bits, bbits, counts, n, H, W, rho)

    pred_b, gt_b = raster[:, 1, :H, :W] >= 0, gt != 0

    def composition():
        return torch_silhouette(pred_b, gt_b, rho)

    with torch.no_grad():
        counts.zero_()
        pixels_all()
        boundary()
        want = composition()
        torch.cuda.synchronize()
        if not torch.equal(counts[:, :8], want):
            raise SystemExit('reproj_bench.py: the native counts %s differ from the torch composition %s' % (counts[:, :8].tolist(), want.tolist()))
        first = counts.cpu().numpy().copy()
        times = {k: [] for k in ('pixels_silhouette', 'pixels_all', 'boundary', 'torch_silhouette')}
        reps = {}
        for _ in range(7):                                                    # alternate, so that the host's other load hits all alike
            for name, fn in (('pixels_silhouette', pixels_sil), ('pixels_all', pixels_all), ('boundary', boundary),
                             ('torch_silhouette', composition)):
                t, reps[name] = timed(fn, args.window)
                times[name] += t
    px = n * H * W
    stat = {k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), calls_per_window=reps[k])
            for k, v in times.items()}
    # raster plane 1 and the annotation of every pixel, flow + occlusion + frame (19 bytes) of the anchored ones, the two maps written
    anchored = int(first[:, 11].sum())
    floor = dict(pixels_silhouette=px * 5 + 2 * n * H * WW * 8, pixels_all=px * 5 + anchored * 19 + 2 * n * H * WW * 8,
                 boundary=3 * 2 * n * H * WW * 8)
    for k, b in floor.items():
        stat[k].update(floor_bytes=int(b), gb_per_s_on_floor_bytes=b / stat[k]['median_us'] * 1e-3)
    native = stat['pixels_silhouette']['median_us'] + stat['boundary']['median_us']
    doc = dict(frames=n, size=[H, W], faces=int(F), radius=rho, windows=7, window_seconds=args.window,
               counts_frame0=dict(zip(reproj.COUNTS, (int(x) for x in first[0]))), times=stat,
               native_silhouette_us=native, torch_over_native=stat['torch_silhouette']['median_us'] / native)
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
