#!/usr/bin/env python3
"""Export dense long-range point tracks of the meshes extract.py wrote (this project's own addition; the reference has no
counterpart -- DESIGN.md section 4.14).

    python scripts/export_tracks.py --testdir log/camel-5/ --seqname camel \\
        [--query_frame 0] [--stride 4] [--queries q.npy] [--snap_radius 0] \\
        [--window 1] [--outpath DIR/tracks.npz] [--preview out.gif] [--radius 2]

Reads what bake_texture.py reads: the frames of configs/<seqname>.config and, per frame id i, <testdir>/pred<i>.ply (or .obj) in
camera space and the intrinsics row of cam<i>.txt.  The queries are the centres of every --stride-th covered pixel (rows and
columns) of the frame at position --query_frame, or the rows (t, y, x) of --queries, t a position in the frame list.  Every query
is anchored on the surface of its frame and followed through all frames (lasr_amd/nnutils/tracks.py, csrc/tracks.hip).  Writes an
.npz with tracks [Q,T,2] float32 (x, y), visible [Q,T] bool, state [Q,T] uint8 (1 visible, 2 hidden, 3 outside the frame, 4 behind
the camera, 0 no anchor), queries [Q,3] (t, y, x), frame_ids [T] and size (H, W), and with --preview a GIF of the frames with the
visible points drawn, coloured by where they sit in their query frame.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import recon_io                   # noqa: E402
from lasr_amd.recon_io import check_topology    # noqa: E402,F401  (imported from here too)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Export dense point tracks and their visibility from the reconstructed meshes.')
    p.add_argument('--testdir', default='', help='directory holding pred<i>.ply / .obj and cam<i>.txt')
    p.add_argument('--seqname', default='camel', help='sequence name: its frames are listed by configs/<seqname>.config')
    p.add_argument('--query_frame', default=0, type=int, help='position in the frame list of the frame the default queries cover')
    p.add_argument('--stride', default=4, type=int, help='default queries: covered pixels on every stride-th row and column')
    p.add_argument('--queries', default='', help='.npy of [Q,3] rows (t, y, x) to track instead of the default queries')
    p.add_argument('--snap_radius', default=0, type=int, help='move a query on an empty pixel to the nearest covered one within this many pixels')
    p.add_argument('--window', default=1, type=int, help='half-width in pixels of the visibility window (0, 1 or 2)')
    p.add_argument('--outpath', default='', help='output .npz (default: <testdir>/tracks.npz)')
    p.add_argument('--preview', default='', help='GIF to write: the frames with the visible points drawn')
    p.add_argument('--radius', default=2, type=int, help='radius in pixels of the points of the preview')
    return p.parse_args(argv)


def check_queries(q, T):
    """[Q,3] rows (t, y, x) with t a whole frame position in 0 .. T-1 -> float32."""
    q = np.asarray(q)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError('queries must be [Q, 3] rows (t, y, x), got %s' % (q.shape,))
    q = q.astype(np.float32)
    if len(q) and not ((q[:, 0] == np.round(q[:, 0])) & (q[:, 0] >= 0) & (q[:, 0] < T)).all():
        raise ValueError('the frame position of every query must be a whole number in 0..%d' % (T - 1))
    return q


def summary_line(state):
    """state [Q,T] -> the line the script prints; the visible share is the mean over the anchored queries."""
    state = np.asarray(state)
    anchored = (state != 0).any(1) if state.size else np.zeros(len(state), bool)
    vis = float((state[anchored] == 1).mean()) if anchored.any() else 0.
    return 'tracked %d queries, anchored %.1f %%, visible in %.1f %% of the frames on average' % (
        len(state), 100. * float(anchored.mean()) if len(state) else 0., 100. * vis)


def query_colours(queries, H, W):
    """uint8 [Q,3] on the device: the flow colour (lasr_amd/ext_utils/flowlib.py) of each query's offset from the frame centre."""
    from lasr_amd.ext_utils import flowlib
    off = torch.stack([queries[:, 2] - W / 2., queries[:, 1] - H / 2.], 1)
    return flowlib.flow_to_image(off[None, None].contiguous())[0, 0]


def main(argv=None):
    args = parse_args(argv)
    from PIL import Image
    from lasr_amd.nnutils import tracks as tk
    dev = torch.device('cuda', 0)
    names = recon_io.frame_list(args.seqname)
    if not names:
        raise SystemExit('export_tracks.py: no frames for sequence %s' % args.seqname)
    T = len(names)
    if not 0 <= args.query_frame < T:
        raise SystemExit('export_tracks.py: --query_frame %d is outside the %d frames' % (args.query_frame, T))
    try:
        rec = recon_io.read(args.testdir, names)
    except recon_io.ReadError as e:
        raise SystemExit('export_tracks.py: %s' % e)
    imgs, ids = rec.imgs, rec.ids
    H, W = imgs[0].shape[:2]
    tv = torch.from_numpy(np.stack(rec.verts)).to(dev)
    tf = torch.from_numpy(rec.face).to(dev)
    tK = torch.from_numpy(rec.K).to(dev)
    with torch.no_grad():
        if args.queries:
            try:
                queries = torch.from_numpy(check_queries(np.load(args.queries), T)).to(dev)
            except (OSError, ValueError) as e:
                raise SystemExit('export_tracks.py: --queries %s: %s' % (args.queries, e))
        else:
            raster = tk.frame_raster(tv, tf, tK, args.query_frame, H, W)
            queries = tk.covered_queries(raster, args.query_frame, args.stride, H, W)
        try:
            tracks, state, anchors = tk.track_points(tv, tf, tK, queries, H, W, snap_radius=args.snap_radius, window=args.window)
        except ValueError as e:
            raise SystemExit('export_tracks.py: %s' % e)
    out = args.outpath or os.path.join(args.testdir, 'tracks.npz')
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    st = state.cpu().numpy()
    np.savez(out, tracks=tracks.cpu().numpy(), visible=st == 1, state=st, queries=queries.cpu().numpy(),
             frame_ids=np.asarray(ids, np.int64), size=np.asarray([H, W], np.int64))
    print(summary_line(st))

    if args.preview:
        frames = torch.from_numpy(np.stack(imgs)).to(dev)
        # colour by the position the anchor was computed at, so a snapped query takes the colour of where it landed
        pos = torch.cat([queries[:, :1], anchors['snapped']], 1)
        with torch.no_grad():
            drawn = tk.splat(frames, tracks, state, query_colours(pos, H, W), args.radius)
        pil = [Image.fromarray(p) for p in drawn.cpu().numpy()]
        pil[0].save(args.preview, save_all=True, append_images=pil[1:], duration=5000. / len(pil), loop=0)
        print('wrote %d frames to %s' % (len(pil), args.preview))
    return tracks, state


if __name__ == '__main__':
    main()
