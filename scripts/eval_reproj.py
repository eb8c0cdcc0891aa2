#!/usr/bin/env python3
"""Score a reconstruction by reprojection, without ground-truth geometry (this project's own addition; the reference has no
counterpart -- DESIGN.md section 4.15).

    python scripts/eval_reproj.py --testdir log/camel-5/ --seqname camel \\
        [--bound_th 0.008] [--outpath reproj.json] [--vis DIR] [--worst 5]

Reads what export_tracks.py reads: the frames of configs/<seqname>.config and, per frame id i, <testdir>/pred<i>.ply (or .obj) in
camera space and the intrinsics row of cam<i>.txt; and what the loader was trained on: the annotation of every frame
(JPEGImages -> Annotations, .jpg -> .png) and, when present, the forward flow and occlusion maps FlowFW/.../flo-*.pfm, occ-*.pfm
(the sub-folder <seq>_%02d for dframe > 1, as lasr_amd/dataloader/vid.py).  Per frame the mesh is rasterised with its camera and
compared (lasr_amd/nnutils/reproj.py, csrc/reproj.hip): the silhouette by the DAVIS measures J (region similarity) and F (boundary
measure, tolerance --bound_th: a share of the image diagonal, or pixels when 1 or more), the rendered flow to the next frame by
its end-point error on the pixels the loader counts as valid, the vertex colours of a .ply by their PSNR against the frame.
Writes a JSON (default <testdir>/reproj.json) with the parameters, the frame ids, the per-frame metrics and their means over the
frames (frames without a value left out and counted), prints one summary line and the --worst frames by (J+F)/2; --vis writes per
frame reproj-%05d.png, the frame with the boundary of the prediction in red, of the annotation in green, yellow where they meet.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import recon_io                                    # noqa: E402
from lasr_amd.recon_io import annotation_path, check_topology    # noqa: E402,F401  (imported from here too)

PER_FRAME = ('J', 'F', 'precision', 'recall', 'epe', 'pck1', 'pck3', 'psnr')
COUNTS = ('inter', 'union', 'n_pred', 'n_gt', 'n_pb', 'n_gb', 'pm', 'gm', 'n_flow', 'n_le1', 'n_le3', 'n_rgb')
MEANS = ('J', 'F', 'JF', 'epe', 'psnr')
RED, GREEN, YELLOW = (255, 0, 0), (0, 255, 0), (255, 255, 0)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Silhouette J & F, flow end-point error and colour PSNR of the reconstructed meshes.')
    p.add_argument('--testdir', default='', help='directory holding pred<i>.ply / .obj and cam<i>.txt')
    p.add_argument('--seqname', default='camel', help='sequence name: its frames are listed by configs/<seqname>.config')
    p.add_argument('--bound_th', default=0.008, type=float,
                   help='boundary tolerance of F: below 1 a share of the image diagonal, from 1 a whole number of pixels, 0 exact')
    p.add_argument('--outpath', default='', help='output .json (default: <testdir>/reproj.json)')
    p.add_argument('--vis', default='', help='directory for reproj-%%05d.png: both boundaries drawn over each frame')
    p.add_argument('--worst', default=5, type=int, help='how many of the worst frames by (J+F)/2 to print')
    return p.parse_args(argv)


def flow_paths(name, dframe):
    """(flo, occ) of the forward flow that starts at frame `name`, as the loader names them."""
    seqname = name.split('/')[-2]
    sub = '%s/flo-' % seqname if dframe == 1 else '%s_%02d/flo-' % (seqname, dframe)
    flo = name.replace('JPEGImages', 'FlowFW').replace('.jpg', '.pfm').replace('.png', '.pfm').replace('%s/' % seqname, sub)
    return flo, flo.replace('flo-', 'occ-')


def check_size(what, shape, H, W):
    if tuple(shape[:2]) != (H, W):
        raise ValueError('%s is %d x %d, the frames are %d x %d' % (what, shape[1], shape[0], W, H))


def load_flows(names, dframe, H, W):
    """-> (flows [T-1,H,W,3] float32, occs [T-1,H,W] float32, found): a pair without flo-*.pfm keeps an all-invalid row; None, None,
    0 when no pair has one."""
    from lasr_amd.ext_utils.util_flow import readPFM
    T = len(names)
    flows, occs, found = np.zeros((max(T - 1, 0), H, W, 3), np.float32), np.zeros((max(T - 1, 0), H, W), np.float32), 0
    for i, name in enumerate(names[:-1]):
        flo, occ = flow_paths(name, dframe)
        if not os.path.exists(flo):
            continue
        f = readPFM(flo)[0]
        check_size(flo, f.shape, H, W)
        flows[i] = f
        if os.path.exists(occ):
            o = readPFM(occ)[0]
            check_size(occ, o.shape, H, W)
            occs[i] = o
        found += 1
    return (flows, occs, found) if found else (None, None, 0)


def summarise(res, frame_ids, params):
    """evaluate()'s per-frame arrays -> the JSON document: params, frame_ids, per_frame (lists), means and nan_frames."""
    per = {k: [None if np.isnan(x) else float(x) for x in np.asarray(res[k], np.float64)] for k in PER_FRAME}
    per.update({k: [int(x) for x in res[k]] for k in COUNTS})
    jf = (np.asarray(res['J'], np.float64) + np.asarray(res['F'], np.float64)) / 2
    per['JF'] = [None if np.isnan(x) else float(x) for x in jf]
    means, nans = {}, {}
    for k in MEANS:
        x = jf if k == 'JF' else np.asarray(res[k], np.float64)
        good = np.isfinite(x)
        means[k] = float(x[good].mean()) if good.any() else None
        nans[k] = int((~good).sum())
    return dict(params=params, frame_ids=[int(i) for i in frame_ids], radius=int(np.asarray(res['radius']).reshape(-1)[0]) if len(frame_ids) else 0,
                per_frame=per, means=means, nan_frames=nans)


def _fmt(x, spec='%.4f'):
    return 'n/a' if x is None else spec % x


def summary_line(doc):
    m = doc['means']
    return 'reproj: %d frames, J %s, F %s, (J+F)/2 %s, epe %s px, psnr %s dB' % (
        len(doc['frame_ids']), _fmt(m['J']), _fmt(m['F']), _fmt(m['JF']), _fmt(m['epe'], '%.3f'), _fmt(m['psnr'], '%.2f'))


def worst_lines(doc, count):
    """The `count` frames with the lowest (J+F)/2, lowest first (ties: the earlier frame)."""
    jf = doc['per_frame']['JF']
    order = sorted(range(len(jf)), key=lambda i: (jf[i], i))[:max(count, 0)]
    return ['worst: frame %d (position %d) J %.4f F %.4f (J+F)/2 %.4f' % (doc['frame_ids'][i], i, doc['per_frame']['J'][i],
                                                                           doc['per_frame']['F'][i], jf[i]) for i in order]


def overlay(frame, b_pred, b_gt):
    """uint8 [H,W,3] with the boundary of the prediction in red, of the annotation in green, yellow where they coincide."""
    out = np.array(frame, np.uint8, copy=True)
    out[b_pred & ~b_gt] = RED
    out[b_gt & ~b_pred] = GREEN
    out[b_pred & b_gt] = YELLOW
    return out


def write_vis(directory, imgs, boundary, frame_ids):
    """boundary bool [T,2,H,W] (pred, gt) -> reproj-%05d.png per frame id; returns the paths."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    paths = []
    for img, b, fr in zip(imgs, boundary, frame_ids):
        paths.append(os.path.join(directory, 'reproj-%05d.png' % fr))
        Image.fromarray(overlay(img, b[0], b[1])).save(paths[-1])
    return paths


def main(argv=None, evaluate=None):
    """evaluate: a stand-in for lasr_amd.nnutils.reproj.evaluate taking and returning numpy arrays (the tests without a device
    inject the float64 restatement); by default the tensors go to the GPU."""
    args = parse_args(argv)
    from lasr_amd.dataloader.vid import read_config
    try:
        names = recon_io.frame_list(args.seqname)
        dframe = read_config(args.seqname)['dframe']
    except FileNotFoundError as e:
        raise SystemExit('eval_reproj.py: no config for sequence %s (%s)' % (args.seqname, e))
    if not names:
        raise SystemExit('eval_reproj.py: no frames for sequence %s' % args.seqname)
    try:
        rec = recon_io.read(args.testdir, names, annotations=True)
    except recon_io.ReadError as e:
        raise SystemExit('eval_reproj.py: %s' % e)
    imgs, masks, ids, has_colours = rec.imgs, rec.masks, rec.ids, rec.has_colours      # the .obj fallback's grey is not scored
    H, W = imgs[0].shape[:2]
    try:
        for name, img, m in zip(names, imgs, masks):
            check_size(name, img.shape, H, W)
            check_size(annotation_path(name), m.shape, H, W)
        flows, occs, found = load_flows(names, dframe, H, W)
    except ValueError as e:
        raise SystemExit('eval_reproj.py: %s' % e)
    masks = np.stack([(m.reshape(H, W, -1) != 0).any(-1) for m in masks]).astype(np.uint8)
    if not found:
        print('no FlowFW maps for %s: scored on silhouettes%s alone' % (args.seqname, ' and colours' if has_colours else ''))
    data = dict(verts=np.stack(rec.verts), faces=rec.face, K=rec.K, masks=masks, flows=flows, occs=occs,
                frames=np.stack(imgs) if has_colours else None, colors=np.stack(rec.colors) if has_colours else None)
    try:
        if evaluate is None:
            res, boundary = _evaluate_on_device(data, args.bound_th, bool(args.vis))
        else:
            res = evaluate(bound_th=args.bound_th, **data)
            boundary = res.get('boundary')
    except ValueError as e:
        raise SystemExit('eval_reproj.py: %s' % e)
    doc = summarise(res, ids, dict(testdir=args.testdir, seqname=args.seqname, bound_th=args.bound_th, dframe=dframe, size=[H, W],
                                   flow_pairs=found, colours=bool(has_colours)))
    out = args.outpath or os.path.join(args.testdir, 'reproj.json')
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    print(summary_line(doc))
    for line in worst_lines(doc, args.worst):
        print(line)
    if args.vis:
        paths = write_vis(args.vis, imgs, boundary, ids)
        print('wrote %d overlays to %s' % (len(paths), args.vis))
    return doc


def _evaluate_on_device(data, bound_th, want_boundary):
    import torch
    from lasr_amd.nnutils import reproj
    dev = torch.device('cuda', 0)
    t = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if v is not None else None) for k, v in data.items()}
    with torch.no_grad():
        res = reproj.evaluate(bound_th=bound_th, **t)
    W = data['masks'].shape[2]
    return res, (reproj.unpack_bits(res['boundary_bits'].cpu().numpy(), W) if want_boundary else None)


if __name__ == '__main__':
    main()
