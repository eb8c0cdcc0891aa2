#!/usr/bin/env python3
"""Keypoint-transfer PCK on BADJA (reference: scripts/eval_badja.py).

    python scripts/eval_badja.py --testdir log/camel-5/ --seqname camel [--type mesh|zero] [--badja_root ./database] [--json out.json]

For every ordered pair (i, j), i != j, of annotated frames, frame i's keypoints move with the flow from frame i's reconstruction
(pred<fr>.ply, cam<fr>.txt as extract.py writes them) to frame j's, taken at the nearest pixel with a valid flow; a keypoint
counts as correct when it lands within 0.2 sqrt(silhouette area of frame i) of frame j's annotation, and only where both frames
mark it visible.  The script prints PCK over all pairs.  --type zero scores the zero flow (every prediction stays put).

Per reference frame i one hard-mode raster launch covers all its targets j (frame i's geometry repeated, each target's projected
vertices as vertex colours), at most CHUNK_PIXELS raster pixels per launch: about 24 bytes each (colour planes and the
rasteriser's depth / face planes), 1.6 GB, 18 pairs at 1920 x 1920.  One lasr_kp_transfer launch follows each raster launch and
the results come to the host once per frame i.  --dense instead renders each pair on its own and searches with the reference's
dense [J, H*W] tensor and torch's argmin (for checking and timing; the same numbers).

Kept from the reference: rows of the prediction are scaled by H / 2 and columns by W / 2 although the flow is in units of the
S x S render, S = max(H, W) (eval_badja.py:239-242); PCK of non-square frames carries it.  Departures: frames whose crop is not
contiguous (portrait, H > W) work here, where the reference's .view(-1, 3) fails; every pred<fr>.ply must share one topology
(checked, the reference renders frame i's faces with frame j's vertices without looking); --type flow (VCN and its weights) and
--vis (cv2 drawings) are not shipped and refused.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lasr_amd.ext_utils.badja_data import BADJAData, frame_number      # noqa: E402

CHUNK_PIXELS = 1 << 26


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='BADJA')
    ap.add_argument('--testdir', default='', help='path to test dir')
    ap.add_argument('--seqname', default='camel', help='sequence to test')
    ap.add_argument('--type', default='mesh', help='load mesh data or flow or zero')
    ap.add_argument('--cam_type', default='perspective', help='camera model, orthographic or perspective (ignored, as in the reference)')
    ap.add_argument('--vis', dest='vis', action='store_true', help='whether to draw visualization (not supported)')
    ap.add_argument('--badja_root', default='./database', help='directory holding joint_annotations/ and the DAVIS images')
    ap.add_argument('--json', default='', help='write per-pair idx, pred, correct and the PCK to this file')
    ap.add_argument('--dense', action='store_true', help='one render per pair and the dense torch argmin, as the reference computes')
    return ap.parse_args(argv)


def make_renderer():
    from lasr_amd import soft_renderer as sr
    return sr.SoftRenderer(image_size=256, dist_func='hard', aggr_func_alpha='hard', camera_mode='look_at', perspective=False,
                           aggr_func_rgb='hard', light_mode='vertex', light_intensity_ambient=1., light_intensity_directionals=0.)


def load_meshes(testdir, frames):
    from lasr_amd.ext_utils.ply import read_ply
    verts, cams, faces = [], [], None
    for fr in frames:
        for name in ('pred%d.ply' % fr, 'cam%d.txt' % fr):
            if not os.path.exists(os.path.join(testdir, name)):
                raise FileNotFoundError('%s is missing from --testdir %s' % (name, testdir))
        m = read_ply(os.path.join(testdir, 'pred%d.ply' % fr))
        if faces is None:
            faces = m['faces']
        elif m['faces'].shape != faces.shape or (m['faces'] != faces).any():
            raise ValueError('pred%d.ply does not share the topology of pred%d.ply' % (fr, frames[0]))
        verts.append(np.asarray(m['verts'], np.float64))
        cams.append(np.loadtxt(os.path.join(testdir, 'cam%d.txt' % fr)))
    return np.stack(verts), np.stack(cams), faces


def project(verts, cams, img_size, dev):
    """obj_to_cam + pinhole_cam with cam<fr>.txt in pixels mapped to the NDC of an img_size square (eval_badja.py:209-223),
    every frame at once -> [N,V,4] (NDC x, y, depth, 1)."""
    from lasr_amd.nnutils.geom_utils import obj_to_cam, pinhole_cam
    v = torch.tensor(verts, dtype=torch.float32).to(dev)
    Rmat = torch.tensor(cams[:, :3, :3], dtype=torch.float32).to(dev)
    Tmat = torch.tensor(cams[:, :3, 3], dtype=torch.float32).to(dev)
    ppoint = torch.tensor(cams[:, 3, 2:], dtype=torch.float32).to(dev)
    scale = torch.tensor(cams[:, 3, :1], dtype=torch.float32).to(dev)
    scale = scale / img_size * 2
    ppoint = ppoint / img_size * 2 - 1
    vf = obj_to_cam(v, Rmat, Tmat[:, None], nmesh=1, n_hypo=1, skin=None)
    vf = torch.cat([vf, torch.ones_like(vf[:, :, 0:1])], dim=-1)
    return pinhole_cam(vf, ppoint, scale)


def transfer_mesh(renderer, vproj, faces, i, js, kp, H, W, S):
    """Frame i against frames js: chunked raster launches, one kp_transfer each -> (idx [len(js),J], pred [len(js),J,2]) on the host."""
    from lasr_amd.nnutils.geom_utils import render_flow_colors
    from lasr_amd.nnutils.keypoints import kp_transfer
    renderer.rasterizer.image_size = S
    chunk = max(1, CHUNK_PIXELS // (S * S))
    kpt = torch.tensor(kp, dtype=torch.float32, device=vproj.device)
    idx, pred = [], []
    with torch.no_grad():
        for a in range(0, len(js), chunk):
            jj = torch.tensor(js[a:a + chunk], device=vproj.device)
            B = len(jj)
            colors = render_flow_colors(renderer, vproj[i:i + 1].expand(B, -1, -1), vproj[jj], faces.expand(B, -1, -1))
            ix, pr = kp_transfer(colors, kpt, H, W)
            idx.append(ix)
            pred.append(pr)
            del colors
    return torch.cat(idx).cpu().numpy(), torch.cat(pred).cpu().numpy()


def transfer_dense(renderer, vproj, faces, i, j, kp, H, W, S):
    """The reference's computation for one pair (eval_badja.py:225-242): flow from render_flow_soft_3, the dense key tensor and
    torch's argmin."""
    from lasr_amd.nnutils.geom_utils import render_flow_soft_3
    renderer.rasterizer.image_size = S
    dev = vproj.device
    with torch.no_grad():
        flow, bg, _ = render_flow_soft_3(renderer, vproj[i:i + 1], vproj[j:j + 1], faces)
        flow[bg] = 0.
        flow = torch.cat([flow, torch.zeros_like(flow)[:, :, :, :1]], -1)[:, :H, :W].contiguous()
        kpx = torch.tensor(kp, dtype=torch.float32, device=dev)
        x0, y0 = np.meshgrid(range(W), range(H))
        x0 = torch.tensor(x0, dtype=torch.float32, device=dev)
        y0 = torch.tensor(y0, dtype=torch.float32, device=dev)
        idx = ((flow[:, :, :, :2].norm(2, -1) < 1e-6).float().view(1, -1) * 1e6 + torch.pow(kpx[:, 0:1] - y0.view(1, -1), 2)
               + torch.pow(kpx[:, 1:2] - x0.view(1, -1), 2)).argmin(-1)
        samp = flow.view(-1, 3)[idx][:, :2]
        pred = kpx.clone()
        pred[:, 0] = pred[:, 0] + samp[:, 1] * H / 2
        pred[:, 1] = pred[:, 1] + samp[:, 0] * W / 2
    return idx.cpu().numpy(), pred.cpu().numpy()


def score(pred, refsil, tarkp, refvis, tarvis):
    """eval_badja.py:244-248, in float64: -> the correct flags of the joints both frames mark visible."""
    diff = np.linalg.norm(pred - tarkp, 2, -1)
    sqarea = np.sqrt((refsil[:, :, 0] > 0).sum())
    correct = diff < sqarea * 0.2
    return correct[np.logical_and(tarvis, refvis)]


def main(argv=None):
    args = parse_args(argv)
    if args.type == 'flow':
        sys.exit('eval_badja.py: --type flow needs VCN and its weights, which are not shipped; use --type mesh or --type zero')
    if args.type not in ('mesh', 'zero'):
        sys.exit('eval_badja.py: unknown --type %r (mesh or zero)' % args.type)
    if args.vis:
        sys.exit('eval_badja.py: --vis (the cv2 drawings of the reference) is not supported')
    data = BADJAData(args.seqname, root=args.badja_root)
    print(args.testdir)
    annos, frames = [], []
    for anno in data.get_loader():
        annos.append(anno)
        name = anno[4]
        frames.append(frame_number(name))
        print('%s/%d' % (os.path.basename(os.path.dirname(name)), frames[-1]))
    if len(annos) < 2:
        sys.exit('eval_badja.py: %d annotated frames with images found under %s; at least 2 are needed'
                 % (len(annos), args.badja_root))
    if args.type == 'mesh':
        verts, cams, faces_np = load_meshes(args.testdir, frames)
    if not torch.cuda.is_available():
        sys.exit('eval_badja.py needs a HIP device')
    dev = torch.device('cuda', 0)
    renderer = make_renderer()
    if args.type == 'mesh':
        faces = torch.tensor(faces_np, dtype=torch.int32, device=dev)[None]
    n = len(annos)
    pck_all, pairs = [], []
    proj_of = {}
    for i in range(n):
        refimg, refsil, refkp, refvis, refname = annos[i]
        H, W = refimg.shape[:2]
        S = max(refimg.shape)
        js = [j for j in range(n) if j != i]
        if args.type == 'mesh':
            if S not in proj_of:
                proj_of[S] = project(verts, cams, S, dev)
            vproj = proj_of[S]
            if args.dense:
                res = [transfer_dense(renderer, vproj, faces, i, j, refkp, H, W, S) for j in js]
                idx, pred = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
            else:
                idx, pred = transfer_mesh(renderer, vproj, faces, i, js, refkp, H, W, S)
        else:
            from lasr_amd.nnutils.keypoints import kp_transfer
            kpt = torch.tensor(refkp, dtype=torch.float32, device=dev)[None].expand(len(js), -1, -1)
            idx, pred = kp_transfer(None, kpt, H, W)
            idx, pred = idx.cpu().numpy(), pred.cpu().numpy()
        for k, j in enumerate(js):
            tarimg, tarsil, tarkp, tarvis, tarname = annos[j]
            print('%s vs %s' % (refname, tarname))
            correct = score(pred[k], refsil, tarkp, refvis, tarvis)
            pck_all.append(correct)
            pairs.append({'ref': frames[i], 'tar': frames[j], 'idx': [int(v) for v in idx[k]],
                          'pred': [[float(a), float(b)] for a, b in pred[k]], 'correct': [bool(c) for c in correct]})
    pck = 100 * np.concatenate(pck_all).astype(float).mean()
    print('PCK %.02f' % pck)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump({'seqname': args.seqname, 'type': args.type, 'pck': float(pck), 'pairs': pairs}, fh)
    return pck


if __name__ == '__main__':
    main()
