#!/usr/bin/env python3
"""Optical flow and frame selection for a video (reference: preprocess/auto_gen.py), on the VCN of lasr_amd/ext_nnutils/vcn.py.

    python preprocess/auto_gen.py --datapath database/DAVIS/JPEGImages/Full-Resolution/camel/ --loadmodel vcn_rob.pth

For consecutive frames (i, j) of --datapath with silhouettes under the matching Annotations folder, the forward flow i -> j is
computed; when the median of its norm inside the mask of i, each axis normalised by half the mask's extent, exceeds
--flow_threshold, the backward flow j -> i is computed too and the pair is written under --outdir (default ./<seqname>):
  FlowFW/flo-%05d.pfm, FlowFW/occ-%05d.pfm, FlowBW/flo-%05d.pfm, FlowBW/occ-%05d.pfm  (flow in pixels + a ones channel, rows
  flipped before write_pfm as the reference does), JPEGImages/%05d.jpg (quality 95), Annotations/%05d.png (0 / 1)
and i moves to j; j always moves on.  Without --loadmodel the model keeps its (seeded) random weights: the reference's dry run.
--flow_method variational replaces the network by the classical variational flow of lasr_amd/nnutils/varflow.py (DESIGN.md section
4.16), which needs no checkpoint: no model is built, --loadmodel is refused, and occ-*.pfm holds its forward-backward consistency map.
With it, --vf_gamma 5 adds the gradient-constancy term of preprocess/robust_flow.py for footage whose lighting changes (default 0:
brightness constancy alone, as before; the value is derived on relit fixtures, not on footage), and --vf_match 24 adds the
large-displacement matching stage of preprocess/flow_match.py for small parts that move further than their own size (default 0: off,
as before; the radius is in pixels of the pyramid level --vf_match_level, its tuning is derived on fixtures, not on footage).
Images are read and written with PIL and resized with bilinear interpolation on pixel centres (cv2.INTER_LINEAR's convention;
uint8 images are rounded back to uint8 as cv2 does).
"""
import argparse
import glob
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lasr_amd.ext_utils.util_flow import write_pfm   # noqa: E402


class EmptyMask(ValueError):
    pass


# the tuning parameters of --flow_method variational (lasr_amd/nnutils/varflow.py: DEFAULTS), one flag each
FLOW_TUNING = (('alpha', float, 0.03, 'weight of the smoothness term'),
               ('eps', float, 1e-3, 'regulariser of the two robust penalties sqrt(s^2 + eps^2)'),
               ('omega', float, 1.8, 'SOR relaxation factor, inside (0, 2)'),
               ('NW', int, 5, 'warps per pyramid level'),
               ('NO', int, 3, 'weight updates (lagged diffusivity) per warp'),
               ('NI', int, 10, 'SOR iterations per weight update'))
# the two data terms of --flow_method variational: with --vf_gamma > 0 the flow is preprocess/robust_flow.py's, for footage whose
# lighting changes (5 is the value derived on relit closed-form fixtures, not on footage)
FLOW_ROBUST = (('gamma', float, 0., 'weight of the gradient-constancy term; 0: brightness constancy alone, 5: the derived value'),
               ('beta', float, 1., 'weight of the brightness-constancy term once --vf_gamma > 0'))
# the large-displacement matching stage of --flow_method variational: with --vf_match R > 0 the flow is preprocess/flow_match.py's,
# for small parts that move further than their own size (the tuning is derived on closed-form fixtures, not on footage); the keyword
# of flow_match.make_flow_fn, the flag's suffix, type, default, (lowest, highest) and help
FLOW_MATCH = (('match', '', int, 0, (0, 32), 'search radius R of the block-matching stage in pixels of its level; 0: off, 24: the fixtures\' value'),
              ('patch', '_patch', int, 2, (1, 3), 'patch radius r of the matching cost: (2r+1)^2 pixels'),
              ('level', '_level', int, -1, (-1, 32), 'pyramid level of the stage; -1: the finest whose longer side is <= 512'),
              ('kappa', '_kappa', float, 0.9, (0., 1.), 'a match replaces the flow where its cost is below kappa times the flow\'s, inside (0, 1]'),
              ('prop', '_prop', int, 16, (0, 64), 'iterations that spread accepted matches to their neighbours'))


def add_flow_arguments(p):
    """--flow_method and the vf_* tuning flags, shared with preprocess/propagate_mask.py and preprocess/auto_mask.py."""
    p.add_argument('--flow_method', choices=('vcn', 'variational'), default='vcn',
                   help='vcn: the network (needs --loadmodel to be more than a dry run); variational: the classical flow, no checkpoint')
    for name, kind, default, text in FLOW_TUNING + FLOW_ROBUST:
        p.add_argument('--vf_' + name, type=kind, default=default, help='variational: %s (default %s)' % (text, default))
    for _, suffix, kind, default, _, text in FLOW_MATCH:
        p.add_argument('--vf_match' + suffix, type=kind, default=default, help='variational: %s (default %s)' % (text, default))


def check_flow_arguments(p, args):
    if args.flow_method == 'variational' and args.loadmodel is not None:
        p.error('--flow_method variational uses no network: --loadmodel %s would be ignored, drop it' % args.loadmodel)
    for name, _, _, _ in FLOW_ROBUST:
        v = getattr(args, 'vf_' + name)
        if not (math.isfinite(v) and v >= 0):
            p.error('--vf_%s must be finite and not negative, got %s' % (name, v))
    if args.vf_gamma == 0 and args.vf_beta == 0:
        p.error('--vf_gamma and --vf_beta are both 0: the flow would have no data term')
    for _, suffix, _, _, (lo, hi), _ in FLOW_MATCH:
        v = getattr(args, 'vf_match' + suffix)
        if not (math.isfinite(v) and lo <= v <= hi) or (suffix == '_kappa' and v == 0):
            p.error('--vf_match%s must be %s%s..%s, got %s' % (suffix, 'above ' if suffix == '_kappa' else '', lo, hi, v))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='VCN optical flow and frame selection')
    p.add_argument('--datapath', default='/ssd/kitti_scene/training/', help='folder of the frames (.../JPEGImages/.../<seq>/)')
    p.add_argument('--loadmodel', default=None, help='VCN checkpoint (vcn_rob.pth); none: dry run with random weights')
    p.add_argument('--testres', type=float, default=1, help='resolution')
    p.add_argument('--maxdisp', type=int, default=256, help='maximum disparity; only the coarsest search radius depends on it')
    p.add_argument('--fac', type=float, default=1, help='squeezes the coarsest search window along y')
    p.add_argument('--flow_threshold', type=float, default=0.05, help='median normalised flow below which a frame is skipped')
    p.add_argument('--outdir', default=None, help='output folder (default ./<seqname>)')
    add_flow_arguments(p)
    args = p.parse_args(argv)
    check_flow_arguments(p, args)
    return args


def seqname_of(datapath):
    return os.path.basename(os.path.normpath(datapath.strip()))


def resize(arr, w, h):
    """cv2.resize(arr, (w, h)) with INTER_LINEAR: [H,W] or [H,W,C]; uint8 in, uint8 out (rounded), else float32."""
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    x = t[None, None] if t.dim() == 2 else t.permute(2, 0, 1)[None]
    y = F.interpolate(x, size=(h, w), mode='bilinear', align_corners=False)[0]
    y = y[0] if t.dim() == 2 else y.permute(1, 2, 0)
    y = y.numpy()
    if arr.dtype == np.uint8:
        return np.clip(np.rint(y), 0, 255).astype(np.uint8)
    return y


def read_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def read_mask(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('L')) > 0


def build_model(args, device='cuda'):
    """VCN with md = [int(4 * maxdisp / 256), 4, 4, 4, 4] and fac (auto_gen.py:60), weights from --loadmodel if given."""
    from lasr_amd.ext_nnutils import vcn
    torch.manual_seed(0)
    model = vcn.VCN(md=[int(4 * (args.maxdisp / 256)), 4, 4, 4, 4], fac=args.fac)
    if args.loadmodel is not None:
        vcn.load_checkpoint(model, args.loadmodel)
    else:
        print('dry run')
    print('Number of model parameters: {}'.format(sum(p.numel() for p in model.parameters())))
    return model.to(device).eval()


def flow_inference(model, imgL_o, imgR_o, testres=1., device='cuda'):
    """auto_gen.py:84-148: uint8 RGB [H,W,3] (or [H,W]) pair -> (flow [H,W,3] float32 in pixels with a ones channel,
    occ [H,W] float32)."""
    if imgL_o.ndim == 2:
        imgL_o = np.tile(imgL_o[:, :, None], (1, 1, 3))
        imgR_o = np.tile(imgR_o[:, :, None], (1, 1, 3))
    maxh, maxw = imgL_o.shape[0] * testres, imgL_o.shape[1] * testres
    max_h, max_w = int(maxh // 64 * 64), int(maxw // 64 * 64)
    if max_h < maxh:
        max_h += 64
    if max_w < maxw:
        max_w += 64
    H, W = imgL_o.shape[:2]
    ims = []
    for im, mean in ((imgL_o, model.mean_L), (imgR_o, model.mean_R)):
        x = resize(im, max_w, max_h)[:, :, ::-1] / 255. - mean.detach().cpu().numpy().astype(np.float64).reshape(1, 1, 3)
        ims.append(np.transpose(x, (2, 0, 1)))
    im = torch.from_numpy(np.stack(ims).astype(np.float32)).to(device)
    with torch.no_grad():
        if device != 'cpu':
            torch.cuda.synchronize()
        t0 = time.time()
        flow, occ = model(im)
        if device != 'cpu':
            torch.cuda.synchronize()
        print('time = %.2f' % ((time.time() - t0) * 1000))
    occ = resize(occ.float().cpu().numpy(), W, H)
    flow = flow[0].float().cpu().numpy()
    flow = np.stack([resize(flow[0], W, H), resize(flow[1], W, H)], -1)
    flow[:, :, 0] *= W / max_w
    flow[:, :, 1] *= H / max_h
    return np.concatenate((flow, np.ones(flow.shape[:2] + (1,), flow.dtype)), -1), occ


def variational_flow_fn(args, make=None):
    """flow_fn(imgL, imgR) of --flow_method variational: lasr_amd.nnutils.varflow.make_flow_fn with the vf_* flags.  --testres
    scales the frames before the flow, as it does for the network (without the padding to multiples of 64, which only the network
    needs); flow and occ come back at the frames' size, the flow in their pixels.  With --vf_gamma > 0 the flow is
    preprocess/robust_flow.py's (brightness and gradient constancy), built with gamma= and beta= beside the same flags.  With
    --vf_match > 0 it is preprocess/flow_match.py's, built with match=, patch=, level=, kappa=, prop=, gamma= and beta= beside them."""
    tuning = {name: getattr(args, 'vf_' + name) for name, _, _, _ in FLOW_TUNING}
    if getattr(args, 'vf_match', 0) > 0:
        if make is None:
            here = os.path.dirname(os.path.abspath(__file__))
            if here not in sys.path:
                sys.path.insert(0, here)
            import flow_match                                                      # (beside this file)
            make = flow_match.make_flow_fn
        stage = {key: getattr(args, 'vf_match' + suffix) for key, suffix, _, _, _, _ in FLOW_MATCH}
        inner = make(gamma=args.vf_gamma, beta=args.vf_beta, **stage, **tuning)
    elif getattr(args, 'vf_gamma', 0.) > 0:
        if make is None:
            here = os.path.dirname(os.path.abspath(__file__))
            if here not in sys.path:
                sys.path.insert(0, here)
            import robust_flow                                                     # (beside this file)
            make = robust_flow.make_flow_fn
        inner = make(gamma=args.vf_gamma, beta=args.vf_beta, **tuning)
    else:
        if make is None:
            from lasr_amd.nnutils import varflow
            make = varflow.make_flow_fn
        inner = make(**tuning)
    testres = float(args.testres)
    if testres == 1:
        return inner

    def flow_fn(imgL_o, imgR_o):
        H, W = imgL_o.shape[:2]
        h, w = max(2, int(round(H * testres))), max(2, int(round(W * testres)))
        flow, occ = inner(resize(imgL_o, w, h), resize(imgR_o, w, h))
        flow = np.stack([resize(flow[:, :, 0], W, H) * (W / w), resize(flow[:, :, 1], W, H) * (H / h)], -1).astype(np.float32)
        return np.concatenate((flow, np.ones(flow.shape[:2] + (1,), flow.dtype)), -1), resize(occ, W, H)
    return flow_fn


def median_flow(flow, mask, path=''):
    """auto_gen.py:161-166: the median over the mask of |flow| with x / y divided by half the mask's width / height."""
    ys, xs = np.where(mask)
    if xs.size == 0:
        raise EmptyMask('%s: the mask is empty' % path)
    length = [(xs.max() - xs.min()) // 2, (ys.max() - ys.min()) // 2]
    normed = np.concatenate([flow[:, :, :1] / length[0], flow[:, :, 1:2] / length[1]], -1)
    return float(np.median(np.linalg.norm(normed[mask], 2, -1)))


def run(args, flow_fn):
    """The frame loop of auto_gen.py:150-183 with flow_fn(imgL, imgR) -> (flow [H,W,3], occ [H,W]).  -> list of the (i, j)
    frame-index pairs written, in order."""
    from PIL import Image
    seq = seqname_of(args.datapath)
    out = args.outdir or os.path.join('.', seq)
    for sub in ('JPEGImages', 'FlowFW', 'FlowBW', 'Annotations'):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    frames = sorted(glob.glob('%s/*' % args.datapath))
    masks = sorted(glob.glob('%s/*' % os.path.normpath(args.datapath).replace('JPEGImages', 'Annotations')))
    if len(masks) < len(frames):
        raise FileNotFoundError('%d frames but %d silhouettes for %s' % (len(frames), len(masks), args.datapath))
    kept = []
    inx, jnx, ix = 0, 1, 0
    while jnx < len(frames):
        print('%s/%s' % (frames[inx], frames[jnx]))
        imgL_o, imgR_o = read_rgb(frames[inx]), read_rgb(frames[jnx])
        mask, maskR = read_mask(masks[inx]), read_mask(masks[jnx])
        flowfw, occfw = flow_fn(imgL_o, imgR_o)
        medflow = median_flow(flowfw, mask, masks[inx])
        print('%.3f, %.2f' % (medflow, float(np.median(occfw[mask]))))
        if medflow > args.flow_threshold:
            if not maskR.any():
                raise EmptyMask('%s: the mask is empty' % masks[jnx])
            flowbw, occbw = flow_fn(imgR_o, imgL_o)
            write_pfm('%s/FlowFW/flo-%05d.pfm' % (out, ix), np.ascontiguousarray(flowfw[::-1]).astype(np.float32))
            write_pfm('%s/FlowFW/occ-%05d.pfm' % (out, ix), np.ascontiguousarray(occfw[::-1]).astype(np.float32))
            write_pfm('%s/FlowBW/flo-%05d.pfm' % (out, ix + 1), np.ascontiguousarray(flowbw[::-1]).astype(np.float32))
            write_pfm('%s/FlowBW/occ-%05d.pfm' % (out, ix + 1), np.ascontiguousarray(occbw[::-1]).astype(np.float32))
            Image.fromarray(imgL_o).save('%s/JPEGImages/%05d.jpg' % (out, ix), quality=95)
            Image.fromarray(imgR_o).save('%s/JPEGImages/%05d.jpg' % (out, ix + 1), quality=95)
            Image.fromarray(mask.astype(np.uint8)).save('%s/Annotations/%05d.png' % (out, ix))
            Image.fromarray(maskR.astype(np.uint8)).save('%s/Annotations/%05d.png' % (out, ix + 1))
            kept.append((inx, jnx))
            inx = jnx
            ix += 1
        jnx += 1
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    return kept


def main(argv=None):
    args = parse_args(argv)
    if args.flow_method == 'variational':
        flow_fn = variational_flow_fn(args)
    else:
        model = build_model(args)
        flow_fn = lambda a, b: flow_inference(model, a, b, args.testres)   # noqa: E731
    try:
        run(args, flow_fn)
    except EmptyMask as e:
        sys.exit('auto_gen.py: %s' % e)


if __name__ == '__main__':
    main()
