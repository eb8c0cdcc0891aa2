#!/usr/bin/env python3
"""Chamfer + normal-consistency evaluation of reconstructed meshes against ground truth (reference: /root/reference/scripts/eval_mesh.py).

    python scripts/eval_mesh.py --testdir <dir with pred*.obj> --gtdir <dir with *.obj>

Protocol of the reference (:116-160): both meshes are centred, scaled so that their largest point-to-point distance is
10, 10 000 points are sampled uniformly by area from each, the prediction is aligned to the ground truth with rigid
ICP, and the symmetric Chamfer distance (mean squared nearest-neighbour distance, both directions summed --
pytorch3d.loss.chamfer_distance) of two fresh samples is reported, together with the normal term of the same call
(:165-167, :197-198: `chamfer_distance(X, Y, x_normals=nx, y_normals=ny)` returns as its second value
mean_x(1 - |cos(n_x, n_nn(x))|) + mean_y(1 - |cos(n_y, n_nn(y))|) over the sampled faces' normals; the script prints 1 minus
it as the normal consistency).  pytorch3d / trimesh are not available here: area sampling with face normals, Kabsch ICP,
the Chamfer sum and the normal term are written out; the nearest-neighbour searches run on lasr_nearest_point.
--remesh RESOLUTION > 0 re-meshes every prediction watertight first, as the reference does with the external Manifold binary
for LASR's predictions (:100-105, `manifold in.obj out.obj 10000`): lasr_amd/nnutils/manifold.py:watertight on the GPU.  The
default 0 scores the predictions as they are.
--render also writes the reference's images (:170-200) into --testdir: gt-/pd-/cd-%06d.png, 512 x 512 pytorch3d-style Phong
renders (lasr_amd/phong.py) of the ground truth and the aligned prediction in grey and of the ground truth coloured by its error,
and one GIF of the three side by side (--gif, 5 s in all).  The error colour is matplotlib's plasma of 2 x the squared distance
from each ground-truth vertex to the nearest aligned prediction sample.  This departs from the reference, which indexes
chamfer3D's first output (one entry per prediction sample) by ground-truth vertex (:168, :172) and so colours vertex k with
sample k's error.  The printed scores do not depend on --render.
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lasr_amd import phong, vis                            # noqa: E402
from lasr_amd.nnutils import fused_ops                     # noqa: E402
from lasr_amd.nnutils.icp import iterative_closest_point  # noqa: E402
from lasr_amd.nnutils.manifold import watertight           # noqa: E402
from lasr_amd.soft_renderer.functional import load_obj      # noqa: E402


def sample_points(verts, faces, n, gen, return_normals=False):
    """n points uniformly distributed over the surface (area-weighted faces, uniform barycentrics); with return_normals also the
    unit normal of the face each point was drawn from (pytorch3d.ops.sample_points_from_meshes(..., return_normals=True))."""
    tri = verts[faces]
    cr = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = cr.norm(dim=1)
    pick = torch.multinomial(area / area.sum(), n, replacement=True, generator=gen)
    u = torch.rand(n, 2, device=verts.device, generator=gen)
    su = u[:, :1].sqrt()
    w = torch.cat([1 - su, su * (1 - u[:, 1:]), su * u[:, 1:]], 1)
    pts = (tri[pick] * w[:, :, None]).sum(1)
    if not return_normals:
        return pts
    return pts, cr[pick] / area[pick, None].clamp_min(1e-12)


def diameter(x):
    return float(torch.cdist(x, x).max())


def icp(x, y, iters=100, tol=1e-7):
    """Rigid (R, t) minimising sum |x R + t - nn_y(x R + t)|^2 by alternating nearest neighbours and Kabsch."""
    R = torch.eye(3, device=x.device)
    t = torch.zeros(3, device=x.device)
    prev = None
    for _ in range(iters):
        xt = x @ R + t
        d2, idx = fused_ops.nearest_point(xt[None], y[None])
        err = float(d2.mean())
        if prev is not None and abs(prev - err) < tol * max(prev, 1e-12):
            break
        prev = err
        tgt = y[idx[0]]
        mx, my = x.mean(0), tgt.mean(0)
        U, _, Vt = torch.linalg.svd((x - mx).t() @ (tgt - my))
        D = torch.diag(torch.tensor([1., 1., float(torch.sign(torch.linalg.det(U @ Vt)))], device=x.device))
        R = U @ D @ Vt
        t = my - mx @ R
    return R, t


_icp_fast = icp                                            # evaluate_pair's keyword `icp` hides the function's name there


def chamfer(x, y):
    dx = fused_ops.nearest_point(x[None], y[None])[0].mean()
    dy = fused_ops.nearest_point(y[None], x[None])[0].mean()
    return float(dx + dy)


def chamfer_with_normals(x, nx, y, ny):
    """(Chamfer distance, normal term) of two point sets with unit normals: the two return values of
    pytorch3d.loss.chamfer_distance(x, y, x_normals=nx, y_normals=ny) with its defaults (mean over points, the two directions
    summed, abs_cosine: a flipped face orientation does not count)."""
    dx, ix = fused_ops.nearest_point(x[None], y[None])
    dy, iy = fused_ops.nearest_point(y[None], x[None])
    cos_x = torch.nn.functional.cosine_similarity(nx, ny[ix[0]], dim=1, eps=1e-6).abs()
    cos_y = torch.nn.functional.cosine_similarity(ny, nx[iy[0]], dim=1, eps=1e-6).abs()
    return float(dx.mean() + dy.mean()), float((1 - cos_x).mean() + (1 - cos_y).mean())


def evaluate_pair(pred, gt, n=10000, seed=0, with_normals=False, aligned=None, icp='fast'):
    """pred, gt: (verts [V,3], faces [F,3]) on the GPU -> Chamfer distance after normalisation and ICP; with_normals: the pair
    (Chamfer distance, normal consistency = 1 - normal term) the reference prints per frame (:197).  aligned: a dict that receives
    the normalised ground truth 'gt', the aligned prediction 'pred' and its evaluation sample 'sample' (with_normals only).
    icp: 'fast', the 100-iteration icp() above, or 'reference', the reference's call (:156)
    iterative_closest_point(X, Y, estimate_scale=False, max_iterations=10000) on the device-resident loop of lasr_amd/nnutils/icp.py;
    aligned then also receives its 'icp_iterations' and 'icp_converged'."""
    if icp not in ('fast', 'reference'):
        raise ValueError("icp is 'fast' or 'reference', got %r" % (icp,))
    gen = torch.Generator(device=pred[0].device).manual_seed(seed)
    (xv, xf), (yv, yf) = pred, gt
    yv = yv - yv.mean(0, keepdim=True)
    yv = 10 * yv / diameter(sample_points(yv, yf, 4000, gen))
    xv = xv - xv.mean(0, keepdim=True)
    xv = 10 * xv / diameter(sample_points(xv, xf, 4000, gen))
    xs, ys = sample_points(xv, xf, n, gen), sample_points(yv, yf, n, gen)
    if icp == 'reference':
        sol = iterative_closest_point(xs[None], ys[None], estimate_scale=False, max_iterations=10000)
        R, t = sol.RTs.R[0], sol.RTs.T[0]
        if aligned is not None:
            aligned.update(icp_iterations=sol.iterations, icp_converged=sol.converged)
    else:
        R, t = _icp_fast(xs, ys)
    xv = xv @ R + t
    if not with_normals:
        return chamfer(sample_points(xv, xf, n, gen), sample_points(yv, yf, n, gen))
    x, nx = sample_points(xv, xf, n, gen, True)
    y, ny = sample_points(yv, yf, n, gen, True)
    cd, norm = chamfer_with_normals(x, nx, y, ny)
    if aligned is not None:
        aligned.update(gt=yv, pred=xv, sample=x)
    return cd, 1. - norm


RENDER_SIZE = 512


def error_colors(d2):
    """RGB of matplotlib's plasma at 2 x the squared error d2 (values above 0.5 saturate)."""
    import matplotlib
    return matplotlib.colormaps['plasma'](2 * np.asarray(d2, np.float64))[:, :3]


def render_triplet(gt, pred, sample):
    """The reference's gt / pd / cd images (:170-192): gt (verts, faces) normalised, pred aligned, sample its evaluation points.
    Both meshes are divided by 1.05 max|gt|, x and z negated and z shifted to start at 1; grey 0.5, or the error colours.
    -> uint8 [512, 3 * 512, 3] (np.clip(255 img, 0, 255) truncated)."""
    (yv, yf), (xv, xf) = gt, pred
    d2 = fused_ops.nearest_point(yv[None].contiguous(), sample[None].contiguous())[0][0]
    err = torch.as_tensor(error_colors(d2.cpu().numpy()), dtype=torch.float32, device=yv.device)
    s = 1.05 * yv.abs().max()

    def place(v):
        v = v / s
        v = torch.stack([-v[:, 0], v[:, 1], -v[:, 2]], 1)
        return torch.stack([v[:, 0], v[:, 1], v[:, 2] - (v[:, 2].min() - 1)], 1)
    vy, vx = place(yv), place(xv)
    fy, fx = vis.fix_inversion(vy, yf).to(yv.device), vis.fix_inversion(vx, xf).to(xv.device)
    grey_y = torch.full_like(vy, 0.5)
    gt_cd = phong.render(torch.stack([vy, vy]), fy, torch.stack([grey_y, err]), RENDER_SIZE)
    pd = phong.render(vx[None], fx, torch.full_like(vx, 0.5), RENDER_SIZE)
    img = torch.cat([gt_cd[0, ..., :3], pd[0, ..., :3], gt_cd[1, ..., :3]], 1)
    return np.clip(255 * img.cpu().numpy(), 0, 255).astype(np.uint8)


def write_renders(testdir, i, img):
    from PIL import Image
    S = RENDER_SIZE
    for k, name in enumerate(('gt', 'pd', 'cd')):
        Image.fromarray(np.ascontiguousarray(img[:, k * S:(k + 1) * S])).save(os.path.join(testdir, '%s-%06d.png' % (name, i)))


def write_gif(path, frames):
    """imageio.mimsave(path, frames, duration=5 / len(frames)): 5 s in all."""
    from PIL import Image
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    ims = [Image.fromarray(f) for f in frames]
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=int(round(5000. / len(ims))), loop=0)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='mesh evaluation')
    ap.add_argument('--testdir', required=True)
    ap.add_argument('--gtdir', required=True)
    ap.add_argument('--remesh', type=int, default=0, metavar='RESOLUTION',
                    help='re-mesh each prediction watertight at this resolution first (the reference: 10000); 0: as it is')
    ap.add_argument('--render', action='store_true', help='write gt-/pd-/cd-%%06d.png into --testdir and the --gif')
    ap.add_argument('--icp', choices=('fast', 'reference'), default='fast',
                    help="rigid alignment: 'fast', at most 100 iterations (default), or 'reference', the reference's "
                         'iterative_closest_point(..., max_iterations=10000) with its RMSE stop test')
    ap.add_argument('--gif', default=os.path.join('tmp', 'output.gif'), help='the GIF --render writes (default tmp/output.gif)')
    args = ap.parse_args(argv)
    if args.remesh < 0:
        ap.error('--remesh takes a non-negative resolution')
    return args


def main(argv=None):
    args = parse_args(argv)
    dev = torch.device('cuda', 0)
    gts = sorted(glob.glob('%s/*.obj' % args.gtdir))
    preds = sorted(glob.glob('%s/pred*.obj' % args.testdir)) or sorted(glob.glob('%s/*.obj' % args.testdir))
    assert len(gts) == len(preds) and gts, 'need the same number of predicted and ground-truth meshes'
    cds, ncs, frames, its = [], [], [], []
    for i, (p, g) in enumerate(zip(preds, gts)):
        pm, gm = load_obj(p, device=dev), load_obj(g, device=dev)
        pm = (pm[0].float(), pm[1].long())
        if args.remesh > 0:
            pm = watertight(pm[0], pm[1], args.remesh)
        al = {} if args.render or args.icp == 'reference' else None
        cd, nc = evaluate_pair(pm, (gm[0].float(), gm[1].long()), with_normals=True, aligned=al, icp=args.icp)
        if args.render:
            img = render_triplet((al['gt'], gm[1].long()), (al['pred'], pm[1]), al['sample'])
            write_renders(args.testdir, i, img)
            frames.append(img)
        cds.append(cd); ncs.append(nc)
        if args.icp == 'reference':
            its.append((al['icp_iterations'], al['icp_converged']))
        print('%04d: %.2f, %.2f' % (i, cd, nc))                       # the reference's line (:197): Chamfer, normal consistency
    print('ALL: %.2f, %.2f' % (np.mean(cds), np.mean(ncs)))
    if args.icp == 'reference':
        print('ICP iterations: %s%s' % (' '.join('%d' % k for k, _ in its), '' if all(c for _, c in its) else ' (not all converged)'))
    if args.render:
        write_gif(args.gif, frames)
    main.normal_consistency, main.icp_iterations = ncs, its
    return cds


if __name__ == '__main__':
    main()
