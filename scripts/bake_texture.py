#!/usr/bin/env python3
"""Bake a texture atlas from the video frames onto the meshes extract.py wrote (this project's own addition; the reference has
no counterpart -- DESIGN.md section 4.11).

    python scripts/bake_texture.py --testdir log/camel-5/ --seqname camel \\
        [--texture_res 8] [--power 2] [--pose_frame 0] [--no_mask] [--outpath DIR/baked] [--preview out.gif]
        [--fill none|blend|mirror] [--rig DIR/rig.npz] [--symidx 0] [--sym_tol 0.05] [--fill_iters 64]

Reads what render_vis.py reads: the frames of configs/<seqname>.config, per frame id i <testdir>/pred<i>.ply (or .obj) in camera
space and the intrinsics row of cam<i>.txt, and the silhouettes of the matching Annotations folder.  Every texel of the per-face
surface textures is averaged over the frames that see it (lasr_amd/nnutils/bake.py, csrc/bake.hip); texels no frame sees take
the mesh's vertex colours.  Writes <outpath>.obj / .mtl / .png (the mesh of --pose_frame with the atlas) and <outpath>_weight.npy,
and with --preview a GIF of the baked mesh rendered back into every frame's camera beside the video frame.

--fill (off by default; without it every output is what it was) completes the texels no frame saw, the far side of a monocular
video above all: `mirror` copies the texel of the mirror image over the symmetry plane x[symidx] = 0 of the rest shape (rig.npz of
extract.py --rig), `blend` smooths what is still unfilled from its neighbours (csrc/bake_fill.hip).  Also writes
<outpath>_source.npy (per texel 0 seen, 1 mirrored, 2 blended) and prints `filled: mirrored X %, blended Y %`.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import recon_io                                                          # noqa: E402
from lasr_amd.recon_io import check_topology, annotation_path as silhouette_path      # noqa: E402,F401  (imported from here too)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Bake the video frames onto the reconstructed meshes as a texture atlas.')
    p.add_argument('--testdir', default='', help='directory holding pred<i>.ply / .obj and cam<i>.txt')
    p.add_argument('--seqname', default='camel', help='sequence name: its frames are listed by configs/<seqname>.config')
    p.add_argument('--texture_res', default=8, type=int, help='texels per face edge: each face gets R x R texels')
    p.add_argument('--power', default=2, type=int, help='exponent of the view weight |n . d|^power (0: plain mean)')
    p.add_argument('--pose_frame', default=0, type=int, help='position in the frame list of the mesh the .obj is written for')
    p.add_argument('--no_mask', dest='mask', action='store_false', help='do not restrict the samples to the silhouettes')
    p.add_argument('--outpath', default='', help='output path without extension (default: <testdir>/baked)')
    p.add_argument('--preview', default='', help='GIF to write: the baked mesh in every frame\'s camera, beside the frame')
    p.add_argument('--fill', default='none', choices=('none', 'blend', 'mirror'),
                   help='complete the texels no frame saw: blend = smooth them from their neighbours; mirror = first copy the '
                        'mirror image over the symmetry plane of the rest shape (needs --rig), then blend what is left')
    p.add_argument('--rig', default='', help='rig.npz of extract.py --rig, for its rest shape (default: <testdir>/rig.npz)')
    p.add_argument('--symidx', default=0, type=int, help='the rest shape is symmetric about the plane x[symidx] = 0 (as optimize.py)')
    p.add_argument('--sym_tol', default=0.05, type=float,
                   help='--fill mirror: largest distance of a mirrored point from the surface, as a fraction of the rest '
                        'bounding-box diagonal (a default nobody has measured on a real reconstruction)')
    p.add_argument('--fill_iters', default=64, type=int,
                   help='--fill: Jacobi iterations of the blend; the seam is feathered over about sqrt(iters) texels (a default '
                        'nobody has measured on a real reconstruction)')
    return p.parse_args(argv)


def load_rest_shape(path, face):
    """rest_verts float32 [V,3] of rig.npz, refused (ValueError) when the file is missing or is not the rig of these meshes."""
    if not os.path.exists(path):
        raise ValueError('--fill mirror needs the rest shape: %s does not exist (write it with extract.py --rig)' % path)
    with np.load(path) as npz:
        if 'rest_verts' not in npz.files or 'faces' not in npz.files:
            raise ValueError('%s holds no rest_verts / faces: it is not what extract.py --rig writes' % path)
        rest, rf = np.asarray(npz['rest_verts'], np.float32), np.asarray(npz['faces'])
    face = np.asarray(face)
    if rf.shape != face.shape or (rf != face).any():
        raise ValueError('the faces of %s differ from the topology of the pred<i> meshes: run extract.py --rig on the same '
                         'checkpoint' % path)
    if rest.ndim != 2 or rest.shape[1] != 3 or not np.isfinite(rest).all() or (face.size and face.max() >= rest.shape[0]):
        raise ValueError('rest_verts of %s must be finite [V, 3] and hold every vertex the faces name (extract.py --rig)' % path)
    return rest


def main(argv=None):
    args = parse_args(argv)
    from PIL import Image
    from lasr_amd.nnutils import bake
    from lasr_amd.soft_renderer.functional import save_obj
    dev = torch.device('cuda', 0)
    names = recon_io.frame_list(args.seqname)
    if not names:
        raise SystemExit('bake_texture.py: no frames for sequence %s' % args.seqname)
    if not 0 <= args.pose_frame < len(names):
        raise SystemExit('bake_texture.py: --pose_frame %d is outside the %d frames' % (args.pose_frame, len(names)))
    if args.texture_res < 2:
        raise SystemExit('bake_texture.py: --texture_res must be at least 2 (the atlas writer needs it)')
    try:
        rec = recon_io.read(args.testdir, names, annotations='L' if args.mask else None,
                            no_annotation='no silhouette for %(name)s (%(e)s); pass --no_mask to bake without')
    except recon_io.ReadError as e:
        raise SystemExit('bake_texture.py: %s' % e)
    imgs, face = rec.imgs, rec.face
    rest = None
    if args.fill != 'none':
        if args.symidx not in (0, 1, 2) or not 0 <= args.sym_tol < float('inf') or args.fill_iters < 0:
            raise SystemExit('bake_texture.py: --symidx must be 0, 1 or 2, --sym_tol a finite fraction >= 0, --fill_iters >= 0')
    if args.fill == 'mirror':
        try:
            rest = load_rest_shape(args.rig or os.path.join(args.testdir, 'rig.npz'), face)
        except ValueError as e:
            raise SystemExit('bake_texture.py: %s' % e)
    H, W = imgs[0].shape[:2]
    R = args.texture_res
    tv = torch.from_numpy(np.stack(rec.verts)).to(dev)
    tf = torch.from_numpy(face).to(dev)
    tK = torch.from_numpy(rec.K).to(dev)
    frames = torch.from_numpy(np.stack(imgs)).to(dev)
    masks = torch.from_numpy(np.stack(rec.masks)).to(dev) if args.mask else None
    fallback = torch.from_numpy(rec.colors[args.pose_frame]).to(dev).float() / 255.
    with torch.no_grad():
        textures, weight = bake.bake_texture(tv, tf, tK, frames, masks, texture_res=R, power=args.power, fallback=fallback)
        source = None
        if args.fill != 'none':                        # the .obj / .png and the preview carry the completed atlas
            textures, source, _ = bake.complete_texture(tf, textures, weight, fill=args.fill,
                                                        rest_verts=None if rest is None else torch.from_numpy(rest).to(dev),
                                                        axis=args.symidx, tol=args.sym_tol, iters=args.fill_iters)
    out = args.outpath or os.path.join(args.testdir, 'baked')
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    save_obj(out + '.obj', torch.from_numpy(rec.verts[args.pose_frame]), torch.from_numpy(face), textures, R, 'surface')
    w = weight.cpu().numpy()
    np.save(out + '_weight.npy', w)
    print('baked %d faces x %d texels, seen %.1f %%' % (face.shape[0], R * R, 100. * float((w > 0).mean())))
    if source is not None:
        s = source.cpu().numpy()
        np.save(out + '_source.npy', s)
        print('filled: mirrored %.1f %%, blended %.1f %%' % (100. * float((s == bake.MIRRORED).mean()),
                                                             100. * float((s == bake.BLENDED).mean())))

    if args.preview:
        pil = []                                       # native size, no resampling: the video frame left, the render right
        with torch.no_grad():
            for i in range(0, len(names), bake.CHUNK_FRAMES):
                j = min(i + bake.CHUNK_FRAMES, len(names))
                rgba = bake.render_baked(tv[i:j], tf, tK[i:j], textures, H, W)
                rgb = (rgba[:, :3].clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
                pair = torch.cat([frames[i:j], rgb], 2)
                pil += [Image.fromarray(p) for p in pair.cpu().numpy()]
        pil[0].save(args.preview, save_all=True, append_images=pil[1:], duration=5000. / len(pil), loop=0)
        print('wrote %d frames to %s' % (len(pil), args.preview))
    return textures, weight


if __name__ == '__main__':
    main()
