#!/usr/bin/env python3
"""Render a reconstruction as a GIF (reference: render_vis.py): the meshes extract.py wrote, shaded with a directional light and
its shadow over a white floor, or overlaid on the input video, or turned on a turntable.

    python render_vis.py --testdir log/spot3-1/ --seqname spot3 --outpath spot3.gif [--freeze] [--overlay] [--vis_bones]

Frames come from configs/<seqname>.config (relative paths against the working directory, as in the reference); per frame id i
the script reads <testdir>/pred<i>.ply (or pred<i>.obj), cam<i>.txt and, with --vis_bones, gauss<i>.ply.  extract.py's meshes
are in camera space already (as the reference's, whose cam<i>.txt then holds [I | 0]): only the intrinsics row of cam<i>.txt
is used, and the turntable's [R | T] replaces the identity pose.  Rendering: lasr_amd/vis.py (HIP shading over the hard-mode
rasteriser); DESIGN.md section 4.4.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from lasr_amd.recon_io import frame_id, frame_list, load_mesh   # noqa: E402,F401  (frame_list and load_mesh: imported from here too)


def parse_args(argv=None):
    """The reference's flags (names, destinations and defaults); the help texts are this project's."""
    p = argparse.ArgumentParser(description='Render the meshes extract.py wrote for a sequence into an animated GIF.')
    p.add_argument('--testdir', default='', help='directory holding pred<i>.ply / .obj, cam<i>.txt and gauss<i>.ply')
    p.add_argument('--seqname', default='camel', help='sequence name: its frames are listed by configs/<seqname>.config')
    p.add_argument('--watertight', default='no', help="'yes' would re-mesh through the Manifold binary, which this project does not ship")
    p.add_argument('--outpath', default='/data/gengshay/output.gif', help='GIF file to write')
    p.add_argument('--cam_type', default='perspective', help="camera model; only 'perspective' is supported")
    p.add_argument('--append_img', default='no', help="'yes': put input frames in front of the renders")
    p.add_argument('--append_render', default='yes', help="'no': leave the renders out (with --append_img yes: frames only)")
    p.add_argument('--nosmooth', dest='smooth', action='store_false', help='shade with face normals instead of vertex normals')
    p.add_argument('--gray', dest='gray', action='store_true', help='colour the mesh a uniform dark grey')
    p.add_argument('--overlay', dest='overlay', action='store_true', help='blend a blue mesh half and half with each input frame')
    p.add_argument('--vis_bones', dest='vis_bones', action='store_true',
                   help='draw the bone ellipsoids (gauss<i>.ply) under a translucent surface')
    p.add_argument('--freeze', dest='freeze', action='store_true', help='turn the first frame\'s mesh on a 150-frame turntable')
    return p.parse_args(argv)


def resize(img, size):
    """uint8 [..., H, W, 3] -> [..., h, w, 3], bilinear (align_corners=False), rounded."""
    x = img.float().reshape(-1, *img.shape[-3:]).permute(0, 3, 1, 2)
    y = torch.nn.functional.interpolate(x, size=size, mode='bilinear', align_corners=False)
    return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)


def build_scenes(args, meshes, bones, cams, count, IS, H, W):
    """Per output frame the scene vis.render_sequence takes: the opaque layer (mesh, or the bones with --vis_bones), the floor
    (not with --overlay), then the translucent surface with --vis_bones; camera space, intrinsics from cam<i>.txt or the
    turntable's."""
    from lasr_amd import vis
    scenes = []
    if args.freeze:
        v0, f0, c0 = meshes[0]
        allv = torch.cat([v0] + ([bones[0][0]] if args.vis_bones else []))
        allv = allv - allv.mean(0)
        allv = allv / (1.2 * allv.abs().max())
    for i in range(count):
        if args.freeze:
            R, T = vis.turntable_camera(i, count)
            K = (8 * IS / 2, 8 * IS / 2, W / 2, H / 2)
            posed = allv.double() @ torch.from_numpy(R) + torch.from_numpy(T)
            v, f, c = posed[:len(v0)].float(), f0, c0
            bv = posed[len(v0):].float() if args.vis_bones else None
            bf, bc = (bones[0][1], bones[0][2]) if args.vis_bones else (None, None)
        else:
            v, f, c = meshes[i]
            K = tuple(cams[i][3])
            if args.vis_bones:
                bv, bf, bc = bones[i]
        parts = [(bv, bf, bc)] if args.vis_bones else [(v, f, c)]           # the opaque layer first
        if not args.overlay:
            parts.append(vis.floor_quad(v))
        if args.vis_bones:
            parts.append((v, f, c))                                       # the translucent surface
        vs, fs, cs, caster, base = [], [], [], [], 0
        for k, (pv, pf, pc) in enumerate(parts):
            vs.append(pv)
            fs.append(torch.as_tensor(pf, dtype=torch.long) + base)
            pc = torch.as_tensor(pc)
            cs.append(pc.float() / 255. if pc.dtype == torch.uint8 else pc.float())
            floor = not args.overlay and k == 1
            caster.append(torch.full((len(pv),), not floor, dtype=torch.bool))
            base += len(pv)
        n_opaque = sum(len(x) for x in fs[:-1]) if args.vis_bones else sum(len(x) for x in fs)
        scenes.append(dict(verts=torch.cat(vs), faces=torch.cat(fs), colors=torch.cat(cs), K=K, n_opaque=n_opaque,
                           casters=torch.cat(caster)))
    return scenes


def main(argv=None):
    args = parse_args(argv)
    if args.cam_type != 'perspective':
        raise SystemExit('render_vis.py: only --cam_type perspective is supported (the reference\'s orthographic branch mixes '
                         'pixel and unit coordinates, render_vis.py:220-224, :275)')
    if args.watertight == 'yes':
        raise SystemExit('render_vis.py: --watertight yes needs the Manifold binary, which this project does not ship '
                         '(see lasr_amd/nnutils/remesh.py)')
    from PIL import Image
    from lasr_amd import vis
    from lasr_amd.ext_utils.ply import read_ply
    if args.append_img != 'yes' and args.append_render != 'yes':
        raise SystemExit('render_vis.py: nothing to write: --append_render no needs --append_img yes')
    dev = torch.device('cuda', 0)

    names = frame_list(args.seqname)
    if not names:
        raise SystemExit('render_vis.py: no frames for sequence %s' % args.seqname)
    imgs, meshes, cams, bones = [], [], [], []
    for name in names:
        fr = frame_id(name)
        print('%s/%d' % (args.seqname, fr))
        imgs.append(np.asarray(Image.open(name).convert('RGB')))
        try:
            v, f, c = load_mesh(args.testdir, fr)
            cams.append(np.loadtxt(os.path.join(args.testdir, 'cam%d.txt' % fr)))
        except (OSError, ValueError) as e:
            raise SystemExit('render_vis.py: no mesh for frame %d in %s (%s)' % (fr, args.testdir, e))
        f = vis.fix_inversion(v, f)
        if args.gray:
            c[:] = 64
        if args.overlay:
            c[:, :2], c[:, 2] = 0, 255
        meshes.append((v, f, c))
        if args.vis_bones:
            b = read_ply(os.path.join(args.testdir, 'gauss%d.ply' % fr))
            bones.append((torch.from_numpy(b['verts']).float(), torch.from_numpy(b['faces']), torch.from_numpy(b['colors'])))

    H, W = imgs[0].shape[:2]
    IS = max(H, W)
    out_size = (int(H * 480 / W), 480)
    frames = []
    if args.append_img == 'yes':
        first = torch.from_numpy(np.stack(imgs[:1] if args.append_render == 'yes' else imgs))
        small = resize(first, out_size).numpy()
        if args.append_render == 'yes':
            frames += [small[0]] * (30 if args.freeze else len(imgs) // 5)
        else:
            frames += list(small)

    if args.append_render == 'yes':
        count = 150 if args.freeze else len(imgs)
        scenes = build_scenes(args, meshes, bones, cams, count, IS, H, W)
        with torch.no_grad():                      # chunk by chunk: device memory stays bounded by vis.CHUNK_FRAMES
            for rgb in vis.render_chunks(scenes, IS, H, W, smooth=args.smooth, overlay=args.overlay,
                                         frames=[imgs[0]] * count if args.freeze else imgs, device=dev):
                frames += list(resize(rgb, out_size).cpu().numpy())

    pil = [Image.fromarray(f) for f in frames]
    pil[0].save(args.outpath, save_all=True, append_images=pil[1:], duration=5000. / len(pil), loop=0)
    print('wrote %d frames to %s' % (len(pil), args.outpath))
    return len(pil)


if __name__ == '__main__':
    main()
