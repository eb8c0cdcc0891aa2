#!/usr/bin/env python3
"""Write a reconstruction as one rigged, animated glTF 2.0 binary (this project's own addition; the reference has no exporter --
DESIGN.md section 4.12).

    python extract.py ... --rig                                   # writes <testdir>/rig.npz beside pred<i>.obj
    python scripts/export_gltf.py --testdir log/camel-5/ --outpath camel.glb \\
        [--influences 4|8|auto] [--max_dev 0.005] [--fps 10] [--texture_obj log/camel-5/baked.obj]

The .glb holds the rest mesh, a skin of n_bones - 1 joints under an animated root, one keyframe per video frame, and the
model's vertex colours -- or, with --texture_obj, the atlas scripts/bake_texture.py wrote (its .obj names the .png through its
.mtl; vertices are then split per face corner).  glTF stores 4 influences per vertex (8 with a second attribute set) where
LASR's skin is dense: the k largest weights are kept and renormalised (lasr_amd/nnutils/rig.py, csrc/rig.hip), and the printed
deviation is what that costs against the full-weight blend, as a share of the rest shape's bounding-box diagonal.  `auto` keeps
4 unless that deviation exceeds --max_dev, then 8.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Export the rig extract.py --rig wrote as an animated .glb.')
    p.add_argument('--testdir', default='', help='directory holding rig.npz (extract.py --rig)')
    p.add_argument('--outpath', default='', help='the .glb to write (default: <testdir>/rig.glb)')
    p.add_argument('--influences', default='auto', choices=['4', '8', 'auto'], help='joints per vertex; auto: 4 unless --max_dev is exceeded')
    p.add_argument('--max_dev', default=0.005, type=float, help='auto: largest deviation 4 influences may show, as a fraction of the diagonal')
    p.add_argument('--fps', default=10., type=float, help='keyframes per second')
    p.add_argument('--texture_obj', default='', help='the .obj scripts/bake_texture.py wrote: embed its atlas instead of vertex colours')
    return p.parse_args(argv)


def read_textured_obj(path):
    """-> (faces [F,3] vertex indices, uv [F,3,2] in the .obj's bottom-left convention, path of the material's map_Kd image)."""
    from lasr_amd.soft_renderer.functional.obj_io import parse_obj_materials
    faces = []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if tok and tok[0] == 'f':
                ids = [int(t.split('/')[0]) for t in tok[1:]]
                faces += [(ids[0], ids[i + 1], ids[i + 2]) for i in range(len(ids) - 2)]
    uv, mats, _, files = parse_obj_materials(path)
    used = sorted(set(mats))
    if len(used) != 1 or used[0] not in files:
        raise ValueError('%s must use exactly one material with a map_Kd image, found %s' % (path, used))
    return np.asarray(faces, np.int64).reshape(-1, 3) - 1, uv, files[used[0]]


def split_corners(arrays, faces, uv):
    """One vertex per face corner: every per-vertex array of build_rig gathered by the corner's vertex index, indices 0 .. 3F-1,
    uv [F,3,2] flattened with v -> 1 - v (glTF's origin is the image's top-left corner)."""
    idx = np.asarray(faces, np.int64).reshape(-1)
    out = dict(arrays)
    for key in ('positions', 'colors', 'joints', 'weights'):
        if arrays.get(key) is not None:
            out[key] = arrays[key][idx]
    out['indices'] = np.arange(len(idx), dtype=np.uint32).reshape(-1, 3)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    out['uv'] = np.stack([uv[:, 0], np.float32(1) - uv[:, 1]], 1)
    return out


def report_line(arrays, report):
    T, K = arrays['quat'].shape[:2]
    return ('%d bones, %d vertices, %d keys, %d influences: max deviation %.2f %% of the diagonal (frame %d), rms %.2f %%'
            % (K, arrays['positions'].shape[0], T, report['influences'], 100 * report['max_overall'],
               int(arrays['frame_ids'][report['frame']]), 100 * report['rms_overall']))


def main(argv=None):
    args = parse_args(argv)
    from lasr_amd.ext_utils import gltf
    from lasr_amd.nnutils import rig
    path = os.path.join(args.testdir, 'rig.npz')
    try:
        npz = dict(np.load(path))
    except OSError as e:
        raise SystemExit('export_gltf.py: no rig in %s (%s); run extract.py with --rig first' % (args.testdir, e))
    try:
        arrays, report = rig.build_rig(npz, 4 if args.influences == 'auto' else int(args.influences))
        if args.influences == 'auto' and report['max_overall'] > args.max_dev:
            arrays, report = rig.build_rig(npz, 8)
    except ValueError as e:
        raise SystemExit('export_gltf.py: %s' % e)
    print(report_line(arrays, report))
    out = dict(arrays)
    png = None
    if args.texture_obj:
        try:
            faces, uv, image = read_textured_obj(args.texture_obj)
            with open(image, 'rb') as f:
                png = f.read()
        except Exception as e:                             # parse_obj_materials raises a plain Exception without a material library
            raise SystemExit('export_gltf.py: cannot use %s (%s)' % (args.texture_obj, e))
        if faces.shape != arrays['indices'].shape or (faces != arrays['indices']).any():
            raise SystemExit('export_gltf.py: %s does not share the topology of the rig' % args.texture_obj)
        out = split_corners(arrays, faces, uv)
    outpath = args.outpath or os.path.join(args.testdir, 'rig.glb')
    if os.path.dirname(outpath):
        os.makedirs(os.path.dirname(outpath), exist_ok=True)
    n = gltf.write_glb(outpath, positions=out['positions'], indices=out['indices'], quat=out['quat'], trans=out['trans'],
                       joints=out['joints'], weights=out['weights'], colors=None if png else out['colors'],
                       uv=out.get('uv') if png else None, png=png, fps=args.fps)
    print('wrote %d bytes to %s' % (n, outpath))
    return arrays, report


if __name__ == '__main__':
    main()
