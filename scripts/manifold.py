#!/usr/bin/env python3
"""Make a triangle mesh watertight on the GPU, with the command line of the Manifold binary the reference runs
(reference: scripts/eval_mesh.py:100-105, render_vis.py:98, nnutils/train_utils.py:422):

    python scripts/manifold.py INPUT.obj OUTPUT.obj [RESOLUTION]

RESOLUTION (default 10000) is the least number of surface voxels of the grid; lasr_amd/nnutils/manifold.py:watertight states
the construction and how it departs from Manifold.  The output is a closed, consistently oriented 2-manifold.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description='watertight re-meshing of a triangle mesh (GPU)')
    ap.add_argument('input', help='input .obj')
    ap.add_argument('output', help='output .obj')
    ap.add_argument('resolution', nargs='?', type=int, default=10000, help='least number of surface voxels (default 10000)')
    args = ap.parse_args(argv)
    import torch
    from lasr_amd.nnutils.manifold import remesh
    from lasr_amd.soft_renderer.functional import load_obj, save_obj
    dev = torch.device('cuda', 0)
    verts, faces = load_obj(args.input, device=dev)[:2]
    r = remesh(verts.float(), faces.long(), args.resolution)
    save_obj(args.output, r['verts'], r['faces'].int())
    print('%s: %d vertices, %d faces -> %s: %d vertices, %d faces (grid %d^3, %d repair sweeps, %d guard rounds)'
          % (args.input, verts.shape[0], faces.shape[0], args.output, r['verts'].shape[0], r['faces'].shape[0], r['S'],
             r['repair_sweeps'], r['rounds']))
    return r


if __name__ == '__main__':
    main()
