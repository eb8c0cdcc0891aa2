#!/usr/bin/env python3
"""Score the geometry of a reconstruction without ground truth (this project's own addition; the reference has no counterpart --
DESIGN.md section 4.18).

    python scripts/eval_shape.py --testdir log/camel-5/ --seqname camel \\
        [--outpath shape.json] [--worst 5] [--max_pairs 4096] [--ply DIR] [--neighbours [--fold_deg 20]]

scripts/eval_reproj.py scores what a reconstruction looks like from the camera; a mesh can reproject well and still pass through
itself, be turned inside out or shake from frame to frame.  This script reads the same meshes: the frames of
configs/<seqname>.config and, per frame id i, <testdir>/pred<i>.ply (or .obj), all with one topology.  Per frame it reports
(lasr_amd/nnutils/meshcheck.py, csrc/meshcheck.hip): n_pairs, the number of pairs of faces that intersect (an exact test over all
pairs of faces that share no vertex; touching and coplanar overlap do not count, and a fold between two neighbouring faces goes
unseen unless --neighbours is given), n_faces, the number of faces involved, and ratio = n_faces / F; the signed volume (negative: the mesh is inside out,
`inverted`) and the area; jitter, the mean second difference of the vertex positions over time relative to the diagonal of the
mesh's box (none for the first and the last frame).  Writes a JSON (default <testdir>/shape.json) with the parameters, the frame
ids, the per-frame values and their means over the frames (frames without a value left out and counted), prints one summary line
and the --worst frames by ratio.  A frame with more than --max_pairs intersecting pairs is `truncated`: its counts stay exact.
--ply writes per frame shape-%05d.ply, the mesh with the vertices of the involved faces in red and the rest in grey.

--neighbours adds a second pass over the faces that do share a vertex or an edge (scripts/shape_neighbours.py, csrc/meshnbr.hip):
the commonest defect of an optimised mesh is a vertex that slid across its own ring, a fin folded flat or a limb tip turned inside
out, and none of these makes two distant faces cross.  Per frame: n_pierced, the pairs of faces sharing one vertex of which the
edge opposite that vertex passes through the other face; n_creased, the pairs of faces sharing an edge whose interior dihedral
angle is below --fold_deg (an angle criterion, not an intersection test: non-coplanar faces that share an edge cannot intersect
outside it); n_neighbour_faces, the faces in either; min_dihedral, the sharpest interior dihedral angle in degrees.  The default
--fold_deg 20 is derived from nothing measured on a real reconstruction: judge by min_dihedral.  The parameters gain the topology's
counts (vertex pairs, edge pairs, duplicate faces, degenerate faces, and edges that run in the same direction in both their faces:
an orientation-consistency report), one more summary line is printed, and --ply paints the vertices of faces involved only in
neighbour hits orange.  ratio and the worst frames stay defined as they are.  Without the flag nothing changes.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import recon_io                   # noqa: E402
from lasr_amd.recon_io import check_topology    # noqa: E402,F401  (imported from here too)

PER_FRAME_INT = ('n_pairs', 'n_faces')
PER_FRAME_FLOAT = ('ratio', 'volume', 'area', 'jitter')
PER_FRAME_BOOL = ('inverted', 'truncated')
MEANS = ('n_pairs', 'n_faces', 'ratio', 'volume', 'area', 'jitter')
RED, GREY = (255, 0, 0), (160, 160, 160)
ORANGE = (255, 160, 0)
NBR_INT = ('n_pierced', 'n_creased', 'n_neighbour_faces')                       # --neighbours: the keys it adds
NBR_FLOAT = ('min_dihedral',)
NBR_TOPOLOGY = (('vertex_pairs', 'n_vertex'), ('edge_pairs', 'n_edge'), ('duplicate_faces', 'n_duplicate'),
                ('degenerate_faces', 'n_degenerate'), ('same_direction_edges', 'n_same'))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Self-intersections, signed volume, area and temporal jitter of the reconstructed meshes.')
    p.add_argument('--testdir', default='', help='directory holding pred<i>.ply / .obj')
    p.add_argument('--seqname', default='camel', help='sequence name: its frames are listed by configs/<seqname>.config')
    p.add_argument('--outpath', default='', help='output .json (default: <testdir>/shape.json)')
    p.add_argument('--worst', default=5, type=int, help='how many of the worst frames by ratio to print')
    p.add_argument('--max_pairs', default=4096, type=int,
                   help='intersecting pairs listed per frame; a frame with more is marked truncated, its counts stay exact')
    p.add_argument('--ply', default='', help='directory for shape-%%05d.ply: the vertices of the involved faces in red')
    p.add_argument('--neighbours', action='store_true',
                   help='also test the faces that share a vertex or an edge: folds between neighbours (n_pierced, n_creased, min_dihedral)')
    p.add_argument('--fold_deg', default=20., type=float,
                   help='--neighbours: two faces sharing an edge are creased below this interior dihedral angle, in (0, 90] degrees '
                        '(default 20: unmeasured on any real reconstruction)')
    return p.parse_args(argv)


def check_finite(verts_list, frame_ids):
    for fr, v in zip(frame_ids, verts_list):
        if not np.isfinite(np.asarray(v)).all():
            raise ValueError('pred%d has a vertex that is not finite' % fr)


def summarise(res, frame_ids, params):
    """evaluate()'s per-frame arrays -> the JSON document: params, frame_ids, per_frame (lists; None for a NaN), means over the
    frames that have a value and nan_frames, how many have none.  A result of --neighbours (it holds n_pierced) adds its four keys to
    per_frame, means and nan_frames."""
    nbr = 'n_pierced' in res
    per = {k: [int(x) for x in res[k]] for k in PER_FRAME_INT + (NBR_INT if nbr else ())}
    per.update({k: [None if np.isnan(x) else float(x) for x in np.asarray(res[k], np.float64)]
                for k in PER_FRAME_FLOAT + (NBR_FLOAT if nbr else ())})
    per.update({k: [bool(x) for x in res[k]] for k in PER_FRAME_BOOL})
    means, nans = {}, {}
    for k in MEANS + (NBR_INT + NBR_FLOAT if nbr else ()):
        x = np.asarray(res[k], np.float64)
        good = np.isfinite(x)
        means[k] = float(x[good].mean()) if good.any() else None
        nans[k] = int((~good).sum())
    return dict(params=params, frame_ids=[int(i) for i in frame_ids], per_frame=per, means=means, nan_frames=nans,
                n_inverted=int(np.sum(per['inverted'])), n_truncated=int(np.sum(per['truncated'])))


def _fmt(x, spec='%.4f'):
    return 'n/a' if x is None else spec % x


def summary_line(doc):
    m = doc['means']
    return 'shape: %d frames, %s intersecting pairs and %s of the faces involved per frame, volume %s, area %s, jitter %s, %d inverted' % (
        len(doc['frame_ids']), _fmt(m['n_pairs'], '%.1f'), _fmt(m['ratio']), _fmt(m['volume'], '%.4g'), _fmt(m['area'], '%.4g'),
        _fmt(m['jitter'], '%.3e'), doc['n_inverted'])


def neighbour_line(doc):
    m, p = doc['means'], doc['params']
    return ('neighbours: %s pierced and %s creased pairs (below %g degrees) per frame, %s of the faces involved, sharpest dihedral %s '
            'degrees; %d vertex pairs, %d edge pairs, %d same-direction edges' % (
                _fmt(m['n_pierced'], '%.1f'), _fmt(m['n_creased'], '%.1f'), p['fold_deg'],
                _fmt(None if m['n_neighbour_faces'] is None or not p['faces'] else m['n_neighbour_faces'] / p['faces']),
                _fmt(None if not doc['per_frame']['min_dihedral'] or all(x is None for x in doc['per_frame']['min_dihedral'])
                     else min(x for x in doc['per_frame']['min_dihedral'] if x is not None), '%.3f'),
                p['vertex_pairs'], p['edge_pairs'], p['same_direction_edges']))


def worst_lines(doc, count):
    """The `count` frames with the highest ratio, highest first (ties: the earlier frame)."""
    per = doc['per_frame']
    order = sorted(range(len(per['ratio'])), key=lambda i: (-per['ratio'][i], i))[:max(count, 0)]
    return ['worst: frame %d (position %d) %d pairs, %d faces, ratio %.4f%s%s'
            % (doc['frame_ids'][i], i, per['n_pairs'][i], per['n_faces'][i], per['ratio'][i], ', inverted' if per['inverted'][i] else '',
               ', truncated' if per['truncated'][i] else '') for i in order]


def vertex_colours(face_count, faces, V, nbr_count=None):
    """uint8 [V,3]: red for the vertices of the faces with face_count > 0, grey for the rest.  nbr_count [2,F] (--neighbours): orange
    for the vertices of the faces with a neighbour hit; red wins."""
    col = np.tile(np.array(GREY, np.uint8), (V, 1))
    if nbr_count is not None:
        col[np.unique(np.asarray(faces)[np.asarray(nbr_count).sum(0) > 0].reshape(-1))] = ORANGE
    col[np.unique(np.asarray(faces)[np.asarray(face_count) > 0].reshape(-1))] = RED
    return col


def write_plys(directory, verts, faces, face_count, frame_ids, nbr_count=None):
    from lasr_amd.ext_utils.ply import write_ply
    os.makedirs(directory, exist_ok=True)
    paths = []
    for t, (v, c, fr) in enumerate(zip(verts, face_count, frame_ids)):
        paths.append(os.path.join(directory, 'shape-%05d.ply' % fr))
        write_ply(paths[-1], v, faces, colors=vertex_colours(c, faces, v.shape[0], None if nbr_count is None else nbr_count[t]))
    return paths


def main(argv=None, evaluate=None):
    """evaluate: a stand-in for lasr_amd.nnutils.meshcheck.evaluate taking and returning numpy arrays (the tests without a device
    inject the float64 restatement); by default the tensors go to the GPU.  With --neighbours it is called with the fold angle as a
    fourth argument and returns the keys of scripts/shape_neighbours.py: evaluate besides."""
    args = parse_args(argv)
    try:
        names = recon_io.frame_list(args.seqname)
    except FileNotFoundError as e:
        raise SystemExit('eval_shape.py: no config for sequence %s (%s)' % (args.seqname, e))
    if not names:
        raise SystemExit('eval_shape.py: no frames for sequence %s' % args.seqname)
    if args.max_pairs < 0:
        raise SystemExit('eval_shape.py: --max_pairs must be at least 0')
    if args.neighbours and not 0. < args.fold_deg <= 90.:
        raise SystemExit('eval_shape.py: --fold_deg must be inside (0, 90]')
    try:
        rec = recon_io.read(args.testdir, names, frames=False, cams=False)
        face, ids = rec.face, rec.ids
        check_finite(rec.verts, ids)
        verts = np.stack(rec.verts)
        if args.neighbours:
            res = (evaluate or _evaluate_neighbours_on_device)(verts, face, args.max_pairs, args.fold_deg)
        else:
            res = (evaluate or _evaluate_on_device)(verts, face, args.max_pairs)
    except ValueError as e:
        raise SystemExit('eval_shape.py: %s' % e)
    params = dict(testdir=args.testdir, seqname=args.seqname, max_pairs=args.max_pairs, vertices=int(verts.shape[1]),
                  faces=int(face.shape[0]))
    if args.neighbours:
        params.update(neighbours=True, fold_deg=float(args.fold_deg))
        params.update({name: int(res['topology'][key]) for name, key in NBR_TOPOLOGY})
    doc = summarise(res, ids, params)
    out = args.outpath or os.path.join(args.testdir, 'shape.json')
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    print(summary_line(doc))
    if args.neighbours:
        print(neighbour_line(doc))
    for line in worst_lines(doc, args.worst):
        print(line)
    if args.ply:
        paths = write_plys(args.ply, verts, face, res['face_count'], ids, res['nbr_count'] if args.neighbours else None)
        print('wrote %d meshes to %s' % (len(paths), args.ply))
    return doc


def _evaluate_on_device(verts, faces, max_pairs):
    import torch
    from lasr_amd.nnutils import meshcheck
    dev = torch.device('cuda', 0)
    with torch.no_grad():
        return meshcheck.evaluate(torch.from_numpy(verts).to(dev), torch.from_numpy(np.ascontiguousarray(faces)).to(dev), max_pairs)


def _evaluate_neighbours_on_device(verts, faces, max_pairs, fold_deg):
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import shape_neighbours                                                        # (beside this file)
    dev = torch.device('cuda', 0)
    with torch.no_grad():
        return shape_neighbours.evaluate(torch.from_numpy(verts).to(dev), torch.from_numpy(np.ascontiguousarray(faces)).to(dev),
                                         max_pairs, fold_deg)


if __name__ == '__main__':
    main()
