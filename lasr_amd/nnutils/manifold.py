"""Watertight re-meshing on the GPU (csrc/manifold.hip), in place of the external Manifold binary the reference runs as
`manifold in.obj out.obj 10000` (reference: scripts/eval_mesh.py:100-105, render_vis.py:98, nnutils/train_utils.py:422).

The input is voxelised (lasr_voxelize: surface voxels plus enclosed voxels), the solid is made well-composed, its boundary is
extracted as lattice quads -- a closed 2-manifold, since the boundary of a well-composed set is one (Latecki) -- and every vertex
moves to its closest point on the input.  DESIGN.md section 4.6 states the construction and its costs.
"""
import warnings

import torch

from .. import _lib

MIN_SIZE, MAX_SIZE = 16, 256     # the grids watertight() chooses from (the ABI takes LASR_MANIFOLD_MIN_SIZE = 4 and up)
MARGIN = 3                       # empty voxel layers around the input's bounding cube
MIN_AREA = 1e-4                  # the guard's area bound, in units of h^2


def _ws(S, device):
    n = int(_lib.lib().lasr_manifold_workspace_bytes(S))
    if n == 0:
        raise ValueError('grid size %d outside [4, %d]' % (S, MAX_SIZE))
    return torch.empty(n, dtype=torch.uint8, device=device)


def repair(voxels, ws=None):
    """voxels [S,S,S] int32 on the GPU, rewritten in place: well-composed repair, then the refill.  -> info int32 [2] on the
    device: (sweeps of the repair, or -1 if the solid reaches the grid's outer layer; sweeps of the fill)."""
    S = voxels.shape[0]
    ws = _ws(S, voxels.device) if ws is None else ws
    info = torch.zeros(2, dtype=torch.int32, device=voxels.device)
    _lib.call('lasr_manifold_repair', voxels, info, ws, ws.numel(), S)
    return info


def count(voxels, ws):
    """-> counts int32 [3] on the device: (solid voxels with an empty 6-neighbour, boundary vertices, boundary triangles).
    Leaves in ws what extract() needs."""
    counts = torch.zeros(3, dtype=torch.int32, device=voxels.device)
    _lib.call('lasr_manifold_count', voxels, counts, ws, ws.numel(), voxels.shape[0])
    return counts


def extract(voxels, ws, V, F):
    """The boundary of the solid after count(voxels, ws) gave (V, F): verts [V,3] float32 lattice coordinates, faces [F,3] int64,
    in the orders of include/lasr_ops.h (vertices by lattice index, triangles by voxel index then direction)."""
    verts = torch.empty(V, 3, dtype=torch.float32, device=voxels.device)
    faces = torch.empty(F, 3, dtype=torch.int64, device=voxels.device)
    _lib.call('lasr_manifold_extract', voxels, verts, faces, V, F, ws, ws.numel(), voxels.shape[0])
    return verts, faces


def boundary(voxels, ws=None):
    """repair + count + extract of a solid [S,S,S] int32 (rewritten in place) -> (verts, faces, info as a host list)."""
    ws = _ws(voxels.shape[0], voxels.device) if ws is None else ws
    info = repair(voxels, ws)
    counts = count(voxels, ws)
    host = torch.cat([info, counts]).tolist()                 # the one readback: sizes of the outputs
    if host[0] < 0:
        raise ValueError('the solid reaches the outer voxel layer of the grid')
    verts, faces = extract(voxels, ws, host[3], host[4])
    return verts, faces, host


def project(lattice, in_verts, in_faces):
    """lattice [V,3], in_verts [Vin,3], in_faces [Fin,3] int64, one unit = one voxel -> every lattice point moved to its closest
    point on the input (closest face by lasr_point_mesh_forward)."""
    dev = lattice.device
    V, Vin, Fin = lattice.shape[0], in_verts.shape[0], in_faces.shape[0]
    out = torch.empty_like(lattice)
    if V == 0:
        return out
    dp, df = torch.empty(1, V, device=dev), torch.empty(1, Fin, device=dev)
    ap = torch.empty(1, V, dtype=torch.int32, device=dev)
    af = torch.empty(1, Fin, dtype=torch.int32, device=dev)
    scratch = torch.empty(_lib.lib().lasr_point_mesh_scratch_floats(1, Fin, V), dtype=torch.float32, device=dev)
    _lib.call('lasr_point_mesh_forward', in_verts, in_faces, lattice, dp, ap, df, af, scratch, 1, Vin, Fin, V)
    _lib.call('lasr_manifold_project', lattice, in_verts, in_faces, ap, out, V, Vin, Fin)
    return out


def guard(lattice, verts, faces, min_area=MIN_AREA):
    """Moves back to the lattice, in rounds, every vertex of a face whose normal turned against its lattice normal or whose area
    fell below min_area (lattice units).  verts is changed in place.  -> rounds int32 [1] on the device."""
    rounds = torch.zeros(1, dtype=torch.int32, device=verts.device)
    flags = torch.empty(max(verts.shape[0], 1), dtype=torch.int32, device=verts.device)
    _lib.call('lasr_manifold_guard', lattice, verts, faces, flags, rounds, verts.shape[0], faces.shape[0], float(min_area))
    return rounds


def _check_input(verts, faces, resolution):
    if not isinstance(verts, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise TypeError('verts and faces must be tensors')
    _lib.need_cuda(verts, faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('verts must be [V,3] and faces [F,3], got %s and %s' % (tuple(verts.shape), tuple(faces.shape)))
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError('watertight() needs a non-empty mesh')
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise TypeError('faces must be an integer tensor')
    if resolution <= 0:
        raise ValueError('resolution must be positive, got %r' % (resolution,))
    if not bool(torch.isfinite(verts).all()):
        raise ValueError('verts holds non-finite values')
    if int(faces.min()) < 0 or int(faces.max()) >= verts.shape[0]:
        raise ValueError('faces index past the %d vertices' % verts.shape[0])


def remesh(verts, faces, resolution=10000):
    """watertight() with the intermediate results: a dict of verts, faces (input units), lattice (lattice units), moved (the
    projected vertices, lattice units), S, h, origin (input position of lattice point 0), repair / fill sweeps, guard rounds,
    surface_voxels (of the solid before the repair)."""
    _check_input(verts, faces, resolution)
    v = verts.detach().float().contiguous()
    f = faces.detach().long().contiguous()
    lo, hi = v.min(0).values, v.max(0).values
    L = float((hi - lo).max())
    if not L > 0:
        raise ValueError('the input is a single point')
    centre = (lo + hi) * 0.5
    from ..soft_renderer.functional.voxelization import voxelization
    S = MIN_SIZE
    while True:
        # the bounding cube spans lattice [MARGIN, S - 1 - MARGIN]: voxels MARGIN .. S-1-MARGIN, MARGIN empty layers either side
        h = L / (S - 1 - 2 * MARGIN)
        origin = centre - 0.5 * L - MARGIN * h
        vin = ((v - origin) / h).contiguous()
        voxels = voxelization(vin[f][None], S, normalize=True)[0]
        ws = _ws(S, v.device)
        nsurf = int(count(voxels, ws)[0])
        if nsurf >= resolution or S == MAX_SIZE:
            break
        S *= 2
    if nsurf < resolution:
        warnings.warn('watertight: %d surface voxels at the largest grid (S = %d), fewer than the resolution %d'
                      % (nsurf, S, resolution))
    lattice, tri, host = boundary(voxels, ws)
    moved = project(lattice, vin, f)
    rounds = guard(lattice, moved, tri)
    out = (moved.double() * h + origin.double()).float()
    return dict(verts=out, faces=tri, lattice=lattice, moved=moved, S=S, h=h, origin=origin, repair_sweeps=host[0],
                fill_sweeps=host[1], rounds=int(rounds), surface_voxels=nsurf, voxels=voxels)


def watertight(verts, faces, resolution=10000):
    """verts [V,3] float32 and faces [F,3] integer on the GPU -> (verts [V',3] float32, faces [F',3] int64) on the same device:
    a closed, consistently oriented 2-manifold near the input, from which it can be far apart only where the input is open or
    thin.  Raises ValueError for an empty or non-finite input and a non-positive resolution.

    Pipeline: the input's bounding cube goes into an S^3 grid with 3 empty layers around it; lasr_voxelize gives the solid
    (surface voxels and enclosed voxels); the well-composed repair and the refill (lasr_manifold_repair); one quad per solid voxel
    face with an empty 6-neighbour, two triangles each (lasr_manifold_count / _extract); each vertex to its closest point on
    the input (lasr_point_mesh_forward + lasr_manifold_project); the reverting guard (lasr_manifold_guard).

    Departures from Manifold:
    - a dense grid instead of an octree: S is the smallest power of two in [16, 256] at which the solid has at least
      `resolution` voxels with an empty 6-neighbour (Manifold splits its octree until `resolution` leaf cells touch the
      surface); a warning if even S = 256 falls short;
    - the solid is made well-composed (critical 2x2 squares and antipodal 2x2x2 blocks filled in) instead of splitting the
      non-manifold vertices and edges of the voxel boundary;
    - instead of Manifold's iterative projection, a guard moves back to the lattice every vertex of a face whose normal turned
      against its lattice normal or whose area fell below 1e-4 h^2 (h: the voxel edge), until no face is flagged;
    - on thin or open inputs both sides of the voxel slab can project onto the same sheet: the output is closed and manifold,
      but may touch itself there.
    """
    r = remesh(verts, faces, resolution)
    return r['verts'], r['faces']
