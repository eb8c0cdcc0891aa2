"""ASCII .ply meshes in the layout of the reference's fusion.meshwrite (third_party/ext_utils/fusion.py:25-60): x y z nx ny nz as
float, red green blue as uchar, a triangle list.  extract.py writes pred<i>.ply / gauss<i>.ply with it, render_vis.py reads them."""
import numpy as np


def write_ply(filename, verts, faces, norms=None, colors=None):
    """verts [V,3], faces [F,3], norms [V,3] (default 0), colors [V,3] in 0-255 (default 1, as fusion.meshwrite)."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    norms = np.zeros(verts.shape) if norms is None else np.asarray(norms, np.float64).reshape(-1, 3)
    colors = np.ones(verts.shape) if colors is None else np.asarray(colors, np.float64).reshape(-1, 3)
    lines = ['ply', 'format ascii 1.0', 'element vertex %d' % verts.shape[0],
             'property float x', 'property float y', 'property float z',
             'property float nx', 'property float ny', 'property float nz',
             'property uchar red', 'property uchar green', 'property uchar blue',
             'element face %d' % faces.shape[0], 'property list uchar int vertex_index', 'end_header']
    lines += ['%f %f %f %f %f %f %d %d %d' % (tuple(v) + tuple(n) + tuple(int(c) for c in col))
              for v, n, col in zip(verts, norms, colors)]
    lines += ['3 %d %d %d' % tuple(f) for f in faces]
    with open(filename, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


def read_ply(filename):
    """-> dict(verts float [V,3], faces int64 [F,3], colors uint8 [V,3] or None, normals [V,3] or None).  ASCII files with one
    vertex and one face element (any vertex properties; polygons are fanned into triangles)."""
    with open(filename) as fh:
        if fh.readline().strip() != 'ply':
            raise ValueError('%s: not a .ply file' % filename)
        elems, props = [], {}
        for line in fh:
            tok = line.split()
            if not tok or tok[0] in ('comment', 'obj_info'):
                continue
            if tok[0] == 'format' and tok[1] != 'ascii':
                raise ValueError('%s: only ASCII .ply is read (found %s)' % (filename, tok[1]))
            if tok[0] == 'element':
                elems.append((tok[1], int(tok[2])))
                props[tok[1]] = []
            elif tok[0] == 'property':
                props[elems[-1][0]].append(tok[-1])
            elif tok[0] == 'end_header':
                break
        body = fh.read().split('\n')
    rows, k = {}, 0
    for name, count in elems:
        rows[name] = [r.split() for r in body[k:k + count]]
        k += count
    vp = props.get('vertex', [])
    vals = np.asarray(rows.get('vertex', []), np.float64).reshape(-1, len(vp))
    col = lambda names: vals[:, [vp.index(n) for n in names]] if all(n in vp for n in names) else None
    verts = col(['x', 'y', 'z'])
    rgb = col(['red', 'green', 'blue'])
    tris = []
    for r in rows.get('face', []):
        idx = [int(t) for t in r[1:1 + int(r[0])]]
        tris += [[idx[0], idx[i], idx[i + 1]] for i in range(1, len(idx) - 1)]
    return dict(verts=verts, faces=np.asarray(tris, np.int64).reshape(-1, 3),
                colors=None if rgb is None else rgb.astype(np.uint8), normals=col(['nx', 'ny', 'nz']))
