"""Numpy restatement of the rig export (include/lasr_ops.h: lasr_rig_pack / _quats / _skin / _stats), an
independent GLB reader and evaluator written from the glTF 2.0 layout the issue spells out, and the fixtures the two test files
share.  Every restated function takes the arithmetic's dtype: float64 is the reference, float32 -- the same operations in the
same order, each rounded once, as the kernels are compiled with contraction off -- gives the error a float32 evaluation is
entitled to, from which the tests take their bounds (bound()).
"""
import json
import struct

import numpy as np


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def ulp32(x):
    return float(np.spacing(np.float32(np.max(np.abs(x)))))


def bound(restated32, reference64, magnitude=None):
    """4 x the error of the float32 restatement against the float64 reference of the comparison, and at least one float32 ulp
    of the largest magnitude involved."""
    err = float(np.max(np.abs(np.asarray(restated32, np.float64) - np.asarray(reference64, np.float64)))) if np.size(reference64) else 0.
    return max(4. * err, ulp32(reference64 if magnitude is None else magnitude) if np.size(reference64) else 0.)


def ratio(kernel, restated32, reference64):
    """kernel error / float32-restatement error (DESIGN.md 4.12 records it); 0 / 0 counts as 0."""
    ref = np.asarray(reference64, np.float64)
    ek = float(np.max(np.abs(np.asarray(kernel, np.float64) - ref)))
    er = float(np.max(np.abs(np.asarray(restated32, np.float64) - ref)))
    return 0. if ek == 0 else (ek / er if er > 0 else float('inf'))


# ---- the four kernels -----------------------------------------------------------------------------------------------------
def pack(skin, k, dtype=np.float64):
    """skin [J,V] -> joints uint8 [V,k], weights [V,k], dropped [V]."""
    skin = np.asarray(skin, dtype)
    J, V = skin.shape
    joints, weights, dropped = np.zeros((V, k), np.uint8), np.zeros((V, k), dtype), np.zeros(V, dtype)
    for v in range(V):
        w = skin[:, v]
        order = sorted(range(J), key=lambda j: (-w[j], j))[:k]               # larger first, then the lower bone index
        s = dtype(0)
        for j in order:
            s = dtype(s + w[j])
        d = dtype(0)
        for j in range(J):
            if j not in order:
                d = dtype(d + w[j])
        dropped[v] = d
        if not s > 0:
            weights[v, 0] = 1
            continue
        for i, j in enumerate(order):
            q = dtype(w[j] / s)
            if q > 0:
                joints[v, i], weights[v, i] = j, q
    return joints, weights, dropped


def quats(R, dtype=np.float64):
    """R [T,K,3,3] (row vectors) -> [T,K,4]: unit (x, y, z, w) of R^T by Shepperd's method, sign-continuous along T."""
    R = np.asarray(R, dtype)
    T, K = R.shape[:2]
    out = np.zeros((T, K, 4), dtype)
    h, qr, one = dtype(0.5), dtype(0.25), dtype(1)
    for b in range(K):
        for t in range(T):
            m = R[t, b].T
            tr = (m[0, 0] + m[1, 1]) + m[2, 2]
            if tr >= m[0, 0] and tr >= m[1, 1] and tr >= m[2, 2]:
                w = h * np.sqrt(one + tr)
                f = qr / w
                x, y, z = (m[2, 1] - m[1, 2]) * f, (m[0, 2] - m[2, 0]) * f, (m[1, 0] - m[0, 1]) * f
            elif m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
                x = h * np.sqrt(((one + m[0, 0]) - m[1, 1]) - m[2, 2])
                f = qr / x
                w, y, z = (m[2, 1] - m[1, 2]) * f, (m[0, 1] + m[1, 0]) * f, (m[0, 2] + m[2, 0]) * f
            elif m[1, 1] >= m[2, 2]:
                y = h * np.sqrt(((one + m[1, 1]) - m[0, 0]) - m[2, 2])
                f = qr / y
                w, x, z = (m[0, 2] - m[2, 0]) * f, (m[0, 1] + m[1, 0]) * f, (m[1, 2] + m[2, 1]) * f
            else:
                z = h * np.sqrt(((one + m[2, 2]) - m[0, 0]) - m[1, 1])
                f = qr / z
                w, x, y = (m[1, 0] - m[0, 1]) * f, (m[0, 2] + m[2, 0]) * f, (m[1, 2] + m[2, 1]) * f
            n = np.sqrt(((x * x + y * y) + z * z) + w * w)
            q = np.array([x / n, y / n, z / n, w / n], dtype)
            if t == 0:
                flip = q[3] < 0
            else:
                p = out[t - 1, b]
                flip = (((q[0] * p[0] + q[1] * p[1]) + q[2] * p[2]) + q[3] * p[3]) < 0
            out[t, b] = -q if flip else q
    return out


def quat_matrix(q, dtype=np.float64):
    """[...,4] (x, y, z, w), as stored (no normalisation) -> [...,3,3], column convention: the standard formula."""
    q = np.asarray(q, dtype)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = dtype(1), dtype(2)
    rows = [[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
            [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
            [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]]
    return np.stack([np.stack(r, -1) for r in rows], -2).astype(dtype)


def _apply(m, t, p):
    """M [3,3], t [3], p [V,3] -> M p + t per row, ((m0 x + m1 y) + m2 z) + t."""
    return np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + t[r] for r in range(3)], 1)


def skin(rest, joints, weights, quat, trans, dtype=np.float64):
    """glTF's skinning: out[t] = M_0 (sum_i weights_i M_{joints_i + 1} [rest; 1]); joints None: M_0 [rest; 1].  -> [T,V,3]."""
    rest, quat, trans = np.asarray(rest, dtype), np.asarray(quat, dtype), np.asarray(trans, dtype)
    T, K = quat.shape[:2]
    M = quat_matrix(quat, dtype)
    out = np.zeros((T,) + rest.shape, dtype)
    for t in range(T):
        acc = rest
        if joints is not None:
            w = np.asarray(weights, dtype)
            acc = np.zeros_like(rest)
            for i in range(joints.shape[1]):
                b = joints[:, i].astype(np.int64) + 1
                per = np.zeros_like(rest)
                for bone in np.unique(b):
                    if bone < K:
                        sel = b == bone
                        per[sel] = w[sel, i, None] * _apply(M[t, bone], trans[t, bone], rest[sel])
                acc = acc + per
        out[t] = _apply(M[t, 0], trans[t, 0], acc)
    return out


def stats(posed, ref, dtype=np.float64):
    """[T,V,3] x 2 -> [T,8]: max |posed - ref|, sum |posed - ref|^2 (lane i folds vertices i, i + 256, ... in order, then the 256
    lanes fold across halves), min xyz, max xyz of posed."""
    posed, ref = np.asarray(posed, dtype), np.asarray(ref, dtype)
    T, V = posed.shape[:2]
    out = np.zeros((T, 8), dtype)
    for t in range(T):
        d = posed[t] - ref[t]
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        rows = -(-V // 256)
        pad = np.zeros(rows * 256, dtype)
        pad[:V] = dd
        lanes = np.zeros(256, dtype)
        for r in pad.reshape(rows, 256):
            lanes = lanes + r
        o = 128
        while o:
            lanes = lanes[:o] + lanes[o:2 * o]
            o //= 2
        out[t, 0] = np.sqrt(dd.max()) if V else 0
        out[t, 1] = lanes[0]
        out[t, 2:5], out[t, 5:8] = posed[t].min(0), posed[t].max(0)
    return out


def lbs_rows(rest, skin_w, R, T):
    """The convention rig.npz is written in (the reference's obj_to_cam), float64, every weight kept:
    p_cam = (sum_k w_k (p R_k + T_k)) R_0 + T_0.  rest [V,3], skin_w [J,V], R [T,K,3,3], T [T,K,3] -> [T,V,3]."""
    rest, R, T = np.asarray(rest, np.float64), np.asarray(R, np.float64), np.asarray(T, np.float64)
    out = []
    for t in range(R.shape[0]):
        p = rest
        if R.shape[1] > 1:
            w = np.asarray(skin_w, np.float64)
            p = sum(w[k - 1][:, None] * (rest @ R[t, k] + T[t, k]) for k in range(1, R.shape[1]))
        out.append(p @ R[t, 0] + T[t, 0])
    return np.stack(out)


def report(posed, ref, rest):
    """(max per frame, rms per frame, overall max, its frame, overall rms) as fractions of the rest bounding-box diagonal."""
    posed, ref, rest = (np.asarray(a, np.float64) for a in (posed, ref, rest))
    diag = np.linalg.norm(rest.max(0) - rest.min(0))
    d = np.linalg.norm(posed - ref, axis=2)
    mx = d.max(1) / diag
    return mx, np.sqrt((d ** 2).mean(1)) / diag, float(mx.max()), int(mx.argmax()), float(np.sqrt((d ** 2).mean()) / diag)


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def icosahedron():
    g = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64) / np.sqrt(1 + g * g)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], np.int32)
    return v.astype(np.float32), f


def axis_angle(axis, angle):
    """Column-convention rotation matrix (Rodrigues), float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def softmax_skin(J, V, seed):
    """Softmax over the bones of seeded float32 logits -> float32 [J,V]."""
    logits = (2 * np.random.RandomState(seed).randn(J, V)).astype(np.float32)
    e = np.exp(logits - logits.max(0))
    return (e / e.sum(0)).astype(np.float32)


def no_ties(skin_w, k):
    """True when no vertex has two equal weights among its k + 1 largest."""
    top = -np.sort(-np.asarray(skin_w), 0)[:k + 1]
    return bool((np.diff(top, axis=0) < 0).all()) if top.shape[0] > 1 else True


def rotations(T, K, seed):
    """[T,K,3,3] float32 row-vector rotations.  Bone 0 turns gently (the trace branch, with the identity at frame 0 when K > 1
    leaves room); bones 1, 2, 3 start within 1e-3 rad of a half turn about (nearly) x, y and z -- one per Shepperd branch --
    and come back 0.3 rad per frame; further bones turn at random, 0.4 rad per frame.  Consecutive keys of a bone are at most
    0.4 rad apart, so their quaternions' dot product is at least cos(0.2): the sign rule is decided."""
    rs = np.random.RandomState(seed)
    R = np.zeros((T, K, 3, 3))
    tilt = 0.05
    half = {1: (1, tilt, -tilt), 2: (-tilt, 1, tilt), 3: (tilt, -tilt, 1)}
    for b in range(K):
        axis = rs.randn(3)
        start = rs.uniform(0, 2 * np.pi)
        for t in range(T):
            if b == 0:
                M = axis_angle(axis, 0.25 * t)
            elif b in half:
                M = axis_angle(half[b], np.pi - 5e-4 - 0.3 * t)
            else:
                M = axis_angle(axis, start + 0.4 * t)
            R[t, b] = M.T
    return R.astype(np.float32)


def handmade_rig(J=3, T=4, seed=0):
    """The rig the round-trip tests write: an icosahedron (V = 12, F = 20), J part bones, T frames -> a dict in rig.npz's layout."""
    v, f = icosahedron()
    rs = np.random.RandomState(seed + 100)
    K = J + 1
    trans = (0.2 * rs.randn(T, K, 3)).astype(np.float32)
    trans[:, 0] += np.array([0.1, -0.2, 5.], np.float32)                    # the body sits in front of the camera
    return dict(rest_verts=v, faces=f, colors=rs.uniform(0, 1, (12, 3)).astype(np.float32),
                skin=softmax_skin(J, 12, seed) if J else np.zeros((0, 12), np.float32), frame_ids=np.arange(T, dtype=np.int64) + 3,
                R=rotations(T, K, seed), T=trans, intrinsics=np.tile(np.float32([60, 60, 32, 32]), (T, 1)))


def restated_arrays(npz, k, dtype=np.float32):
    """pack, quats and skin of the restatement on a rig -> the arrays lasr_amd.ext_utils.gltf.build_gltf takes, plus 'posed'."""
    K = npz['R'].shape[1]
    joints = weights = None
    if K > 1:
        joints, weights, _ = pack(npz['skin'], k, dtype)
    q = quats(npz['R'], dtype)
    posed = skin(npz['rest_verts'], joints, weights, q, npz['T'], dtype)
    return dict(positions=npz['rest_verts'], indices=npz['faces'], colors=npz['colors'], joints=joints, weights=weights, quat=q,
                trans=np.asarray(npz['T'], dtype)), posed


# ---- an independent GLB reader -----------------------------------------------------------------------------------------------
COMPONENTS = {5121: ('B', 1), 5123: ('H', 2), 5125: ('I', 4), 5126: ('f', 4)}
WIDTHS = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT4': 16}


def read_glb(blob):
    """-> (gltf dict, binary chunk); asserts the container rules: magic, version, declared lengths against the file size, chunk
    types, 4-byte chunk lengths, space / zero padding."""
    assert len(blob) >= 20 and len(blob) % 4 == 0
    magic, version, total = struct.unpack_from('<III', blob, 0)
    assert magic == 0x46546C67 and version == 2 and total == len(blob)
    n0, t0 = struct.unpack_from('<II', blob, 12)
    assert t0 == 0x4E4F534A and n0 % 4 == 0 and 20 + n0 <= total
    js = blob[20:20 + n0]
    assert js.rstrip(b' ').endswith(b'}') and b'\0' not in js                # padded with spaces only
    n1, t1 = struct.unpack_from('<II', blob, 20 + n0)
    assert t1 == 0x004E4942 and n1 % 4 == 0 and 28 + n0 + n1 == total
    binary = blob[28 + n0:]
    gltf = json.loads(js.decode('utf-8'))
    assert gltf['asset']['version'] == '2.0' and len(gltf['buffers']) == 1
    declared = gltf['buffers'][0]['byteLength']
    assert declared <= n1 < declared + 4 and not any(binary[declared:])      # padded with zeros only
    return gltf, binary


def read_accessor(gltf, binary, index):
    """-> numpy array [count, width] (float64 for floats, int64 otherwise); asserts bounds and alignment."""
    a = gltf['accessors'][index]
    view = gltf['bufferViews'][a['bufferView']]
    code, size = COMPONENTS[a['componentType']]
    width = WIDTHS[a['type']]
    start = view.get('byteOffset', 0) + a.get('byteOffset', 0)
    assert 'byteStride' not in view
    assert start % size == 0 and a.get('byteOffset', 0) % size == 0          # offsets are multiples of the component size
    assert a['count'] * width * size + a.get('byteOffset', 0) <= view['byteLength']
    assert view.get('byteOffset', 0) + view['byteLength'] <= gltf['buffers'][0]['byteLength']
    flat = struct.unpack_from('<%d%s' % (a['count'] * width, code), binary, start)
    return np.asarray(flat, np.float64 if code == 'f' else np.int64).reshape(a['count'], width)


def _trs_matrix(node):
    m = np.eye(4)
    x, y, z, w = node.get('rotation', [0, 0, 0, 1])
    m[:3, :3] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]) * np.asarray(node.get('scale', [1, 1, 1]))
    m[:3, 3] = node.get('translation', [0, 0, 0])
    return m


def _globals(nodes, roots):
    out = {}

    def walk(i, parent):
        assert i not in out                                                   # a node has one parent
        out[i] = parent @ _trs_matrix(nodes[i])
        for c in nodes[i].get('children', []):
            walk(c, out[i])
    for r in roots:
        walk(r, np.eye(4))
    return out


def check_rules(gltf, binary):
    """The writer's rules that concern the file as a whole (the numeric ones are checked where the arrays are read)."""
    views = gltf['bufferViews']
    spans = sorted((v.get('byteOffset', 0), v.get('byteOffset', 0) + v['byteLength']) for v in views)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))               # no overlap
    prim = gltf['meshes'][0]['primitives'][0]
    attr_views = {gltf['accessors'][i]['bufferView'] for i in prim['attributes'].values()}
    index_view = gltf['accessors'][prim['indices']]['bufferView']
    untargeted = set(range(len(views))) - attr_views - {index_view}
    for i in attr_views:
        assert views[i]['target'] == 34962 and views[i].get('byteOffset', 0) % 4 == 0
    assert views[index_view]['target'] == 34963
    assert all('target' not in views[i] for i in untargeted)                 # inverse binds, animation data, images
    for name, i in prim['attributes'].items():
        a = gltf['accessors'][i]
        assert (COMPONENTS[a['componentType']][1] * WIDTHS[a['type']]) % 4 == 0, name     # vertex elements are 4-byte aligned
    assert prim['mode'] == 4 and gltf['materials'][prim['material']]['doubleSided'] is True
    pbr = gltf['materials'][prim['material']]['pbrMetallicRoughness']
    assert pbr['metallicFactor'] == 0 and pbr['roughnessFactor'] == 1
    pos = gltf['accessors'][prim['attributes']['POSITION']]
    got = read_accessor(gltf, binary, prim['attributes']['POSITION'])
    assert pos['min'] == list(got.min(0)) and pos['max'] == list(got.max(0))
    for n in gltf['nodes']:
        assert 'matrix' not in n                                              # TRS nodes only
    scene = gltf['scenes'][gltf['scene']]['nodes']
    mesh_nodes = [i for i, n in enumerate(gltf['nodes']) if 'mesh' in n]
    assert len(mesh_nodes) == 1
    if 'skin' in gltf['nodes'][mesh_nodes[0]]:
        assert mesh_nodes[0] in scene                                         # a skinned mesh sits at the scene root


def evaluate(gltf, binary):
    """The vertices of every keyframe as a viewer computes them, float64 -> (positions [T,N,3] with the flip undone, times [T]).
    Also asserts the rules on animation inputs, rotations, weights and joints."""
    nodes = [dict(n) for n in gltf['nodes']]
    prim = gltf['meshes'][0]['primitives'][0]
    p = read_accessor(gltf, binary, prim['attributes']['POSITION'])
    ph = np.concatenate([p, np.ones((len(p), 1))], 1)
    anim = gltf['animations'][0]
    inputs = {s['input'] for s in anim['samplers']}
    assert len(inputs) == 1
    ia = gltf['accessors'][inputs.pop()]
    times = read_accessor(gltf, binary, gltf['accessors'].index(ia))[:, 0]
    assert ia['componentType'] == 5126 and ia['type'] == 'SCALAR' and (np.diff(times) > 0).all()
    assert ia['min'] == [times.min()] and ia['max'] == [times.max()]
    mesh_node = [i for i, n in enumerate(nodes) if 'mesh' in n][0]
    sets = len([a for a in prim['attributes'] if a.startswith('JOINTS_')])
    if sets:
        J = np.concatenate([read_accessor(gltf, binary, prim['attributes']['JOINTS_%d' % s]) for s in range(sets)], 1)
        W = np.concatenate([read_accessor(gltf, binary, prim['attributes']['WEIGHTS_%d' % s]) for s in range(sets)], 1)
        assert (W >= 0).all()
        nz = (W > 0).sum(1)
        w32 = W.astype(np.float32)
        assert (np.abs(w32.astype(np.float64).sum(1) - 1) <= 2e-7 * nz).all()
        assert (J[W == 0] == 0).all()                                         # a zero weight carries joint 0
        for row_j, row_w in zip(J, W):
            used = row_j[row_w > 0]
            assert len(set(used.tolist())) == len(used)                       # no joint twice with a non-zero weight
        skin = gltf['skins'][nodes[mesh_node]['skin']]
        assert J.max() < len(skin['joints'])
        ibm = read_accessor(gltf, binary, skin['inverseBindMatrices']).reshape(-1, 4, 4).transpose(0, 2, 1)   # column major
        assert len(ibm) == len(skin['joints'])
    out = []
    for i in range(len(times)):
        for ch in anim['channels']:
            s = anim['samplers'][ch['sampler']]
            assert s['interpolation'] == 'LINEAR' and ch['target']['path'] in ('translation', 'rotation')
            keys = read_accessor(gltf, binary, s['output'])
            assert len(keys) == len(times)
            if ch['target']['path'] == 'rotation':
                n32 = np.linalg.norm(keys, axis=1)
                assert np.abs(n32 - 1).max() <= 4 * 2. ** -24                 # unit, to float32 rounding of four components
            nodes[ch['target']['node']][ch['target']['path']] = list(keys[i])
        if i == 0:                                                            # the rest pose of every node is key 0
            for a, b in zip(nodes, gltf['nodes']):
                assert a.get('rotation') == b.get('rotation') and a.get('translation') == b.get('translation')
        g = _globals(nodes, gltf['scenes'][gltf['scene']]['nodes'])
        if sets:
            jm = np.stack([g[j] @ ibm[n] for n, j in enumerate(skin['joints'])])
            v = np.zeros_like(ph)
            for c in range(J.shape[1]):
                v += W[:, c, None] * np.einsum('nij,nj->ni', jm[J[:, c]], ph)
        else:
            v = ph @ g[mesh_node].T
        out.append(v[:, :3] * np.array([1., -1., -1.]))                      # undo the half turn about x
    return np.stack(out), times
