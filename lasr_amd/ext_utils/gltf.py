"""A minimal glTF 2.0 binary (.glb) writer for one skinned, animated mesh (scripts/export_gltf.py).
Pure Python (struct, json) over numpy arrays: no dependency, no device.

The scene: node `flip` (a static half turn about x, taking OpenCV camera axes to glTF's +Y up, -Z forward) -> node `root`
(animated with the body's rotation and translation) -> one joint node per part bone (animated alike).  With part bones the mesh
node sits at the scene root and carries the skin (a skinned mesh's own transform is ignored); its inverse bind matrices are
identity, so a vertex is flip . M_0 . sum_i w_i M_{j_i} [p; 1].  Without part bones the mesh node is a child of `root` and there
is no skin.  Every accessor has a buffer view of its own, 4-byte aligned.
"""
import json
import struct

import numpy as np

GLB_MAGIC, JSON_CHUNK, BIN_CHUNK = 0x46546C67, 0x4E4F534A, 0x004E4942
U8, U32, F32 = 5121, 5125, 5126
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
_DTYPES = {U8: np.uint8, U32: np.uint32, F32: np.float32}
_WIDTH = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT4': 16}
FLIP_QUAT = (1., 0., 0., 0.)                                 # (x, y, z, w): 180 degrees about x


class _Buffer:
    """The binary chunk under construction and the bufferViews / accessors that index it."""

    def __init__(self):
        self.data, self.views, self.accessors = bytearray(), [], []

    def view(self, raw, target=None):
        self.data += b'\0' * (-len(self.data) % 4)
        v = {'buffer': 0, 'byteOffset': len(self.data), 'byteLength': len(raw)}
        if target is not None:
            v['target'] = target
        self.data += raw
        self.views.append(v)
        return len(self.views) - 1

    def accessor(self, array, component, kind, target=None, minmax=False):
        a = np.ascontiguousarray(np.asarray(array).reshape(-1, _WIDTH[kind]), dtype=np.dtype(_DTYPES[component]).newbyteorder('<'))
        acc = {'bufferView': self.view(a.tobytes(), target), 'byteOffset': 0, 'componentType': component, 'count': int(a.shape[0]),
               'type': kind}
        if minmax:                                         # of the values as stored: float32 widens to a JSON double exactly
            acc['min'], acc['max'] = [float(x) for x in a.min(0)], [float(x) for x in a.max(0)]
        self.accessors.append(acc)
        return len(self.accessors) - 1


def build_gltf(positions, indices, quat, trans, joints=None, weights=None, colors=None, uv=None, png=None, fps=10.):
    """-> (gltf dict, binary chunk bytes).  positions [N,3]; indices [F,3]; quat [T,K,4] unit (x, y, z, w) and trans [T,K,3]:
    column-convention keys, bone 0 the body; joints uint8 [N,k] / weights [N,k] with k 4 or 8 when K > 1; colors [N,3] (0-1) for
    COLOR_0, or uv [N,2] (already flipped to glTF's top-left origin) with the bytes of a PNG for TEXCOORD_0 and a base colour
    texture.  Key i is at i / fps seconds; the rest pose of every node is key 0."""
    positions = np.asarray(positions, np.float32)
    quat, trans = np.asarray(quat, np.float32), np.asarray(trans, np.float32)
    N = positions.shape[0]
    if quat.ndim != 3 or quat.shape[2] != 4 or quat.shape[0] < 1 or quat.shape[1] < 1 or trans.shape != quat.shape[:2] + (3,):
        raise ValueError('gltf: quat must be [T >= 1, K >= 1, 4] and trans [T, K, 3], got %s and %s' % (quat.shape, trans.shape))
    T, K = quat.shape[:2]
    if not fps > 0:
        raise ValueError('gltf: fps must be positive, got %r' % (fps,))
    if (uv is None) != (png is None) or (uv is None) == (colors is None):
        raise ValueError('gltf: pass either colors, or uv together with png')
    if K > 1:
        if joints is None or weights is None:
            raise ValueError('gltf: %d bones need joints and weights' % K)
        joints, weights = np.asarray(joints), np.asarray(weights, np.float32)
        if joints.shape != weights.shape or joints.shape[0] != N or joints.ndim != 2 or joints.shape[1] not in (4, 8):
            raise ValueError('gltf: joints and weights must be [N = %d, 4 or 8], got %s and %s' % (N, joints.shape, weights.shape))
        if joints.max(initial=0) >= K - 1:
            raise ValueError('gltf: a joint index exceeds the %d joints' % (K - 1))
    buf = _Buffer()
    attributes = {'POSITION': buf.accessor(positions, F32, 'VEC3', ARRAY_BUFFER, minmax=True)}
    if colors is not None:
        attributes['COLOR_0'] = buf.accessor(np.asarray(colors, np.float32), F32, 'VEC3', ARRAY_BUFFER)
    else:
        attributes['TEXCOORD_0'] = buf.accessor(np.asarray(uv, np.float32), F32, 'VEC2', ARRAY_BUFFER)
    if K > 1:
        for s in range(joints.shape[1] // 4):
            attributes['JOINTS_%d' % s] = buf.accessor(joints[:, 4 * s:4 * s + 4], U8, 'VEC4', ARRAY_BUFFER)
            attributes['WEIGHTS_%d' % s] = buf.accessor(weights[:, 4 * s:4 * s + 4], F32, 'VEC4', ARRAY_BUFFER)
    primitive = {'attributes': attributes, 'indices': buf.accessor(np.asarray(indices).reshape(-1), U32, 'SCALAR', ELEMENT_ARRAY_BUFFER),
                 'material': 0, 'mode': 4}
    material = {'pbrMetallicRoughness': {'metallicFactor': 0, 'roughnessFactor': 1}, 'doubleSided': True}
    gltf = {'asset': {'version': '2.0', 'generator': 'lasr_amd'}, 'scene': 0}

    def trs(name, k):
        return {'name': name, 'rotation': [float(x) for x in quat[0, k]], 'translation': [float(x) for x in trans[0, k]]}
    # nodes: 0 flip, 1 root, 2 .. K joints, K + 1 the mesh
    nodes = [{'name': 'flip', 'rotation': list(FLIP_QUAT), 'children': [1]}, trs('root', 0)]
    nodes += [trs('bone%d' % k, k) for k in range(1, K)]
    mesh_node = {'name': 'mesh', 'mesh': 0}
    if K > 1:
        nodes[1]['children'] = list(range(2, K + 1))
        mesh_node['skin'] = 0
        eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (K - 1, 1))     # column major; the identity either way
        gltf['skins'] = [{'joints': list(range(2, K + 1)), 'inverseBindMatrices': buf.accessor(eye, F32, 'MAT4'), 'skeleton': 1}]
        gltf['scenes'] = [{'nodes': [0, K + 1]}]
    else:
        nodes[1]['children'] = [K + 1]
        gltf['scenes'] = [{'nodes': [0]}]
    nodes.append(mesh_node)
    gltf['nodes'] = nodes
    gltf['meshes'] = [{'primitives': [primitive]}]

    times = buf.accessor(np.arange(T, dtype=np.float64) / fps, F32, 'SCALAR', minmax=True)
    samplers, channels = [], []
    for k in range(K):
        for path, keys, kind in (('translation', trans[:, k], 'VEC3'), ('rotation', quat[:, k], 'VEC4')):
            samplers.append({'input': times, 'output': buf.accessor(keys, F32, kind), 'interpolation': 'LINEAR'})
            channels.append({'sampler': len(samplers) - 1, 'target': {'node': 1 + k, 'path': path}})
    gltf['animations'] = [{'name': 'sequence', 'samplers': samplers, 'channels': channels}]
    if png is not None:
        material['pbrMetallicRoughness']['baseColorTexture'] = {'index': 0}
        gltf['textures'] = [{'sampler': 0, 'source': 0}]
        gltf['images'] = [{'bufferView': buf.view(bytes(png)), 'mimeType': 'image/png'}]
        gltf['samplers'] = [{'magFilter': 9729, 'minFilter': 9729, 'wrapS': 33071, 'wrapT': 33071}]
    gltf['materials'] = [material]
    buf.data += b'\0' * (-len(buf.data) % 4)
    gltf['buffers'] = [{'byteLength': len(buf.data)}]
    gltf['bufferViews'], gltf['accessors'] = buf.views, buf.accessors
    return gltf, bytes(buf.data)


def pack_glb(gltf, binary):
    """The GLB container: 12-byte header, the JSON chunk padded with spaces, the binary chunk padded with zeros."""
    js = json.dumps(gltf, separators=(',', ':')).encode('utf-8')
    js += b' ' * (-len(js) % 4)
    binary = bytes(binary) + b'\0' * (-len(binary) % 4)
    total = 12 + 8 + len(js) + 8 + len(binary)
    return b''.join([struct.pack('<III', GLB_MAGIC, 2, total), struct.pack('<II', len(js), JSON_CHUNK), js,
                     struct.pack('<II', len(binary), BIN_CHUNK), binary])


def write_glb(path, **arrays):
    """build_gltf(**arrays) packed into `path`; -> the number of bytes written."""
    blob = pack_glb(*build_gltf(**arrays))
    with open(path, 'wb') as f:
        f.write(blob)
    return len(blob)
