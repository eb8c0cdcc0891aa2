"""Rigged glTF export without a device: the writer (lasr_amd/ext_utils/gltf.py) against the independent reader of
tests/rig_restated.py on hand-made rigs, the C ABI's host-side checks, what the Python layer refuses, and the script's arguments."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

import rig_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gltf():
    from lasr_amd.ext_utils import gltf
    return gltf


def _script():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import export_gltf
    return export_gltf


def _png(pixels):
    """A minimal 8-bit RGB PNG of pixels [H,W,3] uint8."""
    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))
    h, w = pixels.shape[:2]
    raw = b''.join(b'\0' + pixels[r].tobytes() for r in range(h))
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw)) \
        + chunk(b'IEND', b'')


def _round_trip(tmp_path, npz, k, **extra):
    arrays, posed32 = rr.restated_arrays(npz, k, np.float32)
    path = str(tmp_path / 'rig.glb')
    n = _gltf().write_glb(path, fps=10., **dict(arrays, **extra))
    blob = open(path, 'rb').read()
    assert n == len(blob)
    gltf, binary = rr.read_glb(blob)
    rr.check_rules(gltf, binary)
    got, times = rr.evaluate(gltf, binary)
    return gltf, binary, got, times, arrays, posed32


def test_fixture_has_one_rotation_per_shepperd_branch_near_a_half_turn():
    npz = rr.handmade_rig()
    assert npz['rest_verts'].shape == (12, 3) and npz['faces'].shape == (20, 3) and npz['skin'].shape == (3, 12) and npz['R'].shape == (4, 4, 3, 3)
    R0 = npz['R'][0].astype(np.float64)
    angle = np.arccos(np.clip((np.trace(R0, axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert (np.abs(angle[1:] - np.pi) < 1e-3).all()
    assert [int(np.argmax(np.diag(R0[b]))) for b in (1, 2, 3)] == [0, 1, 2]   # the x, y and z branch
    assert np.trace(R0[0]) >= np.diag(R0[0]).max()                           # the body: the trace branch
    q = rr.quats(npz['R'])
    assert np.abs(rr.quat_matrix(q) - npz['R'].transpose(0, 1, 3, 2)).max() < 1e-6      # float32 inputs are orthogonal to ~1e-7
    assert (q[0, :, 3] >= 0).all() and ((q[1:] * q[:-1]).sum(-1) > 0.1).all()


def test_round_trip_with_every_weight_kept_equals_the_row_vector_formula(tmp_path):
    npz = rr.handmade_rig(J=3, T=4)
    assert rr.no_ties(npz['skin'], 4)
    gltf, binary, got, times, arrays, posed32 = _round_trip(tmp_path, npz, 4)
    want = rr.lbs_rows(npz['rest_verts'], npz['skin'], npz['R'], npz['T'])   # all weights: k = 4 > J = 3
    tol = rr.bound(posed32, want)
    err = np.abs(got - want).max()
    print('round trip: error %.3g, bound %.3g' % (err, tol))
    assert got.shape == (4, 12, 3) and err <= tol
    assert np.array_equal(times, (np.arange(4) / 10.).astype(np.float32).astype(np.float64))     # i / fps, stored as float32
    # layout of the scene: flip -> root -> three joints; the skinned mesh beside flip at the scene root; identity inverse binds
    nodes = gltf['nodes']
    assert nodes[0]['rotation'] == [1, 0, 0, 0] and nodes[0]['children'] == [1] and nodes[1]['children'] == [2, 3, 4]
    assert gltf['scenes'][0]['nodes'] == [0, 5] and nodes[5] == {'name': 'mesh', 'mesh': 0, 'skin': 0}
    skin = gltf['skins'][0]
    assert skin['joints'] == [2, 3, 4] and skin['skeleton'] == 1
    assert (rr.read_accessor(gltf, binary, skin['inverseBindMatrices']) == np.eye(4).reshape(16)).all()
    prim = gltf['meshes'][0]['primitives'][0]
    assert sorted(prim['attributes']) == ['COLOR_0', 'JOINTS_0', 'POSITION', 'WEIGHTS_0']
    assert (rr.read_accessor(gltf, binary, prim['indices']).reshape(-1, 3) == npz['faces']).all()
    assert np.array_equal(rr.read_accessor(gltf, binary, prim['attributes']['COLOR_0']), npz['colors'].astype(np.float64))
    assert gltf['accessors'][prim['attributes']['JOINTS_0']]['componentType'] == 5121
    assert len(gltf['animations'][0]['channels']) == 8 and {c['target']['node'] for c in gltf['animations'][0]['channels']} == {1, 2, 3, 4}
    assert 'textures' not in gltf and 'images' not in gltf


def test_round_trip_with_eight_influences_and_truncation(tmp_path):
    npz = rr.handmade_rig(J=6, T=3, seed=1)
    assert rr.no_ties(npz['skin'], 4) and rr.no_ties(npz['skin'], 8)
    full = rr.lbs_rows(npz['rest_verts'], npz['skin'], npz['R'], npz['T'])
    gltf, binary, got, _, arrays, posed32 = _round_trip(tmp_path, npz, 8)
    prim = gltf['meshes'][0]['primitives'][0]
    assert {'JOINTS_1', 'WEIGHTS_1'} <= set(prim['attributes'])
    assert np.abs(got - full).max() <= rr.bound(posed32, full)
    # four influences of six bones: the file evaluates to the float64 restatement of the truncated rig, not to the full blend
    gltf, binary, got, _, arrays, posed32 = _round_trip(tmp_path, npz, 4)
    j64, w64, dropped = rr.pack(npz['skin'], 4)
    want = rr.skin(npz['rest_verts'], j64, w64, rr.quats(npz['R']), npz['T'])
    assert (arrays['joints'] == j64).all() and dropped.max() > 1e-3
    assert np.abs(got - want).max() <= rr.bound(posed32, want)
    assert np.abs(got - full).max() > 100 * rr.bound(posed32, want)


def test_round_trip_of_the_body_alone_has_no_skin(tmp_path):
    npz = rr.handmade_rig(J=0, T=4)
    gltf, binary, got, _, arrays, posed32 = _round_trip(tmp_path, npz, 4)
    want = rr.lbs_rows(npz['rest_verts'], npz['skin'], npz['R'], npz['T'])
    assert np.abs(got - want).max() <= rr.bound(posed32, want)
    assert 'skins' not in gltf and gltf['scenes'][0]['nodes'] == [0]
    assert gltf['nodes'][1]['children'] == [2] and gltf['nodes'][2] == {'name': 'mesh', 'mesh': 0}
    assert sorted(gltf['meshes'][0]['primitives'][0]['attributes']) == ['COLOR_0', 'POSITION']
    assert len(gltf['animations'][0]['channels']) == 2


def test_texture_obj_splits_the_corners_flips_v_and_embeds_the_png_unchanged(tmp_path):
    eg = _script()
    npz = rr.handmade_rig(J=3, T=2)
    npz['rest_verts'], npz['faces'] = npz['rest_verts'][:4], np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    npz['colors'], npz['skin'] = npz['colors'][:4], npz['skin'][:, :4]
    png = _png(np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]], np.uint8))
    (tmp_path / 'baked.png').write_bytes(png)
    (tmp_path / 'baked.mtl').write_text('newmtl material_1\nmap_Kd baked.png\n')
    vt = np.array([[0.25, 0.125], [0.75, 0.125], [0.5, 0.875], [0.125, 0.25], [0.875, 0.75], [0.125, 0.75]])
    with open(str(tmp_path / 'baked.obj'), 'w') as f:
        f.write('mtllib baked.mtl\n' + ''.join('v %.8f %.8f %.8f\n' % tuple(p) for p in npz['rest_verts']))
        f.write(''.join('vt %.8f %.8f\n' % tuple(p) for p in vt) + 'usemtl material_1\nf 1/1 2/2 3/3\nf 1/4 3/5 4/6\n')
    faces, uv, image = eg.read_textured_obj(str(tmp_path / 'baked.obj'))
    assert (faces == npz['faces']).all() and uv.shape == (2, 3, 2) and image == str(tmp_path / 'baked.png')
    arrays, posed32 = rr.restated_arrays(npz, 4, np.float32)
    split = eg.split_corners(arrays, faces, uv)
    assert split['positions'].shape == (6, 3) and split['joints'].shape == (6, 4) and split['weights'].shape == (6, 4)
    assert (split['indices'] == np.arange(6).reshape(2, 3)).all()
    path = str(tmp_path / 'tex.glb')
    _gltf().write_glb(path, positions=split['positions'], indices=split['indices'], quat=split['quat'], trans=split['trans'],
                      joints=split['joints'], weights=split['weights'], uv=split['uv'], png=open(image, 'rb').read())
    gltf, binary = rr.read_glb(open(path, 'rb').read())
    rr.check_rules(gltf, binary)
    got, _ = rr.evaluate(gltf, binary)
    want = rr.lbs_rows(npz['rest_verts'], npz['skin'], npz['R'], npz['T'])[:, faces.reshape(-1)]
    assert got.shape == (2, 6, 3) and np.abs(got - want).max() <= rr.bound(posed32[:, faces.reshape(-1)], want)
    prim = gltf['meshes'][0]['primitives'][0]
    assert 'COLOR_0' not in prim['attributes']
    st = rr.read_accessor(gltf, binary, prim['attributes']['TEXCOORD_0'])
    assert np.array_equal(st, np.stack([vt[:, 0], 1 - vt[:, 1]], 1))          # eighths: exact in float32
    img = gltf['images'][0]
    view = gltf['bufferViews'][img['bufferView']]
    assert img['mimeType'] == 'image/png' and 'target' not in view
    assert binary[view['byteOffset']:view['byteOffset'] + view['byteLength']] == png
    assert gltf['materials'][0]['pbrMetallicRoughness']['baseColorTexture'] == {'index': 0}
    assert gltf['textures'] == [{'sampler': 0, 'source': 0}] and len(gltf['samplers']) == 1


def test_tie_rule_and_the_all_zero_column():
    col = np.array([[0.2, 0.], [0.3, 0.], [0.2, 0.], [0.1, 0.], [0.2, 0.], [0., 0.]], np.float32)
    for dtype in (np.float32, np.float64):
        j, w, d = rr.pack(col, 4, dtype)
        assert j[0].tolist() == [1, 0, 2, 4] and j[1].tolist() == [0, 0, 0, 0]
        assert w[1].tolist() == [1, 0, 0, 0] and d[1] == 0
        assert d[0] == dtype(np.float32(0.1)) and abs(float(w[0].sum()) - 1) < 1e-6
    j, w, d = rr.pack(col[:, :1], 8, np.float32)
    assert j[0].tolist() == [1, 0, 2, 4, 3, 0, 0, 0] and w[0, 5:].tolist() == [0, 0, 0] and d[0] == 0   # the zero weight: joint 0


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, p = None, 1 << 20                                                      # p: any non-null address; no launch reads it
    pack = lambda J=3, V=5, k=4, a=n: h.lasr_rig_pack(a, J, V, k, a, a, a, n)                                  # noqa: E731
    assert pack() == -1 and pack(V=0) == 0 and pack(J=64, V=0) == 0 and pack(J=65, V=0) == -1 and pack(J=65, a=p) == -1
    for k in (0, 1, 3, 5, 7, 9, 16):
        assert pack(k=k, V=0) == -1 and pack(k=k, a=p) == -1
    assert pack(k=8, V=0) == 0 and pack(J=-1, V=0) == -1 and pack(V=-1) == -1
    quats = lambda T=2, K=3, a=n: h.lasr_rig_quats(a, T, K, a, n)                                               # noqa: E731
    assert quats() == -1 and quats(T=0) == 0 and quats(K=0) == 0 and quats(T=0, K=65) == 0 and quats(T=0, K=66) == -1 and quats(T=-1) == -1
    skin = lambda T=2, K=3, V=5, k=4, a=n: h.lasr_rig_skin(a, a, a, a, a, T, K, V, k, a, n)                     # noqa: E731
    assert skin() == -1 and skin(T=0) == 0 and skin(V=0) == 0 and skin(T=0, k=8) == 0
    assert skin(T=0, k=0) == -1 and skin(T=0, k=5) == -1 and skin(T=0, K=1, k=0) == 0 and skin(T=0, K=1, k=4) == -1
    assert skin(T=0, K=66) == -1 and skin(T=0, K=0) == -1 and skin(T=1 << 20, V=1 << 20) == -1
    stats = lambda T=2, V=5, a=n: h.lasr_rig_stats(a, a, T, V, a, n)                                            # noqa: E731
    assert stats() == -1 and stats(T=0) == 0 and stats(V=0) == 0 and stats(T=-1) == -1 and stats(T=1 << 20, V=1 << 20) == -1
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert names[-1] == b'bake_resolve_kernel' and not any(b'rig' in x for x in names)     # the kernel-name table is not extended
    assert (_lib.RIG_MAX_BONES, _lib.RIG_MAX_INFLUENCES) == (64, 8)
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    assert '#define LASR_RIG_MAX_BONES 64\n' in hdr and '#define LASR_RIG_MAX_INFLUENCES 8\n' in hdr


def test_python_layer_refuses_cpu_tensors_and_what_is_no_rig():
    import torch
    from lasr_amd.nnutils import rig
    with pytest.raises(TypeError):
        rig.pack_influences(torch.rand(3, 5), 4)
    with pytest.raises(TypeError):
        rig.rotation_keys(torch.eye(3).expand(2, 3, 3, 3))
    with pytest.raises(TypeError):
        rig.skin_packed(torch.zeros(5, 3), None, None, torch.zeros(2, 1, 4), torch.zeros(2, 1, 3))
    with pytest.raises(TypeError):
        rig.deviation(torch.zeros(2, 5, 3), torch.zeros(2, 5, 3))
    good = rr.handmade_rig()
    rig.check_rig(good)

    def changed(key, fn):
        bad = {k: v.copy() for k, v in good.items()}
        fn(bad[key])
        return bad
    mirror, shear = np.diag([1., 1., -1.]).astype(np.float32), np.array([[1, 0.01, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    for bad, what in ((changed('R', lambda R: R.__setitem__((1, 2), R[1, 2] @ mirror)), 'reflection'),
                      (changed('R', lambda R: R.__setitem__((0, 0), R[0, 0] @ shear)), 'not orthogonal'),
                      (changed('skin', lambda s: s.__setitem__((0, 0), -1e-3)), 'non-negative'),
                      (changed('skin', lambda s: s.__setitem__((1, 3), np.nan)), 'finite')):
        with pytest.raises(ValueError, match=what):
            rig.build_rig(bad, 4)                                             # refused before any device is touched


def test_script_arguments():
    eg = _script()
    a = eg.parse_args(['--testdir', 'log/camel-5/', '--outpath', 'camel.glb'])
    assert (a.testdir, a.outpath, a.influences, a.max_dev, a.fps, a.texture_obj) == ('log/camel-5/', 'camel.glb', 'auto', 0.005, 10., '')
    a = eg.parse_args('--testdir t --outpath o.glb --influences 8 --max_dev 0.01 --fps 24 --texture_obj t/baked.obj'.split())
    assert (a.influences, a.max_dev, a.fps, a.texture_obj) == ('8', 0.01, 24., 't/baked.obj')
    assert eg.parse_args(['--influences', '4']).influences == '4'
    with pytest.raises(SystemExit):
        eg.parse_args(['--influences', '5'])
    sys.path.insert(0, ROOT)
    import extract
    assert extract.parse_flags([]).rig is False and extract.parse_flags(['--rig']).rig is True and extract.parse_flags(['--rig']).render is False
    line = eg.report_line(dict(quat=np.zeros((4, 5, 4)), positions=np.zeros((12, 3)), frame_ids=np.array([3, 4, 5, 6])),
                          dict(influences=4, max_overall=0.01234, frame=2, rms_overall=0.0021))
    assert line == '5 bones, 12 vertices, 4 keys, 4 influences: max deviation 1.23 % of the diagonal (frame 5), rms 0.21 %'
