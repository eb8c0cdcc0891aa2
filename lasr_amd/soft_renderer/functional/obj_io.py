"""Wavefront .obj read/write (reference: soft_renderer/functional/load_obj.py:9-167, save_obj.py:44-87): geometry, per-vertex
colours, and -- for textured models such as the one scripts/render_syn.py:71 of the reference renders -- per-face surface
textures sampled from the material's atlas image by lasr_load_textures (the reference's load_textures CUDA extension).
Writing surface textures (save_obj.py:9-37, the create_texture_image CUDA extension) goes through the HIP kernel
lasr_create_texture_image; save_voxel (save_obj.py:90-98) writes occupied voxels as a vertex-only .obj."""
import os

import numpy as np
import torch

from ... import _lib


def parse_obj_materials(filename_obj):
    """The texture side of an .obj (load_obj.py:28-71, 9-25): -> (faces_uv [F,3,2] float32 in [0,1), material name per triangle,
    {material: Kd colour}, {material: texture file path}).  Triangles are the same fan triangulation as the geometry's; a corner
    without a texture index takes index 0, i.e. -1 after the 1-based shift -- the LAST vt entry, as in the reference; uv
    coordinates above 1 wrap (x % 1).  Raises if the file names no material library."""
    vts, tri, mats, mat, mtl = [], [], [], '', None
    with open(filename_obj) as f:
        lines = f.readlines()
    for line in lines:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == 'vt':
            vts.append([float(v) for v in tok[1:3]])
        elif tok[0] == 'usemtl':
            mat = tok[1]
        elif tok[0] == 'mtllib':
            mtl = os.path.join(os.path.dirname(filename_obj), tok[1])
        elif tok[0] == 'f':
            idx = [int(t.split('/')[1]) if ('/' in t and '//' not in t) else 0 for t in tok[1:]]
            for i in range(len(idx) - 2):
                tri.append((idx[0], idx[i + 1], idx[i + 2]))
                mats.append(mat)
    if mtl is None:
        raise Exception('Failed to load textures.')                 # the reference's message (load_obj.py:143)
    vts = np.asarray(vts, np.float32).reshape(-1, 2)
    uv = vts[np.asarray(tri, np.int64).reshape(-1, 3) - 1]          # [F,3,2]; index -1 = last entry
    uv = np.where(uv > 1, uv % 1, uv).astype(np.float32)
    colors, files, name = {}, {}, ''
    with open(mtl) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == 'newmtl':
                name = tok[1]
            elif tok[0] == 'map_Kd':
                files[name] = os.path.join(os.path.dirname(filename_obj), tok[1])
            elif tok[0] == 'Kd':
                colors[name] = np.asarray([float(v) for v in tok[1:4]], np.float32)
    return uv, mats, colors, files


def _surface_textures(filename_obj, texture_res, device):
    """[F, R*R, 3] surface texels: ones, then each material's Kd colour, then each material's atlas sampled by the HIP kernel."""
    from PIL import Image
    from .load_textures import load_textures
    uv, mats, colors, files = parse_obj_materials(filename_obj)
    F = uv.shape[0]
    mats = np.asarray(mats)
    textures = torch.ones(F, texture_res ** 2, 3, dtype=torch.float32, device=device)
    for name, color in colors.items():
        sel = torch.from_numpy(mats == name).to(device)
        textures[sel] = torch.from_numpy(color).to(device)[None, None, :]
    faces_uv = torch.from_numpy(uv).to(device)
    for name, path in files.items():
        # grey, palette and RGBA atlases all become RGB (the reference stacks grey images and drops the alpha channel, :84-89)
        image = np.asarray(Image.open(path).convert('RGB')).astype(np.float32) / 255.
        image = np.ascontiguousarray(image[::-1])                   # v = 0 is the BOTTOM row of the picture
        upd = torch.from_numpy((mats == name).astype(np.int32)).to(device)
        sampled = load_textures(torch.from_numpy(image).to(device), faces_uv, texture_res, upd)
        sel = upd.bool()
        textures[sel] = sampled[sel]
    return textures


def load_obj(filename_obj, normalization=False, load_texture=False, texture_res=4, texture_type='surface',
             device=None):
    assert texture_type in ['surface', 'vertex']
    device = device or ('cuda' if torch.cuda.is_available() else 'cpu')
    verts, cols, faces = [], [], []
    with open(filename_obj) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == 'v':
                verts.append([float(v) for v in tok[1:4]])
                cols.append([float(v) for v in tok[4:7]])
            elif tok[0] == 'f':
                ids = [int(t.split('/')[0]) for t in tok[1:]]
                for i in range(len(ids) - 2):                     # fan triangulation
                    faces.append((ids[0], ids[i + 1], ids[i + 2]))
    vertices = torch.from_numpy(np.asarray(verts, np.float32)).to(device)
    faces = torch.from_numpy(np.asarray(faces, np.int32)).to(device) - 1
    if normalization:                                              # unit cube centred at zero
        vertices -= vertices.min(0)[0][None, :]
        vertices /= torch.abs(vertices).max()
        vertices *= 2
        vertices -= vertices.max(0)[0][None, :] / 2
    if load_texture and texture_type == 'surface':
        return vertices, faces, _surface_textures(filename_obj, texture_res, vertices.device)
    if load_texture:
        return vertices, faces, torch.from_numpy(np.asarray(cols, np.float32)).to(device)
    return vertices, faces


def create_texture_image(textures, texture_res=16):
    """textures [F, R_in*R_in, 3] (float32 or float64) -> (image [H, W, 3] numpy, vt [F, 3, 2] numpy), save_obj.py:9-37.
    Face fn owns tile (fn % tile_width, fn // tile_width) of texture_res x texture_res pixels, tile_width = int((F-1)**0.5) + 1;
    its triangle has the reference's corners in that tile, and every pixel copies the texel of R_in x R_in its barycentric
    coordinates pick (lasr_create_texture_image).  vt is divided by (W-1, H-1); the image is flipped so that v = 0 is its bottom
    row.  Departure: the reference computes the tile row as face_nums / tile_width, a true division under every torch since
    1.7, which shifts the vt triangle of each face outside the first column by (fn % tile_width) / tile_width of a tile while
    its kernel fills tiles by integer row -- its atlas does not load back onto the faces that wrote it.  The row here is
    the integer one the kernel indexes by."""
    _lib.need_cuda(textures)
    if textures.dtype not in (torch.float32, torch.float64):
        raise TypeError('create_texture_image takes float32 or float64 textures, got %s' % textures.dtype)
    num_faces, R_out = textures.shape[0], int(texture_res)
    R_in = int(round(textures.shape[1] ** 0.5))
    if textures.ndimension() != 3 or textures.shape[2] != 3 or R_in * R_in != textures.shape[1] or num_faces < 1 or R_out < 1:
        raise ValueError('textures must be [F >= 1, R*R, 3] and texture_res >= 1, got %s, %d' % (tuple(textures.shape), R_out))
    tile_width = int((num_faces - 1.) ** 0.5) + 1
    tile_height = int((num_faces - 1.) / tile_width) + 1
    dt = np.float64 if textures.dtype == torch.float64 else np.float32
    face_nums = np.arange(num_faces)
    column, row = face_nums % tile_width, face_nums // tile_width
    vertices = np.zeros((num_faces, 3, 2), dt)
    vertices[:, 0, 0] = column * R_out + R_out / 2
    vertices[:, 0, 1] = row * R_out + 1
    vertices[:, 1, 0] = column * R_out + 1
    vertices[:, 1, 1] = (row + 1) * R_out - 1 - 1
    vertices[:, 2, 0] = (column + 1) * R_out - 1 - 1
    vertices[:, 2, 1] = (row + 1) * R_out - 1 - 1
    dev = textures.device
    image = torch.empty(tile_height * R_out, tile_width * R_out, 3, dtype=textures.dtype, device=dev)
    tex = textures.detach().contiguous()
    fuv = torch.from_numpy(vertices).to(dev)
    _lib.call('lasr_create_texture_image_f64' if textures.dtype == torch.float64 else 'lasr_create_texture_image', fuv, tex, image,
              num_faces, R_in, R_out, 1e-5)
    vertices[:, :, 0] /= dt(image.shape[1] - 1)
    vertices[:, :, 1] /= dt(image.shape[0] - 1)
    image = image.cpu().numpy()[::-1, ::1]
    return image, vertices


def save_obj(filename, vertices, faces, textures=None, texture_res=16, texture_type='surface'):
    """save_obj.py:40-87.  With surface textures it also writes <name>.png (the atlas of create_texture_image, clipped to [0, 1]
    and truncated to uint8) and <name>.mtl naming it, and the .obj gets the vt of every face corner."""
    assert vertices.ndimension() == 2 and faces.ndimension() == 2
    assert texture_type in ['surface', 'vertex']
    assert texture_res >= 2
    surface = textures is not None and texture_type == 'surface'
    if surface:
        from PIL import Image
        filename_mtl = filename[:-4] + '.mtl'
        filename_texture = filename[:-4] + '.png'
        material_name = 'material_1'
        texture_image, vertices_textures = create_texture_image(textures, texture_res)
        texture_image = (texture_image.clip(0, 1) * 255).astype('uint8')
        Image.fromarray(np.ascontiguousarray(texture_image)).save(filename_texture)
    v = vertices.detach().cpu().numpy()
    fc = faces.detach().cpu().numpy()
    tx = textures.detach().cpu().numpy() if textures is not None and not surface else None
    with open(filename, 'w') as f:
        f.write('# %s\n#\n\n' % os.path.basename(filename))
        if surface:
            f.write('mtllib %s\n\n' % os.path.basename(filename_mtl))
        for i, p in enumerate(v):
            if tx is not None:
                f.write('v %.8f %.8f %.8f %.8f %.8f %.8f\n' % (p[0], p[1], p[2], tx[i, 0], tx[i, 1], tx[i, 2]))
            else:
                f.write('v %.8f %.8f %.8f\n' % (p[0], p[1], p[2]))
        f.write('\n')
        if surface:
            for p in vertices_textures.reshape((-1, 2)):
                f.write('vt %.8f %.8f\n' % (p[0], p[1]))
            f.write('\n')
            f.write('usemtl %s\n' % material_name)
            for i, t in enumerate(fc):
                f.write('f %d/%d %d/%d %d/%d\n' % (t[0] + 1, 3 * i + 1, t[1] + 1, 3 * i + 2, t[2] + 1, 3 * i + 3))
            f.write('\n')
        else:
            for t in fc:
                f.write('f %d %d %d\n' % (t[0] + 1, t[1] + 1, t[2] + 1))
    if surface:
        with open(filename_mtl, 'w') as f:
            f.write('newmtl %s\n' % material_name)
            f.write('map_Kd %s\n' % os.path.basename(filename_texture))


def save_voxel(filename, voxel):
    """save_obj.py:90-98: every voxel (i, j, k) equal to 1 of voxel [S0,S1,S2] becomes the vertex (i/S0, j/S1, k/S2), in index
    order.  Departure: the reference hands a 1-D empty faces tensor to a save_obj that asserts 2-D faces and so always fails;
    this writes the vertex-only .obj it evidently means."""
    vox = voxel.detach().cpu().numpy() if torch.is_tensor(voxel) else np.asarray(voxel)
    idx = np.argwhere(vox == 1).astype(np.float64)
    vertices = (idx / np.asarray(vox.shape, np.float64)).astype(np.float32)
    return save_obj(filename, torch.from_numpy(vertices.reshape(-1, 3)), torch.zeros(0, 3, dtype=torch.int32))
