"""The reconstruction on disk: what extract.py writes for a sequence, as render_vis.py and the tools under scripts/ read it.

The frames are those of configs/<seqname>.config (frame_list); per frame id i the directory holds pred<i>.ply (or .obj) in camera
space and cam<i>.txt, whose row 3 is the intrinsics fx fy px py in pixels; the annotation of a frame lies where the loader looks
for it (annotation_path).  read() gathers these for a list of frames and refuses (ReadError) what is missing or does not share
the topology of the first mesh.  Host only: numpy, and torch for the tensors load_mesh returns.
"""
import collections
import glob
import os

import numpy as np
import torch


class ReadError(ValueError):
    """Why read() gave up; the text carries no script name, the caller puts its own in front."""


Reconstruction = collections.namedtuple('Reconstruction', 'ids verts face colors has_colours cams K imgs masks')
Reconstruction.__doc__ = """ids: frame ids; verts: list of float32 [V,3]; face: the shared [F,3]; colors: list of uint8 [V,3];
has_colours: every frame had a .ply (the .obj fallback's grey is no colour); cams: list of the cam<i>.txt arrays and K float32 [T,4],
their row 3; imgs: list of uint8 [H,W,3]; masks: list of the annotations.  What read() was told to leave out is None."""


def frame_list(seqname):
    """Frame paths of the sequence, as the video loader selects them (lasr_amd/dataloader/vid.py)."""
    from lasr_amd.dataloader.vid import read_config
    cfg = read_config(seqname)
    names = sorted(glob.glob('%s/*' % cfg['datapath']))
    if cfg['end_frame'] > 0:
        names = names[:cfg['end_frame']]
    return names[cfg['init_frame']:][::cfg['dframe']]


def frame_id(name):
    """.../00012.jpg -> 12."""
    return int(os.path.basename(name).split('.')[-2])


def annotation_path(name):
    """.../JPEGImages/<res>/<seq>/00000.jpg -> .../Annotations/<res>/<seq>/00000.png, the loader's substitution
    (lasr_amd/dataloader/vid.py)."""
    return name.replace('JPEGImages', 'Annotations').replace('.jpg', '.png')


def load_mesh(testdir, fr):
    """pred<fr>.ply (with its colours) or pred<fr>.obj (grey 102) -> verts [V,3] float32, faces [F,3] long, colours uint8 [V,3]."""
    from lasr_amd.ext_utils.ply import read_ply
    ply = os.path.join(testdir, 'pred%d.ply' % fr)
    if os.path.exists(ply):
        m = read_ply(ply)
        v, f = torch.from_numpy(m['verts']).float(), torch.from_numpy(m['faces'])
        c = m['colors'] if m['colors'] is not None else np.full((len(v), 3), 102, np.uint8)
        return v, f, torch.from_numpy(c.astype(np.uint8))
    from lasr_amd.soft_renderer.functional import load_obj
    v, f = load_obj(os.path.join(testdir, 'pred%d.obj' % fr))
    return v.float().cpu(), f.long().cpu(), torch.full((v.shape[0], 3), 102, dtype=torch.uint8)


def check_topology(faces_list, frame_ids):
    """Every pred<i> must share the faces of the first: the tools stack the frames over one face list.  -> those faces."""
    first = np.asarray(faces_list[0])
    for fr, f in zip(frame_ids[1:], faces_list[1:]):
        f = np.asarray(f)
        if f.shape != first.shape or (f != first).any():
            raise ReadError('pred%d does not share the topology of pred%d' % (fr, frame_ids[0]))
    return first


def read(testdir, names, frames=True, cams=True, annotations=None, no_annotation='no annotation for frame %(fr)d (%(e)s)'):
    """The meshes of the frames `names` (paths, as frame_list gives them) in testdir -> Reconstruction.  frames: open the images
    (RGB); cams: read cam<i>.txt; annotations: None, the PIL mode to convert each annotation to, or True to keep it as stored.
    no_annotation words the refusal of a missing annotation from name, fr and e."""
    from PIL import Image
    ids, verts, faces, colors, cam_list, imgs, masks, has_colours = [], [], [], [], [], [], [], True
    for name in names:
        fr = frame_id(name)
        if frames:
            imgs.append(np.asarray(Image.open(name).convert('RGB')))
        try:
            v, f, c = load_mesh(testdir, fr)
            if cams:
                cam_list.append(np.loadtxt(os.path.join(testdir, 'cam%d.txt' % fr)))
        except (OSError, ValueError) as e:
            raise ReadError('no mesh for frame %d in %s (%s)' % (fr, testdir, e))
        has_colours &= os.path.exists(os.path.join(testdir, 'pred%d.ply' % fr))
        if annotations is not None:
            try:
                m = Image.open(annotation_path(name))
                masks.append(np.asarray(m if annotations is True else m.convert(annotations)))
            except OSError as e:
                raise ReadError(no_annotation % dict(name=name, fr=fr, e=e))
        ids.append(fr), verts.append(v.numpy()), faces.append(f.numpy()), colors.append(c.numpy())
    return Reconstruction(ids, verts, check_topology(faces, ids), colors, has_colours, cam_list if cams else None,
                          np.stack([c[3] for c in cam_list]).astype(np.float32) if cams else None, imgs if frames else None,
                          masks if annotations is not None else None)
