"""A reconstruction as a rig: the arrays of a glTF 2.0 skin and animation from what extract.py --rig writes (scripts/export_gltf.py;
DESIGN.md section 4.12).

This is the project's own addition: the reference has no exporter.  rig.npz holds the rest mesh, the dense skin [J,V] and per
frame one row-vector transform per bone, p_cam = (sum_k w_k (p R_k + T_k)) R_0 + T_0 (geom_utils.obj_to_cam).  glTF wants at
most 4 (or 8) influences per vertex and unit quaternions, so: pack_influences keeps the k largest weights and renormalises,
rotation_keys turns every R_k^T into a sign-continuous quaternion, skin_packed evaluates glTF's own skinning on exactly those
arrays, and deviation compares it with the full-weight blend (lasr_rig_* of csrc/rig.hip).  build_rig does the four in order
and reports what the truncation costs as a fraction of the rest shape's bounding-box diagonal.
"""
import numpy as np
import torch

from .. import _lib
from . import geom_utils

ORTHO_TOL = 1e-4                                             # |R R^T - I| a transform may show and still count as a rotation


def pack_influences(skin, k):
    """skin [J,V] (dense, >= 0) -> joints uint8 [V,k], weights float32 [V,k] (the k largest, renormalised; a zero weight carries
    joint 0), dropped float32 [V] (the weight left out, before renormalisation).  k is 4 or 8."""
    _lib.need_cuda(skin)
    k = int(k)
    if skin.ndimension() != 2 or skin.shape[0] > _lib.RIG_MAX_BONES:
        raise ValueError('pack_influences: skin must be [J <= %d, V], got %s' % (_lib.RIG_MAX_BONES, tuple(skin.shape)))
    if k not in (4, _lib.RIG_MAX_INFLUENCES):
        raise ValueError('pack_influences: k must be 4 or %d, got %d' % (_lib.RIG_MAX_INFLUENCES, k))
    skin = skin.detach().float().contiguous()
    J, V = skin.shape
    joints = torch.empty(V, k, dtype=torch.uint8, device=skin.device)
    weights = torch.empty(V, k, dtype=torch.float32, device=skin.device)
    dropped = torch.empty(V, dtype=torch.float32, device=skin.device)
    _lib.call('lasr_rig_pack', skin, J, V, k, joints, weights, dropped)
    return joints, weights, dropped


def rotation_keys(R):
    """R [T,K,3,3] (row-vector convention: p' = p R) -> float32 [T,K,4]: unit (x, y, z, w) of R^T, w >= 0 at the first frame
    and no sign flip between consecutive frames of a bone."""
    _lib.need_cuda(R)
    if R.ndimension() != 4 or tuple(R.shape[2:]) != (3, 3) or R.shape[1] > _lib.RIG_MAX_BONES + 1:
        raise ValueError('rotation_keys: R must be [T, K <= %d, 3, 3], got %s' % (_lib.RIG_MAX_BONES + 1, tuple(R.shape)))
    R = R.detach().float().contiguous()
    T, K = R.shape[:2]
    quat = torch.empty(T, K, 4, dtype=torch.float32, device=R.device)
    _lib.call('lasr_rig_quats', R, T, K, quat)
    return quat


def skin_packed(rest, joints, weights, quat, trans):
    """glTF's skinning of the file's arrays: rest [V,3], joints uint8 [V,k] / weights [V,k] (both None for a rig of the body
    alone), quat [T,K,4], trans [T,K,3] -> float32 [T,V,3] in OpenCV camera space, comparable with pred<i>."""
    _lib.need_cuda(rest, joints, weights, quat, trans)
    if rest.ndimension() != 2 or rest.shape[1] != 3:
        raise ValueError('skin_packed: rest must be [V, 3], got %s' % (tuple(rest.shape),))
    V = rest.shape[0]
    if quat.ndimension() != 3 or quat.shape[2] != 4 or not 1 <= quat.shape[1] <= _lib.RIG_MAX_BONES + 1:
        raise ValueError('skin_packed: quat must be [T, 1 <= K <= %d, 4], got %s' % (_lib.RIG_MAX_BONES + 1, tuple(quat.shape)))
    T, K = quat.shape[:2]
    if tuple(trans.shape) != (T, K, 3):
        raise ValueError('skin_packed: trans must be [%d, %d, 3], got %s' % (T, K, tuple(trans.shape)))
    if (joints is None) != (weights is None) or (joints is None) != (K == 1):
        raise ValueError('skin_packed: joints and weights go with K > 1 bones, and only with them')
    k = 0
    if joints is not None:
        k = joints.shape[1] if joints.ndimension() == 2 else -1
        if joints.dtype != torch.uint8 or k not in (4, _lib.RIG_MAX_INFLUENCES) or tuple(joints.shape) != (V, k) \
                or tuple(weights.shape) != (V, k):
            raise ValueError('skin_packed: joints must be uint8 [V = %d, 4 or 8] and weights alike, got %s %s and %s'
                             % (V, joints.dtype, tuple(joints.shape), tuple(weights.shape)))
        joints, weights = joints.contiguous(), weights.detach().float().contiguous()
    rest, quat, trans = (t.detach().float().contiguous() for t in (rest, quat, trans))
    out = torch.empty(T, V, 3, dtype=torch.float32, device=rest.device)
    _lib.call('lasr_rig_skin', rest, joints if k else None, weights if k else None, quat, trans, T, K, V, k, out)
    return out


def deviation(posed, ref):
    """posed, ref [T,V,3] -> float32 [T,8]: per frame the largest |posed - ref|, the sum of |posed - ref|^2, and the bounding
    box of posed (min xyz, max xyz).  The same bits on every run."""
    _lib.need_cuda(posed, ref)
    if posed.ndimension() != 3 or posed.shape[2] != 3 or posed.shape != ref.shape:
        raise ValueError('deviation: posed and ref must both be [T, V, 3], got %s and %s' % (tuple(posed.shape), tuple(ref.shape)))
    posed, ref = posed.detach().float().contiguous(), ref.detach().float().contiguous()
    T, V = posed.shape[:2]
    stats = torch.zeros(T, 8, dtype=torch.float32, device=posed.device)
    _lib.call('lasr_rig_stats', posed, ref, T, V, stats)
    return stats


def check_rig(npz):
    """The arrays of rig.npz as float64 / integer numpy arrays, refused (ValueError) when they are no rig: shapes that do not
    fit, transforms that are no rotations (|R R^T - I| > 1e-4, det <= 0), a skin that is negative or not finite."""
    rest = np.asarray(npz['rest_verts'], np.float64)
    faces = np.asarray(npz['faces']).astype(np.int64)
    colors = np.asarray(npz['colors'], np.float64)
    skin = np.asarray(npz['skin'], np.float64)
    R, T_ = np.asarray(npz['R'], np.float64), np.asarray(npz['T'], np.float64)
    ids = np.asarray(npz['frame_ids']).astype(np.int64)
    if rest.ndim != 2 or rest.shape[1] != 3 or rest.shape[0] < 1 or colors.shape != rest.shape:
        raise ValueError('rig: rest_verts and colors must both be [V >= 1, 3], got %s and %s' % (rest.shape, colors.shape))
    V = rest.shape[0]
    if faces.ndim != 2 or faces.shape[1] != 3 or (faces.size and (faces.min() < 0 or faces.max() >= V)):
        raise ValueError('rig: faces must be [F, 3] indices into the %d vertices' % V)
    if R.ndim != 4 or R.shape[2:] != (3, 3) or R.shape[0] < 1 or not 1 <= R.shape[1] <= _lib.RIG_MAX_BONES + 1:
        raise ValueError('rig: R must be [T >= 1, 1 <= K <= %d, 3, 3], got %s' % (_lib.RIG_MAX_BONES + 1, R.shape))
    T, K = R.shape[:2]
    if T_.shape != (T, K, 3) or ids.shape != (T,):
        raise ValueError('rig: T must be [%d, %d, 3] and frame_ids [%d], got %s and %s' % (T, K, T, T_.shape, ids.shape))
    if skin.size == 0:
        skin = skin.reshape(0, V)
    if skin.shape != (K - 1, V):
        raise ValueError('rig: skin must be [K - 1 = %d, V = %d], got %s' % (K - 1, V, skin.shape))
    if not (np.isfinite(rest).all() and np.isfinite(R).all() and np.isfinite(T_).all()):
        raise ValueError('rig: rest_verts, R and T must be finite')
    if not np.isfinite(skin).all() or (skin < 0).any():
        raise ValueError('rig: the skin must be finite and non-negative')
    err = np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max()
    if err > ORTHO_TOL:
        raise ValueError('rig: R is not orthogonal (|R R^T - I| = %.3g > %g): glTF animates rotations only' % (err, ORTHO_TOL))
    if (np.linalg.det(R) <= 0).any():
        raise ValueError('rig: R holds a reflection (det <= 0): glTF animates rotations only')
    return dict(rest_verts=rest, faces=faces, colors=colors, skin=skin, R=R, T=T_, frame_ids=ids)


def build_rig(npz, influences=4, device=None):
    """npz: rig.npz of extract.py --rig (or a dict of its arrays); influences 4 or 8 -> (arrays, report).
    arrays (numpy): positions [V,3] float32, indices [F,3] uint32, colors [V,3] float32, joints uint8 [V,k] / weights float32
    [V,k] (None, None without part bones), quat [T,K,4] and trans [T,K,3] float32, frame_ids [T], posed [T,V,3] (the rig as a
    viewer will pose it, camera space).  report: influences, diag (rest bounding-box diagonal), max / rms [T] (deviation of the
    k-influence rig from the full-weight obj_to_cam, as fractions of diag), max_overall with its frame (position in frame_ids),
    rms_overall, dropped_max (the largest weight mass a vertex lost), bbox [T,2,3] of the posed frames."""
    a = check_rig(npz)
    dev = torch.device(device if device is not None else 'cuda:0')
    if dev.type != 'cuda':
        raise TypeError('build_rig runs its kernels on a cuda (HIP) device; there is no CPU fallback')
    f32 = dict(dtype=torch.float32, device=dev)
    rest = torch.as_tensor(a['rest_verts'], **f32)
    R, Tm = torch.as_tensor(a['R'], **f32), torch.as_tensor(a['T'], **f32)
    T, K = R.shape[:2]
    V = rest.shape[0]
    joints = weights = None
    dropped_max = 0.
    skin = None
    if K > 1:
        skin = torch.as_tensor(a['skin'], **f32)
        joints, weights, dropped = pack_influences(skin, influences)
        dropped_max = float(dropped.max())
    quat = rotation_keys(R)
    posed = skin_packed(rest, joints, weights, quat, Tm)
    with torch.no_grad():                                  # the full-weight blend: the project's own LBS
        ref = geom_utils.obj_to_cam(rest[None].expand(T, V, 3).contiguous(), R.reshape(T * K, 3, 3), Tm.reshape(T * K, 1, 3), K, 1,
                                    skin[None, :, :, None] if skin is not None else None)
    stats = deviation(posed, ref).double().cpu().numpy()
    diag = float(np.linalg.norm(a['rest_verts'].max(0) - a['rest_verts'].min(0))) or 1.
    mx = stats[:, 0] / diag
    report = dict(influences=int(influences) if K > 1 else 0, diag=diag, max=mx, rms=np.sqrt(stats[:, 1] / V) / diag,
                  max_overall=float(mx.max()), frame=int(mx.argmax()), rms_overall=float(np.sqrt(stats[:, 1].sum() / (T * V)) / diag),
                  dropped_max=dropped_max, bbox=stats[:, 2:].reshape(T, 2, 3))
    arrays = dict(positions=a['rest_verts'].astype(np.float32), indices=a['faces'].astype(np.uint32),
                  colors=a['colors'].astype(np.float32), joints=joints.cpu().numpy() if joints is not None else None,
                  weights=weights.cpu().numpy() if weights is not None else None, quat=quat.cpu().numpy(), trans=Tm.cpu().numpy(),
                  frame_ids=a['frame_ids'], posed=posed.cpu().numpy())
    return arrays, report
