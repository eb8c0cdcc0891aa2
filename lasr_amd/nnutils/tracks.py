"""Dense long-range point tracks of a reconstruction (scripts/export_tracks.py).

This is the project's own addition: the reference only transfers annotated keypoints between frame pairs.  A query (t, v, u) =
(frame position, row, column) is anchored on the surface of frame t's mesh (face + barycentrics, lasr_track_anchor) and carried
through every frame with a visibility decision (lasr_track_project, csrc/tracks.hip); include/lasr_ops.h states the arithmetic.

Scenes are the posed sequences of lasr_amd/nnutils/posed.py, which states the conventions and holds the raster of side IS =
max(H, W).  Frames are walked CHUNK_FRAMES at a time (posed.py's default), twice: the anchoring walk rasterises only the chunks
that hold a query frame (one chunk for the default query set), the projection walk every chunk.  The rasters are NOT kept
between the two walks: a raster is 8 IS^2 bytes a frame (2.6 GB for 90 frames at 1080p), and keeping them would save the one
raster launch of the query chunk.
"""
import torch

from .. import _lib
from . import posed

CHUNK_FRAMES = posed.CHUNK_FRAMES
STATE_NONE, STATE_VISIBLE, STATE_HIDDEN, STATE_OUTSIDE, STATE_BEHIND = 0, 1, 2, 3, 4


def covered_queries(raster_of_frame, t, stride=1, H=None, W=None):
    """Default query set of frame position t: the centres of the covered pixels on every stride-th row and column (row % stride ==
    0 and col % stride == 0) of raster_of_frame = that frame's aggrs_info [2,IS,IS] (or its plane 1 [IS,IS]), cropped to H x W
    when given.  -> queries [Q,3] float32 (t, row + 0.5, col + 0.5) on the raster's device, in row-major order."""
    if not torch.is_tensor(raster_of_frame):
        raise TypeError('covered_queries: raster_of_frame must be a tensor')
    plane = raster_of_frame[1] if raster_of_frame.ndimension() == 3 else raster_of_frame
    if plane.ndimension() != 2:
        raise ValueError('covered_queries: raster_of_frame must be [2, IS, IS] or [IS, IS], got %s' % (tuple(raster_of_frame.shape),))
    stride = int(stride)
    if stride < 1:
        raise ValueError('covered_queries: stride must be at least 1, got %d' % stride)
    plane = plane[:H, :W][::stride, ::stride]
    rc = torch.nonzero(plane >= 0).float() * stride + 0.5
    return torch.cat([torch.full_like(rc[:, :1], float(t)), rc], 1)


def frame_raster(verts, faces, K, t, H, W):
    """aggrs_info [2,IS,IS] of frame position t alone (IS = max(H, W)): what covered_queries takes."""
    _lib.need_cuda(verts, faces, K)
    T = verts.shape[0]
    if not 0 <= int(t) < T:
        raise ValueError('frame_raster: frame position %d is outside the %d frames' % (int(t), T))
    one = posed.Posed(verts[int(t):int(t) + 1], faces, K.reshape(T, 4)[int(t):int(t) + 1], H, W)
    return posed.face_index_raster(one.verts, one.faces32, one.K, one.IS)[0]


def track_points(verts, faces, K, queries, H, W, snap_radius=0, window=1):
    """verts [T,V,3] camera space, faces [F,3] (shared), K [T,4] = fx fy px py (pixels), queries [Q,3] = (t, v, u): frame position
    (a whole number in 0 .. T-1), row and column coordinate in pixels of the H x W frame.
    -> (tracks [Q,T,2] float32 (u, v), state [Q,T] uint8, anchors) on the device, query-major as in TAP-Vid; state 1 visible,
    2 hidden, 3 outside the frame, 4 behind the camera (track NaN), 0 no anchor (track NaN).  anchors is a dict: 'face' [Q] int32
    (-1: none), 'bary' [Q,3] float32 (c0, c1, c2), 'facing' [Q] float32 and 'snapped' [Q,2] float32 (v, u), the position the
    anchor was computed at (moved to a covered pixel's centre when snap_radius > 0 found one for a query on an empty pixel)."""
    if not torch.is_tensor(queries):
        raise TypeError('track_points: queries must be a tensor')
    _lib.need_cuda(queries)
    snap_radius, window = int(snap_radius), int(window)
    seq = posed.sequence('track_points', verts, faces, K, H, W, _lib.TRACK_MAX_SIZE)
    dev, faces32, T, V, F, IS, H, W = seq.device, seq.faces32, seq.T, seq.V, seq.F, seq.IS, seq.H, seq.W
    if queries.ndimension() != 2 or queries.shape[1] != 3 or not queries.is_floating_point():
        raise ValueError('track_points: queries must be floating point [Q, 3] (t, v, u), got %s %s' % (queries.dtype, tuple(queries.shape)))
    Q = queries.shape[0]
    if not 0 <= snap_radius <= _lib.TRACK_MAX_SNAP:
        raise ValueError('track_points: snap_radius must be 0..%d, got %d' % (_lib.TRACK_MAX_SNAP, snap_radius))
    if not 0 <= window <= _lib.TRACK_MAX_WINDOW:
        raise ValueError('track_points: window must be 0..%d, got %d' % (_lib.TRACK_MAX_WINDOW, window))
    queries = queries.detach().float().contiguous()
    if Q:
        qt = queries[:, 0]
        if not bool(((qt == qt.round()) & (qt >= 0) & (qt < T)).all()):
            raise ValueError('track_points: the frame position of every query must be a whole number in 0..%d' % (T - 1))

    rec = torch.zeros(Q, 4, dtype=torch.float32, device=dev)
    rec.view(torch.int32)[:, 0] = -1                                 # no anchor until the anchoring walk writes one
    snapped = queries[:, 1:3].clone()
    frame_major = torch.empty(T, Q, 2, dtype=torch.float32, device=dev)
    state_major = torch.empty(T, Q, dtype=torch.uint8, device=dev)
    if Q and T:
        held = set((queries[:, 0].long() // CHUNK_FRAMES).unique().tolist())
        for i, j, v, k, raster in seq.chunks(CHUNK_FRAMES, only=held):          # anchoring walk
            _lib.call('lasr_track_anchor', v, faces32, k, raster, queries, rec, snapped, i, j - i, Q, V, F, IS, H, W, snap_radius)
        for i, j, v, k, raster in seq.chunks(CHUNK_FRAMES):                     # projection walk
            _lib.call('lasr_track_project', v, faces32, k, raster, rec, frame_major[i:j], state_major[i:j], j - i, Q, V, F, IS, H, W,
                      window)
    c1, c2 = rec[:, 1], rec[:, 2]
    anchors = dict(face=rec.view(torch.int32)[:, 0].clone(), bary=torch.stack([1. - c1 - c2, c1, c2], 1), facing=rec[:, 3].clone(),
                   snapped=snapped)
    return frame_major.transpose(0, 1).contiguous(), state_major.transpose(0, 1).contiguous(), anchors


def splat(frames, tracks, state, colors, radius=2):
    """Preview: frames uint8 [T,H,W,3], tracks [Q,T,2] (u, v), state [Q,T] uint8, colors uint8 [Q,3] -> uint8 [T,H,W,3] with a disc
    of `radius` pixels blended over the frame at every visible (state 1) point; the highest query index wins an overlap."""
    for name, t in (('frames', frames), ('tracks', tracks), ('state', state), ('colors', colors)):
        if not torch.is_tensor(t):
            raise TypeError('splat: %s must be a tensor' % name)
    _lib.need_cuda(frames, tracks, state, colors)
    radius = int(radius)
    if frames.dtype != torch.uint8 or frames.ndimension() != 4 or frames.shape[3] != 3:
        raise ValueError('splat: frames must be uint8 [T, H, W, 3], got %s %s' % (frames.dtype, tuple(frames.shape)))
    T, H, W = (int(x) for x in frames.shape[:3])
    if tracks.ndimension() != 3 or tracks.shape[1] != T or tracks.shape[2] != 2:
        raise ValueError('splat: tracks must be [Q, T = %d, 2], got %s' % (T, tuple(tracks.shape)))
    Q = tracks.shape[0]
    if state.dtype != torch.uint8 or tuple(state.shape) != (Q, T):
        raise ValueError('splat: state must be uint8 [%d, %d], got %s %s' % (Q, T, state.dtype, tuple(state.shape)))
    if colors.dtype != torch.uint8 or tuple(colors.shape) != (Q, 3):
        raise ValueError('splat: colors must be uint8 [%d, 3], got %s %s' % (Q, colors.dtype, tuple(colors.shape)))
    if not (1 <= H <= _lib.TRACK_MAX_SIZE and 1 <= W <= _lib.TRACK_MAX_SIZE):
        raise ValueError('splat: frames of %d x %d: each side must be 1..%d' % (H, W, _lib.TRACK_MAX_SIZE))
    if not 0 <= radius <= _lib.TRACK_MAX_RADIUS:
        raise ValueError('splat: radius must be 0..%d, got %d' % (_lib.TRACK_MAX_RADIUS, radius))
    frames = frames.contiguous()
    out = torch.empty_like(frames)
    if T == 0:
        return out
    tr = tracks.detach().float().transpose(0, 1).contiguous()        # the ABI is frame-major
    st = state.transpose(0, 1).contiguous()
    colors = colors.contiguous()
    keys = torch.zeros(T, H, W, dtype=torch.int32, device=frames.device)
    _lib.call('lasr_track_splat_keys', tr, st, keys, T, Q, H, W, radius)
    _lib.call('lasr_track_splat_resolve', keys, colors if Q else None, frames, out, T, Q, H, W)
    return out
