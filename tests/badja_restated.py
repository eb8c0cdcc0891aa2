"""numpy restatement of the keypoint transfer and PCK of the reference's scripts/eval_badja.py (steps after the flow render):
the yardstick of lasr_kp_transfer (csrc/keypoints.hip) and scripts/eval_badja.py.  All flow arithmetic is float32 in the
reference's operation order; the score is float64, as numpy computes it there."""
import numpy as np

F32 = np.float32


def flow_from_colors(colors):
    """colors [4,S,S] float32 raster of render_flow_soft_3 -> flow [S,S,2] (x, y) with the background (channel 2 < 1e-9) at 0.
    The grid is p * 2 / (S - 1) - 1 as torch computes it on the device: the division by a scalar multiplies by the float32
    reciprocal."""
    c = np.asarray(colors, F32)
    S = c.shape[1]
    inv = F32(1) / F32(S - 1)
    p = np.arange(S, dtype=F32)
    g = (p * F32(2)) * inv - F32(1)
    fx = c[0] - g[None, :]
    fy = c[1] - g[:, None]
    bg = c[2] < F32(1e-9)
    return np.where(bg[..., None], F32(0), np.stack([fx, fy], -1)).astype(F32)


def transfer(flow, kp, H, W):
    """flow [>=H, >=W, 2] float32 (cropped to its top-left H x W here), kp [J,2] (row, col) -> (idx int64 [J], pred float32 [J,2]).
    invalid = |flow| < 1e-6; idx = first argmin of (invalid * 1e6 + (row - y)^2) + (col - x)^2; pred = kp + flow[idx] scaled by
    (H / 2, W / 2) -- rows by H / 2 although the flow is in units of the square render (the reference's quirk)."""
    f = np.asarray(flow, F32)[:H, :W].reshape(-1, 2)
    kp = np.asarray(kp, F32)
    invalid = np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) < F32(1e-6)
    y, x = np.divmod(np.arange(H * W), W)
    y, x = y.astype(F32), x.astype(F32)
    dr = kp[:, 0:1] - y[None]
    dc = kp[:, 1:2] - x[None]
    key = (invalid.astype(F32)[None] * F32(1e6) + dr * dr) + dc * dc
    idx = key.argmin(-1)
    s = f[idx]
    pred = kp.copy()
    pred[:, 0] = pred[:, 0] + (s[:, 1] * F32(H)) * F32(0.5)
    pred[:, 1] = pred[:, 1] + (s[:, 0] * F32(W)) * F32(0.5)
    return idx.astype(np.int64), pred


def score(pred, refsil, tarkp, refvis, tarvis):
    """-> correct flags (bool) of the joints visible in both frames: |pred - tarkp| < 0.2 sqrt(#(refsil[..., 0] > 0)), float64."""
    diff = np.linalg.norm(np.asarray(pred, F32) - np.asarray(tarkp, np.int64), 2, -1)
    sqarea = np.sqrt((np.asarray(refsil)[:, :, 0] > 0).sum())
    return (diff < sqarea * 0.2)[np.logical_and(tarvis, refvis)]


def pck(flags):
    return 100 * np.concatenate(flags).astype(float).mean()
