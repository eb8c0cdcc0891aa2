"""Restatements for the VCN tests (lasr_amd/ext_nnutils/vcn.py, csrc/vcn.hip) and the fixture generator tools/gen_vcn_golden.py.

* `vcn_test_weights(name, shape)`: the deterministic weights both sides load (no weight file is committed).
* `input_pair()`: the 320x384 input pair of the fixture.
* `corr_proj64` / `flow_reg64`: float64 restatements of the two matching kernels, written from the reference's semantics
  (third_party/ext_nnutils/VCNplus.py:68-148, 350-406; conv4d.py:226-235), one displacement at a time.
* `corr_proj_reference_shaped` / `flow_reg_reference_shaped`: the reference's own shape of the matching stage in fp32 (the dense
  [b, C, U, V, h, w] cost volume by slice assignment, projfeat4d, flow_reg's ~15 passes), for tools/vcn_matching_bench.py.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

PAIR_SHAPE = (320, 384)
PAIR_SHIFT = (1.75, -0.5)            # (dx, dy) in pixels of the second image against the first


def vcn_test_weights(name, shape):
    """Deterministic tensor for state_dict entry `name`: conv weights N(0, sqrt(2 / fan_in)), biases N(0, 0.01), BN weight and
    running_var U(0.5, 1.5), BN bias and running_mean N(0, 0.1); a numpy generator seeded by crc32(name) per tensor."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    shape = tuple(int(s) for s in shape)
    leaf = name.rsplit('.', 1)[-1]
    if leaf == 'num_batches_tracked':
        return np.zeros(shape, np.int64)
    if leaf == 'running_var' or (leaf == 'weight' and len(shape) == 1):
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if leaf == 'running_mean' or (leaf == 'bias' and _is_bn(name)):
        return rng.normal(0., 0.1, shape).astype(np.float32)
    if leaf == 'bias':
        return rng.normal(0., 0.01, shape).astype(np.float32)
    fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    return rng.normal(0., math.sqrt(2. / fan_in), shape).astype(np.float32)


def _is_bn(name):
    """A BatchNorm parameter of VCN's state_dict: its module is `bn` (projfeat4d) or index 1 of a Sequential (conv + BN)."""
    return name.rsplit('.', 2)[-2] in ('bn', '1')


def fill_state_dict(model):
    """Load vcn_test_weights into every parameter and BatchNorm statistic of `model`, each under its first registered name (the
    reference's VCN also reaches its modules through aliases such as f_modules.0 for f6, which must not reseed them)."""
    with torch.no_grad():
        for k, t in list(model.named_parameters()) + list(model.named_buffers()):
            if k.endswith(('.running_mean', '.running_var')) or isinstance(t, torch.nn.Parameter):
                t.copy_(torch.from_numpy(vcn_test_weights(k, t.shape)))
    return model


def input_pair():
    """-> (im0, im1) uint8 [320, 384, 3] RGB: a smooth multi-frequency texture, the second shifted by PAIR_SHIFT."""
    H, W = PAIR_SHAPE
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')

    def tex(x, y):
        r = 0.5 + 0.25 * np.sin(0.21 * x + 0.5 * np.sin(0.05 * y)) + 0.2 * np.cos(0.13 * y - 0.07 * x)
        g = 0.5 + 0.3 * np.sin(0.11 * x * 0.7 + 0.17 * y) * np.cos(0.031 * x)
        b = 0.5 + 0.35 * np.cos(0.09 * np.hypot(x - 150., y - 120.)) + 0.1 * np.sin(0.37 * x)
        return np.clip(np.stack([r, g, b], -1), 0, 1)
    dx, dy = PAIR_SHIFT
    im0 = np.round(255 * tex(xx, yy)).astype(np.uint8)
    im1 = np.round(255 * tex(xx - dx, yy - dy)).astype(np.uint8)
    return im0, im1


def pair_input(im0, im1, mean=(0.33, 0.33, 0.33)):
    """auto_gen.py:104-107 for an already padded pair: BGR, /255, minus the mean -> [2, 3, H, W] float32."""
    out = []
    for im in (im0, im1):
        x = im[:, :, ::-1].astype(np.float64) / 255. - np.asarray(mean)[None, None]
        out.append(np.transpose(x, (2, 0, 1)))
    return torch.from_numpy(np.stack(out).astype(np.float32))


# ---- float64 restatements of the two kernels ----------------------------------------------------------------------------
def _normalise(c):
    return c / (c.norm(dim=1, keepdim=True) + 1e-9)


def warp64(x, flow):
    """WarpModule.forward (VCNplus.py:129-148): grid_sample(align_corners=True) of x at q + flow in x's dtype, zeroed unless
    |vgrid| < 1, the mask evaluated on the fp32 grid as the reference computes it."""
    B, C, H, W = x.shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=x.dtype, device=x.device), torch.arange(W, dtype=x.dtype, device=x.device),
                            indexing='ij')
    g = torch.stack((2.0 * (xx + flow[:, 0].to(x.dtype)) / max(W - 1, 1) - 1.0,
                     2.0 * (yy + flow[:, 1].to(x.dtype)) / max(H - 1, 1) - 1.0), -1)
    out = F.grid_sample(x, g, align_corners=True)
    # the mask in IEEE fp32 with a true division (numpy; torch on a GPU multiplies by the reciprocal of a scalar divisor)
    f32 = flow.detach().float().cpu().numpy()
    one, two = np.float32(1), np.float32(2)
    gx = two * (np.arange(W, dtype=np.float32)[None, None] + f32[:, 0]) / np.float32(max(W - 1, 1)) - one
    gy = two * (np.arange(H, dtype=np.float32)[None, :, None] + f32[:, 1]) / np.float32(max(H - 1, 1)) - one
    mask = torch.from_numpy((np.abs(gx) < 1) & (np.abs(gy) < 1)).to(x.device)
    return out * mask[:, None].to(x.dtype)


def corr_proj64(c1, c2, flow, weight, scale, shift, md, mdv, dtype=torch.float64):
    """-> [b, F, 2md+1, 2mdv+1, h, w] in `dtype`: scale * (W @ lrelu(c1n * shift_d(t))) + shift per displacement d, t = c2n at
    level 0 (flow None), else the masked warp of c2n."""
    c1, c2 = c1.to(dtype), c2.to(dtype)
    c1n, c2n = _normalise(c1), _normalise(c2)
    t = c2n if flow is None else warp64(c2n, flow)
    b, C, h, w = c1.shape
    Wm = weight.to(dtype).reshape(weight.shape[0], C)
    sc, sh = scale.to(dtype), shift.to(dtype)
    U, V = 2 * md + 1, 2 * mdv + 1
    out = torch.empty(b, Wm.shape[0], U, V, h, w, dtype=dtype, device=c1.device)
    for i in range(U):
        du = i - md
        for j in range(V):
            dv = j - mdv
            sh_t = torch.zeros_like(t)
            ys0, ys1 = max(0, -dv), min(h, h - dv)
            xs0, xs1 = max(0, -du), min(w, w - du)
            if ys1 > ys0 and xs1 > xs0:
                sh_t[:, :, ys0:ys1, xs0:xs1] = t[:, :, ys0 + dv:ys1 + dv, xs0 + du:xs1 + du]
            cost = F.leaky_relu(c1n * sh_t, 0.1)
            out[:, :, i, j] = torch.einsum('fc,bchw->bfhw', Wm, cost) * sc[None, :, None, None] + sh[None, :, None, None]
    return out


def flow_reg64(cost, up_flow, md, mdv, dtype=torch.float64):
    """flow_reg.forward (VCNplus.py:68-112, truncated, ent=True) + cost_matching's up-flow addition (:401-406) in `dtype`:
    cost [b, F, U, V, h, w] -> (flow [b, 2F, h, w], ent [b, 2F, h, w])."""
    b, Fh, U, V, h, w = cost.shape
    x = cost.to(dtype).reshape(b * Fh, U * V, h, w)
    idx = x.argmax(1, keepdim=True)
    onehot = torch.zeros_like(x).scatter_(1, idx, 1.).view(b * Fh, 1, U, V, h * w)
    mask = F.max_pool3d(onehot, (7, 7, 1), stride=1, padding=(3, 3, 0))[:, 0].view(b * Fh, U * V, h, w) > 0
    xm = torch.where(mask, x, torch.full_like(x, -math.inf))
    p = F.softmax(xm, 1).view(b * Fh, U, V, h, w)
    du = torch.arange(-md, md + 1, dtype=dtype, device=cost.device).view(1, U, 1, 1, 1)
    dv = torch.arange(-mdv, mdv + 1, dtype=dtype, device=cost.device).view(1, 1, V, 1, 1)
    fx = (p * du).sum((1, 2))
    fy = (p * dv).sum((1, 2))
    hl = (-p * p.clamp(1e-9, 1 - 1e-9).log()).sum((1, 2)) / math.log(49)
    pg = F.softmax(x, 1)
    hg = (-pg * pg.clamp(1e-9, 1 - 1e-9).log()).sum(1) / math.log(U * V)
    flow = torch.stack((fx, fy), 1).view(b, Fh, 2, h, w)
    if up_flow is not None:
        flow = flow + up_flow.to(dtype)[:, None]
    ent = torch.stack((hl, hg), 1).view(b, Fh, 2, h, w)
    return flow.reshape(b, 2 * Fh, h, w), ent.reshape(b, 2 * Fh, h, w)


def patch_vcn_matching(vcn_module, dtype=torch.float64):
    """Replace vcn.corr_proj / vcn.flow_reg by the restatements (results cast back to fp32) -> a function that undoes it."""
    saved = vcn_module.corr_proj, vcn_module.flow_reg

    def cp(c1, c2, flow, weight, scale, shift, md, mdv):
        return corr_proj64(c1, c2, flow, weight, scale, shift, md, mdv, dtype).float()

    def fr(cost, up_flow, md, mdv):
        f, e = flow_reg64(cost, up_flow, md, mdv, dtype)
        return f.float(), e.float()
    vcn_module.corr_proj, vcn_module.flow_reg = cp, fr

    def undo():
        vcn_module.corr_proj, vcn_module.flow_reg = saved
    return undo


# ---- the reference's shape of the matching stage (fp32, for the memory / time comparison) ---------------------------------
def corr_proj_reference_shaped(c1, c2, flow, weight, scale, shift, md, mdv):
    """cost_matching's normalisation and warp, corrf's slice-assigned [b, C, U, V, h, w] volume, LeakyReLU, projfeat4d's 1x1
    Conv3d and (folded) BatchNorm, in the reference's tensor shapes (VCNplus.py:350-394, conv4d.py:226-235)."""
    c1n, c2n = _normalise(c1), _normalise(c2)
    t = c2n if flow is None else warp64(c2n, flow)
    b, c, h, w = c1.shape
    cost = c1.new_zeros(b, c, 2 * md + 1, 2 * mdv + 1, h, w)
    for i in range(2 * md + 1):
        ind = i - md
        for j in range(2 * mdv + 1):
            indd = j - mdv
            feata = c1n[:, :, max(0, -indd):h - indd, max(0, -ind):w - ind]
            featb = t[:, :, max(0, indd):h + indd, max(0, ind):w + ind]
            cost[:, :, i, j, max(0, -indd):h - indd, max(0, -ind):w - ind] = feata * featb
    cost = F.leaky_relu(cost, 0.1, inplace=True)
    y = F.conv3d(cost.view(b, c, 2 * md + 1, 2 * mdv + 1, h * w), weight.view(weight.shape[0], c, 1, 1, 1))
    y = y * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    return y.view(b, -1, 2 * md + 1, 2 * mdv + 1, h, w)


def flow_reg_reference_shaped(cost, up_flow, md, mdv):
    """flow_reg.forward with its buffers, mask, max-pool, masking, softmaxes and sums (VCNplus.py:68-112), fp32."""
    b, Fh, U, V, h, w = cost.shape
    x = cost.reshape(b * Fh, U, V, h, w)
    oldx = x
    xv = x.view(b * Fh, U * V, h, w)
    idx = xv.argmax(1)[:, None]
    mask = torch.zeros_like(xv).scatter_(1, idx, 1).view(b * Fh, 1, U, V, -1)
    mask = F.max_pool3d(mask, (7, 7, 1), stride=1, padding=(3, 3, 0))[:, 0].view(b * Fh, U, V, h, w)
    x = torch.where(mask.bool(), oldx, torch.full_like(oldx, -math.inf))
    x = F.softmax(x.view(b * Fh, -1, h, w), 1).view(b * Fh, U, V, h, w)
    flowx = torch.arange(-md, md + 1, dtype=cost.dtype, device=cost.device).view(1, U, 1, 1, 1).expand(b * Fh, U, V, h, w)
    flowy = torch.arange(-mdv, mdv + 1, dtype=cost.dtype, device=cost.device).view(1, 1, V, 1, 1).expand(b * Fh, U, V, h, w)
    outx = torch.sum(torch.sum(x * flowx, 1), 1, keepdim=True)
    outy = torch.sum(torch.sum(x * flowy, 1), 1, keepdim=True)
    le = (-x * torch.clamp(x, 1e-9, 1 - 1e-9).log()).sum(1).sum(1)[:, None] / math.log(49)
    x = F.softmax(oldx.view(b * Fh, -1, h, w), 1).view(b * Fh, U, V, h, w)
    ge = (-x * torch.clamp(x, 1e-9, 1 - 1e-9).log()).sum(1).sum(1)[:, None] / math.log(U * V)
    flow = torch.cat([outx, outy], 1).view(b, Fh, 2, h, w)
    if up_flow is not None:
        flow = flow + up_flow[:, None]
    return flow.view(b, -1, h, w), torch.cat([le, ge], 1).view(b, -1, h, w)
