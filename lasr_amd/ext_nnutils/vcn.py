"""VCN optical flow, inference path (reference: third_party/ext_nnutils/VCNplus.py `VCN`, submodule.py `pspnet`, conv4d.py
`butterfly4D`, `sepConv4d`, `sepConv4dBlock`, `projfeat4d`), for preprocess/auto_gen.py.

The feature pyramid, the separable 4-D convolutions, the trilinear upsamplings of butterfly4D, the hypothesis fusion and the
final upsampling run in torch.  Matching runs on two HIP kernels (csrc/vcn.hip): `corr_proj` replaces normalisation, warp,
the cost volume, LeakyReLU and butterfly4D's 1x1 projection with BatchNorm; `flow_reg` replaces the truncated soft-argmin and
the entropies.  There is no torch matching path here: a missing kernel is an error.  Nothing depends on the input size (the
reference rebuilds flow_reg and WarpModule per size, auto_gen.py:109-116).

Module and parameter names follow the reference, so a `vcn_rob.pth` state_dict loads (`load_checkpoint`); the modules the
inference path does not use (training-only warps, the out-of-range heads of levels 0-3) are left out.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib

MAX_DISP = 7                     # LASR_VCN_MAX_DISP (include/lasr_ops.h)


# ---- the two matching kernels ---------------------------------------------------------------------------------------------
def fold_bn(bn):
    """BatchNorm in eval mode as (scale, shift): y = x * scale + shift."""
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias - bn.running_mean * scale


def corr_proj(c1, c2, flow, weight, scale, shift, md, mdv):
    """c1, c2 [b,C,h,w]; flow [b,2,h,w] or None (level 0); weight [F,C]; scale, shift [F] -> [b,F,2md+1,2mdv+1,h,w] fp32:
    projfeat4d(LeakyReLU(corrf(c1n, warp(c2n, flow)))) with BatchNorm folded (lasr_vcn_corr_proj)."""
    _lib.need_cuda(c1, c2, flow, weight)
    b, C, h, w = c1.shape
    Fo = weight.shape[0]
    if c2.shape != c1.shape or weight.shape != (Fo, C) or (flow is not None and flow.shape != (b, 2, h, w)):
        raise ValueError('corr_proj: c1 %s, c2 %s, flow %s, weight %s' % (tuple(c1.shape), tuple(c2.shape),
                                                                          None if flow is None else tuple(flow.shape),
                                                                          tuple(weight.shape)))
    f32 = dict(dtype=torch.float32, device=c1.device)
    c1, c2 = c1.to(**f32).contiguous(), c2.to(**f32).contiguous()
    flow = None if flow is None else flow.to(**f32).contiguous()
    weight, scale, shift = (t.detach().to(**f32).contiguous() for t in (weight, scale, shift))
    out = torch.empty(b, Fo, 2 * md + 1, 2 * mdv + 1, h, w, **f32)
    ws = torch.empty(max(int(_lib.lib().lasr_vcn_corr_proj_workspace_bytes(b, h, w)), 4) // 4, **f32)
    _lib.call('lasr_vcn_corr_proj', c1, c2, flow, weight, scale, shift, out, ws, ws.numel() * 4, b, C, Fo, h, w, int(md), int(mdv))
    return out


def flow_reg(cost, up_flow, md, mdv):
    """cost [b,F,2md+1,2mdv+1,h,w]; up_flow [b,2,h,w] or None -> (flow [b,2F,h,w], ent [b,2F,h,w]) as flow_reg.forward
    followed by cost_matching's `+ up_flow` and views (VCNplus.py:399-406) (lasr_vcn_flow_reg)."""
    _lib.need_cuda(cost, up_flow)
    b, Fo, U, V, h, w = cost.shape
    if U != 2 * md + 1 or V != 2 * mdv + 1 or (up_flow is not None and up_flow.shape != (b, 2, h, w)):
        raise ValueError('flow_reg: cost %s for md %d, mdv %d' % (tuple(cost.shape), md, mdv))
    f32 = dict(dtype=torch.float32, device=cost.device)
    cost = cost.to(**f32).contiguous()
    up_flow = None if up_flow is None else up_flow.to(**f32).contiguous()
    flow = torch.empty(b, 2 * Fo, h, w, **f32)
    ent = torch.empty(b, 2 * Fo, h, w, **f32)
    _lib.call('lasr_vcn_flow_reg', cost, up_flow, flow, ent, b, Fo, h, w, int(md), int(mdv))
    return flow, ent


# ---- building blocks (names as in the reference's state_dict) --------------------------------------------------------------
def _lrelu():
    return nn.LeakyReLU(0.1, inplace=True)


def conv(cin, cout, k=3, stride=1, padding=1, dilation=1):
    """Conv2d with bias, BatchNorm, LeakyReLU(0.1) (submodule.py:68-73)."""
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, padding, dilation, bias=True), nn.BatchNorm2d(cout), _lrelu())


class CBR(nn.Module):
    """conv2DBatchNormRelu / conv2DBatchNorm (submodule.py:76-122): bias-free conv, BatchNorm, optional LeakyReLU."""

    def __init__(self, cin, cout, k, stride, padding, dilation=1, relu=True):
        super().__init__()
        layers = [nn.Conv2d(cin, cout, k, stride, padding, dilation, bias=False), nn.BatchNorm2d(cout)]
        if relu:
            layers.append(_lrelu())
        seq = nn.Sequential(*layers)
        setattr(self, 'cbr_unit' if relu else 'cb_unit', seq)
        self._seq = [seq]

    def forward(self, x):
        return self._seq[0](x)


class ResBlock(nn.Module):
    """residualBlock with a strided 1x1 downsample (submodule.py:37-66)."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.convbnrelu1 = CBR(cin, cout, 3, stride, 1)
        self.convbn2 = CBR(cout, cout, 3, 1, 1, relu=False)
        self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))
        self.relu = _lrelu()

    def forward(self, x):
        return self.relu(self.convbn2(self.convbnrelu1(x)) + self.downsample(x))


class PyramidPooling(nn.Module):
    """pyramidPooling with 3 levels (submodule.py:124-156)."""

    def __init__(self, ch, levels=3):
        super().__init__()
        self.levels = levels
        self.path_module_list = nn.ModuleList([CBR(ch, ch, 1, 1, 0) for _ in range(levels)])
        self.relu = _lrelu()

    def forward(self, x):
        h, w = x.shape[2:]
        sizes = [(int(h / s), int(w / s)) for s in np.linspace(1, min(h, w) // 2, self.levels, dtype=int)][::-1]
        acc = x
        for k, path in zip(sizes, self.path_module_list):
            y = path(F.avg_pool2d(x, k, stride=k, padding=0))
            acc = acc + 1. / self.levels * F.interpolate(y, size=(h, w), mode='bilinear', align_corners=False)
        return self.relu(acc / 2.)


class PSPNet(nn.Module):
    """The feature pyramid (submodule.py:158-271, is_proj=False): features at 1/64, 1/32, 1/16, 1/8, 1/4."""

    def __init__(self):
        super().__init__()
        self.convbnrelu1_1 = CBR(3, 16, 3, 2, 1)
        self.convbnrelu1_2 = CBR(16, 16, 3, 1, 1)
        self.convbnrelu1_3 = CBR(16, 32, 3, 1, 1)
        self.res_block3 = nn.Sequential(ResBlock(32, 64, 2))
        self.res_block5 = nn.Sequential(ResBlock(64, 128, 2))
        self.res_block6 = nn.Sequential(ResBlock(128, 128, 2))
        self.res_block7 = nn.Sequential(ResBlock(128, 128, 2))
        self.pyramid_pooling = PyramidPooling(128)
        # upconvN.0 is the reference's unused nn.Upsample; its conv sits at index 1
        self.upconv6 = nn.Sequential(nn.Identity(), CBR(128, 64, 3, 1, 1))
        self.iconv5 = CBR(192, 128, 3, 1, 1)
        self.upconv5 = nn.Sequential(nn.Identity(), CBR(128, 64, 3, 1, 1))
        self.iconv4 = CBR(192, 128, 3, 1, 1)
        self.upconv4 = nn.Sequential(nn.Identity(), CBR(128, 64, 3, 1, 1))
        self.iconv3 = CBR(128, 64, 3, 1, 1)
        self.upconv3 = nn.Sequential(nn.Identity(), CBR(64, 32, 3, 1, 1))
        self.iconv2 = CBR(64, 64, 3, 1, 1)

    @staticmethod
    def _up(x, like):
        return F.interpolate(x, size=like.shape[2:], mode='bilinear', align_corners=False)

    def forward(self, x):
        pool1 = F.max_pool2d(self.convbnrelu1_3(self.convbnrelu1_2(self.convbnrelu1_1(x))), 3, 2, 1)
        r3 = self.res_block3(pool1)
        r4 = self.res_block5(r3)
        r5 = self.res_block6(r4)
        c6 = self.pyramid_pooling(self.res_block7(r5))
        c5 = self.iconv5(torch.cat((r5, self.upconv6[1](self._up(c6, r5))), 1))
        c4 = self.iconv4(torch.cat((r4, self.upconv5[1](self._up(c5, r4))), 1))
        c3 = self.iconv3(torch.cat((r3, self.upconv4[1](self._up(c4, r3))), 1))
        c2 = self.iconv2(torch.cat((pool1, self.upconv3[1](self._up(c3, pool1))), 1))
        return c6, c5, c4, c3, c2


class Proj4d(nn.Module):
    """projfeat4d (conv4d.py:226-235): 1x1x1 Conv3d over (u, v, h*w) with stride (s, s, 1), no bias, then BatchNorm3d."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.stride = stride
        self.conv1 = nn.Conv3d(cin, cout, 1, (stride, stride, 1), padding=0, bias=False)
        self.bn = nn.BatchNorm3d(cout)

    def forward(self, x):
        b, c, u, v, h, w = x.shape
        y = self.bn(self.conv1(x.reshape(b, c, u, v, h * w)))
        return y.view(b, -1, y.shape[2], y.shape[3], h, w)


class Sep4d(nn.Module):
    """sepConv4d (conv4d.py:237-289) for in == out channels: a (k,k,1) Conv3d over (u, v) with stride s, ReLU, then a (1,k,k)
    Conv3d over (h, w), strided as well when `full`; each with BatchNorm (bn=True) or a bias."""

    def __init__(self, ch, stride=1, bn=True, k=3, full=True):
        super().__init__()
        p = k // 2

        def unit(kernel, strd, pad):
            c3 = nn.Conv3d(ch, ch, kernel, stride=strd, padding=pad, bias=not bn)
            return nn.Sequential(c3, nn.BatchNorm3d(ch)) if bn else c3
        self.conv1 = unit((1, k, k), (1, stride, stride) if full else 1, (0, p, p))
        self.conv2 = unit((k, k, 1), (stride, stride, 1), (p, p, 0))

    def forward(self, x):
        b, c, u, v, h, w = x.shape
        x = F.relu(self.conv2(x.reshape(b, c, u, v, h * w)))
        u, v = x.shape[2], x.shape[3]
        x = self.conv1(x.reshape(b, c, u * v, h, w))
        return x.view(b, c, u, v, x.shape[3], x.shape[4])


class Sep4dBlock(nn.Module):
    """sepConv4dBlock (conv4d.py:292-321): residual pair of Sep4d, strided shortcut when stride > 1."""

    def __init__(self, ch, stride, full):
        super().__init__()
        if stride == 1:
            self.downsample = None
        elif full:
            self.downsample = Sep4d(ch, stride, k=1, full=True)
        else:
            self.downsample = Proj4d(ch, ch, stride)
        self.conv1 = Sep4d(ch, stride, full=full)
        self.conv2 = Sep4d(ch, 1, full=full)

    def forward(self, x):
        out = F.relu(self.conv1(x))
        if self.downsample is not None:
            x = self.downsample(x)
        return F.relu(x + self.conv2(out))


class Butterfly4d(nn.Module):
    """butterfly4D (conv4d.py:152-195).  Its first step, proj (Proj4d + ReLU), is taken by the corr_proj kernel; `forward`
    starts from that step's output."""

    def __init__(self, cin, ch, full):
        super().__init__()
        self.proj = nn.Sequential(Proj4d(cin, ch, 1), nn.ReLU(inplace=True))
        self.conva1 = Sep4dBlock(ch, 2, full)
        self.conva2 = Sep4dBlock(ch, 2, full)
        self.convb3 = Sep4dBlock(ch, 1, full)
        self.convb2 = Sep4dBlock(ch, 1, full)
        self.convb1 = Sep4dBlock(ch, 1, full)

    def projection(self):
        """(weight [F,C], scale [F], shift [F]) of proj's conv and folded BatchNorm."""
        p = self.proj[0]
        scale, shift = fold_bn(p.bn)
        return p.conv1.weight.reshape(p.conv1.weight.shape[0], -1), scale, shift

    @staticmethod
    def _resize(x, u, v, h, w):
        """The two trilinear upsamplings of butterfly4D.forward: (u, v) first, then (h, w)."""
        b, c, u0, v0, h0, w0 = x.shape
        x = F.interpolate(x.reshape(b, c, u0, v0, h0 * w0), (u, v, h0 * w0), mode='trilinear', align_corners=False)
        x = F.interpolate(x.reshape(b, c, u * v, h0, w0), (u * v, h, w), mode='trilinear', align_corners=False)
        return x.view(b, c, u, v, h, w)

    def forward(self, out):
        out1 = self.conva1(out)
        out2 = self.convb3(self.conva2(out1))
        out1 = self.convb2(self._resize(out2, *out1.shape[2:]) + out1)
        return self.convb1(self._resize(out1, *out.shape[2:]) + out)


def _head(cin, cout):
    """The dilated 7-layer stack of the dc* fusion and out-of-range heads (VCNplus.py:214-333)."""
    return [conv(cin, 128, 3, 1, 1, 1), conv(128, 128, 3, 1, 2, 2), conv(128, 128, 3, 1, 4, 4), conv(128, 96, 3, 1, 8, 8),
            conv(96, 64, 3, 1, 16, 16), conv(64, 32, 3, 1, 1, 1), nn.Conv2d(32, cout, 3, 1, 1, bias=True)]


class VCN(nn.Module):
    """VCN inference: forward(im [2b,3,H,W], H and W multiples of 64) -> (flow [b,2,H,W], occ [H/4, W/4]) of the first pair,
    as VCNplus.py:513-543.  md: the per-level search radius (md[0] = int(4 * maxdisp / 256)); fac squeezes level 0 along y."""

    LEVELS = ('6', '5', '4', '3', '2')

    def __init__(self, md=(4, 4, 4, 4, 4), fac=1.):
        super().__init__()
        if not all(1 <= int(m) <= MAX_DISP for m in md):
            raise ValueError('VCN: search radii %s outside [1, %d] (LASR_VCN_MAX_DISP)' % (tuple(md), MAX_DISP))
        self.md = [int(m) for m in md]
        self.facs = [fac, 1, 1, 1, 1]
        self.pspnet = PSPNet()
        fa = (128, 128, 128, 64, 64)
        fb = (16, 16, 16, 16, 12)
        for i, lv in enumerate(self.LEVELS):
            full = i == 4
            setattr(self, 'f' + lv, Butterfly4d(fa[i], fb[i], full))
            setattr(self, 'p' + lv, Sep4d(fb[i], 1, bn=False, full=full))
        # fusion heads dc<l>_conv1..7: inputs are entropies, flows (2 channels each per hypothesis) and c1
        cins = (128 + 4 * 16, 128 + 8 * 16, 128 + 12 * 16, 64 + 16 * 16, 64 + 16 * 16 + 4 * 12)
        couts = (2 * 16, 4 * 16, 6 * 16, 8 * 16, 8 * 16 + 2 * 12)
        for lv, cin, cout in zip(self.LEVELS, cins, couts):
            for k, m in enumerate(_head(cin, cout)):
                setattr(self, 'dc%s_conv%d' % (lv, k + 1), m)
        self.dc2_convo = nn.Sequential(*_head(cins[4], 1))
        self.register_buffer('mean_L', torch.full((1, 3), 0.33), persistent=False)
        self.register_buffer('mean_R', torch.full((1, 3), 0.33), persistent=False)

    def _fuse(self, lv, x):
        for k in range(1, 8):
            x = getattr(self, 'dc%s_conv%d' % (lv, k))(x)
        return x

    def mdv(self, level):
        return int(self.md[level] // self.facs[level])

    def cost_matching(self, up_flow, c1, c2, flowh, enth, level):
        """VCNplus.py:375-427 in eval mode -> (flow, flowh, enth, oor or None)."""
        lv = self.LEVELS[level]
        md, mdv = self.md[level], self.mdv(level)
        bfly, post = getattr(self, 'f' + lv), getattr(self, 'p' + lv)
        w, scale, shift = bfly.projection()
        feat = F.relu_(corr_proj(c1, c2, up_flow, w, scale, shift, md, mdv))
        cost = post(bfly(feat))
        flowhh, enthh = flow_reg(cost, up_flow, md, mdv)
        if level == 0:
            flowh, enth = flowhh, enthh
        else:
            size = flowhh.shape[2:]
            flowh = torch.cat((flowhh, F.interpolate(flowh * 2, size, mode='bilinear', align_corners=False)), 1)
            enth = torch.cat((enthh, F.interpolate(enth, size, mode='bilinear', align_corners=False)), 1)
        x = torch.cat((enth, flowh, c1), 1)
        oor = self.dc2_convo(x)[:, 0] if level == 4 else None
        va = self._fuse(lv, x)
        b, _, h, w_ = flowh.shape
        va = va.view(b, -1, 2, h, w_)
        flow = (flowh.view(b, -1, 2, h, w_) * F.softmax(va, 1)).sum(1)
        return flow, flowh, enth, oor

    def forward(self, im, return_levels=False):
        bs = im.shape[0] // 2
        H, W = im.shape[2], im.shape[3]
        if H % 64 or W % 64:
            raise ValueError('VCN takes images padded to multiples of 64, got %dx%d' % (H, W))
        feats = self.pspnet(im)
        flow = flowh = enth = None
        levels = []
        for level, c in enumerate(feats):
            up = None
            if level > 0:
                up = F.interpolate(flow, [H // 2 ** (6 - level), W // 2 ** (6 - level)], mode='bilinear',
                                   align_corners=False) * 2
            flow, flowh, enth, oor = self.cost_matching(up, c[:bs], c[bs:], flowh, enth, level)
            levels.append((flow, flowh, enth))
        flow2 = F.interpolate(flow, [H, W], mode='bilinear', align_corners=False) * 4
        if return_levels:
            return flow2, oor[0], levels
        return flow2, oor[0]


def load_checkpoint(model, path_or_dict, verbose=True):
    """Load a VCN checkpoint ({'state_dict', 'mean_L', 'mean_R'}, keys optionally prefixed with 'module.') non-strictly, as
    auto_gen.py:64-69 does, and print how many keys were missing and unexpected.  -> (missing, unexpected) key lists."""
    ck = torch.load(path_or_dict, map_location='cpu') if isinstance(path_or_dict, str) else path_or_dict
    sd = ck.get('state_dict', ck)
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    res = model.load_state_dict(sd, strict=False)
    for name in ('mean_L', 'mean_R'):
        if name in ck:
            val = torch.as_tensor(np.asarray(ck[name], np.float32)).reshape(-1, 3)
            getattr(model, name).copy_(val.mean(0, keepdim=True))
    if verbose:
        print('VCN checkpoint: %d missing keys, %d unexpected keys' % (len(res.missing_keys), len(res.unexpected_keys)))
    return res.missing_keys, res.unexpected_keys
