"""Training monitor of optimize.py --monitor (reference: the tensorboard calls of nnutils/train_utils.py:301-355).

Once per epoch `images` composes the reference's nine pictures into one 3 x 3 contact sheet on the device (lasr_monitor_sheet: one
statistics launch, one compose launch) and copies its bytes to the host once; every step `push` averages the step's loss and
gradient-norm scalars into a ring in device memory (lasr_scalar_ring_push: one launch, no host read); `flush` drains the ring into
`scalars.csv` at the end of an epoch.  DESIGN.md section 4.10 holds the definitions.
"""
import ctypes
import os

import numpy as np
import torch

from .. import _lib, synth

SHEET_PANELS = ('flowobs', 'flowrd', 'flow_error', 'mask', 'maskgt', 'part', 'img1', 'img2', 'texture')


def scalar_names(opts):
    """Columns of scalars.csv, in the reference's logging order (:330-344)."""
    names = ['total_loss', 'mask_loss', 'flow_rd_loss', 'texture_loss']
    if opts.n_hypo > 1:
        for h in range(opts.n_hypo):
            names += ['mask_hypo_%d' % h, 'flow_hypo_%d' % h, 'tex_hypo_%d' % h]
    names.append('triangle_loss')
    if opts.n_bones > 1:
        names.append('lmotion_loss')
    return names + ['grad_meanv_norm', 'grad_cam_norm']


def write_scalar_rows(path, names, steps, rows):
    """Append `step,name=value,...` lines (float32 values, %.9g: they read back bit for bit); a new file opens with the header
    `step,<names>`."""
    new = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, 'a') as fh:
        if new:
            fh.write('step,' + ','.join(names) + '\n')
        for step, row in zip(steps, rows):
            fh.write('%d,' % step + ','.join('%s=%.9g' % (n, v) for n, v in zip(names, row)) + '\n')


def read_scalar_rows(path):
    """-> (names, steps [n] int64, values [n, len(names)] float32) of a scalars.csv."""
    with open(path) as fh:
        lines = [ln.strip() for ln in fh if ln.strip()]
    head = lines[0].split(',')
    if head[0] != 'step':
        raise ValueError('%s: no header line' % path)
    names = head[1:]
    steps, vals = [], []
    for ln in lines[1:]:
        cells = ln.split(',')
        got = dict(c.split('=', 1) for c in cells[1:])
        if list(got) != names:
            raise ValueError('%s: row %r does not carry the header\'s columns' % (path, ln))
        steps.append(int(cells[0]))
        vals.append([np.float32(got[n]) for n in names])
    return names, np.asarray(steps, np.int64), np.asarray(vals, np.float32).reshape(len(steps), len(names))


def _plane(t, chan_dim=None):
    """lasr_sheet_plane of a float32 device tensor whose last two dimensions (or, with a trailing channel dimension, the two before
    it) are the image: planar [C,IS,IS] / [IS,IS] (chan_dim=0 / None) or interleaved [IS,IS,C] (chan_dim=-1); views pass as they
    are as long as the image's rows are dense."""
    if t is None:
        return _lib.SheetPlane(None, 0, 0), None
    if t.dtype != torch.float32:
        t = t.float()
    if chan_dim == -1:
        rows, cols, cs = t.stride(0), t.stride(1), t.stride(2)
    elif chan_dim == 0:
        cs, rows, cols = t.stride(0), t.stride(1), t.stride(2)
    else:
        cs, rows, cols = 0, t.stride(0), t.stride(1)
    if rows != cols * t.shape[-2 if chan_dim == -1 else -1]:
        t = t.contiguous()
        return _plane(t, chan_dim)
    return _lib.SheetPlane(t.data_ptr(), cs, cols), t


def sheet(planes, ctl, palette, IS, scratch):
    """lasr_monitor_sheet on prepared tensors.  planes: dict name -> (tensor, chan_dim) for flow_obs, flow_rd (2 channels),
    vis_mask, flow_err, mask_pred, mask_gt (1), part (3 or None), img1, img2, texture (3); ctl [n,>=2] / palette [n,3] float32 or
    None.  -> uint8 [3 IS, 3 IS, 3] on the device."""
    keep, inp = [], _lib.SheetInputs()
    for name, _ in _lib.SheetInputs._fields_[:10]:
        t, cd = planes[name]
        p, t = _plane(t, cd)
        setattr(inp, name, p)
        keep.append(t)
    dev = scratch.device
    if ctl is not None and ctl.shape[0] > 0:
        ctl = ctl.detach().float().contiguous()
        palette = palette.float().contiguous()
        inp.ctl, inp.palette, inp.n_ctl, inp.ctl_stride = ctl.data_ptr(), palette.data_ptr(), ctl.shape[0], ctl.shape[1]
    out = torch.empty(3 * IS, 3 * IS, 3, dtype=torch.uint8, device=dev)
    _lib.call('lasr_monitor_sheet', ctypes.byref(inp), out, scratch, IS)
    return out


class ScalarRing:
    """[capacity, K] float32 means in device memory, filled by one launch per push; tables of (address, count) rows are cached per
    address set, like the fused tail's (train_utils._tail_table): the captured graphs of --use_graph keep their outputs at
    different addresses, eager steps get theirs from the caching allocator."""

    def __init__(self, K, capacity, device):
        h = _lib.lib()
        if h.lasr_scalar_ring_bytes(capacity, K) == 0:
            raise ValueError('ScalarRing: capacity %r / %r scalars out of range' % (capacity, K))
        self.K, self.capacity, self.device = K, capacity, device
        self.ring = torch.zeros(capacity, K, dtype=torch.float32, device=device)
        self.head = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.empty(capacity, K, dtype=torch.float32).pin_memory()
        self.pushed = 0                                   # host mirror of the device head
        self._tables = {}

    def table(self, tensors):
        """Device table for these K tensors (None = no value this step: NaN)."""
        rows = tuple((t.data_ptr(), t.numel()) if t is not None else (0, 0) for t in tensors)
        tab = self._tables.get(rows)
        if tab is None:
            for t in tensors:
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.ring.device):
                    raise TypeError('ScalarRing: scalars are contiguous float32 tensors on the ring\'s device')
            if len(self._tables) > 16:
                self._tables.clear()                      # addresses keep changing (eager steps): bounded
            tab = self._tables[rows] = torch.tensor(rows, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
        return tab

    def push(self, tensors):
        if len(tensors) != self.K:
            raise ValueError('ScalarRing.push: %d tensors for %d columns' % (len(tensors), self.K))
        tab = self.table(tensors)
        _lib.call('lasr_scalar_ring_push', tab, self.K, self.ring, self.head, self.capacity)
        self.pushed += 1

    def drain(self, since):
        """Rows of pushes since .. pushed - 1 (at most `capacity` of them, oldest first) as float32 numpy: one device-to-host
        copy of the ring and one stream synchronisation."""
        n = self.pushed - since
        if n <= 0:
            return np.zeros((0, self.K), np.float32)
        if n > self.capacity:
            raise ValueError('ScalarRing.drain: %d rows asked of a ring of %d' % (n, self.capacity))
        self.host.copy_(self.ring, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        a = self.host.numpy()
        return np.stack([a[i % self.capacity] for i in range(since, self.pushed)]).copy()


class TrainMonitor:
    def __init__(self, dir, opts, device, capacity=256):
        if torch.device(device).type != 'cuda':
            raise RuntimeError('--monitor needs a HIP device (the contact sheet and the scalar ring are device kernels)')
        self.dir, self.opts, self.device = dir, opts, torch.device(device)
        os.makedirs(dir, exist_ok=True)
        self.names = scalar_names(opts)
        self.ring = ScalarRing(len(self.names), capacity, self.device)
        self.csv = os.path.join(dir, 'scalars.csv')
        if os.path.exists(self.csv):
            os.remove(self.csv)                           # a run's file starts with its header
        self.flushed, self.steps = 0, []
        self.scratch = torch.zeros(_lib.lib().lasr_monitor_sheet_scratch_bytes() // 4, dtype=torch.int32, device=self.device)
        self.palette = torch.from_numpy(synth.label_palette(max(opts.n_bones - 1, 1))).to(self.device)
        self.host_sheet = None

    # ---- once per epoch ---------------------------------------------------------------------------------------------------
    def sheet(self, module, aux, optim_cam):
        """The epoch's contact sheet as a uint8 device tensor [3 IS, 3 IS, 3] (train_utils.py:303-329)."""
        o = self.opts
        IS, H, B = o.img_size, o.n_hypo, o.batch_size
        flow_rd = aux['flow_rd'].view(2 * B, H, IS, IS, 2)[0, optim_cam]
        part = aux.get('part_render') if o.n_bones > 1 else None
        planes = dict(flow_obs=(module.flow[0, :2], 0), flow_rd=(flow_rd, -1), vis_mask=(aux['vis_mask'][0, optim_cam], None),
                      flow_err=(aux['flow_rd_map'][0, optim_cam], None), mask_pred=(aux['mask_pred'][optim_cam], None),
                      mask_gt=(module.masks[0], None), part=(part[0] if part is not None else None, 0),
                      img1=(module.imgs[0], 0), img2=(module.imgs[B], 0), texture=(aux['texture_render'][optim_cam], 0))
        planes = {k: (t.detach() if t is not None else None, cd) for k, (t, cd) in planes.items()}
        ctl = aux['ctl_proj'][optim_cam] if (o.n_bones > 1 and 'ctl_proj' in aux) else None
        return sheet(planes, ctl, self.palette, IS, self.scratch)

    def images(self, epoch, module, aux, optim_cam):
        from PIL import Image
        dev_sheet = self.sheet(module, aux, optim_cam)
        if self.host_sheet is None or self.host_sheet.shape != dev_sheet.shape:
            self.host_sheet = torch.empty(dev_sheet.shape, dtype=torch.uint8).pin_memory()
        self.host_sheet.copy_(dev_sheet, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        path = os.path.join(self.dir, 'epoch-%04d.png' % epoch)
        Image.fromarray(self.host_sheet.numpy()).save(path)
        return path

    # ---- every step -------------------------------------------------------------------------------------------------------
    def push(self, aux, trainer, step=None):
        if self.ring.pushed - self.flushed >= self.ring.capacity:
            self.flush()                                  # ring full: drain before the oldest row is overwritten
        vals = []
        for n in self.names:
            v = aux.get(n)
            if v is None and n.startswith('grad_'):
                v = getattr(trainer, n, None)
            vals.append(v.detach() if torch.is_tensor(v) and v.is_cuda else None)
        self.ring.push(vals)
        self.steps.append(len(self.steps) + self.flushed if step is None else step)

    def flush(self):
        rows = self.ring.drain(self.flushed)
        write_scalar_rows(self.csv, self.names, self.steps, rows)
        self.flushed += len(rows)
        self.steps = []
