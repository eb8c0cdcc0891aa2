"""Guard-banded, poisoned allocations for the operator tests (imported by tests; no pytest hooks, no settings).

The wrappers of lasr_amd allocate outputs and scratch with torch.empty / torch.empty_like.  From the caching allocator such a
tensor is a recycled block rounded up to 512 bytes: a kernel that writes one element past its output lands in the slack, an
element nobody writes usually still holds the right answer of the previous call.  `guarded(fill)` swaps the `torch` global of
every loaded lasr_amd module for a proxy whose empty / empty_like carve the tensor out of the middle of a uint8 buffer

    | BAND bytes of `fill` | nbytes (also `fill`) | BAND bytes of `fill` |

so that the interior ends exactly at nbytes, a stray write shows in a band, and a value that depends on what memory held before
the call differs between two fills.  `run_case` runs a case plain, under 0xFF (floats NaN, ints -1) and under 0x7F (floats
3.4e38 / 1.4e306, ints 2139062143) and asserts

  a. no band of either guarded run was touched,
  b. the same bits in all three runs (exact=False: the same NaN / inf pattern and the borrowed tolerance),
  c. the run was not vacuous: a guarded allocation was made, the natives reached are exactly the declared ones, and some
     returned tensor holds more than one distinct value.

torch itself is never patched; the modules' globals are put back on exit, also after an exception."""
import contextlib
import sys
import types

import torch as _torch

BAND = 65536                                             # bytes on either side; a multiple of 512 keeps the allocator's alignment
assert BAND % 512 == 0
FILLS = (0xFF, 0x7F)


class Allocation:
    __slots__ = ('backing', 'nbytes', 'shape', 'dtype', 'ordinal')

    def __init__(self, backing, nbytes, shape, dtype, ordinal):
        self.backing, self.nbytes, self.shape, self.dtype, self.ordinal = backing, nbytes, shape, dtype, ordinal


def _size_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
        args = tuple(args[0])
    return tuple(int(a) for a in args)


class Guard:
    """State of one `guarded` block: the allocations made, the natives reached."""

    def __init__(self, fill, guard_cpu=False):
        self.fill, self.guard_cpu = int(fill), bool(guard_cpu)
        self.allocations, self.natives = [], []

    # -- allocation -----------------------------------------------------------------------------------------------------------
    def _wants(self, device, kw):
        if any(k not in ('dtype', 'device') for k in kw):
            return False
        if device is None:
            return self.guard_cpu
        return _torch.device(device).type == 'cuda' or self.guard_cpu

    def allocate(self, shape, dtype, device):
        dtype = dtype or _torch.get_default_dtype()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * _torch.empty((), dtype=dtype).element_size()
        backing = _torch.full((BAND + nbytes + BAND,), self.fill, dtype=_torch.uint8, device=device)
        self.allocations.append(Allocation(backing, nbytes, tuple(shape), dtype, len(self.allocations)))
        return backing[BAND:BAND + nbytes].view(dtype).view(shape)

    def empty(self, *size, **kw):
        if not self._wants(kw.get('device'), kw):
            return _torch.empty(*size, **kw)
        return self.allocate(_size_of(size), kw.get('dtype'), kw.get('device'))

    def empty_like(self, t, **kw):
        device = kw.get('device', t.device)
        if not self._wants(device, kw):
            return _torch.empty_like(t, **kw)
        return self.allocate(tuple(t.shape), kw.get('dtype', t.dtype), device)      # (contiguous, whatever t's strides are)

    # -- checks ---------------------------------------------------------------------------------------------------------------
    def violations(self):
        """[{ordinal, shape, dtype, side}] for every band that holds a byte other than the fill (synchronises the device)."""
        bad = []
        for a in self.allocations:
            for side, band in (('before', a.backing[:BAND]), ('after', a.backing[BAND + a.nbytes:])):
                if bool((band != self.fill).any()):
                    bad.append({'ordinal': a.ordinal, 'shape': a.shape, 'dtype': a.dtype, 'side': side})
        return bad


class _TorchProxy(types.ModuleType):
    """Forwards every attribute to torch except empty / empty_like (instance attributes set by `guarded`)."""

    def __getattr__(self, name):
        return getattr(_torch, name)


def _product_modules():
    return [m for n, m in list(sys.modules.items()) if m is not None and (n == 'lasr_amd' or n.startswith('lasr_amd.'))]


@contextlib.contextmanager
def guarded(fill, modules=None, lib=None, guard_cpu=False):
    """Context manager: see the module docstring.  modules: the modules to patch (default: every loaded lasr_amd.* module);
    lib: the object whose `call(name, ...)` launches natives (default: lasr_amd._lib); guard_cpu: guard CPU tensors too (the
    harness's own CPU test).  Yields the Guard."""
    if lib is None:
        from lasr_amd import _lib as lib
    g = Guard(fill, guard_cpu)
    proxy = _TorchProxy('torch')
    proxy.empty, proxy.empty_like = g.empty, g.empty_like
    real_call = lib.call

    def call(name, *args, **kw):
        g.natives.append(name)
        return real_call(name, *args, **kw)

    undo = []
    try:
        for m in (_product_modules() if modules is None else list(modules)):
            d = vars(m)
            if d.get('torch') is _torch:
                undo.append((d, 'torch', _torch))
                d['torch'] = proxy
            if d.get('call') is real_call:                 # `from .._lib import call`, and _lib itself
                undo.append((d, 'call', real_call))
                d['call'] = call
        if vars(lib).get('call') is real_call:
            undo.append((vars(lib), 'call', real_call))
            lib.call = call
        yield g
    finally:
        for d, k, v in reversed(undo):
            d[k] = v


class Case:
    """One row of the table: fn(device) -> flat tuple of tensors (inputs rebuilt from a fixed seed on every call), the natives it
    must reach, and whether its results are bit-reproducible.  exact=False needs the float atomic that feeds the result
    (`atomic`, 'file: kernel'), and the tolerance of the operator's own test (`tol`, relative to the largest magnitude of the
    tensor, and `tol_from`, the test it is borrowed from); `inexact`: the positions of the returned tuple the atomic feeds (the
    others stay bit-exact; default: every floating tensor)."""

    def __init__(self, name, fn, natives, exact=True, atomic=None, tol=None, tol_from=None, inexact=None):
        given = [atomic is not None, tol is not None, tol_from is not None]
        if exact and (any(given) or inexact is not None):
            raise ValueError('%s: exact=True takes none of atomic=, tol=, tol_from=, inexact=' % name)
        if not exact and not (all(given) and atomic and tol_from):
            raise ValueError('%s: exact=False needs atomic=, tol= and tol_from=' % name)
        self.name, self.fn, self.natives, self.exact = name, fn, frozenset(natives), bool(exact)
        self.atomic, self.tol, self.tol_from = atomic, tol, tol_from
        self.inexact = None if inexact is None else frozenset(inexact)      # positions of the returned tuple the atomic feeds

    def __repr__(self):
        return 'Case(%s)' % self.name


def _bits(t):
    flat = t.detach().reshape(-1)
    return _torch.empty(flat.shape, dtype=flat.dtype, device=flat.device).copy_(flat).view(_torch.uint8)   # (dense whatever t's strides)


def _flat(out):
    out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
    assert out and all(isinstance(t, _torch.Tensor) for t in out), 'a case returns a flat tuple of tensors'
    return tuple(t.detach() for t in out)


def _same(case, a, b, what):
    assert len(a) == len(b), '%s: %s: %d tensors against %d' % (case.name, what, len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        where = '%s: tensor %d %s %s, %s' % (case.name, i, tuple(x.shape), x.dtype, what)
        assert x.shape == y.shape and x.dtype == y.dtype, where + ': shape / dtype differ'
        if case.exact or not x.dtype.is_floating_point or (case.inexact is not None and i not in case.inexact):
            if not _torch.equal(_bits(x), _bits(y)):
                diff = (_bits(x) != _bits(y)).nonzero().reshape(-1)
                first = int(diff[0]) // max(x.element_size(), 1)
                assert False, '%s: bits differ in %d bytes, first at element %d: %r against %r' % (
                    where, diff.numel(), first, x.reshape(-1)[first].item(), y.reshape(-1)[first].item())
        else:
            xd, yd = x.double(), y.double()
            assert _torch.equal(_torch.isnan(xd), _torch.isnan(yd)) and _torch.equal(_torch.isinf(xd), _torch.isinf(yd)), \
                where + ': NaN / inf pattern differs'
            fin = _torch.isfinite(xd)
            if bool(fin.any()):
                err = float((xd[fin] - yd[fin]).abs().max())
                scale = max(float(yd[fin].abs().max()), 1e-30)
                assert err <= case.tol * scale, '%s: |difference| %.3e over %.3e * %.3e (%s)' % (where, err, case.tol, scale,
                                                                                                case.tol_from)


def run_case(case, device, modules=None, lib=None, guard_cpu=False):
    """Run the case plain and under both fills; assert rules a, b and c of the module docstring."""
    plain = _flat(case.fn(device))
    runs = []
    for fill in FILLS:
        with guarded(fill, modules=modules, lib=lib, guard_cpu=guard_cpu) as g:
            out = _flat(case.fn(device))
            bad = g.violations()
        # c. not vacuous
        assert g.allocations, '%s: no guarded allocation under fill 0x%02X' % (case.name, fill)
        assert frozenset(g.natives) == case.natives, '%s: natives reached %s, declared %s' % (
            case.name, sorted(set(g.natives)), sorted(case.natives))
        # a. bands intact
        assert not bad, '%s: fill 0x%02X: guard band touched: %s' % (case.name, fill, bad)
        runs.append(out)
    assert any(t.numel() > 1 and bool((t.reshape(-1) != t.reshape(-1)[0]).any()) for t in plain), \
        '%s: every returned tensor is constant' % case.name
    # b. same bits
    _same(case, runs[0], runs[1], 'fill 0xFF against fill 0x7F')
    _same(case, plain, runs[0], 'plain against fill 0xFF')
    _same(case, plain, runs[1], 'plain against fill 0x7F')
