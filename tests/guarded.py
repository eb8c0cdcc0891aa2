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

Inputs come from the case, not from a wrapper: ordinary caching-allocator blocks, rounded up, with the same stale slack in all
three runs.  `guarded(fill, relocate=True)` therefore also moves every tensor ARGUMENT of a native that is not one of the
Guard's own allocations, at the call boundary: the bytes the argument can address (its span: data_ptr() and
(1 + sum (size_i - 1) * stride_i) * itemsize, from its own shape and strides, so a view is tight) are copied into

    | BAND bytes of `fill` (+ the address's residue) | span | BAND bytes of `fill` |

whose first byte keeps the original address modulo 256 (the kernels that choose a 16-byte or a scalar form from the pointer take
the path they took in the plain run), the native gets a tensor of the same dtype, shape and strides over the copy, and the bytes
that changed are copied back afterwards (in/out buffers).  Arguments of one call whose spans overlap or touch in one storage move
as one block; the same span gets the same block again for the whole `guarded` block, refreshed before each call.  `run_relocated`
is run_case with relocate=True and the bands of the inputs among those of rule a.

torch itself is never patched; the modules' globals are put back on exit, also after an exception."""
import contextlib
import ctypes
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


class Block:
    """One relocated span: backing[lead:lead + nbytes] holds a copy of the bytes start .. start + nbytes of the original."""
    __slots__ = ('backing', 'lead', 'start', 'nbytes', 'native', 'arg')

    def __init__(self, backing, lead, start, nbytes, native, arg):
        self.backing, self.lead, self.start, self.nbytes, self.native, self.arg = backing, lead, start, nbytes, native, arg

    def span(self):
        return self.backing[self.lead:self.lead + self.nbytes]


class RelocationError(AssertionError):
    """An argument that cannot follow its tensor to the relocated copy (a pointer computed by hand)."""


def span_bytes(t):
    """Bytes a tensor can address from its data_ptr(): (1 + sum (size_i - 1) * stride_i) * itemsize."""
    return (1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))) * t.element_size()


def _alias(storage, device, offset, nbytes):
    """A fresh uint8 tensor over bytes offset .. offset + nbytes of an untyped storage: writing through it bumps no version counter
    of the tensors that share the storage (save_for_backward holds some of them)."""
    return _torch.empty(0, dtype=_torch.uint8, device=device).set_(storage, offset, (nbytes,), (1,))


class Guard:
    """State of one `guarded` block: the allocations made, the natives reached, the inputs relocated."""

    def __init__(self, fill, guard_cpu=False, relocate=False):
        self.fill, self.guard_cpu, self.relocate = int(fill), bool(guard_cpu), bool(relocate)
        self.allocations, self.natives = [], []
        self.blocks = {}                                     # (device, start, nbytes) of the original span -> Block
        self.relocated = {}                                  # native -> {'args': tensor arguments moved, 'bytes': bytes copied in}
        self._own = set()                                    # addresses of the storages behind self.allocations

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
        self._own.add(backing.untyped_storage().data_ptr())
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

    # -- relocation of the tensor arguments of one native ------------------------------------------------------------------------
    def _is_input(self, t):
        if t.numel() == 0 or (t.device.type != 'cuda' and not self.guard_cpu):
            return False
        return t.untyped_storage().data_ptr() not in self._own

    def _block(self, device, start, nbytes, native, arg):
        key = (device, start, nbytes)
        b = self.blocks.get(key)
        if b is None:
            align = 256 if device.type == 'cuda' else 64
            lead = BAND + start % align                      # the span's first byte keeps the original address modulo `align`
            backing = _torch.full((lead + nbytes + BAND,), self.fill, dtype=_torch.uint8, device=device)
            assert backing.data_ptr() % align == 0 and backing.storage_offset() == 0, \
                'a backing buffer of %s at 0x%x is not %d-byte aligned' % (device, backing.data_ptr(), align)
            assert (backing.data_ptr() + lead - start) % align == 0
            b = self.blocks[key] = Block(backing, lead, start, nbytes, native, arg)
        return b

    def _refuse_pointers(self, name, pos, values):
        for v in values:
            if v is None or v < 2 ** 32:
                continue
            for b in self.blocks.values():
                if b.start <= v < b.start + b.nbytes:
                    raise RelocationError('%s: argument %d holds the integer 0x%x, an address inside a tensor that was relocated '
                                          '(argument %d of %s): a pointer computed by hand does not follow the copy'
                                          % (name, pos, v, b.arg, b.native))
            for a in self.allocations:
                if a.backing.data_ptr() <= v < a.backing.data_ptr() + a.backing.numel():
                    raise RelocationError('%s: argument %d holds the integer 0x%x, an address inside guarded allocation %d: pass '
                                          'the tensor, not a pointer computed by hand' % (name, pos, v, a.ordinal))

    def call(self, real_call, name, args, kw):
        """real_call(name, *args, **kw) with every input tensor among args (and among the `.tensors` of a ctypes pointer array,
        lasr_amd._lib.pointers) replaced by a view of a relocated copy; the changed bytes go back afterwards."""
        found = []                                           # (position, index in .tensors or None, tensor)
        for pos, a in enumerate(args):
            if isinstance(a, _torch.Tensor):
                found.append((pos, None, a))
            elif isinstance(a, ctypes.Array) and hasattr(a, 'tensors'):
                found += [(pos, j, t) for j, t in enumerate(a.tensors)]
        moved = [(pos, j, t, t.data_ptr(), t.data_ptr() + span_bytes(t)) for pos, j, t in found if self._is_input(t)]
        # groups: spans of one storage that overlap or touch
        groups = []
        for item in sorted(moved, key=lambda m: (str(m[2].device), m[2].untyped_storage().data_ptr(), m[3])):
            t, start, end = item[2], item[3], item[4]
            last = groups[-1] if groups else None
            if (last is not None and last['device'] == t.device and last['base'] == t.untyped_storage().data_ptr()
                    and start <= last['end']):
                last['end'] = max(last['end'], end)
                last['items'].append(item)
            else:
                groups.append({'device': t.device, 'base': t.untyped_storage().data_ptr(), 'storage': t.untyped_storage(),
                               'start': start, 'end': end, 'items': [item]})
        new, work, nbytes = {}, [], 0
        for grp in groups:
            n = grp['end'] - grp['start']
            first = grp['items'][0]
            b = self._block(grp['device'], grp['start'], n, name, first[0])
            original = _alias(grp['storage'], grp['device'], grp['start'] - grp['base'], n)
            b.span().copy_(original)                         # (on the current stream, like the launch that follows)
            work.append((b, original, original.clone()))
            nbytes += n
            for pos, j, t, start, _ in grp['items']:
                at = b.lead + start - grp['start']
                assert at % t.element_size() == 0, '%s: argument %d is not aligned to its element size' % (name, pos)
                new[(pos, j)] = _torch.empty(0, dtype=t.dtype, device=t.device).set_(
                    b.backing.untyped_storage(), at // t.element_size(), t.shape, t.stride())
        out = []
        for pos, a in enumerate(args):
            if isinstance(a, _torch.Tensor):
                a = new.get((pos, None), a)
            elif isinstance(a, ctypes.Array) and hasattr(a, 'tensors'):
                ts = tuple(new.get((pos, j), t) for j, t in enumerate(a.tensors))
                a = type(a)(*[t.data_ptr() for t in ts])
                a.tensors = ts
            elif isinstance(a, ctypes.Array) and getattr(a, '_type_', None) is ctypes.c_void_p:
                self._refuse_pointers(name, pos, list(a))
            elif isinstance(a, int):
                self._refuse_pointers(name, pos, [a])
            out.append(a)
        rec = self.relocated.setdefault(name, {'args': 0, 'bytes': 0})
        rec['args'] += len(moved)
        rec['bytes'] += nbytes
        result = real_call(name, *out, **kw)
        for b, original, before in work:                     # only the bytes the native changed: the original may have been
            now = b.span()                                   # written meanwhile through an address a device table holds
            original.copy_(_torch.where(now != before, now, original))
        return result

    # -- checks ---------------------------------------------------------------------------------------------------------------
    def violations(self):
        """[{ordinal, shape, dtype, side}] for every band that holds a byte other than the fill, and [{input, arg, side}] (the
        native and the position of the argument the block was made for) for the bands of the relocated inputs (synchronises the
        device)."""
        bad = []
        for b in self.blocks.values():
            for side, band in (('before', b.backing[:b.lead]), ('after', b.backing[b.lead + b.nbytes:])):
                if bool((band != self.fill).any()):
                    bad.append({'input': b.native, 'arg': b.arg, 'side': side})
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
def guarded(fill, modules=None, lib=None, guard_cpu=False, relocate=False):
    """Context manager: see the module docstring.  modules: the modules to patch (default: every loaded lasr_amd.* module);
    lib: the object whose `call(name, ...)` launches natives (default: lasr_amd._lib); guard_cpu: guard CPU tensors too (the
    harness's own CPU test); relocate: move the natives' input tensors into tight, poisoned copies.  Yields the Guard."""
    if lib is None:
        from lasr_amd import _lib as lib
    g = Guard(fill, guard_cpu, relocate)
    proxy = _TorchProxy('torch')
    proxy.empty, proxy.empty_like = g.empty, g.empty_like
    real_call = lib.call

    def call(name, *args, **kw):
        g.natives.append(name)
        if g.relocate:
            return g.call(real_call, name, args, kw)
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


def run_relocated(case, device, modules=None, lib=None, guard_cpu=False, not_relocated=()):
    """run_case with the inputs relocated (relocate=True): the case plain, under 0xFF and under 0x7F; assert that no band was
    touched, around outputs, scratch or inputs (a), the same bits in all three runs, by the case's own rule (b), and that the run
    was not vacuous (c): the natives reached are the declared ones, each of them outside `not_relocated` had a tensor argument
    relocated, with more than zero bytes, and some returned tensor holds more than one distinct value.  Returns the
    Guard.relocated record of the last run."""
    plain = _flat(case.fn(device))
    runs = []
    for fill in FILLS:
        with guarded(fill, modules=modules, lib=lib, guard_cpu=guard_cpu, relocate=True) as g:
            out = _flat(case.fn(device))
            bad = g.violations()
        # c. not vacuous
        assert frozenset(g.natives) == case.natives, '%s: natives reached %s, declared %s' % (
            case.name, sorted(set(g.natives)), sorted(case.natives))
        idle = sorted(n for n in case.natives if n not in not_relocated
                      and not (g.relocated.get(n, {}).get('args', 0) > 0 and g.relocated[n]['bytes'] > 0))
        assert not idle, '%s: fill 0x%02X: no tensor argument was relocated for %s' % (case.name, fill, idle)
        # a. bands intact
        assert not bad, '%s: fill 0x%02X: guard band touched: %s' % (case.name, fill, bad)
        runs.append(out)
    assert any(t.numel() > 1 and bool((t.reshape(-1) != t.reshape(-1)[0]).any()) for t in plain), \
        '%s: every returned tensor is constant' % case.name
    # b. same bits
    _same(case, runs[0], runs[1], 'fill 0xFF against fill 0x7F')
    _same(case, plain, runs[0], 'plain against fill 0xFF')
    _same(case, plain, runs[1], 'plain against fill 0x7F')
    return g.relocated
