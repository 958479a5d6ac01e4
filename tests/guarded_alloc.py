"""Guard bands around every buffer the product's Python allocates (a helper module of the tests, not a conftest).

    with guarded(monkeypatch, fill=0xFF) as ledger:
        ... run an operator ...
        ledger.check()

While the context is active, every allocation that code under `roots` (default: dhd_amd/) makes on a device in `devices`
through one of the FORMS below comes back inside a parent buffer

    [ GUARD bytes of 0xA5 | nbytes of the tensor, every byte `fill` (zero for the zeros forms) | GUARD bytes of 0xA5 ]

GUARD = 4096 is a multiple of the caching allocator's 512-byte granule, so the tensor keeps the alignment a fresh allocation
has today and no wrapper changes path (dense16, the library's 16-byte checks).  The rear guard begins at the exact byte after
the tensor: nbytes is not rounded.  The tensor is built with set_() on the parent's storage, not as a view of the parent:
autograd treats a view created inside a Function.forward differently from a fresh tensor.

Shape, strides and dtype are taken from the real function on device='meta', so sizes as a tuple or as varargs, dtype=,
memory_format=channels_last and empty_like's stride preservation are honoured exactly as torch honours them.  Zero-byte
requests, other devices, out= and non-strided layouts go to the real function.

On entry the product's module-level caches of device memory start empty (CACHES), so that pooled scratch is allocated under
guard at the size THIS call advertises rather than at whatever an earlier test left behind.  Everything is done with
monkeypatch.setattr and undone on exit, also when the body raises.

Limits: a write more than GUARD bytes outside a buffer is not seen; buffers torch itself allocates (autograd, .contiguous(),
.to(), .clone()) are not guarded."""
import contextlib
import importlib
import os
import sys

import torch

GUARD = 4096
GUARD_BYTE = 0xA5
PRODUCT_ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dhd_amd')
_HERE = os.path.abspath(__file__)

# (owner, attribute, kind, zero interior?)   kind: 'factory' f(*size, device=...), 'like' f(tensor, ...), 'new' tensor.f(size, ...)
FORMS = (
    (torch, 'empty', 'factory', False),
    (torch, 'zeros', 'factory', True),
    (torch, 'empty_like', 'like', False),
    (torch, 'zeros_like', 'like', True),
    (torch.Tensor, 'new_zeros', 'new', True),
)
PATCHED_NAMES = frozenset(('torch.' if owner is torch else 'Tensor.') + name for owner, name, _, _ in FORMS)

# module-level caches of device memory in the product: (module, attribute, factory of the empty cache)
CACHES = (
    ('dhd_amd.mghs_op', 'scratch_pool', lambda m: m._ScratchPool()),
    ('dhd_amd.bev_pool_v2', '_fused_scratch', lambda m: {}),
    ('dhd_amd.bev_pool_v2', '_regroup_cache', lambda m: {}),
    ('dhd_amd.bev_pool_v2', '_state_cache', lambda m: {}),
    ('dhd_amd.bev_pool_v2', '_fused_size_cache', lambda m: {}),
)


class GuardError(AssertionError):
    pass


class Entry:
    __slots__ = ('parent', 'nbytes', 'site', 'form')

    def __init__(self, parent, nbytes, site, form):
        self.parent, self.nbytes, self.site, self.form = parent, nbytes, site, form


class Ledger:
    """Every guarded allocation: its parent buffer, its size in bytes, the allocation site (`file:line`, the innermost stack
    frame under the guarded roots) and the form it came through."""

    def __init__(self):
        self.entries = []

    def __len__(self):
        return len(self.entries)

    def total_bytes(self):
        return sum(e.nbytes for e in self.entries)

    def sites_under(self, root=PRODUCT_ROOT):
        return [e for e in self.entries if _under(e.site.rsplit(':', 1)[0], (root,))]

    def check(self):
        """Synchronise and compare both guards of every entry on the device.  Raises GuardError naming, per damaged guard, the
        allocation site, which guard, and the offset of the first changed byte relative to the tensor's end (or start)."""
        bad = []
        synced = set()
        for e in self.entries:
            dev = e.parent.device
            if dev.type == 'cuda' and dev not in synced:
                torch.cuda.synchronize(dev)
                synced.add(dev)
            for which, band in (('front', e.parent[:GUARD]), ('rear', e.parent[GUARD + e.nbytes:])):
                assert band.numel() == GUARD
                wrong = band != GUARD_BYTE
                if bool(wrong.any()):
                    first = int(wrong.nonzero()[0])
                    where = (f'{GUARD - first} bytes before the start' if which == 'front' else f'{first} bytes past the end')
                    bad.append(f'{e.site} ({e.form}, {e.nbytes} bytes): {which} guard changed, first at {where} of the tensor '
                               f'({int(wrong.sum())} guard bytes differ)')
        if bad:
            raise GuardError('guard bytes changed:\n  ' + '\n  '.join(bad))


def _under(filename, roots):
    f = os.path.abspath(filename)
    return any(f == r or f.startswith(r.rstrip(os.sep) + os.sep) for r in roots)


def _site(roots):
    """`file:line` of the innermost frame whose file lies under `roots`, or None."""
    f = sys._getframe(2)
    while f is not None:
        name = f.f_code.co_filename
        if name != _HERE and _under(name, roots):
            return f'{os.path.relpath(name, os.path.dirname(PRODUCT_ROOT))}:{f.f_lineno}'
        f = f.f_back
    return None


def _span(meta):
    """Bytes from the first to one past the last element of a strided tensor."""
    if meta.numel() == 0:
        return 0
    return (1 + sum((n - 1) * s for n, s in zip(meta.shape, meta.stride()))) * meta.element_size()


def _default_device():
    get = getattr(torch, 'get_default_device', None)
    return get() if get is not None else torch.device('cpu')


def _make(real, real_empty, kind, zero, name, fill, devices, roots, ledger):
    def patched(*args, **kwargs):
        if kwargs.get('out') is not None or kwargs.get('layout', torch.strided) is not torch.strided or kwargs.get('names') is not None:
            return real(*args, **kwargs)
        device = kwargs.get('device')
        if device is None:
            device = _default_device() if kind == 'factory' else args[0].device
        device = torch.device(device)
        if device.type not in devices:
            return real(*args, **kwargs)
        site = _site(roots)
        if site is None:
            return real(*args, **kwargs)
        plain = {k: v for k, v in kwargs.items() if k not in ('requires_grad', 'pin_memory')}
        meta = real(*args, **dict(plain, device='meta'))
        nbytes = _span(meta)
        if nbytes == 0:
            return real(*args, **kwargs)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        es = meta.element_size()
        assert GUARD % es == 0
        parent = real_empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        parent[:GUARD] = GUARD_BYTE
        parent[GUARD:GUARD + nbytes] = 0 if zero else fill
        parent[GUARD + nbytes:] = GUARD_BYTE
        t = real_empty(0, dtype=meta.dtype, device=device).set_(parent.untyped_storage(), GUARD // es, meta.shape, meta.stride())
        assert t.data_ptr() == parent.data_ptr() + GUARD
        ledger.entries.append(Entry(parent, nbytes, site, name))
        if kwargs.get('requires_grad'):
            t.requires_grad_()
        return t
    patched.__name__ = 'guarded_' + name.replace('.', '_')
    return patched


@contextlib.contextmanager
def guarded(monkeypatch, fill, devices=('cuda',), roots=(PRODUCT_ROOT,), fresh_caches=True):
    """-> Ledger.  fill: the byte (0..255) every `empty` interior starts with; devices: device types that are guarded;
    roots: directories or files whose code is guarded (an allocation with no frame under them goes to the real function)."""
    assert 0 <= int(fill) <= 255
    roots = tuple(os.path.abspath(r) for r in roots)
    ledger = Ledger()
    real_empty = torch.empty
    with monkeypatch.context() as mp:
        if fresh_caches:
            for module, attr, new in CACHES:
                m = importlib.import_module(module)
                mp.setattr(m, attr, new(m))
        for owner, attr, kind, zero in FORMS:
            name = ('torch.' if owner is torch else 'Tensor.') + attr
            mp.setattr(owner, attr, _make(getattr(owner, attr), real_empty, kind, zero, name, int(fill), tuple(devices), roots, ledger))
        yield ledger
