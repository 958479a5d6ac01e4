"""ctypes binding of the optimizer-step surface of libdhd_amd.so (dhd_amd/capi_optim/dhd_amd_optim.h): the `dhdw_*` entry points.

They live in the same library and are reached through the same handle as every other surface; the prototypes here are set on
that handle on first use, on the pattern of _occ_loss_head.py.  The table is separate for the reason the header gives: the other
tables are closed lists, so the family ships beside them with its own surface tests (tests/test_optim_capi.py).  Return codes go
through `_lib.check`, the one place that turns them into DhdError.  The structs of the header are mirrored here: `Tables` for
ctypes, CHUNK_DTYPE / GROUP_DTYPE for the numpy arrays the device tables are uploaded from."""
import ctypes as C

import numpy as np

from . import _lib

CHUNK = 1 << 16                                              # DHDW_OPTIM_CHUNK
RECORD_AT, MULT_AT, FOUND_AT, PARTIALS_AT = 0, 16, 20, 64    # DHDW_OPTIM_*_AT

CHUNK_DTYPE = np.dtype([('p', '<u8'), ('g', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'), ('ema', '<u8'), ('half', '<u8'),
                        ('len', '<i4'), ('group', '<i4'), ('half_dtype', '<i4'), ('slot', '<i4')])           # dhdw_optim_chunk
GROUP_DTYPE = np.dtype([(n, '<f8') for n in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay')])                # dhdw_optim_group
assert CHUNK_DTYPE.itemsize == 64 and GROUP_DTYPE.itemsize == 40


class Tables(C.Structure):                                   # dhdw_optim_tables
    _fields_ = ([(n, C.c_void_p) for n in ('chunks', 'groups', 'slot_group', 'steps', 'slot_scalars', 'group_scalars', 'decay_pair',
                                           'scale', 'growth_tracker')] +
                [(n, C.c_int32) for n in ('n_chunks', 'n_groups', 'n_slots', 'n_partials')])


_P = C.c_void_p
_I = C.c_int
_Z = C.c_size_t
_F = C.c_float
_PROTOTYPES = {
    'dhdw_optim_workspace_bytes': ([_I], _Z),
    #                        tables            workspace bytes stream
    'dhdw_optim_grad_norm': ([C.POINTER(Tables), _P, _Z, _P], _I),
    #                       tables             max_norm growth backoff interval workspace bytes stream
    'dhdw_optim_finalize': ([C.POINTER(Tables), _F, _F, _F, _I, _P, _Z, _P], _I),
    'dhdw_optim_adamw_update': ([C.POINTER(Tables), _P, _Z, _P], _I),
}

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_bound = None


def load():
    """The handle of _lib.load() with the prototypes of this surface set (once per handle)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib and isinstance(lib, C.CDLL):    # (a test's call recorder in place of the handle is not bound to)
        for name, (argtypes, restype) in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _bound = lib
    return lib


def call(name, *args):
    """Entry point `name` of the surface with `args`; a non-zero return code raises DhdError."""
    _lib.check(getattr(load(), name)(*args), name)


def value(name, *args):
    """Entry point `name` where it returns a value rather than an error code (`*_workspace_bytes`)."""
    return getattr(load(), name)(*args)
