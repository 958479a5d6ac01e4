"""ctypes binding of the occupancy head + losses surface of libdhd_amd.so (dhd_amd/capi_occ_loss/dhd_amd_occ_head_loss.h): the
`dhdl_*` entry points.

They live in the same library and are reached through the same handle as every other surface; the prototypes here are set on
that handle on first use, on the pattern of _occ_train.py.  The table is separate for the reason the header gives: the other
tables are closed lists, so the family ships beside them with its own surface tests (tests/test_occ_head_loss_capi.py).  Return
codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

_P = C.c_void_p
_I = C.c_int
_Z = C.c_size_t
_PROTOTYPES = {
    'dhdl_occ_head_loss_supported': ([_I] * 6, _I),
    'dhdl_occ_head_loss_workspace_bytes': ([], _Z),
    'dhdl_occ_head_loss_scratch_bytes': ([_P, _I, _I, _I, _I, C.POINTER(_Z), C.POINTER(_Z)], _I),
    #                              x  dtype layout w  b  dy  dx | labels mask cw | ignore non_empty | logits losses workspace scratch | bytes stream
    'dhdl_occ_head_loss_forward': ([_P, _I, _I, _P, _I, _I, _I] + [_P] * 3 + [_I, _I] + [_P] * 4 + [_Z, _P], _I),
    #                               x  dtype layout w  b  dy  dx | logits labels mask cw | ignore non_empty | grad_losses workspace dx_out db1 db2
    #                               act dhid g scratch | bytes stream
    'dhdl_occ_head_loss_backward': ([_P, _I, _I, _P, _I, _I, _I] + [_P] * 4 + [_I, _I] + [_P] * 9 + [_Z, _P], _I),
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
    """Entry point `name` where it returns a value rather than an error code (`*_supported`, `*_workspace_bytes`)."""
    return getattr(load(), name)(*args)
