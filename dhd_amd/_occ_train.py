"""ctypes binding of the occupancy head's training surface of libdhd_amd.so (dhd_amd/capi/dhd_amd_occ_train.h): the `dhdo_*`
entry points.

They live in the same library and are reached through the same handle as every other surface; the prototypes here are set on
that handle on first use, on the pattern of _ffn_train.py.  The table is separate for the reason the header gives: the other
tables are closed lists, so the family ships beside them with its own surface tests (tests/test_occ_head_train_capi.py).  Return
codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

_P = C.c_void_p
_I = C.c_int
_Z = C.c_size_t
_PROTOTYPES = {
    'dhdo_occ_head_backward_supported': ([_I] * 6, _I),
    'dhdo_occ_head_backward_scratch_bytes': ([_P, _I, _I, _I, _I, C.POINTER(_Z)], _I),
    #                          x  dtype layout w  b  dy  dx | glogits dx_out db1 db2 act dhid ghalf scratch | bytes stream
    'dhdo_occ_head_backward': ([_P, _I, _I, _P, _I, _I, _I] + [_P] * 8 + [_Z, _P], _I),
}

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_bound = None


def load():
    """The handle of _lib.load() with the training prototypes set (once per handle)."""
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
    """Entry point `name` of the training surface with `args`; a non-zero return code raises DhdError."""
    _lib.check(getattr(load(), name)(*args), name)


def value(name, *args):
    """Entry point `name` where it returns a value rather than an error code (`*_supported`)."""
    return getattr(load(), name)(*args)
