"""ctypes binding of the deformable convolution's training surface of libdhd_amd.so (dhd_amd/capi_deform/dhd_amd_deform_train.h):
the `dhdd_*` entry points.

They live in the same library and are reached through the same handle as every other surface; the prototypes here are set on
that handle on first use, on the pattern of _occ_train.py.  The table is separate for the reason the header gives: the other
tables are closed lists, so the family ships beside them with its own surface tests (tests/test_deform_conv_train_capi.py).
Return codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

_P = C.c_void_p
_I = C.c_int
_Z = C.c_size_t
_PROTOTYPES = {
    #                                       c_in c_out groups k h w x_dtype x_layout g_layout
    'dhdd_deform_conv_backward_supported': ([_I] * 9, _I),
    #                                           b + the nine above | bytes
    'dhdd_deform_conv_backward_scratch_bytes': ([_I] * 10 + [C.POINTER(_Z)], _I),
    #                             x  dtype layout offset weight gout g_layout dx doffset col | b c_in c_out groups h w k pad dil | scratch bytes stream
    'dhdd_deform_conv_backward': ([_P, _I, _I, _P, _P, _P, _I, _P, _P, _P] + [_I] * 9 + [_P, _Z, _P], _I),
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
