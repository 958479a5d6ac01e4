"""ctypes binding of the stage-seam surface of libdhd_amd.so (include/dhd_amd_seam.h): the `dhds_*` entry points.

They live in the same library and are reached through the same handle as the `dhd_*` surface of _lib.py; the prototypes here are
set on that handle on first use.  The table is separate from `_lib._PROTOTYPES`, `_ext._PROTOTYPES` and the two FFN tables for
the reason the header gives: those are closed lists held by existing tests, so the family ships beside them with its own surface
tests (tests/test_swin_seam_capi.py).  Return codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

_P = C.c_void_p
_I = C.c_int
_PROTOTYPES = {
    'dhds_merge_norm_supported': ([_I, _I, _I], _I),
    'dhds_merge_norm_forward': ([_P, _P, _P, _P] + [_I] * 6 + [C.c_float, _P], _I),
    'dhds_merge_norm_backward_scratch_bytes': ([C.c_long, _I], C.c_size_t),
    'dhds_merge_norm_backward': ([_P] * 7 + [C.c_size_t] + [_I] * 6 + [C.c_float, _P], _I),
    'dhds_embed_norm_supported': ([_I, _I, _I], _I),
    'dhds_embed_norm_forward': ([_P, _P, _P, _P] + [_I] * 4 + [C.c_long, C.c_float, _P], _I),
    'dhds_embed_norm_backward_scratch_bytes': ([C.c_long, _I], C.c_size_t),
    'dhds_embed_norm_backward': ([_P] * 7 + [C.c_size_t] + [_I] * 4 + [C.c_long, C.c_float, _P], _I),
}

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_bound = None


def load():
    """The handle of _lib.load() with the seam prototypes set (once per handle)."""
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
    """Entry point `name` of the seam surface with `args`; a non-zero return code raises DhdError."""
    _lib.check(getattr(load(), name)(*args), name)


def value(name, *args):
    """Entry point `name` where it returns a value rather than an error code (`*_supported`, `*_bytes`)."""
    return getattr(load(), name)(*args)
