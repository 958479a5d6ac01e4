"""ctypes binding of the wide Swin FFN surface of libdhd_amd.so (include/dhd_amd_ffn_wide.h): the `dhdg_*` entry points, the
operator of _ffn.py for C = 512 and 1024.

They live in the same library and are reached through the same handle as the `dhd_*` surface of _lib.py, the `dhdx_*` surface
of _ext.py and the `dhdf_*` surface of _ffn.py; the prototypes here are set on that handle on first use.  The table is separate
for the reason the header gives: the other three tables are closed lists, so the family ships beside them with its own surface
tests (tests/test_swin_ffn_wide_capi.py).  Return codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

_P = C.c_void_p
_I = C.c_int
_PROTOTYPES = {
    'dhdg_swin_ffn_wide_supported': ([_I, _I, _I, _I], _I),
    'dhdg_swin_ffn_wide_scratch_bytes': ([_I, _I, _I], C.c_size_t),
    'dhdg_swin_ffn_wide_infer': ([_P] * 9 + [C.c_size_t, _I, _I, C.c_long, _I, _I, C.c_float, _P], _I),
}

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_bound = None


def load():
    """The handle of _lib.load() with the wide FFN prototypes set (once per handle)."""
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
    """Entry point `name` of the wide FFN surface with `args`; a non-zero return code raises DhdError."""
    _lib.check(getattr(load(), name)(*args), name)


def value(name, *args):
    """Entry point `name` where it returns a value rather than an error code (`*_supported`, `*_bytes`)."""
    return getattr(load(), name)(*args)
