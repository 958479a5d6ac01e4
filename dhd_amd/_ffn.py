"""ctypes binding of the Swin FFN surface of libdhd_amd.so (include/dhd_amd_ffn.h): the `dhdf_*` entry points.

They live in the same library and are reached through the same handle as the `dhd_*` surface of _lib.py and the `dhdx_*` surface
of _ext.py; the prototypes here are set on that handle on first use.  The table is separate for the reason the header gives:
the other two tables are closed lists, so the family ships beside them with its own surface tests
(tests/test_swin_ffn_capi.py).  Return codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

_P = C.c_void_p
_I = C.c_int
_PROTOTYPES = {
    'dhdf_swin_ffn_supported': ([_I, _I, _I, _I], _I),
    'dhdf_swin_ffn_scratch_bytes': ([_I, _I, _I], C.c_size_t),
    'dhdf_swin_ffn_infer': ([_P] * 9 + [C.c_size_t, _I, _I, C.c_long, _I, _I, C.c_float, _P], _I),
}

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_bound = None


def load():
    """The handle of _lib.load() with the FFN prototypes set (once per handle)."""
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
    """Entry point `name` of the FFN surface with `args`; a non-zero return code raises DhdError."""
    _lib.check(getattr(load(), name)(*args), name)


def value(name, *args):
    """Entry point `name` where it returns a value rather than an error code (`*_supported`, `*_bytes`)."""
    return getattr(load(), name)(*args)
