"""ctypes binding of the Swin FFN training surface of libdhd_amd.so for C = 512 (dhd_amd/include/dhd_amd_ffn_wide_train.h): the
`dhdu_*` entry points.

They live in the same library and are reached through the same handle as every other surface; the prototypes here are set on
that handle on first use, on the pattern of _ffn_train.py.  The table is separate for the reason the header gives: the other
tables are closed lists, so the family ships beside them with its own surface tests (tests/test_swin_ffn_wide_train_capi.py).
Return codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

_P = C.c_void_p
_I = C.c_int
_L = C.c_long
_Z = C.c_size_t
_PROTOTYPES = {
    'dhdu_swin_ffn_wide_supported': ([_I, _I, _I, _I], _I),
    'dhdu_swin_ffn_wide_forward_scratch_bytes': ([_I, _I, _I], _Z),
    'dhdu_swin_ffn_wide_forward': ([_P] * 8 + [_L, _P, _P, _Z, _I, _I, _L, _I, _I, C.c_float, _P], _I),
    'dhdu_swin_ffn_wide_backward_scratch_bytes': ([_L, _I, _I, _I], _Z),
    'dhdu_swin_ffn_wide_backward': ([_P] * 8 + [_L] + [_P] * 7 + [_Z, _I, _I, _L, _I, _I, C.c_float, _P], _I),
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
    """Entry point `name` where it returns a value rather than an error code (`*_supported`, `*_bytes`)."""
    return getattr(load(), name)(*args)
