"""ctypes binding of the stereo cost volume surface of libdhd_amd.so (dhd_amd/capi_stereo/dhd_amd_stereo_cv.h): the `dhdv_*`
entry points.

They live in the same library and are reached through the same handle as every other surface; the prototypes here are set on
that handle on first use, on the pattern of _unet_seam.py.  The table is separate for the reason the header gives: the other
tables are closed lists, so the family ships beside them with its own surface tests (tests/test_stereo_cv_capi.py).  Return
codes go through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

NCHW, NHWC = 0, 1                      # DHDV_NCHW, DHDV_NHWC
MAX_C, MAX_D = 1024, 256               # DHDV_MAX_C, DHDV_MAX_D

_P = C.c_void_p
_I = C.c_int
_Z = C.c_size_t
_F = C.c_float
_PROTOTYPES = {
    #                            dtype bn c h w n_depth
    'dhdv_stereo_cv_supported': ([_I] * 6, _I),
    #                                dtype layout bn c h w
    'dhdv_stereo_cv_scratch_bytes': ([_I] * 6, _Z),
    #                    six view arrays, u v dep, grid | bn h w n_depth hi wi | stream
    'dhdv_stereo_grid': ([_P] * 10 + [_I] * 6 + [_P], _I),
    #                           prev curr out | dtype layout | six view arrays, u v dep | bn c h w n_depth hi wi | bias flag_channel |
    #                           scratch bytes stream
    'dhdv_stereo_cost_volume': ([_P] * 3 + [_I] * 2 + [_P] * 9 + [_I] * 7 + [_F, _I, _P, _Z, _P], _I),
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
