"""ctypes binding of the UNet-seam surface of libdhd_amd.so (dhd_amd/capi_unet/dhd_amd_unet_seam.h): the `dhdn_*` entry points.

They live in the same library and are reached through the same handle as every other surface; the prototypes here are set on
that handle on first use, on the pattern of _optim.py.  The table is separate for the reason the header gives: the other tables
are closed lists, so the family ships beside them with its own surface tests (tests/test_unet_seam_capi.py).  Return codes go
through `_lib.check`, the one place that turns them into DhdError."""
import ctypes as C

from . import _lib

NCHW, NHWC = 0, 1                      # DHDN_NCHW, DHDN_NHWC
UP_ROWS, UP_COLS = 32, 128             # DHDN_UP_ROWS, DHDN_UP_COLS

_P = C.c_void_p
_I = C.c_int
_Z = C.c_size_t
_PROTOTYPES = {
    #                            dtype layout b c h w
    'dhdn_max_pool2_supported': ([_I] * 6, _I),
    #                          x   y   dtype layout b c h w  stream
    'dhdn_max_pool2_forward': ([_P, _P] + [_I] * 6 + [_P], _I),
    #                           x   gy  gx
    'dhdn_max_pool2_backward': ([_P, _P, _P] + [_I] * 6 + [_P], _I),
    #                         dtype layout b cin cout c2 h w H W
    'dhdn_up_cat_supported': ([_I] * 10, _I),
    #                             dtype b cin cout h w backward
    'dhdn_up_cat_scratch_bytes': ([_I] * 7, _Z),
    #                       x1  x2  weight wdtype bias out scratch bytes | dtype layout b cin cout c2 h w H W | stream
    'dhdn_up_cat_forward': ([_P, _P, _P, _I, _P, _P, _P, _Z] + [_I] * 10 + [_P], _I),
    #                        gout weight wdtype gx1 gx2 gop dbias scratch bytes
    'dhdn_up_cat_backward': ([_P, _P, _I, _P, _P, _P, _P, _P, _Z] + [_I] * 10 + [_P], _I),
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
