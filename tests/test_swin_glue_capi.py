"""The extension surface `dhdx_*` of libdhd_amd.so (include/dhd_amd_ext.h, dhd_amd/_ext.py) without a GPU: its own copies of the
guarantees tests/test_capi.py holds for the `dhd_*` surface -- header, binding table and exports agree; every entry point
refuses bad input on the host with the documented code -- plus the host-side pieces of the Swin glue: the scratch size, the
float64 twin's index map, and the switch that is off."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_glue_inputs as SG  # noqa: E402
from conftest import golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'dhd_amd_ext.h')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3


def declared_symbols():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|size_t)\s+(dhdx_[a-z0-9_]+)\s*\(', src)))


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _lib
    want = ['dhdx_ln_rows_backward', 'dhdx_ln_rows_backward_scratch_bytes', 'dhdx_ln_rows_forward', 'dhdx_ln_rows_supported',
            'dhdx_window_reverse_add']
    assert declared_symbols() == want == sorted(_ext.EXPORTED_SYMBOLS)
    lib = _ext.load()
    assert lib is _lib.load()                                        # the same library, the same handle
    for name, (argtypes, restype) in _ext._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdx_[a-z0-9_]+)', out)) == set(want)
    # the dhd_* surface is what it was: nothing of the family leaked into its tables, the ABI number did not move
    assert not any(n.startswith('dhdx') for n in _lib._PROTOTYPES)
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    assert re.search(r'#define DHD_ABI_VERSION 6\b', open(os.path.join(ROOT, 'include', 'dhd_amd.h')).read())
    assert '#include "dhd_amd.h"' in open(HEADER).read()


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_ext.h"\nint main(void) { return dhdx_ln_rows_supported(8, DHD_F32, DHD_BF16) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_builds_the_translation_unit():
    mk = open(os.path.join(ROOT, 'dhd_amd', 'csrc', 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert 'swin_glue.hip' in srcs and os.path.exists(os.path.join(ROOT, 'dhd_amd', 'csrc', 'swin_glue.hip'))
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:'))
    assert 'window_geom.h' in rule and 'dhd_amd_ext.h' in rule        # a change of either header rebuilds the objects


def test_supported_range():
    from dhd_amd import _ext
    lib = _ext.load()
    for c in (8, 96, 128, 1024, 1536, 2048):
        for a in (0, 1, 2):
            for b in (0, 1, 2):
                assert lib.dhdx_ln_rows_supported(c, a, b) == 1, (c, a, b)
    for c in (0, -8, 4, 12, 100, 2056, 4096):
        assert lib.dhdx_ln_rows_supported(c, 0, 0) == 0, c
    for bad in (3, -1):
        assert lib.dhdx_ln_rows_supported(128, bad, 0) == 0 and lib.dhdx_ln_rows_supported(128, 0, bad) == 0


def _each_pointer(fn, args, slots, optional=()):
    """fn(*args) with each pointer of `slots` NULL, then 4 and 2 bytes off a 16-byte boundary -> DHD_EINVAL; an `optional` slot may
    be NULL but not misaligned."""
    for s in slots + tuple(optional):
        for bad in ((None,) if s not in optional else ()) + (C.c_void_p(0x10004), C.c_void_p(0x10002)):
            a = list(args)
            a[s] = bad
            assert fn(*a) == EINVAL, (fn.__name__, s, bad)


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named,
    and where the pointer test comes first the same call with good pointers reaches the later check."""
    from dhd_amd import _ext
    lib = _ext.load()
    P = C.c_void_p(0x10000)
    fwd = [P, P, P, P, 0, 2, 2, 10, 15, 96, 7, 3, 1e-5, None]                  # x gamma beta out | dtypes | b h w c window shift | eps
    bwd = [P, P, P, P, P, P, P, 1 << 20, 0, 2, 2, 10, 15, 96, 7, 3, 1e-5, None]  # x dy gamma dx dgamma dbeta scratch bytes | dtypes | ...
    add = [P, P, P, P, 2, 0, 2, 10, 15, 96, 7, 3, None]                         # win identity scale out | dtypes | b h w c window shift
    _each_pointer(lib.dhdx_ln_rows_forward, fwd, (0, 1, 2, 3))
    _each_pointer(lib.dhdx_ln_rows_backward, bwd, (0, 1, 2, 3, 4, 5, 6))
    _each_pointer(lib.dhdx_window_reverse_add, add, (0, 1, 3))
    a = list(add)
    a[2] = C.c_void_p(0x10002)                                                  # scale: float32, 4-byte aligned
    assert lib.dhdx_window_reverse_add(*a) == EINVAL
    for fn, args, c_at in ((lib.dhdx_ln_rows_forward, fwd, 9), (lib.dhdx_ln_rows_backward, bwd, 13), (lib.dhdx_window_reverse_add, add, 9)):
        def with_(**kw):
            a = list(args)
            for k, val in kw.items():
                a[c_at + dict(b=-3, h=-2, w=-1, c=0, window=1, shift=2)[k]] = val
            return fn(*a)
        for c in (12, 100, 0, 2056, 4096):
            assert with_(c=c) == EUNSUPPORTED, (fn.__name__, c)
        assert with_(shift=7) == EUNSUPPORTED and with_(shift=8) == EUNSUPPORTED and with_(shift=-1) == EUNSUPPORTED
        assert with_(window=-1) == EUNSUPPORTED
        assert with_(window=0, shift=3) == EUNSUPPORTED                          # a shift without windows
        for k in 'bhw':
            assert with_(**{k: 0}) == EINVAL and with_(**{k: -1}) == EINVAL, (fn.__name__, k)
        assert with_(b=1 << 30, h=1 << 10, w=1) == EUNSUPPORTED                  # 2^40 rows
        # the pointer test comes first: with a bad pointer the same calls are DHD_EINVAL
        a = list(args)
        a[0], a[c_at] = None, 12
        assert fn(*a) == EINVAL
    # the identity map: LayerNorm rows take it, reverse + add has no meaning without windows
    assert lib.dhdx_window_reverse_add(*(add[:10] + [0, 0, None])) == EUNSUPPORTED
    # dtype codes
    for bad in (3, -1):
        for fn, args, slots in ((lib.dhdx_ln_rows_forward, fwd, (4, 5)), (lib.dhdx_ln_rows_backward, bwd, (8, 9)),
                                (lib.dhdx_window_reverse_add, add, (4, 5))):
            for s in slots:
                a = list(args)
                a[s] = bad
                assert fn(*a) == EUNSUPPORTED, (fn.__name__, s, bad)
    # scratch: exactly the advertised size passes the size check (and would launch: not called here), one byte less is refused
    need = lib.dhdx_ln_rows_backward_scratch_bytes(2 * 10 * 15, 96)
    assert need > 0
    for short in (0, 8 * 96 - 1, need - 1):
        a = list(bwd)
        a[7] = short
        assert lib.dhdx_ln_rows_backward(*a) == ENOSPACE, short
    a = list(bwd)
    a[7], a[13] = 0, 12                                                          # the size check comes after the shape checks
    assert lib.dhdx_ln_rows_backward(*a) == EUNSUPPORTED


def test_scratch_bytes():
    from dhd_amd import _ext
    lib = _ext.load()
    f = lib.dhdx_ln_rows_backward_scratch_bytes
    for c in (8, 96, 128, 1024, 2048):
        last = 0
        for rows in list(range(1, 300)) + [1728, 8448, 33792, 135168, 540672, 540673, 10 ** 7, 10 ** 9]:
            n = f(rows, c)
            assert n >= max(last, 8 * c) and n % (8 * c) == 0, (rows, c, n, last)     # whole row pairs, at least one, non-decreasing
            last = n
        assert last <= 4096 * 8 * c                                              # bounded: the partial rows stay a small table
    for rows, c in ((0, 128), (-5, 128), (1 << 40, 128), (100, 12), (100, 4), (100, 2056), (100, 0)):
        assert f(rows, c) == 0, (rows, c)
    # ws12_c128: 1728 tokens span at least three workgroups and no equal split of them exists, so one workgroup is ragged
    B, H, W, ws, sh, Cc = SG.CASES['ws12_c128']
    groups = f(B * H * W, Cc) // (8 * Cc)
    assert B * H * W == 1728 and groups >= 3 and 1728 % groups != 0, groups


def _window_rows_map(B, H, W, ws, sh):
    """The partition's index map as csrc/window.hip states it: window row -> token id + 1, 0 in the padding."""
    nh, nw = -(-H // ws), -(-W // ws)
    Hp, Wp = nh * ws, nw * ws
    out = np.zeros((B, nh * nw, ws * ws), np.int64)
    for b in range(B):
        for wy in range(nh):
            for wx in range(nw):
                for i in range(ws * ws):
                    y, x = (wy * ws + i // ws + sh) % Hp, (wx * ws + i % ws + sh) % Wp
                    if y < H and x < W:
                        out[b, wy * nw + wx, i] = (b * H + y) * W + x + 1
    return out


@pytest.mark.parametrize('case', SG.WINDOW_CASES)
def test_the_twin_cuts_windows_where_window_rows_does(case):
    B, H, W, ws, sh, Cc = SG.CASES[case]
    ids = (torch.arange(B * H * W, dtype=torch.float64) + 1).view(B, H * W, 1)
    want = _window_rows_map(B, H, W, ws, sh)
    part = SG.partition64(ids, H, W, ws, sh)[..., 0]
    assert tuple(part.shape) == SG.out_shape(case)[:3] and np.array_equal(part.numpy().astype(np.int64), want)
    assert np.array_equal(SG.pad_rows(case).numpy(), want == 0)
    # reverse: every token comes back from the row the map put it in, and the padding is dropped
    assert torch.equal(SG.reverse64(part.unsqueeze(-1), H, W, ws, sh), ids)
    if case == 'pad_shift_c96':
        assert (want == 0).sum() == B * (14 * 21 - 10 * 15) and sh > 0          # padding on both axes and a seam
    if case == 'one_window_c1024':
        assert (want != 0).sum() == 15 and want.shape[1:] == (1, 49)            # mostly padding


def test_twin_gradients_are_those_of_layer_norm():
    """The twin's autograd gradients of the identity-map case against the closed form the kernel evaluates."""
    v = SG.inputs('rows_c96', 'f32')
    y, dx, dg, db = SG.ln_twin('rows_c96', 'f32')
    x, g, dy = v['x'].double(), v['gamma'].double(), v['dy'].double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + SG.EPS)
    xh = (x - mean) * rstd
    gg = dy * g
    want = rstd * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    assert torch.allclose(dx, want, rtol=0, atol=1e-12) and torch.allclose(dg, (dy * xh).sum((0, 1)), rtol=0, atol=1e-12)
    assert torch.allclose(db, dy.sum((0, 1)), rtol=0, atol=1e-12) and torch.allclose(y, xh * g + v['beta'].double(), rtol=0, atol=1e-12)


def test_the_switch_is_off_and_cpu_tensors_take_todays_path(monkeypatch):
    """G10 on the CPU (the bound of tests/test_host_logic.py): with the switch off, and with it on (CPU tensors never qualify),
    SwinBlock.forward is today's two lines and no dhdx_* entry point is reached."""
    import dhd_amd
    from dhd_amd import _lib
    from dhd_amd.swin import SwinBlock
    from test_host_logic import swin_from_fixture
    assert 'DHD_SWIN_GLUE' in os.environ or SwinBlock.fused_glue is False      # off unless the environment asks
    seen = []
    real = _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (seen.append(what), real(rc, what))[1])
    g = golden('g10_swin')
    outs = {}
    for on in (False, True):
        net = swin_from_fixture(g)
        blocks = dhd_amd.fused_swin_glue(net, on)
        assert len(blocks) == 6 and all(isinstance(b, SwinBlock) and b.fused_glue is on for b in blocks)
        x = torch.from_numpy(g['x']).requires_grad_()
        o = net(x)
        sum(t.sum() for t in o).backward()
        outs[on] = [t.detach() for t in o] + [x.grad]
    for i in range(3):
        ref = g[f'out{i}']
        assert np.abs(outs[False][i].numpy() - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), i
    assert all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))
    assert not any(w.startswith('dhdx') for w in seen), seen
    assert callable(dhd_amd.layer_norm_rows) and callable(dhd_amd.window_reverse_add)
    with pytest.raises(_lib.DhdError):                                          # no fallback: the operators are HIP only
        dhd_amd.layer_norm_rows(torch.rand(2, 3, 8), torch.ones(8), torch.zeros(8), 1e-5)
    with pytest.raises(_lib.DhdError):
        dhd_amd.window_reverse_add(torch.rand(1, 1, 16, 8), torch.rand(1, 9, 8), 3, 3, 4, 0)
