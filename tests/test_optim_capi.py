"""The optimizer-step surface `dhdw_*` of libdhd_amd.so (dhd_amd/capi_optim/dhd_amd_optim.h, dhd_amd/_optim.py) without a GPU:
header, binding table and exports agree and leave the other surfaces alone; the header is plain C; the structs the kernels are
compiled with and the ones the binding uploads are the header's; the build keeps its 22 units; the entry points refuse bad
input on the host with the documented code."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
CAPI = os.path.join(ROOT, 'dhd_amd', 'capi_optim')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
HEADER = os.path.join(CAPI, 'dhd_amd_optim.h')
EINVAL, ENOSPACE = -1, -2
WANT = ['dhdw_optim_adamw_update', 'dhdw_optim_finalize', 'dhdw_optim_grad_norm', 'dhdw_optim_workspace_bytes']


def _uncommented(path):
    return re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)


def _declarations():
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(?:int|size_t)\s+(dhdw_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _uncommented(HEADER))}


def _structs(text):
    """name -> the members' text with white space squeezed, of every `typedef struct name { ... } name;`."""
    return {m.group(1): ' '.join(m.group(2).split()) for m in re.finditer(r'typedef struct (\w+) \{(.*?)\} \1;', text, flags=re.S)}


def test_header_binding_table_and_exports_agree():
    from dhd_amd import (_deform_train, _ext, _ffn, _ffn_train, _ffn_wide, _ffn_wide_train, _lib, _occ_loss_head, _occ_train, _optim,
                         _seam)
    decl = _declarations()
    assert sorted(decl) == WANT == sorted(_optim.EXPORTED_SYMBOLS)
    lib = _optim.load()
    assert lib is _lib.load()                                        # the same library, the same handle
    for name, (argtypes, restype) in _optim._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
        assert len(argtypes) == len([p for p in decl[name].split(',') if p.strip() != 'void']), name
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdw_[a-z0-9_]+)', out)) == set(WANT)
    for other in (_lib, _ext, _ffn, _ffn_wide, _seam, _ffn_train, _ffn_wide_train, _occ_train, _deform_train, _occ_loss_head):
        assert not any(n.startswith('dhdw') for n in other._PROTOTYPES), other.__name__
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert os.listdir(CAPI) == ['dhd_amd_optim.h']


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_optim.h"\n'
                   'int main(void) { dhdw_optim_tables t; t.n_chunks = 0; return dhdw_optim_workspace_bytes(t.n_chunks) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, '-I' + CAPI, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_kernels_and_the_binding_use_the_headers_structs(tmp_path):
    from dhd_amd import _optim
    header, kernels = _uncommented(HEADER), re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, 'optim_step.h')).read())
    want = _structs(header)
    assert sorted(want) == ['dhdw_optim_chunk', 'dhdw_optim_group', 'dhdw_optim_tables'] and _structs(kernels) == want
    macros = dict(re.findall(r'#define (DHDW_OPTIM_\w+) (\d+)', header))
    assert macros == dict(re.findall(r'#define (DHDW_OPTIM_\w+) (\d+)', kernels)) and len(macros) == 5
    assert (_optim.CHUNK, _optim.RECORD_AT, _optim.MULT_AT, _optim.FOUND_AT, _optim.PARTIALS_AT) == tuple(
        int(macros['DHDW_OPTIM_' + k]) for k in ('CHUNK', 'RECORD_AT', 'MULT_AT', 'FOUND_AT', 'PARTIALS_AT'))
    # sizes and offsets as the C compiler lays the header's structs out, against ctypes and numpy
    src = tmp_path / 'layout.c'
    fields = {'dhdw_optim_chunk': [n for n in _optim.CHUNK_DTYPE.names], 'dhdw_optim_group': [n for n in _optim.GROUP_DTYPE.names],
              'dhdw_optim_tables': [n for n, _ in _optim.Tables._fields_]}
    body = ''.join(f'  printf("{s} %zu", sizeof({s}));' + ''.join(f' printf(" %zu", offsetof({s}, {f}));' for f in fs) + ' printf("\\n");\n'
                   for s, fs in fields.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dhd_amd_optim.h"\nint main(void) {\n' + body + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I' + INCLUDE, '-I' + CAPI, str(src), '-o', str(exe)], check=True, capture_output=True)
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()}
    assert got['dhdw_optim_chunk'] == [64] + [_optim.CHUNK_DTYPE.fields[n][1] for n in _optim.CHUNK_DTYPE.names]
    assert got['dhdw_optim_group'] == [40] + [_optim.GROUP_DTYPE.fields[n][1] for n in _optim.GROUP_DTYPE.names]
    assert got['dhdw_optim_tables'] == [C.sizeof(_optim.Tables)] + [getattr(_optim.Tables, n).offset for n, _ in _optim.Tables._fields_]


def test_the_build_keeps_its_units_and_knows_the_headers():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert len(srcs) == 22 and not [f for f in os.listdir(CSRC) if f.endswith('.hip') and 'optim' in f]      # no new translation unit
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    for h in ('optim_step.h', '../capi_optim/dhd_amd_optim.h'):
        assert h in rule, h
    text = open(os.path.join(CSRC, 'ema.hip')).read()
    assert text.index('float ema1(') < text.index('#include "optim_step.h"')          # the EMA arithmetic is the one definition
    assert 'ema1(' in open(os.path.join(CSRC, 'optim_step.h')).read()


def _tables(**kw):
    from dhd_amd import _optim
    P = 0x10000
    base = dict(chunks=P, groups=P, slot_group=P, steps=P, slot_scalars=P, group_scalars=P, decay_pair=P, scale=P, growth_tracker=P,
                n_chunks=3, n_groups=2, n_slots=2, n_partials=4)
    base.update(kw)
    return _optim.Tables(**base)


def test_workspace_bytes():
    from dhd_amd import _optim
    lib = _optim.load()
    assert lib.dhdw_optim_workspace_bytes(-1) == 0 and lib.dhdw_optim_workspace_bytes(0) == 64
    for n in (1, 2, 3, 4, 2300, 1 << 20):
        got = lib.dhdw_optim_workspace_bytes(n)
        assert got % 16 == 0 and 64 + 12 * n <= got < 64 + 12 * n + 16, n


def test_the_entry_points_refuse_bad_input_on_the_host():
    """Fake addresses, no device: every call below returns before any launch."""
    from dhd_amd import _optim
    lib = _optim.load()
    W = C.c_void_p(0x20000)
    need = lib.dhdw_optim_workspace_bytes(4)
    calls = {
        'dhdw_optim_grad_norm': lambda t, ws=W, n=need: lib.dhdw_optim_grad_norm(t, ws, n, None),
        'dhdw_optim_finalize': lambda t, ws=W, n=need, max_norm=5.0: lib.dhdw_optim_finalize(t, max_norm, 2.0, 0.5, 2000, ws, n, None),
        'dhdw_optim_adamw_update': lambda t, ws=W, n=need: lib.dhdw_optim_adamw_update(t, ws, n, None),
    }
    for name, call in calls.items():
        assert call(None) == EINVAL, name
        assert call(C.byref(_tables()), ws=None) == EINVAL, name
        assert call(C.byref(_tables()), ws=C.c_void_p(0x20008)) == EINVAL, name             # 16-byte alignment of the workspace ...
        assert call(C.byref(_tables(chunks=0x10008))) == EINVAL, name                       # ... and of the chunk table
        assert call(C.byref(_tables(chunks=None))) == EINVAL, name
        for bad in (dict(n_chunks=-1), dict(n_groups=-1), dict(n_slots=-1), dict(n_partials=2)):
            assert call(C.byref(_tables(**bad))) == EINVAL, (name, bad)
        for n in (0, 64, need - 1):
            assert call(C.byref(_tables()), n=n) == ENOSPACE, (name, n)
        assert call(C.byref(_tables(chunks=None)), n=0) == EINVAL, name                     # the pointer test first, the size check last
    fin, norm, upd = calls['dhdw_optim_finalize'], calls['dhdw_optim_grad_norm'], calls['dhdw_optim_adamw_update']
    assert fin(C.byref(_tables()), max_norm=float('nan')) == EINVAL
    assert fin(C.byref(_tables(growth_tracker=None))) == EINVAL and norm(C.byref(_tables(growth_tracker=None))) == EINVAL
    for member in ('groups', 'slot_group', 'steps', 'slot_scalars', 'group_scalars'):
        assert fin(C.byref(_tables(**{member: None}))) == EINVAL, member
    for member in ('groups', 'slot_scalars', 'group_scalars'):
        assert upd(C.byref(_tables(**{member: None}))) == EINVAL, member
    # nothing to do is not an error, and launches nothing
    empty = _tables(chunks=None, n_chunks=0, n_partials=0)
    assert norm(C.byref(empty), n=64) == 0 and upd(C.byref(empty), n=64) == 0
