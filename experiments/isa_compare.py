"""Did a refactor of dhd_amd/csrc/sfa_stage.hip move anything in the generated gfx950 code?  Pairs every kernel of the device assembly
at a base commit with the same kernel of the working tree and reports registers, spills, scratch, LDS and whether the instruction
streams are equal.  No GPU needed: hipcc cross-compiles (the Makefile's flags, --cuda-device-only -S, as tests/test_build_lint.py).

usage: python experiments/isa_compare.py [--base REV]            build both (REV: default HEAD) into a temporary directory
       python experiments/isa_compare.py --asm OLD.s NEW.s       compare two assembly files that exist
       ... [name-substring ...]                                  only kernels whose name contains one of these

The element-wise passes of the stage were one kernel per storage family up to r8 (`blend2_bn_kernel<TO>` for float32 storage,
`blend2_bn_h_kernel<TS>` for half storage) and are `blend2_bn_kernel<TS, TO>` since; `unified_name` maps the old names to the new.
An instruction is compared as mnemonic + operand kinds + modifiers (nt, glc, offset: ... count), register numbers and branch labels
normalised.  Verdicts, each difference listed below the table:
  same     the whole stream
  scalar   only s_* instructions differ
  address  besides, per-lane integer address arithmetic differs (ADDRESS below, and the immediate offset of a memory instruction);
           the memory, LDS, MFMA and floating-point instructions are the same sequence
  order    those are the same multiset in another order
  DIFF     they are not
Exit status 1 on an order / DIFF verdict or on a kernel that gained a VGPR, an AGPR, a spill or scratch."""
import collections, difflib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt',
         '-munsafe-fp-atomics', '-Wno-unused-function', '--cuda-device-only', '-S']
TWO_TYPES = ('blend2_bn', 'blend2_bn_bwd', 'stage_gx')         # <TS, TO>
ONE_TYPE = ('pair_sums', 'blend1_da', 'plane_mean_pack')       # <TS>
META = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
        'group_segment_fixed_size')


def device_asm(csrc, out):
    subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + [os.path.join(csrc, 'sfa_stage.hip'), '-o', out],
                   check=True, capture_output=True)
    return out


def short_name(demangled):
    """'void (anonymous namespace)::k<float, 3>(float const*, ...)' -> 'k<float, 3>'"""
    s = re.sub(r'^void ', '', demangled)
    s = re.sub(r'^(?:\(anonymous namespace\)::|dhd_sfa::|dhd::)+', '', s)
    m = re.match(r'\w+', s)
    end = m.end()
    if s[end:end + 1] == '<':
        depth = 0
        for end in range(m.end(), len(s)):
            depth += {'<': 1, '>': -1}.get(s[end], 0)
            if depth == 0:
                break
        end += 1
    return s[:end].replace('(anonymous namespace)::', '')


def unified_name(name):
    m = re.match(r'(\w+?)(_h)?_kernel(?:<(.*)>)?$', name)
    if not m or m.group(1) not in TWO_TYPES + ONE_TYPE:
        return name
    base, half, args = m.group(1), m.group(2), [a.strip() for a in (m.group(3) or '').split(',') if a.strip()]
    if len(args) == (2 if base in TWO_TYPES else 1) and not half:
        return name                                             # the new spelling already
    ts = args[0] if half else 'float'
    new = [ts, ts if half else args[0]] if base in TWO_TYPES else [ts]
    return '%s_kernel<%s>' % (base, ', '.join(new))


def normalise(line):
    line = line.split(';')[0].strip()
    line = re.sub(r'\.LBB\d+_\d+', 'L', line)
    line = re.sub(r'\b([vsa])\[(\d+):(\d+)\]', lambda m: '%s%d' % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1), line)
    line = re.sub(r'\b([vsa])\d+\b', r'\1', line)
    return re.sub(r'\s+', ' ', line)


def kernels(path):
    """{short name: (metadata dict, [normalised instructions])}"""
    text = open(path).read()
    meta = {}
    for blk in text[text.index('amdhsa.kernels:'):].split('\n  - .agpr_count')[1:]:
        blk = '.agpr_count' + blk
        meta[re.search(r'\.name:\s+(\S+)', blk).group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)) for k in META}
    names = sorted(meta)
    # binutils' c++filt does not know DF16_ (_Float16) and DF16b (__bf16): lend them the codes of two builtin types no kernel uses
    lent = '\n'.join(names).replace('DF16_', 'Dh').replace('DF16b', 'Ds')
    dem = subprocess.run(['c++filt'], input=lent, capture_output=True, text=True).stdout.replace('half', '_Float16').replace('char16_t', '__bf16')
    dem = dem.split('\n')
    out = {}
    for sym, d in zip(names, dem):
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end' % re.escape(sym), text, re.S | re.M).group(1)
        ins = [normalise(l) for l in body.split('\n') if l.startswith('\t') and not l.lstrip().startswith(('.', ';'))]
        out[short_name(d)] = (meta[sym], [i for i in ins if i])
    return out


def is_scalar(ins):
    return ins.startswith('s_')


# per-lane integer address arithmetic and register moves; an immediate offset of a memory instruction belongs to it
ADDRESS = ('v_mov_b32_e32', 'v_lshl_add_u64', 'v_add_co_u32_e32', 'v_addc_co_u32_e32', 'v_ashrrev_i32_e32', 'v_lshlrev_b64')


def without_address(stream):
    return [re.sub(r' offset:-?\d+', '', i) for i in stream if i.split(' ')[0] not in ADDRESS]


def main():
    argv = sys.argv[1:]
    if argv[:1] == ['--asm']:
        old_s, new_s, pats = argv[1], argv[2], argv[3:]
    else:
        base = 'HEAD'
        if argv[:1] == ['--base']:
            base, argv = argv[1], argv[2:]
        pats = argv
        tmp = tempfile.mkdtemp(prefix='isa_compare_')
        tar = subprocess.run(['git', '-C', ROOT, 'archive', base, 'dhd_amd/csrc', 'include'], check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', tmp], input=tar, check=True)
        old_s = device_asm(os.path.join(tmp, 'dhd_amd', 'csrc'), os.path.join(tmp, 'old.s'))
        new_s = device_asm(os.path.join(ROOT, 'dhd_amd', 'csrc'), os.path.join(tmp, 'new.s'))
    old = {unified_name(k): (k, v) for k, v in kernels(old_s).items()}
    new = kernels(new_s)
    bad, notes = [], []
    print('| kernel (was) | vgpr | agpr | sgpr | spill v/s | scratch | LDS | instructions | stream |')
    print('|---|---|---|---|---|---|---|---|---|')
    for name in sorted(set(old) | set(new)):
        if pats and not any(p in name for p in pats):
            continue
        if name not in old or name not in new:
            print('| %s | only in the %s build |' % (name, 'old' if name in old else 'new'))
            bad.append(name)
            continue
        was, (mo, io) = old[name]
        mn, inn = new[name]
        vo, vn = [i for i in io if not is_scalar(i)], [i for i in inn if not is_scalar(i)]
        if io == inn:
            verdict = 'same'
        elif vo == vn:
            verdict = 'scalar'
            so, sn = [i for i in io if is_scalar(i)], [i for i in inn if is_scalar(i)]
            notes.append((name, [l for l in difflib.unified_diff(so, sn, 'old', 'new', lineterm='', n=0) if not l.startswith(('---', '+++', '@@'))]))
        else:
            verdict = ('address' if without_address(vo) == without_address(vn) else
                       'order' if collections.Counter(without_address(vo)) == collections.Counter(without_address(vn)) else 'DIFF')
            notes.append((name, [l for l in difflib.unified_diff(vo, vn, 'old', 'new', lineterm='', n=0) if not l.startswith(('---', '+++', '@@'))]))
        pair = lambda k: '%d' % mn[k] if mo[k] == mn[k] else '%d -> %d' % (mo[k], mn[k])
        grew = any(mn[k] > mo[k] for k in ('vgpr_count', 'agpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size'))
        if grew or verdict in ('order', 'DIFF'):
            bad.append(name)
        label = name if was == name else '%s (%s)' % (name, was)
        print('| `%s` | %s | %s | %s | %s / %s | %s | %s | %s | %s |' % (
            label, pair('vgpr_count'), pair('agpr_count'), pair('sgpr_count'), pair('vgpr_spill_count'), pair('sgpr_spill_count'),
            pair('private_segment_fixed_size'), pair('group_segment_fixed_size'),
            '%d' % len(inn) if len(io) == len(inn) else '%d -> %d' % (len(io), len(inn)), verdict))
    for name, lines in notes:
        print('\n%s:' % name)
        for l in lines[:40]:
            print('    ' + l)
        if len(lines) > 40:
            print('    ... %d more' % (len(lines) - 40))
    print('\n%s' % ('every kernel: same registers, same vector instruction sequence' if not bad else 'TO LOOK AT: %s' % ', '.join(bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
