"""The Swin training step in the configuration DHD-L trains in -- net.train() with DropPath drawing, checkpointed blocks, autocast,
and window attention (fused_inference / fused_training), the block glue, the stage seams, fused_swin_ffn and
fused_swin_ffn_training all switched on -- against a float64 copy of the same network on the CPU into which the DropPath masks
of the run are replayed (tests/swin_train_step_inputs.py; its CPU test shows that the replay is wired to the right modules).
Weights, input, loss and sizes are fixture G20's (tests/swin_wide_inputs.py): (2, 3, 96, 136), token maps 24 x 34 -> 3 x 5;
drop_path_rate is 0.5, so the blocks' rates are 0, 1/14, ..., 1/2.  The helpers, the recorder and the float32 bar are those of
tests/test_gpu_swin_composed.py.

What is compared, element by element: the three outputs, the input gradient and the gradient of every parameter, the Linear
weights included (36.3 M elements; fixture G20 holds only a norm and a projection of those).

Seeds.  DropPath.forward draws floor(keep + torch.rand((2, 1, 1))) in the dtype of its input, the attention's DropPath and then
the FFN's in every block but the first: 14 draws in float32, or in the autocast type under autocast.  `_seed` makes those draws
itself after torch.cuda.manual_seed and takes the first seed of SEEDS at which some block of stage 0 or 1 drops exactly one of the
two images in its FFN DropPath and some block drops exactly one in its attention DropPath, so that a per-image factor handed to
the wrong image shows.  The choice never looks at a fused result, and `_case` asserts that today's path drew what was predicted.

Bounds.  float32: the composed test's n x 1e-4 x max(1, |R|max), R the float64 tensor and n the fused calls upstream, counted
from the expected-calls table below; a tensor at which today's float32 path is itself outside that bound is held to 1.5 x today's
error (DESIGN.md section 6 lists them).  Autocast: the relative L2 error against float64 may be at most 1.5 x the error today's
autocast path makes under the same seed, tensor by tensor; a gradient that is exactly zero in float64 (the parameters of a branch
whose DropPath dropped both images) must be exactly zero.  No bound is taken from the fused path."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_train_step_inputs as TS  # noqa: E402
import swin_wide_inputs as SW  # noqa: E402
import test_gpu_swin_composed as TC  # noqa: E402
from test_gpu_swin_composed import (ADD, ATTN, ATTN_B, BAR, EMBED, EMBED_B, LN, LN_B, MERGE, MERGE_B, ROWS, _calls_upto,  # noqa: E402
                                    _net, _recorder, _route_all, _switch, _sync)

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
MARGIN = 1.5
FWD, BWD = 'dhdt_swin_ffn_forward', 'dhdt_swin_ffn_backward'
FAMILY = dict(TC.FAMILY, ffn_train=('dhdt_',))
SWITCHES = ('attn', 'glue', 'seams', 'ffn', 'ffn_train')      # attn: fused_inference and fused_training together
SEEDS = range(100, 164)
pytestmark = pytest.mark.gpu

# What the routing tables route as shipped, by the dtype of the run (float32, or the autocast type): the stages whose FFN is the
# training operator (swin_ffn.ROUTED_TRAIN: C = 256 only with half tokens) and the merges that are patch_merge_norm
# (swin_seam.ROUTED: not C = 512, and C = 256 with fp16 tokens was not measured).
SHIPPED_FFN = {F32: (0,), BF16: (0, 1), F16: (0, 1)}
SHIPPED_MERGES = {F32: (0, 1), BF16: (0, 1), F16: (0,)}


def _expected(dtype=F32, routing='shipped', off=None):
    """The calls of one step with grad (train mode, or eval mode with grad) -> (forward [(label, names)] in order, backward as a
    multiset, {stage: fused calls of its backward}; stage -1 is the patch embed), on the pattern of TC._expected / TC._grad_tables.
    Per block: norm1 into the windows, the attention, reverse + add, then the second half as the training operator where it is
    routed; elsewhere under autocast norm2 is layer_norm_rows (it emits the dtype fc1 reads) and in float32 it is torch's."""
    glue, attn, seams, ffn_train = (off != k for k in ('glue', 'attn', 'seams', 'ffn_train'))
    everything = routing == 'all_routed'
    ffn_stages = (0, 1) if everything else SHIPPED_FFN[dtype]
    merges = (0, 1, 2) if everything else SHIPPED_MERGES[dtype]
    forward, backward, per_stage = [('embed', [EMBED] if seams else [])], collections.Counter([EMBED_B] if seams else []), {-1: int(seams)}
    for s in range(4):
        f, b = ([LN, ATTN, ADD], [ROWS, ATTN_B, LN_B]) if glue else ([ROWS, ATTN, ROWS], [ROWS, ATTN_B, ROWS])
        if not attn:
            f, b = [n for n in f if n != ATTN], [n for n in b if n != ATTN_B]
        if ffn_train and s in ffn_stages:
            f, b = f + [FWD], b + [BWD]
        elif glue and dtype != F32:
            f, b = f + [LN], b + [LN_B]
        forward.append((f'stage{s}', f * 2))
        names = b * 2
        if s < 3:
            merged = seams and s in merges
            forward.append((f'merge{s}', [MERGE] if merged else []))
            names = names + ([MERGE_B] if merged else [])
        backward.update(names)
        per_stage[s] = sum(n != ROWS for n in names)
    return forward, backward, per_stage


def _calls_of(name, forward, per_stage):
    """The fused calls upstream of an output, of the input gradient or of a parameter's gradient."""
    if name.startswith('out'):
        return _calls_upto(forward, TC.LABEL_OF[name])
    return TC._grad_calls(None if name == 'x_grad' else name, forward, per_stage)


def _route(monkeypatch, routing):
    if routing == 'all_routed':
        from dhd_amd import swin_ffn
        _route_all(monkeypatch)
        monkeypatch.setattr(swin_ffn, 'ROUTED_TRAIN', TC._Everything())


def _train_net(gpu, with_cp=False, off=None, on=True):
    """G20's network with drop_path_rate 0.5 in train mode, every switch on but `off` (on=False: every switch off, today's path)."""
    import dhd_amd
    net = _net(gpu, drop_path_rate=TS.DROP_PATH_RATE, with_cp=with_cp).train()
    sw = {k: on and k != off for k in SWITCHES}
    _switch(net, attn=sw['attn'], train=sw['attn'], glue=sw['glue'], ffn=sw['ffn'], seams=sw['seams'])
    assert len(dhd_amd.fused_swin_ffn_training(net, sw['ffn_train'])) == 8
    return net


def _step(net, x, auto=None, seed=None):
    """TC._grad_step from a seeded generator with the forward under autocast -> ({name: tensor} of the outputs, x_grad and every
    parameter gradient, the generator's state afterwards)."""
    if seed is not None:
        torch.cuda.manual_seed(seed)
    x = x.clone().requires_grad_()
    net.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=auto or BF16, enabled=auto is not None):
        outs = net(x)
    SW.backward_of(outs)
    _sync()
    got = {f'out{i}': o.detach() for i, o in enumerate(outs)}
    got['x_grad'] = x.grad
    got.update({n: p.grad for n, p in net.named_parameters()})
    return got, torch.cuda.get_rng_state(x.device)


def _typed(monkeypatch):
    """(name, args) of every call of the training-FFN and seam surfaces: the dtype codes are among the arguments."""
    from dhd_amd import _ffn_train, _seam
    calls = []
    for m in (_ffn_train, _seam):
        m.load()

        def call(name, *args, real=m.call):
            calls.append((name, args))
            return real(name, *args)
        monkeypatch.setattr(m, 'call', call)
    return calls


# ------------------------------------------------------------------------------------------------ seeds, today's path, the reference

_cache = {}


def _seed(gpu, dtype):
    """(seed, its 14 draws as [[image 0, image 1]]): the first of SEEDS that meets the condition of the module docstring."""
    if ('seed', dtype) not in _cache:
        keeps = [1 - dp.drop_prob for _, dp in TS.drop_paths(TS.net())]
        assert len(keeps) == TS.DRAWS
        found = None
        for seed in SEEDS:
            torch.cuda.manual_seed(seed)
            draws = [(k + torch.rand((2, 1, 1), dtype=dtype, device=gpu)).floor().view(-1).tolist() for k in keeps]
            one = [sorted(d) == [0.0, 1.0] for d in draws]                   # draw i: block i // 2 + 1, the attention's when i is even
            if any(one[i] for i in (1, 3, 5)) and any(one[0::2]):            # FFN of blocks 1, 2, 3 (stages 0 and 1); any attention
                found = (seed, draws)
                break
        assert found is not None, f'no seed of {SEEDS} meets the condition in {dtype}'
        print(f'\n{dtype}: seed {found[0]}; kept (image 0, image 1) per draw, attention then FFN of blocks 1 .. 7: '
              + ' '.join(f'{int(a)}{int(b)}' for a, b in found[1]))
        _cache['seed', dtype] = found
    return _cache['seed', dtype]


def _case(gpu, dtype):
    """Per dtype, made once and left unchanged: the seed, today's path (every switch off, with_cp=False) with its masks recorded
    and the generator state it ends in, the float64 replay of those masks on the CPU, and today's errors against it."""
    if ('case', dtype) not in _cache:
        seed, draws = _seed(gpu, dtype)
        auto = None if dtype == F32 else dtype
        net = _train_net(gpu, on=False)
        with pytest.MonkeyPatch.context() as m:
            seen = _recorder(m)
            with TS.record_masks(net) as masks:
                today, state = _step(net, TC._x(gpu), auto, seed)
        assert not any(n.startswith(s) for stems in FAMILY.values() for s in stems for n in seen), seen
        assert len(masks) == TS.DRAWS and all(mk.dtype == dtype for mk in masks)
        assert [mk.view(-1).tolist() for mk in masks] == draws               # today's path drew what _seed predicted
        outs, xg, grads, taken = TS.reference_step([mk.double().cpu() for mk in masks], state=TC._state())
        assert taken == TS.DRAWS
        ref = {f'out{i}': o for i, o in enumerate(outs)}
        ref['x_grad'] = xg
        ref.update(grads)
        assert list(ref) == list(today)
        ref = {k: v.to(gpu) for k, v in ref.items()}
        case = dict(seed=seed, state=state, ref=ref, ref_max={k: float(v.abs().max()) for k, v in ref.items()},
                    ref_norm={k: float(v.norm()) for k, v in ref.items()}, dtypes={k: v.dtype for k, v in today.items()})
        case['today_abs'], case['today_rel'] = _errors(today, case)
        _cache['case', dtype] = case
    return _cache['case', dtype]


def _errors(got, case):
    """-> ({name: max |got - ref|}, {name: ||got - ref|| / ||ref||}) against the float64 replay."""
    ea, er = {}, {}
    for k, r in case['ref'].items():
        assert got[k].shape == r.shape, k
        d = got[k].double() - r
        # a branch whose DropPath drops both images has gradients that are exactly zero: then 0 for zeros and inf for anything else
        size, dn = case['ref_norm'][k], float(d.norm())
        ea[k], er[k] = float(d.abs().max()), dn / size if size else (0.0 if dn == 0 else float('inf'))
    return ea, er


def _hold_float32(got, case, forward, per_stage, what):
    """Print fused error | today's float32 error | bound for every tensor, then assert."""
    ea, _ = _errors(got, case)
    rows = []
    for k, e in ea.items():
        n, t = _calls_of(k, forward, per_stage), case['today_abs'][k]
        b = n * BAR * max(1.0, case['ref_max'][k])
        rows.append((k, e, t, n, b, b if t <= b else MARGIN * t))
    print(f'\n{what}\n  fused error   today         calls  bound       tensor')
    for k, e, t, n, b, limit in rows:
        print(f'  {e:.3e}     {t:.3e}     {n:>3}    {b:.3e}   {k}' + (f'   today is outside the bound: held to {limit:.3e}' if limit != b else ''))
    failures = [(k, f'{e:.3e} > {limit:.3e}') for k, e, t, n, b, limit in rows if not e <= limit]
    assert not failures, (what, failures)


def _hold_autocast(got, case, what):
    """Print fused | today's relative L2 error against float64 and their ratio for every tensor, then assert the ratio."""
    _, er = _errors(got, case)
    print(f'\n{what}\n  fused rel L2  today         ratio   tensor')
    failures = []
    for k, e in er.items():
        t = case['today_rel'][k]
        print(f'  {e:.3e}     {t:.3e}     {e / t if t else float("inf"):.3f}   {k}')
        assert got[k].dtype == case['dtypes'][k], k
        if not e <= MARGIN * t:                                             # (today exact: the fused path has to be exact too)
            failures.append((k, f'{e:.3e} against {t:.3e} today'))
    assert not failures, (what, failures)


def _hold_calls(calls, forward, backward, doubled=False):
    """The recorded calls against the table: the forward in order, the backward as a multiset.  With checkpointing (`doubled`)
    every block's forward runs a second time inside the backward, so the whole list is held as a multiset."""
    flat = TC._flat(forward)
    nf = len(flat)
    assert calls[:nf] == flat, (calls[:nf], flat)
    rest = collections.Counter(calls[nf:])
    if doubled:
        rest -= collections.Counter(n for label, names in forward if label.startswith('stage') for n in names)
        assert sum(rest.values()) == sum(backward.values())
    assert rest == backward, (rest, backward)


# ------------------------------------------------------------------------------------------------ a. float32, train mode

@pytest.mark.parametrize('routing', ['shipped', 'all_routed'])
def test_float32_train_step(gpu, monkeypatch, routing):
    case = _case(gpu, F32)
    _route(monkeypatch, routing)
    forward, backward, per_stage = _expected(F32, routing)
    net = _train_net(gpu)
    seen = _recorder(monkeypatch)
    got, state = _step(net, TC._x(gpu), None, case['seed'])
    calls = list(seen)
    _hold_calls(calls, forward, backward)
    stages_with_ffn = [label for label, names in forward if FWD in names]
    assert stages_with_ffn == (['stage0'] if routing == 'shipped' else ['stage0', 'stage1'])
    for name in (ATTN_B, LN_B, EMBED_B, MERGE_B, FWD, BWD):
        assert name in calls, name
    assert torch.equal(state, case['state'])
    _hold_float32(got, case, forward, per_stage, f'float32, train mode, everything on, routing {routing}, seed {case["seed"]}')


# ------------------------------------------------------------------------------------------------ b. autocast, train mode, with_cp

@pytest.mark.parametrize('routing', ['shipped', 'all_routed'])
@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'fp16'])
def test_autocast_train_step_with_cp(gpu, monkeypatch, dtype, routing):
    from dhd_amd._lib import DTYPE_CODE
    case = _case(gpu, dtype)
    _route(monkeypatch, routing)
    forward, backward, _ = _expected(dtype, routing)
    net = _train_net(gpu, with_cp=True)
    seen, typed = _recorder(monkeypatch), _typed(monkeypatch)
    got, state = _step(net, TC._x(gpu), dtype, case['seed'])
    _hold_calls(list(seen), forward, backward, doubled=True)
    # the half routes: the training FFN of stage 1 (C = 256) on half tokens, forward and backward, and a seam backward that is
    # handed a half gradient (... x code, GEMM code, rows, C, hidden, eps, stream; merge: x, dy, ..., x code, dy code, B, H, W, C, ...)
    half = DTYPE_CODE[dtype]
    for name, count in ((FWD, 4), (BWD, 2)):
        wide = [a for n, a in typed if n == name and a[-4] == 256]
        assert len(wide) == count and all(a[-7] == half and a[-6] == half for a in wide), (name, [(a[-7], a[-6]) for a in wide])
        narrow = [a for n, a in typed if n == name and a[-4] == 128]
        assert len(narrow) == count and all(a[-7] == DTYPE_CODE[F32] and a[-6] == half for a in narrow), name
    merges = [a for n, a in typed if n == MERGE_B]
    assert merges and all(a[9] == half for a in merges) and any(a[8] == half for a in merges) == (routing == 'all_routed' or dtype == BF16)
    assert [a[9] for n, a in typed if n == EMBED_B] == [DTYPE_CODE[F32]]
    assert torch.equal(state, case['state'])                                 # the generator ends where today's path leaves it
    _hold_autocast(got, case, f'{dtype} autocast, train mode, with_cp, everything on, routing {routing}, seed {case["seed"]}')


# ------------------------------------------------------------------------------------------------ c. leave one out

@pytest.mark.parametrize('off', SWITCHES)
def test_leave_one_out_float32(gpu, monkeypatch, off):
    case = _case(gpu, F32)
    _route(monkeypatch, 'all_routed')
    forward, backward, per_stage = _expected(F32, 'all_routed', off)
    net = _train_net(gpu, off=off)
    seen = _recorder(monkeypatch)
    got, state = _step(net, TC._x(gpu), None, case['seed'])
    calls = list(seen)
    assert not any(n.startswith(FAMILY[off]) for n in calls), (off, calls)
    _hold_calls(calls, forward, backward)
    assert torch.equal(state, case['state'])
    _hold_float32(got, case, forward, per_stage, f'float32, train mode, everything on but {off}, seed {case["seed"]}')


# ------------------------------------------------------------------------------------------------ d. checkpointing

@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16_autocast'])
def test_with_cp_gives_the_bits_of_the_unchecked_step(gpu, monkeypatch, dtype):
    """Train mode, everything on: every block runs twice with with_cp=True, both fused draws (the attention's in the glue, the
    FFN's in _ffn_half) are made again from the restored generator, and outputs, x.grad, every gradient and the generator's final
    state are those of the with_cp=False step.  torch's convolution is asked for its deterministic weight gradient."""
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    seed, _ = _seed(gpu, dtype)
    auto = None if dtype == F32 else dtype
    forward, backward, _ = _expected(dtype)
    seen = _recorder(monkeypatch)
    plain, state = _step(_train_net(gpu), TC._x(gpu), auto, seed)
    _hold_calls(list(seen), forward, backward)
    plain = {k: v.clone() for k, v in plain.items()}
    del seen[:]
    cp, cp_state = _step(_train_net(gpu, with_cp=True), TC._x(gpu), auto, seed)
    _hold_calls(list(seen), forward, backward, doubled=True)
    differ = [k for k in plain if not (cp[k].dtype == plain[k].dtype and torch.equal(cp[k], plain[k]))]
    for k in differ:
        print(f'  with_cp: {k}: max difference {float((cp[k].double() - plain[k].double()).abs().max()):.3e} of {float(plain[k].abs().max()):.3e}')
    assert not differ, differ
    assert torch.equal(cp_state, state)
    torch.cuda.manual_seed(seed)
    assert not torch.equal(torch.cuda.get_rng_state(gpu), state)             # and draws there were


# ------------------------------------------------------------------------------------------------ e. graph capture

@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16_autocast'])
def test_graph_capture_of_forward_and_backward(gpu, monkeypatch, dtype):
    """Eval mode with grad (no draw, so a replay is comparable), with_cp=False, everything on: forward + backward captured once as
    one graph; after the static input is refilled, two replays each give the bits of the eager step on that input."""
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    net = _train_net(gpu).eval()
    params = dict(net.named_parameters())
    static = TC._x(gpu).requires_grad_()
    other = TC._x(gpu).flip(0).flip(-1).contiguous()
    weights = [torch.from_numpy(SW.loss_weight(i, shape)).to(gpu, F32) for i, shape in enumerate(SW.OUT_SHAPES)]

    def run():
        with torch.autocast('cuda', dtype=BF16, enabled=dtype != F32):
            outs = net(static)
        sum((o * w).sum() for o, w in zip(outs, weights)).backward()
        # detached: a grad-tracking output of an earlier eager step that is still held while forward + backward are captured
        # crashes the capture in PyTorch-ROCm (tests/test_gpu_parity.py, the captured SFA step, met the same)
        return [o.detach() for o in outs]

    def clear():
        static.grad = None
        net.zero_grad(set_to_none=True)

    def collect(outs):
        got = {f'out{i}': o.detach().clone() for i, o in enumerate(outs)}
        got['x_grad'] = static.grad.clone()
        got.update({n: p.grad.clone() for n, p in params.items()})
        return got

    forward, backward, _ = _expected(dtype)
    with monkeypatch.context() as m:
        seen = _recorder(m)
        clear()
        eager = {}
        for key, x in (('first', TC._x(gpu)), ('other', other)):
            with torch.no_grad():
                static.copy_(x)
            clear()
            del seen[:]
            outs = run()
            _sync()
            eager[key] = collect(outs)
        _hold_calls(list(seen), forward, backward)
    assert all(o.dtype == F32 for o in outs) and not torch.equal(eager['first']['out2'], eager['other']['out2'])
    with torch.no_grad():
        static.copy_(TC._x(gpu))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        clear()
        run()
    torch.cuda.current_stream().wait_stream(side)
    _sync()
    clear()                                                                  # the captured backward allocates the gradients: static memory of the graph
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    _sync()
    graph.replay()
    _sync()
    got = collect(outs)
    differ = [k for k in got if not torch.equal(got[k], eager['first'][k])]
    assert not differ, ('replay on the captured input', differ)
    with torch.no_grad():
        static.copy_(other)
    for attempt in (1, 2):
        graph.replay()
        _sync()
        got = collect(outs)
        differ = [k for k in got if not torch.equal(got[k], eager['other'][k])]
        assert not differ, (f'replay {attempt} on the refilled input', differ)
