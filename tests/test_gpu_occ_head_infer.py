"""dhd_occ_head_infer on the GPU: the fused occupancy head of inference against a float64 reference, through the C ABI, through
dhd_amd.occ_head_infer and through predictor.predict_occ / DHD.simple_test_occ on the G17 fixtures.

Inputs: occ_head_inputs.py.  Reference: float64 torch on the CPU.  One logit bound E per precision:
  float32 x (bf16x3)   E = 1e-3, the project's bar on the voxel logits (BASELINE north_star)
  fp16 / bf16 x        E = 2 E0 with E0 = max |reference - autocast chain| computed here on the CPU (operands rounded to the
                       half type, float32 accumulation, every Linear / Softplus output rounded); the factor 2 covers summation
                       order and rounding flips of the hidden.
Measured errors are printed by test_logits_and_class_map and recorded in docs/LAB_NOTEBOOK.md."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
from occ_head_inputs import DZ, N_CLS, autocast_chain_logits, first_argmax, head_params, make_head, make_x, reference_logits

pytestmark = pytest.mark.gpu

PRECISIONS = {'f32_bf16x3': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
LAYOUTS = ('nchw', 'channels_last')
SHAPES = [(1, 200, 200), (3, 20, 28), (2, 7, 9), (1, 1, 1)]     # (B, Dy, Dx): full size; tails, Dy != Dx; tails; one cell

prec_layout_shape = lambda f: pytest.mark.parametrize('prec', list(PRECISIONS))(
    pytest.mark.parametrize('layout', LAYOUTS)(pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))(f)))


def bound_of(prec, shape):
    if prec == 'f32_bf16x3':
        return 1e-3
    e0 = float((reference_logits(shape) - autocast_chain_logits(shape, PRECISIONS[prec]).double()).abs().max())
    return 2 * e0


def device_x(shape, prec, layout, gpu):
    x = make_x(shape).to(gpu).to(PRECISIONS[prec])
    if layout == 'channels_last':
        x = x.contiguous(memory_format=torch.channels_last)
    return x


_PARAMS = {}


def device_params(gpu):
    """The head's parameters on the device, copied once (a host-to-device copy cannot be captured into a graph)."""
    if gpu not in _PARAMS:
        _PARAMS[gpu] = head_params(make_head(), gpu)
    return _PARAMS[gpu]


def run(x, gpu, **kw):
    from dhd_amd.occ_head import occ_head_infer
    return occ_head_infer(x, *device_params(gpu), dz=DZ, **kw)


@prec_layout_shape
def test_logits_and_class_map(gpu, prec, layout, shape):
    """(1) every logit within E of the float64 reference; (2) pred is the first-maximum argmax of the call's own logits, and the
    same bytes without logits; (3) float32, fp16: pred equals the reference's argmax wherever its top-2 margin is >= 2E, with at
    most 5 % of the voxels excluded; (4) bf16: agreement with float64 no more than 0.5 points below the autocast chain's."""
    x = device_x(shape, prec, layout, gpu)
    ref = reference_logits(shape)
    E = bound_of(prec, shape)
    pred, hist, logits = run(x, gpu, return_logits=True)
    assert hist is None and pred.dtype == torch.uint8 and pred.is_contiguous() and logits.dtype == torch.float32
    b, dy, dx = shape
    assert pred.shape == (b, dx, dy, DZ) and logits.shape == (b, dx, dy, DZ, N_CLS)
    err = float((logits.cpu().double() - ref).abs().max())
    print(f'occ_head_infer {prec} {layout} {shape}: max |logit - float64| = {err:.3e}, bound E = {E:.3e}')
    assert err <= E, (err, E)
    assert torch.equal(pred, first_argmax(logits))
    only = run(x, gpu)
    assert torch.equal(only, pred)
    ref_arg = first_argmax(ref)
    got = pred.cpu()
    if prec == 'bf16':
        mine = float((got == ref_arg).float().mean())
        chain = float((first_argmax(autocast_chain_logits(shape, torch.bfloat16)) == ref_arg).float().mean())
        print(f'   argmax agreement with float64: operator {mine:.4f}, autocast chain {chain:.4f}')
        assert mine >= chain - 0.005, (mine, chain)
    else:
        top2 = ref.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) >= 2 * E
        excluded = 1.0 - float(clear.float().mean())
        print(f'   voxels with a reference top-2 margin below 2E: {100 * excluded:.2f} %')
        assert excluded <= 0.05, excluded             # otherwise the comparison below is vacuous
        assert torch.equal(got[clear], ref_arg[clear])


@prec_layout_shape
def test_histogram_equals_occ_argmax_hist_on_the_operators_logits(gpu, prec, layout, shape):
    """(5) random labels (255 included) and a random mask; a second call accumulates to twice the counts."""
    from dhd_amd.occ_loss import occ_argmax_hist
    x = device_x(shape, prec, layout, gpu)
    b, dy, dx = shape
    gen = torch.Generator().manual_seed(7)
    labels = torch.randint(0, 20, (b, dx, dy, DZ), generator=gen).to(torch.uint8)
    labels[labels >= 18] = 255
    mask = (torch.rand(b, dx, dy, DZ, generator=gen) < 0.6).to(gpu)
    labels = labels.to(gpu)
    pred, hist, logits = run(x, gpu, labels=labels, mask_camera=mask, return_logits=True)
    want_pred, want = occ_argmax_hist(logits, labels, mask)
    assert torch.equal(pred.reshape(-1), want_pred) and torch.equal(hist, want) and hist.dtype == torch.int64
    assert int(hist.sum()) == int(((labels < 18) & mask).sum())
    pred2, hist2, _ = run(x, gpu, labels=labels, mask_camera=mask, hist=hist)
    assert hist2 is hist and torch.equal(hist, 2 * want) and torch.equal(pred2, pred)
    _, nomask, _ = run(x, gpu, labels=labels)
    assert torch.equal(nomask, occ_argmax_hist(logits, labels)[1])


@prec_layout_shape
def test_stale_memory_does_not_matter_and_inputs_are_only_read(gpu, prec, layout, shape):
    """(6) through the C ABI: pred / logits pre-filled with 0xCD / NaN, scratch with 0xCD and with zeros: the same bytes."""
    from dhd_amd import _lib
    lib = _lib.load()
    x = device_x(shape, prec, layout, gpu)
    params = device_params(gpu)
    x0, p0 = x.clone(), [p.clone() for p in params]
    b, dy, dx = shape
    w = _lib.OccHeadWeights()
    w.w1, w.b1, w.w2, w.b2 = (p.data_ptr() for p in params)
    w.c, w.hidden, w.dz, w.n_classes, w.gemm = 256, 512, DZ, N_CLS, 0
    n = C.c_size_t()
    assert lib.dhd_occ_head_infer_scratch_bytes(C.byref(w), _lib.DTYPE_CODE[x.dtype], C.byref(n)) == 0 and n.value % 16 == 0
    res = []
    for fill in (0xCD, 0x00):
        scratch = torch.full((n.value,), fill, dtype=torch.uint8, device=gpu)
        pred = torch.full((b, dx, dy, DZ), 0xCD, dtype=torch.uint8, device=gpu)
        logits = torch.full((b, dx, dy, DZ, N_CLS), float('nan'), device=gpu)
        rc = lib.dhd_occ_head_infer(_lib.ptr(x), _lib.DTYPE_CODE[x.dtype], int(layout == 'channels_last'), C.byref(w), b, dy, dx,
                                    _lib.ptr(pred), _lib.ptr(logits), None, None, None, _lib.ptr(scratch), _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
        assert rc == 0
        res.append((pred, logits))
    assert torch.isfinite(res[0][1]).all() and int(res[0][0].max()) < N_CLS
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    pooled, _, pooled_logits = run(x, gpu, return_logits=True)
    assert torch.equal(pooled, res[0][0]) and torch.equal(pooled_logits, res[0][1])
    assert torch.equal(x, x0) and all(torch.equal(p, q) for p, q in zip(params, p0))


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_a_nan_in_x_reaches_the_logits_of_its_cell_and_no_other(gpu, prec, layout):
    """Softplus hands a NaN on as torch's does (no finite class map from a poisoned input).  The cell is the last one of the
    last sample, the one that the lanes past the end of a tail wave load as well."""
    shape = (2, 7, 9)
    x = device_x(shape, prec, layout, gpu)
    _, _, clean = run(x, gpu, return_logits=True)
    x[1, 5, 6, 8] = float('nan')
    _, _, logits = run(x, gpu, return_logits=True)
    poisoned = torch.zeros(logits.shape[:3], dtype=torch.bool, device=gpu)
    poisoned[1, 8, 6] = True
    assert torch.isnan(logits[poisoned]).all()
    assert torch.equal(logits[~poisoned], clean[~poisoned])


def captured_nodes(g):
    """The topology of a captured graph from the HIP runtime: (type of every node, list of (from, to) node handles)."""
    from dhd_amd import _lib
    hip = _lib.load()                               # the HIP runtime's symbols resolve through the library that links it
    graph = C.c_void_p(g.raw_cuda_graph())
    n = C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
    types = []
    for node in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        types.append(t.value)
    m = C.c_size_t()
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(m)) == 0
    src, dst = (C.c_void_p * max(m.value, 1))(), (C.c_void_p * max(m.value, 1))()
    if m.value:
        assert hip.hipGraphGetEdges(graph, src, dst, C.byref(m)) == 0
    return types, [(src[i], dst[i]) for i in range(m.value)]


@prec_layout_shape
def test_call_is_graph_capturable(gpu, prec, layout, shape):
    """(7) The captured body is the two kernel launches in a straight line (read back from the graph: two kernel nodes, one
    edge); replayed on fresh contents of the static input the graph gives the eager bytes, class map and logits."""
    x = device_x(shape, prec, layout, gpu)
    x2 = (x.float() * 0.5 + 0.25).to(x.dtype)
    if layout == 'channels_last':
        x2 = x2.contiguous(memory_format=torch.channels_last)
    assert x2.stride() == x.stride()
    eager = lambda v: [t.clone() for t in run(v, gpu, return_logits=True)[::2]]
    ref1, ref2 = eager(x), eager(x2)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(x, gpu)                                 # the pool's scratch of the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        cap = run(x, gpu, return_logits=True)[::2]
    types, edges = captured_nodes(g)
    HIP_GRAPH_NODE_TYPE_KERNEL = 0
    assert types == [HIP_GRAPH_NODE_TYPE_KERNEL] * 2, types
    assert len(edges) == 1 and edges[0][0] != edges[0][1], edges    # two nodes, one edge: a chain, nothing in parallel
    g.instantiate()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(cap, ref1))
    x.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(cap, ref2)) and not torch.equal(ref1[1], ref2[1])


# --------------------------------------------------------------------------- the module path on the G17 fixtures

def _g17_eval(gpu, name):
    """build_model and _run_product's wiring (test_voxel_logits.py), eval mode, no autograd: (model, the head's input)."""
    from dhd_amd import synthetic as syn
    from conftest import golden_calib
    from test_gpu_reference_fixtures import inject_reference_matrices
    from test_voxel_logits import build_model, lift_inputs_of, window_of
    g = golden(name)
    model, dims = build_model(g)
    B, N, ih, iw = dims
    model = model.to(gpu).eval()
    inject_reference_matrices(model.img_view_transformer, g, gpu)
    depth, feat, hidx = lift_inputs_of(g, dims)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    calib = [T(a) for a in golden_calib(g)]
    inp = [torch.zeros(B, N, 1, ih // 16, iw // 16, device=gpu)] + calib
    lo, hi = window_of(g)
    with torch.no_grad():
        bev, _, _, b1, b2, b3 = model.img_view_transformer.view_transform(inp, T(depth), T(feat), T(syn.height_probs_from_index(hidx, 65)))
        feats = list(model.encode_maps(*[m[:, :, lo:hi, lo:hi] for m in (bev, b1, b2, b3)]))
    return g, model, feats


def _off_near_ties(g, shape):
    """Where the fixture's argmax map is decided: `clear` of check_logits (small fixture) or the recorded near-tie mask (full)."""
    if 'eval.logits' in g.files:
        ref = g['eval.logits']
        top2 = np.sort(ref, axis=-1)[..., -2:]
        return (top2[..., 1] - top2[..., 0]) > 4e-3, ref.argmax(-1)
    n = int(np.prod(shape))
    return ~np.unpackbits(g['eval.occ_margin_small'])[:n].reshape(shape).astype(bool), g['eval.occ_argmax']


@pytest.mark.parametrize('name', ['g17_voxel_logits', 'g17_voxel_logits_full'])
def test_g17_module_path_and_simple_test_occ(gpu, name):
    """(8) the operator's logits pass check_logits(..., 'eval', 1e-3) on both fixtures; (9) simple_test_occ with fused_infer
    returns the fixture's argmax map off its near-tie set; (10) with fused_infer = False it returns exactly
    get_occ(occ_logits(...)), the parent's path."""
    from dhd_amd import occ_head as op
    from test_voxel_logits import check_logits
    g, model, feats = _g17_eval(gpu, name)
    head = model.occ_head
    calls = []
    orig = op.occ_head_infer
    op.occ_head_infer = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        with torch.no_grad():
            assert type(head).fused_infer is False and head.fused_infer is False
            default = model.simple_test_occ(feats)
            parent = head.get_occ(model.occ_logits(feats))
            assert calls == []                          # (10) the default path does not touch the operator
            assert len(default) == len(parent) and all(np.array_equal(a, b) for a, b in zip(default, parent))
            head.fused_infer = True
            x = model.mixed_feats(feats)
            assert head.fused_applies(x)
            occ, _, logits = head.predict_occ(x, return_logits=True)
            assert calls == [1]
            err = check_logits(logits.cpu().numpy(), g, 'eval', 1e-3)          # (8)
            print(f'G17 {name} eval, fused occupancy head: max logit error {err:.2e}')
            fused = model.simple_test_occ(feats)                                # (9)
            assert calls == [1, 1]
    finally:
        op.occ_head_infer = orig
    assert isinstance(fused, list) and fused[0].dtype == np.uint8 and all(np.array_equal(a, b) for a, b in zip(fused, occ))
    fused = np.stack(fused)
    clear, want = _off_near_ties(g, fused.shape)
    assert clear.mean() > 0.9 and np.array_equal(fused[clear], want[clear])
    # a gradient to record: the module formulation, as before
    head.fused_infer = True
    assert not head.fused_applies(model.mixed_feats(feats))                    # grad mode on, parameters require grad


def test_device_class_grid_feeds_rayiou_without_a_host_copy(gpu):
    """(11) predict_occ(..., to_host=False): a contiguous device uint8 (B, 200, 200, 16) that RayIoU.add_batch uses where it is,
    and one module call allocates the class grid (and, the first time, the pooled scratch) only."""
    import dhd_amd
    from test_gpu_ray_metrics import g19_samples
    g, model, feats = _g17_eval(gpu, 'g17_voxel_logits_full')
    head = model.occ_head
    _, gt, org = g19_samples(golden('g19_rayiou'))[0]
    with torch.no_grad():
        x = model.mixed_feats(feats)
        pred = head.predict_occ(x, to_host=False)
        y = head.final_conv(x)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        again = dhd_amd.occ_head_infer(y, *head_params(head), dz=16)
        torch.cuda.synchronize()
        transient = torch.cuda.max_memory_allocated() - before
        host = head.predict_occ(x)
    assert pred.is_cuda and pred.dtype == torch.uint8 and pred.is_contiguous() and tuple(pred.shape) == (1, 200, 200, 16)
    assert torch.equal(again, pred)
    print('transient bytes of one operator call at (1, 256, 200, 200):', transient, 'class grid', pred.numel())
    assert transient <= pred.numel() + (1 << 20), transient
    assert np.array_equal(host[0], pred[0].cpu().numpy())
    a = dhd_amd.RayIoU()
    a.device = gpu
    assert a._grids(pred, 'pred').data_ptr() == pred.data_ptr()                # no copy
    a.add_batch(pred, gt, org)
    b = dhd_amd.RayIoU()
    b.add_batch(host[0], gt, org)
    assert a.counts[0].sum() > 0 and torch.equal(a.counts, b.counts)
