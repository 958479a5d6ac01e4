"""dhd_sfa_stage_infer on the GPU: every form returns the bytes of dhd_sfa_stage_forward(training = 0), through the C ABI and
through channel_spatial_stage; nothing is written but `out`; no `saved` tensor; capturable in a HIP graph."""
import ctypes as C

import numpy as np
import pytest
import torch

from dhd_amd import synthetic as syn
from test_gpu_parity import GEMM_MODES, T, _check_stage_against_torch, _TIE, gemm_mode
from test_oracle_golden import g5b_inputs

pytestmark = pytest.mark.gpu

FORMS = {'auto': 0, 'unfused': 1, 'two_pass': 2, 'one_pass': 3}
# precision of a call: (name, storage dtype, I/O dtype)
PRECISIONS = [('f32', None, torch.float32), ('f32_io_f16', None, torch.float16), ('f32_io_bf16', None, torch.bfloat16),
              ('f16_storage', torch.float16, torch.float16), ('bf16_storage', torch.bfloat16, torch.bfloat16)]
# (form, kind, C) combinations that return DHD_EUNSUPPORTED (-3); kind = the GEMM precision on float32 storage, 'half' for half
# storage (whose single half products ignore `gemm`).  Half storage has no C = 512 at all, in the forward either.
UNSUPPORTED = {
    'auto': {('half', 512)},
    'unfused': {('half', 512)},
    'two_pass': {('bf16x6', 128), ('bf16x6', 256), ('bf16x6', 512), ('f32', 128), ('f32', 256), ('f32', 512), ('bf16x3', 512),
                 ('half', 512)},
    'one_pass': {(k, c) for k in ('bf16x3', 'bf16x6', 'f32') for c in (128, 256, 512)} | {('half', 512)},
}


def _make_stage(c, gpu, seed):
    from dhd_amd.mix import channel_spatial_stage
    torch.manual_seed(seed)
    st = channel_spatial_stage(2 * c).to(gpu)
    with torch.no_grad():  # non-trivial BatchNorm state
        for bn in (st.spacial_leanring[1], st.spacial_leanring[4]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    return st.eval()


def _abi_forward_and_infer(st, x, gemm, storage, io, forms):
    """(rc, out) of dhd_sfa_stage_forward(training = 0), then {form: (rc, out)} of dhd_sfa_stage_infer on the same arguments."""
    from dhd_amd import _lib
    from dhd_amd.mix import _stage_params, _stage_weights
    lib = _lib.load()
    dev = x.device
    b, c2, h, w = x.shape
    c, hw = c2 // 2, h * w
    st.gemm = gemm
    wts, ps = _stage_weights(st, _stage_params(st), io, storage is not None)
    assert wts.training == 0
    stream = _lib.stream_ptr(dev)
    ns, nt = C.c_size_t(), C.c_size_t()
    rc = lib.dhd_sfa_stage_workspace_bytes(b, c, hw, wts.hidden, wts.storage_dtype, C.byref(ns), C.byref(nt))
    ref = torch.full((b, c, h, w), float('nan'), dtype=io, device=dev)
    if rc == 0:
        saved = torch.empty(ns.value, dtype=torch.uint8, device=dev)
        scratch = torch.empty(nt.value, dtype=torch.uint8, device=dev)
        rc = lib.dhd_sfa_stage_forward(_lib.ptr(x), C.byref(wts), _lib.ptr(ref), _lib.ptr(saved), _lib.ptr(scratch), b, c, hw, stream)
        torch.cuda.synchronize()
        del saved, scratch
    res = {}
    for name in forms:
        form = FORMS[name]
        n = C.c_size_t()
        rs = lib.dhd_sfa_stage_infer_scratch_bytes(b, c, hw, wts.hidden, wts.storage_dtype, wts.gemm, form, C.byref(n))
        sup = lib.dhd_sfa_stage_infer_supported(c, hw, wts.storage_dtype, wts.gemm, form)
        assert (rs == 0) == (sup == 1) and rs in (0, -3), (name, rs, sup)
        # stale bytes in scratch and out: nothing may depend on what an earlier call left
        scratch = torch.full((max(n.value, 16) if rs == 0 else 16,), 0xCD, dtype=torch.uint8, device=dev)
        out = torch.full((b, c, h, w), float('nan'), dtype=io, device=dev)
        ri = lib.dhd_sfa_stage_infer(_lib.ptr(x), C.byref(wts), _lib.ptr(out), _lib.ptr(scratch), b, c, hw, form, stream)
        torch.cuda.synchronize()
        assert ri == rs, (name, ri, rs)
        res[name] = (ri, out)
        del scratch
    del ps
    return (rc, ref), res


@pytest.mark.parametrize('prec', PRECISIONS, ids=[p[0] for p in PRECISIONS])
@pytest.mark.parametrize('gemm', ['bf16x3', 'bf16x6', 'f32'])
@pytest.mark.parametrize('c,b,h,w', [(128, 2, 20, 28), (128, 3, 36, 40), (256, 2, 52, 60),
                                     (256, 6, 12, 20),     # more samples than coefficient tables fit beside the tiles
                                     (256, 1, 18, 76),     # hw = 1368: a multiple of 8, not of 32 or 64
                                     (512, 1, 24, 40)])
def test_every_form_is_bit_identical_to_the_eval_forward(gpu, c, b, h, w, gemm, prec):
    _, storage, io = prec
    st = _make_stage(c, gpu, c + h)
    x = (torch.randn(b, 2 * c, h, w, device=gpu) * 0.7 + 0.1).to(storage or torch.float32)
    state0 = {k: v.clone() for k, v in st.state_dict().items()}
    (rc, ref), res = _abi_forward_and_infer(st, x, gemm, storage, io, list(FORMS))
    kind = 'half' if storage is not None else gemm
    assert rc == (-3 if (kind, c) == ('half', 512) else 0)
    if rc == 0:
        assert torch.isfinite(ref.float()).all()
    for name, (ri, out) in res.items():
        if (kind, c) in UNSUPPORTED[name]:
            assert ri == -3, (name, kind, c, ri)
            continue
        assert ri == 0, (name, kind, c, ri)
        assert torch.equal(out, ref), (name, kind, c, (out.float() - ref.float()).abs().max().item())
    # TWO_PASS must exist for bf16x3 on float32 storage and for both half storages at C = 128 / 256
    if c in (128, 256) and (storage is not None or gemm == 'bf16x3'):
        assert res['two_pass'][0] == 0
    for k, v in st.state_dict().items():   # running statistics, num_batches_tracked and the parameters are only read
        assert torch.equal(v, state0[k]), k


@pytest.mark.parametrize('b,storage,io', [(4, torch.float16, torch.float16), (2, None, torch.float32)], ids=['fp16_storage', 'f32_bf16x3'])
def test_auto_is_bit_identical_at_full_size(gpu, b, storage, io):
    st = _make_stage(256, gpu, 3)
    x = (torch.randn(b, 512, 200, 200, device=gpu) * 0.7 + 0.1).to(storage or torch.float32)
    (rc, ref), res = _abi_forward_and_infer(st, x, 'bf16x3', storage, io, ['auto'])
    assert rc == 0 and res['auto'][0] == 0
    assert torch.equal(res['auto'][1], ref)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('form', [None, 'unfused', 'two_pass', 'one_pass'])
def test_module_takes_the_inference_operator_and_matches_the_training_operator(gpu, dtype, form):
    from dhd_amd import mix
    if form == 'one_pass' and dtype == torch.float32:
        form = 'two_pass'                          # (float32 storage has no one-pass form)
    st = _make_stage(256, gpu, 17)
    st.infer_form = form
    x = (torch.randn(2, 512, 36, 44, device=gpu) * 0.7 + 0.1).to(dtype)
    calls = []
    orig = mix._infer_stage
    mix._infer_stage = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        with torch.no_grad():
            out = st(x)
            assert calls == [1]
            st.infer = False
            ref = st(x)
            assert calls == [1]
    finally:
        mix._infer_stage = orig
    assert out.dtype == dtype and out.grad_fn is None and torch.equal(out, ref)


@pytest.mark.parametrize('gemm', list(GEMM_MODES))
def test_module_inference_vs_float64_oracle(gpu, gemm):
    """The forward bound of test_fused_sfa_stage_vs_float64_oracle (atol = 1e-5 f, rtol = 1e-4), eval mode, on the
    inference operator."""
    from oracle import mghs_oracle as O
    from test_oracle_golden import stage_args
    from dhd_amd.mix import channel_spatial_stage, fused_stage_supported, inference_selected
    st = channel_spatial_stage(512)
    shapes = {k: tuple(v.shape) for k, v in st.state_dict().items() if v.dtype.is_floating_point}
    sd = syn.hashed_state(shapes, 77)
    st.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    st = st.to(gpu).eval()
    x_np = syn.hash_signed(78, (2, 512, 18, 22)) * np.float32(0.7) + np.float32(0.1)
    x = T(x_np, gpu)
    with gemm_mode(gemm) as f, torch.no_grad():
        assert fused_stage_supported(st, x) and inference_selected(st, x)
        out = st(x)
    ref, _, _ = O.sfa_stage(x_np, *stage_args(sd, ''), training=False, out_grad=np.zeros((2, 256, 18, 22), np.float32))
    np.testing.assert_allclose(out.cpu().numpy(), ref, atol=1e-5 * f, rtol=1e-4)


@pytest.mark.parametrize('gemm', list(GEMM_MODES))
def test_module_inference_vs_reference_c128(gpu, gemm):
    """Golden G5b `eval.stage` with the bound of test_fused_sfa_stage_vs_reference_c128."""
    from dhd_amd import SFA
    from dhd_amd.mix import inference_selected
    g, sd, x_np = g5b_inputs()
    sfa = SFA(in_channels=256, out_channels=128)
    sfa.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    sfa = sfa.to(gpu).eval()
    x = T(x_np, gpu)
    with gemm_mode(gemm) as f, torch.no_grad():
        assert inference_selected(sfa.mysk_7, x)
        stage = sfa.mysk_7(x)
    np.testing.assert_allclose(stage.cpu().numpy(), g['eval.stage'], atol=2e-5 * min(f, 5.0), rtol=1e-4)


def test_state_is_only_read_and_a_required_gradient_still_takes_the_training_operator(gpu):
    st = _make_stage(128, gpu, 5)
    x = torch.randn(2, 256, 20, 28, device=gpu) * 0.7 + 0.1
    state0 = {k: v.clone() for k, v in st.state_dict().items()}
    with torch.no_grad():
        st(x)
    torch.cuda.synchronize()
    for k, v in st.state_dict().items():
        assert torch.equal(v, state0[k]), k
    xg = x.clone().requires_grad_()
    out = st(xg)                                   # eval(), grad mode on, x requires a gradient
    assert type(out.grad_fn).__name__ == '_FusedStageBackward'
    for gemm in GEMM_MODES:
        with gemm_mode(gemm) as f:
            for p in st.parameters():
                p.grad = None
            _check_stage_against_torch(st, x.clone().requires_grad_(), tol_x=1e-4 * f, tol_p=5e-4 * f, tol_out=1e-4 * min(f, 3.0),
                                       tie=_TIE * f, rel_l2=3e-3 if f > 1.0 else 1e-4)


def test_no_saved_tensor_is_allocated(gpu):
    """Transient allocation of one module call at (2, 512, 200, 200) fp16, scratch pool warm: `out` (+ 1 MiB) with the inference
    operator, at least the library's `saved` bytes with the training operator."""
    from dhd_amd import _lib
    st = _make_stage(256, gpu, 9)
    x = (torch.randn(2, 512, 200, 200, device=gpu) * 0.7 + 0.1).half()
    lib = _lib.load()
    ns, nt = C.c_size_t(), C.c_size_t()
    assert lib.dhd_sfa_stage_workspace_bytes(2, 256, 40000, st.fc[0].weight.shape[0], 1, C.byref(ns), C.byref(nt)) == 0
    out_bytes = 2 * 256 * 40000 * 2

    def transient():
        with torch.no_grad():
            out = st(x)                             # warms the scratch pool for this kind of call
            del out
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = st(x)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            del out
        return peak - before
    t_infer = transient()
    st.infer = False
    t_train = transient()
    print('transient bytes: infer', t_infer, 'training operator', t_train, 'saved', ns.value, 'out', out_bytes)
    assert t_infer <= out_bytes + (1 << 20), t_infer
    assert t_train >= ns.value, (t_train, ns.value)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_inference_call_is_graph_capturable(gpu, dtype):
    """One stream, no parallel branches: captured, replayed on fresh contents of the static input, equal to eager bit for bit."""
    st = _make_stage(128, gpu, 21)
    x = (torch.randn(2, 256, 20, 24, device=gpu)).to(dtype)
    x2 = (torch.randn(2, 256, 20, 24, device=gpu) * 0.5 + 0.2).to(dtype)
    with torch.no_grad():
        ref1, ref2 = st(x).clone(), st(x2).clone()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            st(x)                                   # scratch and first-launch attributes on the capture stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = st(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, ref1)
        x.copy_(x2)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, ref2) and not torch.equal(ref1, ref2)
