"""Every HIP operator inside guard bands, with the buffers it writes at exactly their advertised sizes.

The views test (test_gpu_views.py) carves the INPUTS out of poisoned parents.  This module does the same for what the operators
write: outputs, gradients, `saved` / `state` blocks, workspaces and pooled scratch, all of which the wrappers allocate with
torch.empty / empty_like / zeros / zeros_like / new_zeros.  tests/guarded_alloc.py puts each such allocation between two
4096-byte bands of 0xA5 at its exact byte size and starts the pools and caches of the product empty, so that scratch is the
size THIS call advertises (dhd_sfa_stage_workspace_bytes, dhd_mghs_workspace_bytes, dhd_bev_pool_v2_fused_workspace_bytes, ...)
and not what an earlier test left in the pool.

One case = one operator at one small shape, run three times on identical inputs:
    plain (today's path) -- guarded with every `empty` byte 0xFF (NaN in every float type) -- guarded with every byte 0x00
and it asserts
  1. no guard byte of any buffer allocated inside dhd_amd/ changed (an overrun of up to 4096 bytes, forwards or backwards);
  2. the three runs give the same results -- torch.equal for the deterministic kernels, the operator's own parity bound where
     its row documents float atomics -- and the 0xFF run is finite wherever the plain run is: a kernel that reads workspace it
     never filled, or accumulates into an output it never initialised, gives different results under the two fills;
  3. the case is not vacuous: allocations were made inside dhd_amd/, and every C entry point the row names was called;
  4. every input equals its clone from before the runs.

Cases: every row of test_gpu_views.ROWS (the table is imported, not copied), plus the operators that table lacks -- window
attention forward and backward, deformable convolution at inference, the SFA stage at ragged pixel counts and at the batch
split of its GEMM launcher, the regrouping of bev_pool_v2, the atomic DCN forms, the static lift, the debug / statistics
read-outs of the view transform and the graph-capture twin of the EMA update.  test_every_entry_point_is_in_a_guarded_case
holds the list of cases against dhd_amd._lib._PROTOTYPES.

Limits: a write more than 4096 bytes outside a buffer is not seen; buffers torch itself allocates (autograd, .contiguous(),
.to(), .clone()) are not guarded."""
import ctypes as C
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
from test_gpu_views import BF16, CL, F16, F32, ROWS, Case, Row, _fresh_run, _randn, _record, _rel_close, _row_values, _vt_inputs  # noqa: E402

ME = os.path.abspath(__file__)
FILLS = (0xFF, 0x00)


def _extra(name, values, run, entries, tol=None, close=None, src='', specified=None):
    """A row for an operator the views table lacks: nothing is presented as a view, the fresh run is the case."""
    row = Row(name, values, run, dict(_=('fresh',)), entries, tol=(lambda t, k: tol) if tol is not None else None, close=close, src=src)
    row.specified = specified
    return row


EXTRA = []


# ---- Swin window attention, forward and fused backward (dhd_amd.window_attn) ---------------------------------------------

def _window_attn_row(case, prec):
    import window_attn_train_inputs as WT
    wh, ww, n, b, nw, nh = WT.geometry(case)

    def values(gpu):
        _, table, regions = WT.inputs(case)
        v = dict(qkv=WT.stored_qkv(case, prec).to(gpu), dout=WT.stored_dout(case, prec).to(gpu), table=table.to(gpu))
        if regions is not None:
            v['regions'] = regions.to(gpu)
        return v

    def run(c, v):
        from dhd_amd import window_attn
        x, t = c.inp('qkv', v['qkv'], grad=True), c.inp('table', v['table'], grad=True)
        out = window_attn(x, t, (wh, ww), nh, WT.SCALE, regions=v.get('regions'))
        out.backward(v['dout'])
        return dict(out=out.detach(), dqkv=x.grad, dtable=t.grad)

    def close(key, got, ref, tol_):
        # test_gpu_window_attn_train.py: out and dqkv are reproducible bit for bit; dtable is accumulated with LDS float atomics
        # and is held to its bound against the float64 gradient, |g - G| <= 1e-4 max(1, |G|max), never compared byte for byte
        if key != 'dtable':
            return torch.equal(got, ref)
        g64, e = WT.gradients(case, prec)[1], WT.bound_dtable(case, prec)
        return all(float((t.detach().cpu().double() - g64).abs().max()) <= e * WT.scale_of(g64) for t in (got, ref))

    return _extra('window_attn_%s_%s' % (case, prec), values, run, ('dhd_window_attn_infer', 'dhd_window_attn_backward'), tol=1.0,
                  close=close, src='test_autograd_gives_the_c_abi_bytes (dtable: bound_dtable against float64)')


EXTRA += [_window_attn_row(case, prec) for case in ('win3x5_nonsquare_nh2', 'ws12_24x36_shift6_b2_nh4')
          for prec in ('f32_bf16x3', 'fp16', 'bf16')]


# ---- deformable convolution at inference (dhd_amd.deform_conv) -----------------------------------------------------------

def _dcn_infer_row(case, prec, layout):
    # the kernel's pixel tile is 128 (csrc/deform_conv.hip: kPix): h * w = 1 is the smallest map of dcn_infer_inputs.CASES, 6 x 10 the
    # smallest case by bytes; both are a single partial tile
    import dcn_infer_inputs as DI
    b, c, o, g, h, w, dil, scale = DI.CASES[case]
    assert (h * w) % 128 != 0

    def values(gpu):
        _, offset, weight = DI.inputs(case)
        x = DI.stored_x(case, prec).to(gpu)
        return dict(x=x.contiguous(memory_format=CL) if layout == 'channels_last' else x, offset=offset.to(gpu), weight=weight.to(gpu))

    def run(c_, v):
        from dhd_amd import deform_conv_infer
        out = deform_conv_infer(c_.inp('x', v['x']), c_.inp('offset', v['offset']), c_.inp('weight', v['weight']), padding=dil, dilation=dil, groups=g)
        assert tuple(out.shape) == (b, o, h, w) and out.dtype == v['x'].dtype
        return dict(out=out)

    return _extra('deform_conv_infer_%s_%s_%s' % (case, prec, layout), values, run, ('dhd_deform_conv_infer',),
                  src='same kernel, no atomics: test_gpu_deform_conv_infer.py')


EXTRA += [_dcn_infer_row(case, prec, layout) for case in ('one_cell_1x256x1x1', 'g13_2x32x6x10') for prec in ('f32_bf16x3', 'fp16')
          for layout in ('nchw', 'channels_last')]


# ---- SFA stage at ragged pixel counts and at the launcher's batch split ---------------------------------------------------

def _sfa_ragged_row(shape, dtype, train, gemm=None):
    b, c2, h, w = shape

    def values(gpu):
        return dict(x=_randn(shape, 111, gpu, dtype), g=_randn((b, c2 // 2, h, w), 112, gpu, dtype))

    def run(c, v):
        from dhd_amd import _lib
        from dhd_amd.mix import channel_spatial_stage, fused_stage_supported, inference_selected
        torch.manual_seed(0)
        st = channel_spatial_stage(c2)
        sp = st.spacial_leanring
        with torch.no_grad():
            for bn in (sp[1], sp[4]):
                bn.running_mean.uniform_(-0.2, 0.2)
                bn.running_var.uniform_(0.5, 1.5)
        st = st.to(v['x'].device).train(train)
        st.gemm = gemm
        x = c.inp('x', v['x'], grad=train)
        assert fused_stage_supported(st, x)
        if dtype != F32:
            assert _lib.value('dhd_sfa_stage_half_storage_supported', c2 // 2, h * w) and st.half_storage
        if not train:
            with torch.no_grad():
                assert inference_selected(st, x)
                return dict(y=st(x))
        y = st(x)
        y.backward(v['g'])
        out = dict(y=y.detach(), gx=x.grad)
        out.update({'d_' + n: p.grad for n, p in st.named_parameters()})
        out.update({'buf_' + n: t for n, t in st.named_buffers()})
        return out

    name = 'sfa_%s_%s_%s%s' % ('train' if train else 'infer', 'x'.join(map(str, shape)), str(dtype)[6:], '_' + gemm if gemm else '')
    return _extra(name, values, run, ('dhd_sfa_stage_forward', 'dhd_sfa_stage_backward') if train else ('dhd_sfa_stage_infer',),
                  src='same kernels: test_sfa_stage_is_bit_reproducible_and_precision_is_per_instance')


EXTRA += [_sfa_ragged_row((3, 256, 6, 10), F32, True), _sfa_ragged_row((3, 256, 6, 10), F32, False),        # hw = 60: one partial tile
          _sfa_ragged_row((1, 256, 10, 10), F32, True),                                                     # hw = 100
          _sfa_ragged_row((1, 256, 8, 9), F16, True), _sfa_ragged_row((1, 256, 8, 9), F16, False),          # hw = 72, half storage
          _sfa_ragged_row((1, 256, 8, 9), BF16, True), _sfa_ragged_row((1, 256, 8, 9), BF16, False),
          # C = 256: six samples are more than fit beside the resident weights, the GEMM launcher splits them 4 + 2
          # (the comment at test_sfa_stage_vs_torch)
          _sfa_ragged_row((6, 512, 2, 6), F32, True, gemm='bf16x3')]


# ---- bev_pool_v2: the regrouping of the backward (test_bev_pool_v2_regroup_vs_argsort) -----------------------------------

def _regroup_row():
    lists = ((5000, 700), (3, 64))

    def values(gpu):
        g = torch.Generator().manual_seed(3)
        v = {}
        for i, (n_points, n_pixels) in enumerate(lists):
            rf = torch.randint(0, n_pixels, (n_points,), generator=g)
            if n_points > 100:
                rf[::3] = 17                     # a heavy pixel
                rf[5] = n_pixels + 4             # out of range: dropped
                rf[6] = -2
            rd = torch.randperm(n_points, generator=g)
            rb = torch.randint(0, 1000, (n_points,), generator=g)
            v.update({'rf%d' % i: rf.int().to(gpu), 'rd%d' % i: rd.int().to(gpu), 'rb%d' % i: rb.int().to(gpu)})
        return v

    def run(c, v):
        import importlib
        from dhd_amd import _lib
        bp = importlib.import_module('dhd_amd.bev_pool_v2')
        out = {}
        for i, (n_points, n_pixels) in enumerate(lists):
            res = bp._regrouped(_lib.load(), c.inp('rd', v['rd%d' % i]), c.inp('rf', v['rf%d' % i]), c.inp('rb', v['rb%d' % i]), n_pixels)
            out.update({'%s%d' % (k, i): t for k, t in zip(('rd_bp', 'rf_bp', 'rb_bp', 'starts', 'lengths'), res)})
        bp.clear_caches()
        return out

    def specified(out):
        # include/dhd_amd.h, dhd_bev_pool_v2_regroup: "The *_bp lists have n_points entries (only the first sum(lengths) are
        # written)" -- the entries behind the kept points are unspecified
        res = dict(out)
        for i in range(len(lists)):
            kept = int(out['lengths%d' % i].sum())
            for k in ('rd_bp', 'rf_bp', 'rb_bp'):
                res['%s%d' % (k, i)] = out['%s%d' % (k, i)][:kept]
        return res

    return _extra('bev_pool_v2_regroup', values, run, ('dhd_bev_pool_v2_regroup',), specified=specified,
                  src='integer counting sort: test_bev_pool_v2_regroup_vs_argsort')


EXTRA.append(_regroup_row())


# ---- the float32 LDS-atomic forms of the DCN sampling (test_dcn_gather_col2im_vs_atomic_form_and_typed_columns) -----------

def _dcn_atomic_row():
    b, ch, h, w, k, dil, scale = 2, 8, 6, 10, 3, 1, 40.0      # that test's smallest case: offsets of +-40 pixels, most taps outside

    def values(gpu):
        return dict(x=_randn((b, ch, h, w), 121, gpu), off=_randn((b, 2 * k * k, h, w), 122, gpu, scale=scale),
                    dcol=_randn((b, ch * k * k, h * w), 123, gpu))

    def run(c, v):
        from dhd_amd import _lib
        from dhd_amd.depthnet import _DeformIm2col
        lib = _lib.load()
        x, off, dcol = c.inp('x', v['x']), c.inp('off', v['off']), c.inp('dcol', v['dcol'])
        st = _lib.stream_ptr(x.device)
        with torch.cuda.device(x.device):
            col32 = torch.empty((b, ch * k * k, h * w), dtype=F32, device=x.device)       # allocated here: guarded as this file is a root
            _lib.check(lib.dhd_deform_im2col(_lib.ptr(x), _lib.ptr(off), _lib.ptr(col32), b, ch, h, w, k, dil, dil, st), 'dhd_deform_im2col')
            dx0, doff0 = torch.empty_like(x), torch.empty_like(off)
            _lib.check(lib.dhd_deform_col2im(_lib.ptr(dcol), _lib.ptr(x), _lib.ptr(off), _lib.ptr(dx0), _lib.ptr(doff0), b, ch, h, w, k, dil, dil, st),
                       'dhd_deform_col2im')
        # the product's node on the same inputs (typed entry points, gather form): the same columns and offset gradient
        xa, offa = x.clone().requires_grad_(), off.clone().requires_grad_()
        col = _DeformIm2col.apply(xa, offa, k, dil, dil, F32)
        col.backward(dcol)
        assert torch.equal(col.detach(), col32) and torch.equal(offa.grad, doff0)
        return dict(col32=col32, dx0=dx0, doff0=doff0, gx=xa.grad)

    def close(key, got, ref, tol_):      # that test: dx of the atomic and of the gather form 2e-5 (summation order), the rest identical
        return _rel_close(key, got, ref, 2e-5) if key in ('dx0', 'gx') else torch.equal(got, ref)

    return _extra('deform_atomic_forms_2x8x6x10', values, run, ('dhd_deform_im2col', 'dhd_deform_col2im', 'dhd_deform_im2col_t', 'dhd_deform_col2im_t'),
                  tol=1.0, close=close, src='test_dcn_gather_col2im_vs_atomic_form_and_typed_columns (dx 2e-5)')


EXTRA.append(_dcn_atomic_row())


# ---- view transform: static lift, debug keys, statistics, the streaming writer on views ----------------------------------

def _mghs_static_row():
    """C = 64, three cameras, 4 x 11 maps (the size of test_accelerate_caches_only_what_is_static), deterministic mode, a
    workspace with a scratch of its own: a full lift, the read-outs, a static lift with another height map, the read-outs, and
    the two phases of the forward on tensor views."""
    state = {}

    def values(gpu):
        cfg, plan, calib, keep, depth, feat, height = _vt_inputs(gpu, 64)
        state.update(cfg=cfg, plan=plan, calib=calib, keep=keep)
        return dict(depth=depth, feat=feat, height=height, height2=height.roll(1, dims=-1).contiguous())

    def run(c, v):
        from dhd_amd import _lib, mghs_op
        cfg, plan, calib = state['cfg'], state['plan'], state['calib']
        lib = _lib.load()
        dev = v['depth'].device
        depth, feat = c.inp('depth', v['depth']), c.inp('feat', v['feat'])
        hr, mr = cfg['height_range'], cfg['mask_range']
        res = {}
        with torch.no_grad():
            ws = plan.new_workspace(dev, private_scratch=True)
            for frame, key in enumerate(('height', 'height2')):
                outs = mghs_op.mghs_lift_pool(plan, calib, c.inp(key, v[key]), hr, mr, depth, feat, ws, static=frame > 0)
                res.update({'frame%d_out%d' % (frame, i): o for i, o in enumerate(outs)})
                res['frame%d_keys' % frame] = mghs_op.debug_keys(plan, ws)
                res['frame%d_stats' % frame] = torch.tensor(mghs_op.stats(plan, ws))
            _, feat_nhwc = mghs_op.lift(plan, calib, c.inp('height', v['height']), hr, mr, feat, ws)
            outs = mghs_op._alloc_outputs(plan, 'collapsed', dev, F32)
            arr = mghs_op._views(plan, 'collapsed', outs)
            with torch.cuda.device(dev):
                st = _lib.stream_ptr(dev)
                _lib.check(lib.dhd_mghs_forward_gather(C.byref(plan.desc), _lib.ptr(depth), _lib.ptr(feat_nhwc), C.byref(ws.c), st),
                           'dhd_mghs_forward_gather')
                _lib.check(lib.dhd_mghs_forward_stream_views(C.byref(plan.desc), _lib.ptr(depth), _lib.ptr(feat_nhwc), C.byref(arr), C.byref(ws.c), st),
                           'dhd_mghs_forward_stream_views')
            res.update({'phases_out%d' % i: o for i, o in enumerate(outs)})
        return res

    return _extra('mghs_static_lift_and_readouts_c64', values, run,
                  ('dhd_mghs_lift', 'dhd_mghs_lift_static', 'dhd_mghs_debug_keys', 'dhd_mghs_stats', 'dhd_mghs_forward_views', 'dhd_mghs_forward_gather',
                   'dhd_mghs_forward_stream_views'), src='deterministic mode: test_accelerate_caches_only_what_is_static')


EXTRA.append(_mghs_static_row())


# ---- EMA: the eager update and its graph-capture twin, called eagerly ------------------------------------------------------

def _ema_dev_row():
    sizes = [1, 3, 64, 1023, 5000]      # test_ema_update_ragged_state_vs_oracle: odd lengths, more than one chunk

    def values(gpu):
        from dhd_amd import synthetic as syn
        total = sum(sizes)
        return dict(flat=torch.from_numpy(syn.hash_signed(310, (total,))).to(gpu), step=torch.from_numpy(syn.hash_signed(311, (total,))).to(gpu))

    def run(c, v):
        from dhd_amd import _lib
        from dhd_amd.ema import ModelEMA

        def net_of(flat):
            net = torch.nn.Module()
            net.p = torch.nn.ParameterList(torch.nn.Parameter(t.clone()) for t in flat.split(sizes))
            return net
        flat, step = c.inp('flat', v['flat']), c.inp('step', v['step'])
        ema = ModelEMA(net_of(flat), decay=0.999, updates=100)
        model = net_of(flat + step)
        ema.update(None, model)                        # eager: dhd_ema_update; allocates the device-side {d, 1 - d}
        after_one = [p.detach().clone() for p in ema.ema.p]
        ema.advance()                                  # the host side of a captured update: the next decay, on the device
        for dev, tab in ema._tables.items():           # the launch a capture would record, made eagerly
            with torch.cuda.device(dev):
                _lib.check(_lib.load().dhd_ema_update_dev(_lib.ptr(tab.ema_addr), _lib.ptr(tab.model_addr), _lib.ptr(tab.len), tab.n,
                                                          _lib.ptr(ema._decay_dev[dev]), _lib.stream_ptr(dev)), 'dhd_ema_update_dev')
        torch.cuda.synchronize()
        res = {'one%d' % i: p for i, p in enumerate(after_one)}
        res.update({'two%d' % i: p.detach().clone() for i, p in enumerate(ema.ema.p)})
        d = ema.decay(ema.updates)                     # sanity: the twin made the second update, with the second decay
        for i, (p1, m) in enumerate(zip(after_one, model.p)):
            assert torch.allclose(res['two%d' % i], p1 * d + m.detach() * (1.0 - d), rtol=1e-5, atol=1e-6), i
        return res

    return _extra('ema_update_and_capture_twin', values, run, ('dhd_ema_update', 'dhd_ema_update_dev'),
                  src='element-wise: test_ema_update_ragged_state_vs_oracle')


EXTRA.append(_ema_dev_row())

ALL = list(ROWS) + EXTRA


# ------------------------------------------------------------------------------------------------ coverage (no GPU needed)

def test_every_entry_point_is_in_a_guarded_case():
    """Every launching entry point of the C ABI is named by a guarded case, whose GPU run proves that it was reached.  Left out:
    the benchmark's bandwidth probe (a caller-owned buffer, no layout) and the two cross-rank phases of the SFA stage (two
    ranks; the layouts of the one-call forms)."""
    from dhd_amd import _lib
    names = {n for n in _lib._PROTOTYPES if not n.endswith(('_supported', '_bytes')) and n != 'dhd_abi_version'}
    names -= {'dhd_hbm_calibrate', 'dhd_sfa_stage_forward_phase', 'dhd_sfa_stage_backward_phase'}
    covered = {e for row in ALL for e in row.entries}
    assert names - covered == set(), sorted(names - covered)
    assert covered <= set(_lib._PROTOTYPES), sorted(covered - set(_lib._PROTOTYPES))
    assert len({row.name for row in ALL}) == len(ALL)


# ------------------------------------------------------------------------------------------------ the cases

def _fresh_target(row):
    return next(t for t, kinds in row.present.items() if 'fresh' in kinds)


def _guarded_run(row, v, fill, monkeypatch):
    with monkeypatch.context() as mp:
        seen = _record(mp)
        with G.guarded(mp, fill, roots=(G.PRODUCT_ROOT, ME)) as ledger:
            try:
                out = row.run(Case(None, 'fresh'), v)
                torch.cuda.synchronize()
            except RuntimeError as e:      # a device fault poisons the process: nothing more is started on the GPU
                if 'HIP error' in str(e) or 'illegal memory access' in str(e) or 'hipError_t' in str(e):
                    pytest.exit(f'{row.name} [fill {fill:#04x}]: GPU fault, stopping the module: {e}', returncode=3)
                raise
            ledger.check()
            out = {k: t.detach().clone() for k, t in out.items()}
    return out, ledger, {name for how, name in seen if how == 'call'}


def _bytes(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize('row', ALL, ids=[row.name for row in ALL])
def test_operator_inside_guard_bands(gpu, monkeypatch, row):
    t0 = time.perf_counter()
    target = _fresh_target(row)
    v, const = _row_values(row, gpu, target, 'fresh')
    snap = {k: t.detach().clone() for k, t in v.items() if torch.is_tensor(t)}
    plain, _, _ = _fresh_run(row, gpu, v, const, monkeypatch)          # asserts that every entry of the row is reached
    tol = row.tol(target, 'fresh')
    specified = getattr(row, 'specified', None) or (lambda out: out)
    plain = specified(plain)
    how = 'torch.equal' if tol is None else 'bound of ' + row.src
    for fill in FILLS:
        got, ledger, called = _guarded_run(row, v, fill, monkeypatch)
        inside = ledger.sites_under(G.PRODUCT_ROOT)
        print(f'{row.name} [fill {fill:#04x}]: {len(ledger)} guarded allocations ({len(inside)} inside dhd_amd/), {ledger.total_bytes()} bytes; '
              f'guards intact; compared with the plain run by {how}')
        # 3. not vacuous
        assert inside, 'no allocation inside dhd_amd/ was guarded'
        assert set(row.entries) <= called, sorted(set(row.entries) - called)
        # 2. the same results as the plain run
        got = specified(got)
        assert set(got) == set(plain)
        for k in plain:
            a, b = got[k], plain[k]
            assert a.shape == b.shape and a.dtype == b.dtype, k
            if a.is_floating_point():
                holes = int((torch.isfinite(b) & ~torch.isfinite(a)).sum())
                assert holes == 0, f'{k} [fill {fill:#04x}]: {holes} elements are not finite where the plain run is finite'
            if tol is None:
                assert torch.equal(a, b), (k, fill, int((a != b).sum()), float((a.double() - b.double()).abs().max()) if a.numel() else 0.0)
            else:
                assert row.close(k, a, b, tol), (k, fill, float((a.double() - b.double()).abs().max()))
    # 4. the inputs are only read
    for k, s in snap.items():
        assert torch.equal(_bytes(v[k]), _bytes(s)), f'input {k} changed'
    print(f'{row.name}: {time.perf_counter() - t0:.2f} s')


@pytest.mark.gpu
def test_a_flipped_guard_byte_on_the_device_is_reported(gpu, monkeypatch):
    """The harness on the device: one byte of a rear guard is changed through the parent, an ordinary in-bounds indexing write."""
    with G.guarded(monkeypatch, 0xFF, roots=(ME,)) as ledger:
        t = torch.empty((3, 5), dtype=torch.float16, device=gpu); line = sys._getframe().f_lineno
        z = torch.zeros(7, dtype=torch.int32, device=gpu)
        assert len(ledger) == 2 and t.is_cuda and t.data_ptr() % 512 == ledger.entries[0].parent.data_ptr() % 512
        assert bool(torch.isnan(t).all()) and bool((z == 0).all())
        ledger.check()
        e = ledger.entries[0]
        e.parent[G.GUARD + e.nbytes + 2] ^= 0xFF
        with pytest.raises(G.GuardError) as err:
            ledger.check()
        msg = str(err.value)
        assert f'test_gpu_guard_bands.py:{line}' in msg and 'rear guard' in msg and '2 bytes past the end' in msg and msg.count('guard changed') == 1
    assert torch.empty(3, device=gpu).untyped_storage().nbytes() == 12
