"""The loss, label and head kernels at their value edges, against float64 (inputs, references and bounds: value_edge_inputs.py;
that the inputs reach the edges: test_value_edge_inputs.py).

  csrc/occ_loss.hip       dhd_occ_loss_forward / _backward, dhd_occ_argmax_hist
  csrc/label_loss.hip     dhd_sparse_bin_labels(_sid), dhd_bin_bce_forward / _backward
  csrc/mghs_softmax.hip   dhd_mghs_softmax_forward / _backward
  csrc/occ_head.hip       the class map of dhd_occ_head_infer (through predictor.predict_occ)

Bounds are the bars the operators already have against torch, taken against float64; where the float32 torch formulation itself
misses a bar, 4 x its own error (value_edge_inputs.bound).  Every case prints the kernel's error next to the reference-alone
error.  The kernels are called through the C ABI with output buffers the test owns, pre-filled with NaN / 0xCD, and every input
is compared with its clone afterwards."""
import numpy as np
import pytest
import torch

import value_edge_inputs as V

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _filled(shape, dtype, dev):
    """A buffer of 0xCD bytes (float32: -4.3e8, int16: -12851, uint8: 205) -- or NaN for a float type -- for a kernel to overwrite."""
    if dtype.is_floating_point:
        return torch.full(shape, NAN, dtype=dtype, device=dev)
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 0xCD, dtype=torch.uint8, device=dev).view(dtype).view(shape)


def _bytes_cd(n, dev):
    return torch.full((n,), 0xCD, dtype=torch.uint8, device=dev)


class _Unchanged:
    """with _Unchanged(a, b, ...): the tensors equal their clones afterwards, bit for bit."""

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if t is not None]

    def __enter__(self):
        self.clones = [t.clone() for t in self.tensors]

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        if exc[0] is None:
            for t, c in zip(self.tensors, self.clones):
                assert torch.equal(t.view(torch.uint8), c.view(torch.uint8)), 'an input was written'


# --------------------------------------------------------------------------- A. occupancy losses

def _occ_run(gpu, z, t, cam, grad_losses):
    """dhd_occ_loss_forward + _backward on buffers of the test's own -> losses (3,) float64, gradient (m, 18) float64 (CPU)."""
    from dhd_amd import _lib
    lib = _lib.load()
    m = z.shape[0]
    zd, td, cd, cw = z.to(gpu), t.to(gpu), cam.to(torch.uint8).to(gpu), V.class_weights().to(gpu)
    gl = torch.tensor(grad_losses, dtype=torch.float32, device=gpu)
    ws = _bytes_cd(lib.dhd_occ_loss_workspace_bytes(), gpu)
    losses, grad = _filled((3,), torch.float32, gpu), _filled((m, V.N_CLS), torch.float32, gpu)
    with _Unchanged(zd, td, cd, cw, gl), torch.cuda.device(gpu):
        st = _lib.stream_ptr(gpu)
        _lib.check(lib.dhd_occ_loss_forward(_lib.ptr(zd), _lib.ptr(td), _lib.ptr(cd), _lib.ptr(cw), m, V.N_CLS, V.IGNORE, V.FREE,
                                            _lib.ptr(losses), _lib.ptr(ws), st), 'dhd_occ_loss_forward')
        _lib.check(lib.dhd_occ_loss_backward(_lib.ptr(zd), _lib.ptr(td), _lib.ptr(cd), _lib.ptr(cw), m, V.N_CLS, V.IGNORE, V.FREE,
                                             _lib.ptr(gl), _lib.ptr(ws), _lib.ptr(grad), st), 'dhd_occ_loss_backward')
    return losses.cpu().double(), grad.cpu().double()


@pytest.mark.parametrize('regime,m', V.OCC_CASES)
def test_occupancy_losses_at_value_edges_vs_float64(gpu, regime, m):
    """The three losses within 2e-5 max(1, |R|) of float64 and the gradient of 0.7 CE + 1.3 sem + 2 geo within 1e-4 |G|max + 1e-9
    (a loss that the formulas make NaN -- 0 / 0 with no valid voxel -- is NaN here too and stays out of the differentiated sum).
    `underflow`: whether class i has `P_i > 0` is decided on float32 sums here as in the reference, where exp(-200) is 0; float64
    keeps 1e-87 and adds that class's precision term, -log(1e-5) / #classes.  Against float64 sem scal then gets 4 x that
    difference as its bound, so it is held to the float32 mirror within the bar as well.  `saturated_even`: every ratio is 1.0 in
    float32, where inverse_sigmoid takes two steps of 1e-5 (one step would be 3e-5 off in sem and geo scal, beyond the bar)."""
    ref = V.occ_reference(regime, m)
    z, t, cam = V.occ_case(regime, m)
    finite = torch.isfinite(ref['losses'])
    gl = [w if bool(f) else 0.0 for w, f in zip(V.LOSS_WEIGHTS, finite)]
    losses, grad = _occ_run(gpu, z, t, cam, gl)
    err = (losses - ref['losses']).abs()
    gerr = float((grad - ref['grad']).abs().max())
    print(f'{regime} m={m}: losses {losses.tolist()} error {err.tolist()} (float32 mirror alone {ref["loss_err"].tolist()}, bound '
          f'{ref["loss_bound"]}); gradient error {gerr:.3g} (mirror alone {ref["grad_err"]:.3g}, bound {ref["grad_bound"]:.3g}, '
          f'|G|max {float(ref["grad"].abs().max()):.3g})')
    assert torch.equal(torch.isnan(losses), torch.isnan(ref['losses'])) and not bool(torch.isinf(losses).any())
    if regime in ('empty_mask', 'all_ignored'):
        assert torch.isnan(losses).tolist() == [True, True, False]
    for i in range(3):
        if bool(finite[i]):
            assert float(err[i]) <= ref['loss_bound'][i], (i, float(err[i]), ref['loss_bound'][i])
    if regime == 'underflow':
        assert abs(float(losses[1]) - float(ref['mirror_losses'][1])) <= 2e-5 * max(1.0, abs(float(ref['mirror_losses'][1])))
    assert bool(torch.isfinite(grad).all())
    assert gerr <= ref['grad_bound'], (gerr, ref['grad_bound'])
    valid = cam & (t != V.IGNORE)
    assert float(grad[~valid].abs().max()) == 0.0 if bool((~valid).any()) else True


def test_occupancy_losses_nan_logits(gpu):
    """The operator's contract for NaN: a NaN logit in a VALID voxel makes all three losses NaN; a NaN logit in a voxel the
    camera mask or the ignore label excludes changes nothing -- the losses and every gradient are bit-identical to the call
    without it, and that voxel's gradient is 0.  (The torch mirror multiplies the masked voxel's cross entropy by 0 and returns
    NaN x 0 = NaN there; the kernel never reads an excluded voxel's logits.  The contract, not a bug.)"""
    from dhd_amd.occ_loss import occ_losses
    z, t, cam = (x.clone() for x in V.occ_case('confident', 257))
    cw = V.class_weights().to(gpu)
    masked = int((~cam & (t != V.IGNORE)).nonzero()[0])
    ignored = 97
    t[ignored], cam[ignored] = V.IGNORE, True                 # camera-visible, label 255
    valid = int((cam & (t != V.IGNORE)).nonzero()[5])

    def run(zz):
        a = zz.to(gpu).requires_grad_()
        ls = occ_losses(a, t.to(gpu), cam.to(gpu), cw)
        sum(w * l for w, l in zip(V.LOSS_WEIGHTS, ls)).backward()
        return torch.stack(ls).detach().cpu(), a.grad.cpu()
    base_l, base_g = run(z)
    assert bool(torch.isfinite(base_l).all())
    zn = z.clone()
    zn[masked, 3] = NAN
    zn[ignored] = NAN
    l, g = run(zn)
    assert torch.equal(l, base_l) and torch.equal(g, base_g)
    assert float(g[masked].abs().max()) == 0.0 and float(g[ignored].abs().max()) == 0.0
    zn = z.clone()
    zn[valid, 7] = NAN
    l, g = run(zn)
    assert bool(torch.isnan(l).all()), l


# --------------------------------------------------------------------------- B. bin labels

def _labels_run(gpu, name):
    """dhd_sparse_bin_labels(_sid) with the scalars dhd_amd.label_loss.bin_labels forms, on pre-filled outputs -> int64 (CPU)."""
    from dhd_amd import _lib
    lib = _lib.load()
    sid, ds = V.LABEL_CASES[name]
    neck, c = V.label_neck(name), V.label_case(name)
    gd, gh = c['gt_depth'].to(gpu), c['gt_height'].to(gpu)
    b, n, h, w = gd.shape
    fh, fw = h // ds, w // ds
    dbin, hbin = (_filled((b * n * fh * fw,), torch.int16, gpu) for _ in range(2))
    dcfg = neck.grid_config['depth']
    with _Unchanged(gd, gh), torch.cuda.device(gpu):
        if sid:
            s0 = float(torch.log(torch.tensor(dcfg[0]).float()))
            s1 = float(torch.log(torch.tensor(dcfg[1] - 1.).float() / dcfg[0]))
            fn, what = lib.dhd_sparse_bin_labels_sid, 'dhd_sparse_bin_labels_sid'
        else:
            s0, s1 = float(dcfg[0] - dcfg[2]), float(dcfg[2])
            fn, what = lib.dhd_sparse_bin_labels, 'dhd_sparse_bin_labels'
        _lib.check(fn(_lib.ptr(gd), _lib.ptr(gh), b * n, fh, fw, ds, s0, s1, neck.D, float(neck.height_range[0]),
                      float(neck.height_interval), neck.H, _lib.ptr(dbin), _lib.ptr(hbin), _lib.stream_ptr(gpu)), what)
    return dbin.cpu().long(), hbin.cpu().long()


@pytest.mark.parametrize('name', list(V.LABEL_CASES))
def test_bin_labels_on_and_around_every_boundary(gpu, name):
    """Values exactly on offset + k step for every k in 0 .. n_bins + 1 and 1, 2 and 64 float32 steps either side of it (in log
    space for sid), a negative-only, an empty and a 1e5 window: the labels EQUAL the module's own float32 expression on the CPU.
    sid keeps its allowance: the device logarithm may differ in the last bit, so a placement within 2 float32 steps of a boundary
    (less than one step of g) may land in the neighbouring bin -- by one bin at most, and nowhere else."""
    from dhd_amd import label_loss
    sid, ds = V.LABEL_CASES[name]
    c, (dref, href) = V.label_case(name), V.label_reference(name)
    dbin, hbin = _labels_run(gpu, name)
    d_diff, h_diff = dbin != dref, hbin != href
    print(f'{name}: depth labels differing {int(d_diff.sum())} of {dref.numel()}, height labels differing {int(h_diff.sum())}')
    assert not bool(h_diff.any())
    if sid:
        near = torch.from_numpy((c['d_k'] >= 0) & (np.abs(c['d_off']) <= V.NEAR))
        wrap = (dbin - dref).abs()                                                   # bin n_bins against "no label" (0) at the last boundary
        neck = V.label_neck(name)
        one_bin = (wrap <= 1) | ((torch.minimum(dbin, dref) == 0) & (torch.maximum(dbin, dref) == neck.D))
        assert not bool((d_diff & ~near).any()) and bool(one_bin.all())
    else:
        assert not bool(d_diff.any())
    # the module-level wrapper gives the same labels
    neck = V.label_neck(name)
    d2, h2 = label_loss.bin_labels(c['gt_depth'].to(gpu), c['gt_height'].to(gpu), ds, neck.grid_config['depth'], neck.D,
                                   neck.height_range[0], neck.height_interval, neck.H, sid=sid)
    assert torch.equal(d2.cpu().long(), dbin) and torch.equal(h2.cpu().long(), hbin)


# --------------------------------------------------------------------------- C. bin BCE

def _bce_run(gpu, pred, bins, fg, weight=V.BCE_WEIGHT, grad_loss=1.0):
    """dhd_bin_bce_forward + _backward on pre-filled buffers -> (loss float, gradient float32 on the CPU)."""
    from dhd_amd import _lib
    lib = _lib.load()
    bn, c, fh, fw = pred.shape
    pd, bd, fd = pred.to(gpu).contiguous(), bins.to(gpu), fg.to(gpu)
    gl = torch.tensor([grad_loss], dtype=torch.float32, device=gpu)
    ws = _bytes_cd(lib.dhd_bin_bce_workspace_bytes(), gpu)
    loss, grad = _filled((1,), torch.float32, gpu), _filled(tuple(pred.shape), torch.float32, gpu)
    with _Unchanged(pd, bd, fd, gl), torch.cuda.device(gpu):
        st = _lib.stream_ptr(gpu)
        _lib.check(lib.dhd_bin_bce_forward(_lib.ptr(pd), _lib.ptr(bd), _lib.ptr(fd), bn, c, fh * fw, weight, _lib.ptr(loss), _lib.ptr(ws),
                                           st), 'dhd_bin_bce_forward')
        _lib.check(lib.dhd_bin_bce_backward(_lib.ptr(pd), _lib.ptr(bd), _lib.ptr(fd), bn, c, fh * fw, weight, _lib.ptr(gl), _lib.ptr(ws),
                                            _lib.ptr(grad), st), 'dhd_bin_bce_backward')
    return float(loss.cpu()), grad.cpu()


@pytest.mark.parametrize('kind,c', V.BCE_CASES)
def test_bin_bce_at_value_edges_vs_float64(gpu, kind, c):
    """Loss within 1e-5 max(1, |R|) and gradient within 1e-5 |G|max of the float64 formula: probabilities of exactly 0 and 1 (both
    logarithms at the -100 clamp, the gradient's 1e-12 floor: |G| = 1e12 / n_fg), 1e-30, 1 - 2^-24, a saturated half softmax, no
    and one foreground pixel, and 66 156 pixels, where the partial sums' grid-stride loop runs."""
    from dhd_amd import label_loss
    pred, bins, fg = V.bce_case(kind, c)
    ref = V.bce_reference(kind, c)
    loss, grad = _bce_run(gpu, pred, bins, fg)
    gerr = float((grad.double() - ref['grad']).abs().max())
    print(f'{kind} C={c}: loss {loss!r} error {abs(loss - ref["loss"]):.3g} (float32 formula alone {ref["loss_err"]:.3g}, bound '
          f'{ref["loss_bound"]:.3g}); gradient error {gerr:.3g} (alone {ref["grad_err"]:.3g}, bound {ref["grad_bound"]:.3g}, |G|max '
          f'{float(ref["grad"].abs().max()):.3g})')
    assert np.isfinite(loss) and abs(loss - ref['loss']) <= ref['loss_bound']
    assert bool(torch.isfinite(grad).all()) and gerr <= ref['grad_bound']
    is_fg = (fg > 0).view(pred.shape[0], 1, *pred.shape[2:]).expand_as(grad)
    assert float(grad[~is_fg].abs().max()) == 0.0
    if kind == 'no_foreground':
        assert loss == 0.0 and float(grad.abs().max()) == 0.0
    if kind in ('stride', 'one_foreground'):                                             # the autograd wrapper is the same operator
        a = pred.to(gpu).requires_grad_()
        l2 = label_loss.fg_bce(a, bins.to(gpu), fg.to(gpu), V.BCE_WEIGHT)
        l2.backward()
        assert float(l2.detach()) == loss and torch.equal(a.grad.cpu(), grad)


@pytest.mark.parametrize('c', V.BCE_CHANNELS)
def test_bin_bce_nan_probabilities(gpu, c):
    """A NaN probability at a FOREGROUND pixel gives a NaN loss (torch's clamp is max(log p, -100) on a NaN-propagating max; a
    plain fmaxf would return -100 and hide it) and a NaN gradient at that element only; at a BACKGROUND pixel it changes neither
    the loss nor any gradient (those gradients are 0) -- bit for bit."""
    pred, bins, fg = V.bce_case('half_softmax', c)
    base_l, base_g = _bce_run(gpu, pred, bins, fg)
    fg_pix, bg_pix = int((fg > 0).nonzero()[2]), int((fg == 0).nonzero()[1])
    hw, fw = pred.shape[2] * pred.shape[3], pred.shape[3]
    at = lambda pix, k: (pix // hw, k, (pix % hw) // fw, pix % fw)
    for k in (int(bins[fg_pix]) - 1 if int(bins[fg_pix]) > 0 else 0, (int(bins[fg_pix]) + 2) % c):    # the label bin and another
        p = pred.clone()
        p[at(fg_pix, k)] = NAN
        loss, grad = _bce_run(gpu, p, bins, fg)
        assert np.isnan(loss), loss
        nan = torch.isnan(grad)
        assert int(nan.sum()) == 1 and bool(nan[at(fg_pix, k)])
        assert torch.equal(grad[~nan], base_g[~nan])
    p = pred.clone()
    p[at(bg_pix, 1)] = NAN
    loss, grad = _bce_run(gpu, p, bins, fg)
    assert loss == base_l and torch.equal(grad, base_g)


# --------------------------------------------------------------------------- D. depth / height head

def _head_run(gpu, kind, shape, dtype_name, layout):
    """dhd_mghs_softmax_forward + _backward through the C ABI on pre-filled outputs -> dict of CPU tensors in NCHW order."""
    from dhd_amd import _lib, mghs_op
    lib = _lib.load()
    bn, d, c, hb, extra, fh, fw = V.HEAD_SHAPES[shape]
    dt = V.HEAD_DTYPES[dtype_name]
    x_d, hl, g_depth, g_feat, g_height = V.head_case(kind, shape, dtype_name)
    nhwc = int(layout == 'channels_last')
    to_mem = (lambda t: t.permute(0, 2, 3, 1).contiguous()) if nhwc else (lambda t: t.contiguous())       # the bytes the kernel sees
    from_mem = (lambda t, ch: t.view(bn, fh, fw, ch).permute(0, 3, 1, 2)) if nhwc else (lambda t, ch: t.view(bn, ch, fh, fw))
    xm, hm = to_mem(x_d).to(gpu), to_mem(hl).to(gpu)
    gs = [g.to(gpu) for g in (g_depth, g_feat, g_height)]
    ct, ht = d + c + extra, hb + extra
    hr, mr = mghs_op._range_arrays(*V.head_ranges(hb))
    depth, feat, height = (_filled((bn, n, fh, fw), torch.float32, gpu) for n in (d, c, hb))
    band = _filled((bn, fh, fw), torch.uint8, gpu)
    g_xd, g_hl = _filled((bn * ct * fh * fw,), dt, gpu), _filled((bn * ht * fh * fw,), dt, gpu)
    code = _lib.dtype_code(dt)
    with _Unchanged(xm, hm, *gs), torch.cuda.device(gpu):
        st = _lib.stream_ptr(gpu)
        _lib.check(lib.dhd_mghs_softmax_forward(_lib.ptr(xm), code, nhwc, ct, _lib.ptr(hm), code, nhwc, ht, bn, fh * fw, d, c, hb, hr, mr,
                                                _lib.ptr(depth), _lib.ptr(feat), _lib.ptr(height), _lib.ptr(band), st),
                   'dhd_mghs_softmax_forward')
        torch.cuda.synchronize()
        with _Unchanged(depth, height):
            _lib.check(lib.dhd_mghs_softmax_backward(_lib.ptr(gs[0]), _lib.ptr(gs[1]), _lib.ptr(gs[2]), _lib.ptr(depth), _lib.ptr(height),
                                                     bn, fh * fw, d, c, hb, _lib.ptr(g_xd), code, nhwc, ct, _lib.ptr(g_hl), code, nhwc, ht,
                                                     st), 'dhd_mghs_softmax_backward')
    return dict(depth=depth.cpu(), feat=feat.cpu(), height=height.cpu(), band=band.cpu(), g_xd=from_mem(g_xd, ct).cpu().double(),
                g_hl=from_mem(g_hl, ht).cpu().double())


def _head_mirror_grad_error(kind, shape, dtype_name, ref):
    """The float32 torch formulation's own gradient error against float64 (softmax in float32, autograd, the cast to the dtype)."""
    bn, d, c, hb, extra, fh, fw = V.HEAD_SHAPES[shape]
    dt = V.HEAD_DTYPES[dtype_name]
    x_d, hl, g_depth, g_feat, g_height = V.head_case(kind, shape, dtype_name)
    errs = []
    for logits, n, g, key in ((x_d, d, g_depth, 'g_xd'), (hl, hb, g_height, 'g_hl')):
        a = logits[:, :n].float().clone().requires_grad_()
        a.softmax(1).backward(g)
        r = ref[key][:, :n]
        ok = torch.isfinite(r)
        errs.append(float((a.grad.to(dt).double() - r)[ok].abs().max()))
    return errs


@pytest.mark.parametrize('layout', V.HEAD_LAYOUTS)
@pytest.mark.parametrize('dtype_name', list(V.HEAD_DTYPES))
@pytest.mark.parametrize('shape', list(V.HEAD_SHAPES))
@pytest.mark.parametrize('kind', V.HEAD_KINDS)
def test_depth_height_head_at_value_edges_vs_float64(gpu, kind, shape, dtype_name, layout):
    """Saturated logits: the type's largest finite value and its negative, a bin at -inf, two equal maxima 200 above the rest
    (0.5 / 0.5 / 0), all bins equal, and the rows torch's softmax defines as NaN (+inf with anything, every bin -inf).
    Probabilities within 1e-6 of the float64 softmax of the stored logits and NaN exactly where it is; the context slice exact;
    the band = the band of the FIRST maximum wherever the float64 top-2 margin is above 1e-6 or an exact tie (a NaN row's band is
    unspecified); gradients finite wherever the reference's are and within 1e-6 / 2e-3 / 1.6e-2 x max(1, |G|max)."""
    bn, d, c, hb, extra, fh, fw = V.HEAD_SHAPES[shape]
    ref = V.head_reference(kind, shape, dtype_name)
    out = _head_run(gpu, kind, shape, dtype_name, layout)
    mirror = _head_mirror_grad_error(kind, shape, dtype_name, ref)
    msg = [f'{kind} {shape} {dtype_name} {layout}:']
    for key in ('depth', 'height'):
        nan_ref = torch.isnan(ref[key])
        assert torch.equal(torch.isnan(out[key]), nan_ref), key
        assert not bool(torch.isinf(out[key]).any())
        err = float((out[key].double() - ref[key])[~nan_ref].abs().max())
        msg.append(f'{key} error {err:.3g}')
        assert err <= 1e-6, (key, err)
    assert torch.equal(out['feat'], ref['feat'])
    clear = ref['band_clear']
    defined = ~torch.isnan(ref['height']).any(1)
    assert int(clear.sum()) >= 0.8 * int(defined.sum()) and torch.equal(out['band'][clear], ref['band'][clear])
    eps = V.HEAD_GRAD_EPS[dtype_name]
    for key, m_err in zip(('g_xd', 'g_hl'), mirror):
        ok = torch.isfinite(ref[key])
        assert bool(torch.isfinite(out[key][ok]).all()), key
        gmax = max(1.0, float(ref[key][ok].abs().max()))
        err = float((out[key] - ref[key])[ok].abs().max())
        bnd = V.bound(eps * gmax, m_err)
        msg.append(f'{key} error {err:.3g} (float32 torch alone {m_err:.3g}, bound {bnd:.3g})')
        assert err <= bnd, (key, err, bnd)
    print(' '.join(msg))
    if extra:
        assert float(out['g_xd'][:, d + c:].abs().max()) == 0.0 and float(out['g_hl'][:, hb:].abs().max()) == 0.0
    assert torch.equal(out['g_xd'][:, d:d + c], ref['g_xd'][:, d:d + c].to(V.HEAD_DTYPES[dtype_name]).double())


# --------------------------------------------------------------------------- E. argmax rows

def test_argmax_rows_and_histogram(gpu):
    """dhd_occ_argmax_hist on rows with all logits equal, all -inf, +0 against -0, the maximum at k = 0 and 17, at 17 only: the
    FIRST maximum wins (numpy argmax of the float64 logits), the 18 x 18 histogram is exact and accumulates over two calls."""
    from dhd_amd import _lib
    from dhd_amd.occ_loss import occ_argmax_hist
    lib = _lib.load()
    z, t, cam = V.argmax_case()
    p_ref, h_ref = V.argmax_reference(z, t, cam)
    m = z.shape[0]
    zd, td, cd = z.to(gpu), t.to(gpu), cam.to(torch.uint8).to(gpu)
    pred = _filled((m,), torch.uint8, gpu)
    hist = torch.zeros(V.N_CLS, V.N_CLS, dtype=torch.int64, device=gpu)                  # accumulated into: the caller zeroes it
    with _Unchanged(zd, td, cd), torch.cuda.device(gpu):
        for n in (1, 2):
            _lib.check(lib.dhd_occ_argmax_hist(_lib.ptr(zd), _lib.ptr(td), _lib.ptr(cd), m, V.N_CLS, _lib.ptr(pred), _lib.ptr(hist),
                                               _lib.stream_ptr(gpu)), 'dhd_occ_argmax_hist')
            assert np.array_equal(pred.cpu().numpy(), p_ref)
            assert np.array_equal(hist.cpu().numpy(), n * h_ref)
    p2, h2 = occ_argmax_hist(zd, td, cam.to(gpu))
    assert np.array_equal(p2.cpu().numpy(), p_ref) and np.array_equal(h2.cpu().numpy(), h_ref)
    assert tuple(p_ref[:8]) == V.ARGMAX_EXPECTED


def test_occupancy_head_class_map_on_exact_ties(gpu):
    """predictor.predict_occ with fused_infer on the smallest case of occ_head_inputs: with W2 = 0 the float64 logits of every voxel
    are b2 exactly, and b2 carries the tie rows (all equal, all -inf, +-0, the maximum at 0 and 17, at 17 only): the class map is
    the first maximum of each row, the histogram is exact and accumulates over two calls."""
    import copy
    from occ_head_inputs import make_head, make_x
    head = copy.deepcopy(make_head()).to(gpu)
    b2 = V.argmax_head_bias()
    with torch.no_grad():
        head.predicter[2].weight.zero_()
        head.predicter[2].bias.copy_(b2.to(gpu))
    head.fused_infer = True
    x = make_x((1, 1, 1)).to(gpu)
    want = np.array(V.ARGMAX_EXPECTED * 2, dtype=np.uint8)
    labels = torch.tensor([0, 17, 3, 255, 0, 17, 17, 1] * 2, dtype=torch.uint8, device=gpu).view(1, 1, 1, 16)
    keep = labels.cpu().numpy().reshape(-1) < V.N_CLS
    h_ref = np.bincount(V.N_CLS * labels.cpu().numpy().reshape(-1)[keep].astype(np.int64) + want[keep],
                        minlength=V.N_CLS ** 2).reshape(V.N_CLS, V.N_CLS)
    with torch.no_grad(), _Unchanged(x, labels):
        assert head.fused_applies(x)
        occ, hist, logits = head.predict_occ(x, labels=labels, return_logits=True)
        ref_logits = b2.view(1, 1, 1, 16, V.N_CLS)
        got = logits.cpu().view(1, 1, 1, 16, V.N_CLS)
        assert torch.equal(got, ref_logits + 0.0)                                        # 0 . h + b2: -0 becomes +0, the ties stay
        assert np.array_equal(occ[0].reshape(-1), want)
        assert np.array_equal(hist.cpu().numpy(), h_ref)
        _, hist, _ = head.predict_occ(x, labels=labels, hist=hist)
        assert np.array_equal(hist.cpu().numpy(), 2 * h_ref)
