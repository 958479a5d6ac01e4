"""The seams between the stages of DHD-L's Swin backbone, 12 images: the operators of dhd_amd/swin_seam.py (csrc/swin_seam.h)
against today's path, forward and forward + backward, and the whole backbone at inference with the seams switched on and off.

Merge: the maps 128 x 352 x 128, 64 x 176 x 256 and 32 x 88 x 512; float32, float32 tokens under bf16 / fp16 autocast (a half
result), and bf16 tokens under bf16 autocast.  Today's path is `PatchMerging.forward` up to the input of `reduction`: the
reshape.permute.reshape copy, nn.LayerNorm, and the cast the Linear's autocast makes.
Embed: the 128-channel 128 x 352 map as the conv leaves it (NCHW); float32, and a bf16 / fp16 conv output under autocast with a
float32 result.  Today's path is flatten.transpose + nn.LayerNorm.

Protocol (that of experiments/swin_ffn_wide_bench.py and profiles/r12): one process, the same tensors, fused and today's path in
alternating windows of `--calls` calls between device events, median / min / max us per call over `--windows` windows.  An entry
is `routed` only where the fused median beats today's by more than the larger min-max spread of the two, forward and
forward + backward both.  Achieved bytes/s of a forward: the bytes of x plus the bytes of the result over the fused median.

Backbone: SwinTransformer of DHD-L at 12 x 3 x 512 x 1408, no_grad, bf16 autocast, fused_inference + fused_swin_glue +
fused_swin_ffn on on both sides, fused_swin_seams on / off alternating, with swin_seam.ROUTED as committed and, with --force,
with every entry routed.

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/swin_seam_bench.py --force --out profiles/r15/swin_seam.json
    (set swin_seam.ROUTED from the record's `routed` list)
    python experiments/swin_seam_bench.py --no-cases --update profiles/r15/swin_seam.json --out profiles/r15/swin_seam.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_ffn_infer_bench as NB  # noqa: E402  (puts the repository root on sys.path)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import dhd_amd  # noqa: E402
from dhd_amd import _lib, swin_seam  # noqa: E402
from dhd_amd.swin import SwinTransformer  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
B, EPS = 12, 1e-5
MERGE_MAPS = {'stage0': (128, 352, 128), 'stage1': (64, 176, 256), 'stage2': (32, 88, 512)}
EMBED_MAP = (128, 128, 352)     # C, H, W
# name -> (x dtype, result dtype, autocast dtype or None)
MERGE_PRECISIONS = {'f32': (F32, F32, None), 'bf16_autocast': (F32, BF16, BF16), 'fp16_autocast': (F32, F16, F16),
                    'bf16_tokens': (BF16, BF16, BF16)}
EMBED_PRECISIONS = {'f32': (F32, F32, None), 'bf16_conv': (BF16, F32, BF16), 'fp16_conv': (F16, F32, F16)}
NAME = {F32: 'float32', F16: 'float16', BF16: 'bfloat16'}


class Everything(dict):
    def get(self, key, default=None):
        return True


def todays_merge(x, norm, H, W, cast_to):
    """PatchMerging.forward (stride 2, even H and W) up to the input of `reduction`; the Linear's autocast cast made explicit."""
    Bn, L, C = x.shape
    x = x.view(Bn, H, W, C)
    x = x.reshape(Bn, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(Bn, (H // 2) * (W // 2), 4 * C)
    y = norm(x)
    return y if cast_to is None else y.to(cast_to)


def make_case(kind, shape, xdt, odt, act, dev):
    torch.manual_seed(11)
    if kind == 'merge':
        H, W, C = shape
        x = (torch.randn(B, H * W, C, device=dev) * 1.5 + 0.5).to(xdt).requires_grad_()
        n, out_shape = 4 * C, (B, (H // 2) * (W // 2), 4 * C)
    else:
        C, H, W = shape
        x = (torch.randn(B, C, H, W, device=dev) * 1.5 + 0.5).to(xdt).requires_grad_()
        n, out_shape = C, (B, H * W, C)
    norm = nn.LayerNorm(n, eps=EPS).to(dev)
    with torch.no_grad():
        norm.weight.add_(0.2 * torch.randn(n, device=dev))
        norm.bias.add_(0.1 * torch.randn(n, device=dev))
    dy = torch.randn(out_shape, device=dev).to(odt)

    def ctx():
        return torch.autocast('cuda', dtype=act) if act is not None else torch.autocast('cuda', enabled=False)

    if kind == 'merge':
        fwd = {'today': lambda: todays_merge(x, norm, H, W, act),
               'fused': lambda: swin_seam.patch_merge_norm(x, norm.weight, norm.bias, EPS, (H, W), odt)}
    else:
        fwd = {'today': lambda: norm(x.flatten(2).transpose(1, 2)),
               'fused': lambda: swin_seam.patch_embed_norm(x, norm.weight, norm.bias, EPS, odt)}

    def forward(f):
        def g():
            with torch.no_grad(), ctx():
                return f()
        return g

    def both(f):
        def g():
            with ctx():
                y = f()
            return torch.autograd.grad(y, (x, norm.weight, norm.bias), dy)
        return g
    paths = {'forward': {k: forward(f) for k, f in fwd.items()}, 'forward_backward': {k: both(f) for k, f in fwd.items()}}
    nbytes = x.numel() * x.element_size() + dy.numel() * dy.element_size()
    return paths, dict(rows=out_shape[0] * out_shape[1], row_length=n, x_dtype=NAME[xdt], out_dtype=NAME[odt], forward_bytes=nbytes)


def measure(paths, calls, windows):
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(windows):
        for k, fn in paths.items():
            times[k].append(NB.window(fn, calls))
    rec = {k: NB.summary(ts) for k, ts in times.items()}
    spread = max(rec[k]['max_us'] - rec[k]['min_us'] for k in paths)
    rec['larger_spread_us'] = round(spread, 1)
    rec['speedup'] = round(rec['today']['median_us'] / rec['fused']['median_us'], 2)
    rec['wins'] = bool(rec['today']['median_us'] - rec['fused']['median_us'] > spread)
    return rec


def backbone(dev, table, runs, steps):
    """ms per forward with fused_swin_seams off ('seams_off') and on with swin_seam.ROUTED set to `table` ('seams_on'), alternating."""
    torch.manual_seed(3)
    net = SwinTransformer(pretrain_img_size=224, patch_size=4, window_size=12, mlp_ratio=4, embed_dims=128, depths=[2, 2, 18, 2],
                          num_heads=[4, 8, 16, 32], strides=(4, 2, 2, 2), out_indices=(2, 3), drop_path_rate=0.1, return_stereo_feat=True,
                          with_cp=False).to(dev).eval()
    net.init_weights()
    dhd_amd.fused_inference(net)
    dhd_amd.fused_swin_glue(net)
    dhd_amd.fused_swin_ffn(net)
    img = torch.randn(B, 3, 512, 1408, device=dev)
    committed = swin_seam.ROUTED
    swin_seam.ROUTED = table

    def fwd():
        with torch.no_grad(), torch.autocast('cuda', dtype=BF16):
            return net(img)
    times, outs = {'seams_off': [], 'seams_on': []}, {}
    try:
        for k in times:
            dhd_amd.fused_swin_seams(net, k == 'seams_on')
            for _ in range(2):
                outs[k] = fwd()
        torch.cuda.synchronize()
        for _ in range(runs):
            for k in times:
                dhd_amd.fused_swin_seams(net, k == 'seams_on')
                times[k].append(NB.window(fwd, steps) / 1e3)
        seen, real = [], _lib.check
        _lib.check = lambda rc, what: (seen.append(what), real(rc, what))[1]
        try:
            dhd_amd.fused_swin_seams(net, True)
            fwd()
            torch.cuda.synchronize()
        finally:
            _lib.check = real
    finally:
        swin_seam.ROUTED = committed
    diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(outs['seams_on'], outs['seams_off']))
    scale = max(float(b.float().abs().max()) for b in outs['seams_off'])
    return {'ms_per_forward': {k: [round(t, 2) for t in v] for k, v in times.items()},
            'seam_calls_per_forward': {n: seen.count(n) for n in ('dhds_embed_norm_forward', 'dhds_merge_norm_forward')},
            'max_abs_diff_on_vs_off': diff, 'max_abs_output': scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--no-cases', action='store_true', help='skip the per-entry measurement (with --update: keep the record\'s)')
    ap.add_argument('--backbone-runs', type=int, default=2)
    ap.add_argument('--backbone-steps', type=int, default=3)
    ap.add_argument('--force', action='store_true', help='also run the backbone with every entry routed')
    ap.add_argument('--update', default=None, help='start from this record and replace only what this run measures')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('swin_seam_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'images': B, 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
              'device': torch.cuda.get_device_name(0), 'hbm_peak_bytes_per_s': 6.3e12, 'cases': {}}
    if args.update:
        with open(args.update) as f:
            record = json.load(f)
    todo = [] if args.no_cases else ([('merge', f'merge_{m}_{p}', shape, prec) for m, shape in MERGE_MAPS.items() for p, prec in MERGE_PRECISIONS.items()]
                                     + [('embed', f'embed_{p}', EMBED_MAP, prec) for p, prec in EMBED_PRECISIONS.items()])
    for kind, key, shape, (xdt, odt, act) in todo:
        paths, rec = make_case(kind, shape, xdt, odt, act, dev)
        for mode in ('forward', 'forward_backward'):
            rec[mode] = measure(paths[mode], args.calls, args.windows)
        rec['forward_bytes_per_s'] = round(rec['forward_bytes'] / (rec['forward']['fused']['median_us'] * 1e-6), -9)
        rec['forward_fraction_of_hbm_peak'] = round(rec['forward_bytes_per_s'] / 6.3e12, 3)
        rec['routed'] = bool(rec['forward']['wins'] and rec['forward_backward']['wins'])
        rec['routing_key'] = [kind, shape[2] if kind == 'merge' else shape[0], NAME[xdt], NAME[odt]]
        a, p = paths['forward']['fused'](), paths['forward']['today']()
        rec['max_abs_diff_fused_vs_today'] = float((a.float() - p.float()).abs().max())
        record['cases'][key] = rec
        print(key, json.dumps(rec), flush=True)
        del paths, a, p
        torch.cuda.empty_cache()
    record['routed'] = sorted(k for k, v in record['cases'].items() if v['routed'])
    record['stay_with_torch'] = sorted(k for k, v in record['cases'].items() if not v['routed'])
    record['not_measured'] = ['odd map sizes (padding)', 'fp16 tokens', 'batch sizes other than 12 images', 'a channels_last conv output',
                              'maps other than DHD-L\'s']
    if args.backbone_runs > 0:
        variants = [('backbone_table_as_committed', dict(swin_seam.ROUTED))]
        if args.force:
            variants.append(('backbone_every_entry_forced', Everything()))
        for name, table in variants:
            record[name] = backbone(dev, table, args.backbone_runs, args.backbone_steps)
            print(name, json.dumps(record[name]), flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({k: v for k, v in record.items() if k != 'cases'}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
