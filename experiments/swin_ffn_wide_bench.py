"""The second half of a SwinBlock at inference at DHD-L's stages 2 and 3 (33 792 x 512 and 8 448 x 1024 tokens), the wide kernel family
(dhd_amd/csrc/swin_ffn_wide.h) against the two forms it replaces, and the whole Swin backbone with swin_ffn.ROUTED_WIDE as committed
against ROUTED_WIDE all-False (the behaviour before the family existed).

The protocol, the three paths (today, today_glue, fused), the record layout and the routing rule are those of
experiments/swin_ffn_infer_bench.py, whose functions this script calls: one process, the same tensors, alternating windows, device
events, median / min / max us per call with the weight-pack launch included, peak bytes above the resident state; `routed` is true
only where the fused median beats BOTH parents' medians by more than the largest min-max spread of the three.

Besides that script's three precisions (float32 tokens under bf16 / fp16 autocast and in float32) the tokens are also measured in
the autocast type itself, parameters float32, under autocast: that is what DHD-L's backbone hands stages 1 to 3 under autocast
(PatchMerging's Linear returns the autocast type, so the residual stream is bf16 there), and it is the (bf16, bf16) / (fp16, fp16)
entry of the routing table.  A half model without autocast (parameters in the half type too) shares that entry and is not timed.

Backbone: SwinTransformer of DHD-L at 12 x 3 x 512 x 1408, no_grad, bf16 autocast, fused_inference + fused_swin_glue + fused_swin_ffn on
on both sides (so stages 0 and 1 take the narrow operator on both sides), ROUTED_WIDE as committed / all-False alternating, two runs
each; `--force` adds the same A/B with every entry of ROUTED_WIDE switched on.

One JSON record (--out).  Needs a GPU: no fallback.  The table follows from the cases, and the backbone A/B of the table as
committed follows from the table, so the record is made in two steps:

    python experiments/swin_ffn_wide_bench.py --force --out profiles/r14/swin_ffn_wide_infer.json
    (set swin_ffn.ROUTED_WIDE from the record's `routed` list)
    python experiments/swin_ffn_wide_bench.py --stages --update profiles/r14/swin_ffn_wide_infer.json --out profiles/r14/swin_ffn_wide_infer.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_ffn_infer_bench as NB  # noqa: E402  (puts the repository root on sys.path)
import torch  # noqa: E402

import dhd_amd  # noqa: E402
from dhd_amd import _lib, swin_ffn  # noqa: E402
from dhd_amd.swin import FFN, SwinTransformer  # noqa: E402
from dhd_amd.swin_glue import layer_norm_rows, swin_glue_supported  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# name -> (token dtype, GEMM dtype)
PRECISIONS = {'bf16_autocast': (F32, BF16), 'fp16_autocast': (F32, F16), 'f32': (F32, F32),
              'bf16_tokens_bf16_autocast': (BF16, BF16), 'fp16_tokens_fp16_autocast': (F16, F16)}


def make_case(stage, xdt, mdt, dev):
    """NB.make_case with the tokens in `xdt`: the same seeds, modules and paths; today_glue is the block's own choice of norm2."""
    if xdt == F32:
        return NB.make_case(stage, mdt, dev)
    (H, W), C = NB.STAGES[stage]
    rows = NB.B * H * W
    torch.manual_seed(7 + stage)
    x = (torch.randn(NB.B, H * W, C, device=dev) * 1.5 + 0.5).to(xdt)
    norm = torch.nn.LayerNorm(C, eps=NB.EPS).to(dev).eval()
    ffn = FFN(C, 4 * C).to(dev).eval()
    with torch.no_grad():
        norm.weight.add_(0.2 * torch.randn(C, device=dev))
        norm.bias.add_(0.1 * torch.randn(C, device=dev))
    fc1, fc2 = ffn.layers[0][0], ffn.layers[1]

    def run(f):
        def g():
            with torch.no_grad(), torch.autocast('cuda', dtype=mdt):
                return f()
        return g

    def glue():
        if not swin_glue_supported(x, plain_ln_to=mdt):
            return ffn(norm(x), identity=x)
        return ffn(layer_norm_rows(x, norm.weight, norm.bias, NB.EPS, mdt), identity=x)
    paths = {'today': run(lambda: ffn(norm(x), identity=x)), 'today_glue': run(glue),
             'fused': run(lambda: swin_ffn.swin_ffn_infer(x, norm.weight, norm.bias, NB.EPS, fc1.weight, fc1.bias, fc2.weight, fc2.bias, mdt))}
    return paths, dict(rows=rows, channels=C, hidden=4 * C, flop=2 * 2 * rows * C * 4 * C)


def backbone(dev, table, runs, steps):
    """ms per forward with ROUTED_WIDE all-False ('wide_off') and set to `table` ('wide_on'), alternating."""
    torch.manual_seed(3)
    net = SwinTransformer(pretrain_img_size=224, patch_size=4, window_size=12, mlp_ratio=4, embed_dims=128, depths=[2, 2, 18, 2],
                          num_heads=[4, 8, 16, 32], strides=(4, 2, 2, 2), out_indices=(2, 3), drop_path_rate=0.1, return_stereo_feat=True,
                          with_cp=False).to(dev).eval()
    net.init_weights()
    dhd_amd.fused_inference(net)
    dhd_amd.fused_swin_glue(net)
    blocks = dhd_amd.fused_swin_ffn(net)
    img = torch.randn(NB.B, 3, 512, 1408, device=dev)
    committed = dict(swin_ffn.ROUTED_WIDE)
    tables = {'wide_off': {k: False for k in committed}, 'wide_on': dict(table)}

    def fwd():
        with torch.no_grad(), torch.autocast('cuda', dtype=BF16):
            return net(img)
    times, outs = {k: [] for k in tables}, {}
    try:
        for k, t in tables.items():
            swin_ffn.ROUTED_WIDE = t
            for _ in range(2):
                outs[k] = fwd()
        torch.cuda.synchronize()
        for _ in range(runs):
            for k, t in tables.items():
                swin_ffn.ROUTED_WIDE = t
                times[k].append(NB.window(fwd, steps) / 1e3)
    finally:
        swin_ffn.ROUTED_WIDE = committed
    # what one forward with `table` really sends to the two families: counted where every entry point's code is checked
    seen, real = [], _lib.check
    _lib.check = lambda rc, what: (seen.append(what), real(rc, what))[1]
    try:
        swin_ffn.ROUTED_WIDE = dict(table)
        fwd()
        torch.cuda.synchronize()
    finally:
        _lib.check = real
        swin_ffn.ROUTED_WIDE = committed
    n_wide, n_narrow = seen.count('dhdg_swin_ffn_wide_infer'), seen.count('dhdf_swin_ffn_infer')
    diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(outs['wide_on'], outs['wide_off']))
    scale = max(float(b.float().abs().max()) for b in outs['wide_off'])
    return {'ms_per_forward': {k: [round(t, 2) for t in v] for k, v in times.items()}, 'blocks_on_the_wide_operator': int(n_wide),
            'blocks_on_the_narrow_operator': int(n_narrow), 'of_blocks': len(blocks), 'max_abs_diff_on_vs_off': diff, 'max_abs_output': scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stages', type=int, nargs='*', default=[2, 3])
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--backbone-runs', type=int, default=2)
    ap.add_argument('--backbone-steps', type=int, default=3)
    ap.add_argument('--force', action='store_true', help='also run the backbone with every entry of ROUTED_WIDE on')
    ap.add_argument('--update', default=None, help='start from this record and replace only what this run measures')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('swin_ffn_wide_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'images': NB.B, 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
              'device': torch.cuda.get_device_name(0), 'cases': {}}
    if args.update:
        with open(args.update) as f:
            record = json.load(f)
    for stage in args.stages:
        for pname, (xdt, mdt) in PRECISIONS.items():
            paths, shape = make_case(stage, xdt, mdt, dev)
            assert 'fused' in paths, (stage, pname)            # no operator is an error here, not a fallback
            for fn in paths.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in paths}
            for _ in range(args.windows):
                for k, fn in paths.items():
                    times[k].append(NB.window(fn, args.calls))
            rec = {k: dict(NB.summary(ts), peak_bytes=NB.peak_bytes(paths[k])) for k, ts in times.items()}
            rec.update(shape)
            spread = max(rec[k]['max_us'] - rec[k]['min_us'] for k in paths)
            best_parent = min(rec['today']['median_us'], rec['today_glue']['median_us'])
            rec['larger_spread_us'] = round(spread, 1)
            rec['speedup_over_best_parent'] = round(best_parent / rec['fused']['median_us'], 2)
            rec['tflops'] = round(shape['flop'] / (rec['fused']['median_us'] * 1e-6) / 1e12, 1)
            rec['routed'] = bool(best_parent - rec['fused']['median_us'] > spread)
            rec['peak_bytes_fused_over_parent'] = round(rec['fused']['peak_bytes'] / rec['today']['peak_bytes'], 3)
            a, p = paths['fused'](), paths['today']()
            rec['max_abs_diff_fused_vs_today'] = float((a.float() - p.float()).abs().max())
            key = f'stage{stage}_{pname}'
            record['cases'][key] = rec
            print(key, json.dumps(rec), flush=True)
            del paths, a, p
            torch.cuda.empty_cache()
    record['routed'] = sorted(k for k, v in record['cases'].items() if v['routed'])
    record['stay_with_torch'] = sorted(k for k, v in record['cases'].items() if not v['routed'])
    record['not_measured'] = ['a half model without autocast (parameters in the half type)', 'batch sizes other than 12 images',
                              'the LayerNorm-free form']
    if args.backbone_runs > 0:
        variants = [('backbone_table_as_committed', dict(swin_ffn.ROUTED_WIDE))]
        if args.force:
            variants.append(('backbone_every_entry_forced', {k: True for k in swin_ffn.ROUTED_WIDE}))
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
