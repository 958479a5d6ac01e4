"""Does the SFA stage of two builds of libdhd_amd.so compute the same bits?  The operator has no float atomics and the tests pin
it as bit-reproducible, so after a refactor every tensor must be equal.  Runs the stage of THIS tree against the library that
DHD_AMD_LIB names (default: the tree's own) and saves every result; run once per library, then compare.
usage: [DHD_AMD_LIB=path/libdhd_amd.so] sfa_bit_identity.py <out.pt> [--no-full-size]     |     sfa_bit_identity.py --compare a.pt b.pt
Covered: float32 storage in every GEMM mode at C = 128 / 256 / 512, half I/O on float32 storage (a shape with hw % 8 == 4 among
them), half storage, each in train and eval mode with the backward; dhd_sfa_stage_infer in every form the plan has; the full size
(4, 512, 200, 200) once per storage type.  A tensor above 2^25 elements is kept as the SHA-256 of its bytes."""
import hashlib, os, sys
import torch
if sys.argv[1] == '--compare':
    a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    same = lambda u, v: u == v if isinstance(u, str) else (u.dtype == v.dtype and torch.equal(u, v))
    bad = [k for k in a if k not in b or not same(a[k], b[k])] + [k for k in b if k not in a]
    print('compared', len(a), 'tensors;', 'ALL BIT-IDENTICAL' if not bad else '%d DIFFERENT: %s' % (len(bad), bad[:8]))
    sys.exit(1 if bad else 0)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dhd_amd import _lib
from dhd_amd.mix import channel_spatial_stage
dev = torch.device('cuda:0')
res = {}


def keep(tag, t):
    t = t.detach().cpu().contiguous()
    res[tag] = t if t.numel() <= 1 << 25 else hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def run(tag, c, b, h, w, train, gemm, dtype=torch.float32, half_storage=False, forms=()):
    torch.manual_seed(c + h)
    st = channel_spatial_stage(2 * c).to(dev).train(train)
    st.gemm, st.half_storage = gemm, half_storage
    with torch.no_grad():   # running statistics and affine parameters away from their initial 0 / 1
        for bn in (st.spacial_leanring[1], st.spacial_leanring[4]):
            bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.2)
    x = (torch.randn(b, 2 * c, h, w, device=dev) * 0.7 + 0.1).to(dtype).requires_grad_()
    g = torch.randn(b, c, h, w, device=dev).to(dtype)
    tag = '%s.%s.c%d.%dx%dx%d.%s.' % (tag, gemm, c, b, h, w, 'train' if train else 'eval')
    out = st(x)
    out.backward(g)
    keep(tag + 'out', out)
    keep(tag + 'gx', x.grad)
    for k, p in st.named_parameters():
        keep(tag + 'grad.' + k, p.grad)
    for k, v in st.named_buffers():
        keep(tag + 'buf.' + k, v)
    for form in forms:      # forward-only inference: eval mode, nothing to differentiate
        st.infer_form = form
        with torch.no_grad():
            keep(tag + 'infer.' + form, st(x.detach()))


full = '--no-full-size' not in sys.argv
for train in (True, False):
    for gemm in ('bf16x3', 'bf16x6', 'f32'):
        for c in (128, 256, 512):
            cu = gemm == 'bf16x3' and c <= 256     # Gemm::cu has the two-pass inference form
            run('f32', c, 2, 100, 100, train, gemm, forms=() if train else ('unfused', 'two_pass') if cu else ('unfused',))
    for dtype, name in ((torch.float16, 'fp16'), (torch.bfloat16, 'bf16')):
        for (c, b, h, w) in ((256, 2, 18, 22), (128, 2, 100, 100), (512, 1, 52, 60)):   # 18 x 22: hw % 8 == 4
            run('f32.io_' + name, c, b, h, w, train, 'bf16x3', dtype, forms=() if train else ('unfused',) + (('two_pass',) if c <= 256 else ()))
        for c in (128, 256):
            for (b, h, w) in ((2, 100, 100), (3, 36, 40)):
                run('half_' + name, c, b, h, w, train, 'bf16x3', dtype, True, forms=() if train else ('unfused', 'two_pass', 'one_pass'))
if full:
    run('f32.full', 256, 4, 200, 200, True, 'bf16x3')
    run('half_fp16.full', 256, 4, 200, 200, True, 'bf16x3', torch.float16, True)
    run('half_bf16.full', 256, 4, 200, 200, True, 'bf16x3', torch.bfloat16, True)
torch.save(res, sys.argv[1])
print('saved', len(res), 'tensors from', _lib.LIB_PATH)
