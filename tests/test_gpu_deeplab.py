"""GPU parity for the DeepLabv3+ / ResNet-50 path (BASELINE config 3): new kernels (add+ReLU, Dropout2d scale,
softmax cross-entropy with ignore_index), the head against the REFERENCE's golden vectors, and the full
EncoderDecoder against the oracle. Tolerances as in test_gpu_modules.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cvpytorch_amd import deeplab, ops
from cvpytorch_amd import lib as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


def cosine(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp(min=1e-30))


def nhwc(x):
    return x.to(dev()).to(BF).contiguous(memory_format=torch.channels_last)


def bf(x):
    return x.to(BF).float()


def test_add_act():
    torch.manual_seed(0)
    a, b = bf(torch.randn(2, 24, 5, 7)), bf(torch.randn(2, 24, 5, 7))
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.relu(ar + br)
    g = bf(torch.randn_like(ref))
    ref.backward(g)
    ad, bd = nhwc(a).requires_grad_(True), nhwc(b).requires_grad_(True)
    out = ops.add_act(ad, bd, L.ACT_RELU)
    out.backward(nhwc(g))
    assert torch.equal(out.detach().float().cpu(), bf(ref.detach()))
    assert torch.equal(ad.grad.float().cpu(), ar.grad) and torch.equal(bd.grad.float().cpu(), br.grad)


def test_dropout2d_semantics():
    torch.manual_seed(0)
    x = nhwc(torch.ones(8, 64, 4, 4)).requires_grad_(True)
    y = ops.dropout2d(x, 0.25, True)
    v = y.detach().float().cpu()
    per = v.amax((2, 3))
    keep = float(torch.tensor(1 / 0.75).to(BF))  # survivors are scaled by 1/(1-p), stored in bf16
    assert set(per.unique().tolist()) <= {0.0, keep}
    assert torch.equal(v, per[:, :, None, None].expand_as(v))  # whole channels are dropped
    assert 0.1 < float((per == 0).float().mean()) < 0.4
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad.float().cpu(), v)
    assert ops.dropout2d(x, 0.25, False) is x


@pytest.mark.parametrize("Cc,H,W", [(19, 9, 11), (8, 4, 4), (21, 16, 16)])
def test_seg_cross_entropy(Cc, H, W):
    torch.manual_seed(0)
    N = 3
    logits = bf(torch.randn(N, Cc, H, W) * 3)
    tgt = torch.randint(0, Cc, (N, H, W))
    tgt[torch.rand(N, H, W) < 0.2] = 255
    lr = logits.clone().requires_grad_(True)
    ref = F.cross_entropy(lr, tgt, ignore_index=255)
    (gref,) = torch.autograd.grad(ref, lr)
    ld = nhwc(logits).requires_grad_(True)
    loss = ops.seg_cross_entropy(ld, tgt.to(dev()), 255)
    (g,) = torch.autograd.grad(loss * 2.0, ld)
    assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    assert rel_l2(g.float(), 2.0 * gref) < 4e-3
    # all pixels ignored -> zero loss and zero gradient (torch returns nan; the reference never hits this)
    allign = torch.full((N, H, W), 255)
    l0 = ops.seg_cross_entropy(nhwc(logits).requires_grad_(True), allign.to(dev()), 255)
    assert float(l0) == 0.0


@pytest.mark.parametrize("Cc,Hi,Wi,Ho,Wo,ac,fused", [(19, 8, 16, 32, 64, False, True),      # x4: DeepLabv3+ head -> label size
                                                    (19, 7, 9, 28, 36, False, True),       # ragged tiles (7 rows, 9 columns of 4 x 8 tiles)
                                                    (19, 8, 16, 32, 64, True, False),      # align_corners: two ops (the fused backward's footprint bound assumes half-pixel mapping)
                                                    (21, 6, 10, 17, 23, False, True),      # non-integer ratio
                                                    (8, 5, 5, 5, 5, False, True),          # identity resize
                                                    (32, 4, 8, 16, 32, False, True),       # widest supported class count
                                                    (19, 3, 4, 36, 48, False, True),       # x12: the footprint is the whole label map
                                                    (19, 2, 2, 64, 64, False, True),       # x32: the footprint exceeds the LDS — walked in row chunks (round 6)
                                                    (19, 16, 32, 256, 512, False, True),   # x16 on a 16 x 32 map: 8 x 8 tiles, 146-row footprints in chunks
                                                    (19, 9, 13, 72, 104, False, True),     # x8, ragged 8 x 8 tiles
                                                    (40, 8, 8, 16, 16, False, False)])     # too many classes -> two ops
def test_seg_cross_entropy_resized_fused(Cc, Hi, Wi, Ho, Wo, ac, fused):
    """ops.seg_cross_entropy_resized == F.cross_entropy(F.interpolate(logits, label size, bilinear), labels) in fp32
    (encoder_decoder.py:93-107), values and the gradient w.r.t. the LOW-resolution logits"""
    torch.manual_seed(1)
    N = 3
    logits = bf(torch.randn(N, Cc, Hi, Wi) * 3)
    tgt = torch.randint(0, Cc, (N, Ho, Wo))
    tgt[torch.rand(N, Ho, Wo) < 0.2] = 255
    lr = logits.clone().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(lr, size=(Ho, Wo), mode="bilinear", align_corners=ac), tgt, ignore_index=255)
    (gref,) = torch.autograd.grad(ref, lr)
    fused_ok = bool(L.load().cvhip_seg_ce_bilinear_ok(Cc, Hi, Wi, Ho, Wo, int(ac)))
    assert fused_ok == fused
    calls = []
    real = L.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    L.call = spy
    try:
        ld = nhwc(logits).requires_grad_(True)
        loss = ops.seg_cross_entropy_resized(ld, tgt.to(dev()), 255, ac)
        (g,) = torch.autograd.grad(loss * 2.0, ld)
    finally:
        L.call = real
    assert ("cvhip_seg_ce_bilinear_fwd" in calls) == fused_ok and ("cvhip_seg_ce_bilinear_bwd" in calls) == fused_ok
    tol = 1e-4 if fused_ok else 3e-3          # fused: fp32 interpolated logits; two-op: they are rounded to bf16 in between
    assert abs(float(loss) - float(ref)) < tol * max(1.0, abs(float(ref)))
    assert rel_l2(g.float(), 2.0 * gref) < 4e-3
    if fused_ok:
        # bit-identical from run to run (a gather, no atomics) and equal to the two-op composition to 16-bit rounding
        ld2 = nhwc(logits).requires_grad_(True)
        (g2,) = torch.autograd.grad(ops.seg_cross_entropy_resized(ld2, tgt.to(dev()), 255, ac) * 2.0, ld2)
        assert torch.equal(g, g2)
        ld3 = nhwc(logits).requires_grad_(True)
        two = ops.seg_cross_entropy(ops.resize_bilinear(ld3, (Ho, Wo), ac), tgt.to(dev()), 255)
        (g3,) = torch.autograd.grad(two * 2.0, ld3)
        assert abs(float(two) - float(loss)) < 3e-3 * max(1.0, abs(float(ref)))
        assert rel_l2(g.float(), g3.float()) < 8e-3
        # pad channels of the gradient buffer are zero (the 1x1 classifier's backward reads the padded pitch)
        base = g._base
        if base is not None and base.dim() == 4 and base.shape[-1] > Cc:   # [N][Hi][Wi][round8(C)]
            assert float(base[..., Cc:].abs().max()) == 0.0
    allign = torch.full((N, Ho, Wo), 255)
    l0 = ops.seg_cross_entropy_resized(nhwc(logits).requires_grad_(True), allign.to(dev()), 255, ac)
    assert float(l0) == 0.0


def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    out = {}
    for k in z.files:
        parts = k.split("/", 1)
        if len(parts) == 1:
            out[k] = z[k]
        else:
            out.setdefault(parts[0], {})[parts[1]] = z[k]
    return out


def test_hip_deeplab_head_vs_reference_vectors():
    g = _load("deeplabv3plus_head")
    T = lambda a: torch.from_numpy(np.asarray(a))
    m = deeplab.Deeplabv3PlusHead(19, in_channels=64, channels=32, dilations=(1, 2, 3, 4), low_in_channels=16, low_channels=8, dropout_ratio=0)
    missing, unexpected = m.load_state_dict({k: T(v) for k, v in g["state"].items()}, strict=True)
    assert not missing and not unexpected
    m.to(dev()).train()
    xs = [nhwc(T(g["x"][str(i)])).requires_grad_(True) for i in range(2)]
    logits = m(xs)
    assert rel_l2(logits.float(), T(g["logits"])) < 3e-2, rel_l2(logits.float(), T(g["logits"]))
    tgt = T(g["target"]).to(dev())
    loss = ops.seg_cross_entropy(ops.resize_bilinear(logits, tgt.shape[-2:], False), tgt, 255)
    assert abs(float(loss) - float(g["loss"])) < 2e-2 * float(g["loss"])
    named = [(n, q) for n, q in m.named_parameters()]
    grads = torch.autograd.grad(loss, xs + [q for _, q in named])
    for i in range(2):
        assert cosine(grads[i].float(), T(g["gx"][str(i)])) > 0.97, (i, cosine(grads[i].float(), T(g["gx"][str(i)])))
    cs = sorted((cosine(a.float(), T(g["gparam"][n])), n) for (n, _), a in zip(named, grads[2:]) if float(T(g["gparam"][n]).norm()) > 1e-7)
    # tiny head, tiny gradients (|g| ~ 1e-5) and BatchNorm over N=2 samples in the pooled branch: bf16 storage noise
    assert np.median([c for c, _ in cs]) > 0.97 and cs[0][0] > 0.8, cs[:4]


@pytest.mark.parametrize("output_stride", [32, 8])
def test_deeplab_end_to_end_vs_oracle(output_stride):
    from oracle import torch_ref as R
    torch.manual_seed(0)
    ref = R.EncoderDecoder(19, output_stride=output_stride, dropout_ratio=0)
    hip = deeplab.EncoderDecoder(19, output_stride=output_stride, dropout_ratio=0)
    hip.load_state_dict(ref.state_dict())
    imgs, tgt = R.synthetic_seg_batch(2, (128, 192), seed=3)
    ref.train()
    lr = ref(imgs, tgt, "train")["loss"]
    lr.backward()
    hip.to(dev()).train()
    lh = hip(imgs.to(dev()), tgt.to(dev()), "train")["loss"]
    lh.backward()
    torch.cuda.synchronize()
    assert abs(float(lh) - float(lr)) < 3e-2 * abs(float(lr)), (float(lh), float(lr))
    rp = dict(ref.named_parameters())
    # noise floor of bf16 storage: the oracle under CPU bf16 autocast
    ref2 = R.EncoderDecoder(19, output_stride=output_stride, dropout_ratio=0)
    ref2.load_state_dict(ref.state_dict())
    ref2.train()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        l2 = ref2(imgs, tgt, "train")["loss"]
    l2.backward()
    # At this size the fp32 gradient below the head is chaotic: the oracle's own bf16 run keeps cosine ~0 with it there, and that
    # median (~0.00 to ~0.08) depends on the host CPU's bf16 kernels. The gradients that survive bf16 storage in the oracle
    # (cosine > 0.9: the classifier, the last fused BatchNorm) must survive it in the engine as well, each one. The backbone's
    # gradients are pinned block by block, teacher-forced, in test_gpu_full_size.py::test_deeplabv3plus_512x1024_bottlenecks_teacher_forced_vs_oracle.
    hp = dict(hip.named_parameters())
    floor = {n: cosine(p.grad.float(), rp[n].grad) for n, p in ref2.named_parameters()}
    kept = {n: (f, cosine(hp[n].grad.float(), rp[n].grad)) for n, f in floor.items() if f > 0.9}
    assert len(kept) >= 2 and "head.cls_seg.weight" in kept, sorted(kept)
    for n, (f, got) in kept.items():
        assert got > f - 0.05, (n, got, f)
    rb = dict(ref.named_buffers())
    for n, b in hip.named_buffers():
        if "running_mean" in n and "layer1.0" in n:
            assert rel_l2(b.float(), rb[n]) < 5e-2, n
    hip.eval()
    with torch.no_grad():
        pred = hip(imgs.to(dev()), tgt.to(dev()), "val")
    assert tuple(pred.shape) == (2, 128, 192) and pred.dtype == torch.int64


@pytest.mark.parametrize("inplanes,planes,stride", [(256, 64, 1), (256, 128, 2)])
def test_residual_tail_merged_pass_equals_two_passes(inplanes, planes, stride):
    """Round 5 (VERDICT r04 task 6, 'ReLU-mask + BN-sums merged at the residual tails'): cvhip_bn_tail_bwd_sums_acc computes
    du = dz * relu'(z), stores it and reduces (sum du, sum du*xhat) in ONE pass; the two-pass form (apply on z, then reduce) must give
    the same du (same 16-bit rounding) and the same sums (same per-thread order): every gradient of a Bottleneck block identical to
    1e-6 relative (fp64 accumulators: arrival order only)."""
    import torch
    from cvpytorch_amd import deeplab, ops
    d = torch.device("cuda:0")
    torch.manual_seed(9)
    ds = None
    if stride != 1 or inplanes != planes * 4:
        ds = torch.nn.Sequential(deeplab.HipConv2d(inplanes, planes * 4, 1, stride=stride, bias=False), deeplab.HipBN(planes * 4))
    blk = deeplab.Bottleneck(inplanes, planes, stride, ds).to(d).train()
    x0 = torch.randn(4, inplanes, 64, 64, device=d).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    g = None
    out = {}
    for flag in (False, True):
        ops._TAIL_MERGE = flag
        for p_ in blk.parameters():
            p_.grad = None
        x = x0.clone().requires_grad_(True)
        z = blk(x)
        if g is None:
            g = (torch.randn_like(z.float()) * 0.1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        z.backward(g)
        torch.cuda.synchronize()
        out[flag] = [x.grad.float().clone()] + [p_.grad.float().clone() for p_ in blk.parameters()]
    ops._TAIL_MERGE = True
    for a, b in zip(out[True], out[False]):
        e = float((a - b).norm() / max(float(b.norm()), 1e-12))
        assert e <= 2e-3, e     # (weight gradients: fp32 atomics in a different order; dx / BN gradients: see the sums)
    # the BatchNorm gradients of the tail layer come straight from the sums: equal to accumulation-order precision
    names = [n for n, _ in blk.named_parameters()]
    for n in ("bn3.weight", "bn3.bias"):
        i = 1 + names.index(n)
        e = float((out[True][i] - out[False][i]).abs().max() / max(float(out[False][i].abs().max()), 1e-12))
        assert e <= 1e-6, (n, e)
