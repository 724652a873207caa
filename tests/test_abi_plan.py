"""CPU-only checks of the C-ABI boundary: libcvhip.so loads without a GPU, exports every symbol that
include/cvhip.h declares, refuses bad descriptors with the documented status codes, and its HOST-SIDE
planning (conv output size, BN partial rows, the dgrad stride-parity decomposition + weight-image
layout) is arithmetically right — verified by interpreting the plan in numpy and comparing with
torch's own conv backward. No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cvpytorch_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "cvhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cvhip_[a-z0-9_]+)\s*\(", src)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = L.load()
    assert lib.cvhip_version() >= 100
    syms = header_symbols()
    assert len(syms) >= 45
    raw = C.CDLL(L.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), "libcvhip.so does not export %s" % s
        assert s in L.SIGNATURES, "cvpytorch_amd.lib has no ctypes signature for %s" % s
    for s in L.SIGNATURES:
        assert s in syms, "%s bound in lib.py but not declared in include/cvhip.h" % s


def test_probes_are_a_library_of_their_own():
    """The measurement / known-answer kernels are NOT in the product library: include/cvhip.h declares no cvhip_probe_* symbol,
    libcvhip.so exports none, and libcvhip_probes.so exports exactly what include/cvhip_probes.h declares (== lib.PROBE_SIGNATURES)."""
    assert not [s for s in header_symbols() if "probe" in s]
    raw = C.CDLL(L.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "cvhip_probes.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cvhip_probe[a-z0-9_]*)\s*\(", src)))
    assert len(declared) >= 12 and "cvhip_probes_last_error" in declared
    probes = C.CDLL(L.PROBES_LIB_PATH)
    for s in declared:
        assert hasattr(probes, s), "libcvhip_probes.so does not export %s" % s
        assert not hasattr(raw, s), "%s is still exported by the product library" % s
        assert s == "cvhip_probes_last_error" or s in L.PROBE_SIGNATURES
    assert sorted(L.PROBE_SIGNATURES) == [s for s in declared if s != "cvhip_probes_last_error"]
    assert not set(L.PROBE_SIGNATURES) & set(L.SIGNATURES)


def test_fp16_abi_is_generated_in_sync_and_exported():
    """csrc/f16_names.h and include/cvhip_f16.h are what tools/gen_f16_names.py produces from the current sources, and the
    library exports every renamed entry point (the fp16-storage build of each 16-bit kernel)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_f16_names", os.path.join(ROOT, "tools", "gen_f16_names.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    a, b, names = gen.render()
    assert open(os.path.join(ROOT, "cvpytorch_amd", "csrc", "f16_names.h")).read() == a
    assert open(os.path.join(ROOT, "include", "cvhip_f16.h")).read() == b
    assert len(names) >= 70 and "cvhip_conv2d_fprop" in names and "cvhip_comm_init_rank" not in names
    raw = C.CDLL(L.LIB_PATH)
    L.load()
    for n in names:
        assert hasattr(raw, n + "_f16"), n
        assert n in L._F16


def desc(N, Cc, H, W, K, R, S, stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1, x_ld=None, y_ld=None):
    return L.ConvDesc(N, Cc, H, W, K, R, S, stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], groups,
                      x_ld or Cc, y_ld or K, 0, 0)


@pytest.mark.parametrize("H,W,R,S,s,p,d", [(640, 640, 6, 6, 2, 2, 1), (80, 80, 3, 3, 1, 1, 1), (81, 77, 3, 3, 2, 1, 1),
                                           (32, 64, 3, 3, 1, 12, 12), (20, 20, 1, 1, 1, 0, 1), (9, 9, 5, 3, 3, 2, 2)])
def test_out_hw_matches_torch(H, W, R, S, s, p, d):
    lib = L.load()
    dd = desc(1, 8, H, W, 8, R, S, (s, s), (p, p), (d, d))
    P, Q = C.c_int32(), C.c_int32()
    assert lib.cvhip_conv2d_out_hw(C.byref(dd), C.byref(P), C.byref(Q)) == 0
    y = F.conv2d(torch.zeros(1, 1, H, W), torch.zeros(1, 1, R, S), stride=s, padding=p, dilation=d)
    assert (P.value, Q.value) == tuple(y.shape[2:])


def test_descriptor_validation_status_codes():
    lib = L.load()
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(2, 3, 8, 8, 16, 3, 3))) == L.ERR_UNSUPPORTED  # C % 8 != 0
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(2, 16, 8, 8, 16, 3, 3, groups=2))) == L.ERR_UNSUPPORTED
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(0, 16, 8, 8, 16, 3, 3))) == L.ERR_INVALID
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(2, 16, 8, 8, 16, 3, 3, x_ld=8))) == L.ERR_INVALID  # pitch < C
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(1, 16, 2, 2, 16, 5, 5))) == L.ERR_INVALID  # empty output
    # null pointers are refused before any launch
    assert lib.cvhip_conv2d_fprop(C.byref(desc(2, 16, 8, 8, 16, 3, 3)), None, None, None, None, None, None) == L.ERR_INVALID
    assert lib.cvhip_bn_act_fwd(None, 8, None, 8, 4, 8, None, None, 0, 0.0, None, 0, None) == L.ERR_INVALID
    assert lib.cvhip_nms_sorted(None, 5, 0.5, None, None, None, None) == L.ERR_INVALID
    with pytest.raises(L.CvhipError):
        L.call("cvhip_conv2d_fprop", C.byref(desc(2, 16, 8, 8, 16, 3, 3)), None, None, None, None, None, None)


def test_stats_rows_tiles():
    lib = L.load()
    # the 8-channel image stem runs on the persistent direct kernel (conv_stem.hip): one partial row per block
    stem = desc(64, 8, 640, 640, 32, 6, 6, (2, 2), (2, 2))
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(stem)) == lib.cvhip_conv_stem_blocks(C.byref(stem)) == 768
    # multi-tap convolutions whose 128-wide output tiles all fit the 512 resident block slots: the patch-resident kernel
    # (conv_patch.hip default policy), one partial row per spatial tile
    def patch_rows(dd):
        buf = (C.c_int32 * (4 * L.PATCH_CLASS_INTS))()
        assert lib.cvhip_conv2d_patch_plan(C.byref(dd), 0, buf, 4) == 1
        return buf[24] // buf[23]   # total_tiles / n_tiles
    mid = desc(64, 128, 40, 40, 128, 3, 3, (1, 1), (1, 1))
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(mid)) == patch_rows(mid) <= 512
    # per-tap implicit GEMM (narrow outputs, stride-2 inputs, too many tiles): block-M is 256 for K <= 64 and 128 / 256 otherwise
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(64, 32, 160, 160, 32, 3, 3, (1, 1), (1, 1)))) == (64 * 160 * 160 + 255) // 256
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(64, 32, 320, 320, 64, 3, 3, (2, 2), (1, 1)))) == (64 * 160 * 160 + 255) // 256
    # 1x1 stride 1 with enough rows: the persistent streaming kernel (conv1x1_stream.hip), balanced grid <= 512
    pw = desc(64, 64, 160, 160, 32, 1, 1)
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(pw)) == lib.cvhip_conv1x1_stream_blocks(32, 64, 64 * 160 * 160, 1) == 512
    small = desc(2, 128, 40, 40, 128, 3, 3, (1, 1), (1, 1))
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(small)) == patch_rows(small)
    assert lib.cvhip_conv2d_fprop_stats_rows(C.byref(desc(2, 128, 80, 80, 128, 3, 3, (2, 2), (1, 1)))) == (2 * 1600 + 127) // 128
    assert lib.cvhip_colreduce_rows(10, 32) == 1
    assert lib.cvhip_colreduce_rows(10 ** 7, 32) == 1024
    assert lib.cvhip_nms_workspace_bytes(100) == (100 * 2 + 2) * 8


def dgrad_plan(dd):
    lib = L.load()
    buf = (C.c_int32 * (16 * L.DGRAD_CLASS_INTS))()
    n = lib.cvhip_conv2d_dgrad_plan(C.byref(dd), buf, 16)
    assert n > 0
    cls = []
    for i in range(n):
        v = [buf[i * L.DGRAD_CLASS_INTS + j] for j in range(L.DGRAD_CLASS_INTS)]
        cls.append(dict(TR=v[0], TS=v[1], r0=v[2], r_step=v[3], dh0=v[4], dh_step=v[5], s0=v[6], s_step=v[7], dw0=v[8],
                        dw_step=v[9], w_off=(v[10] & 0xffffffff) | (v[11] << 32)))
    return cls


def interpret_dgrad(dd, dy_nhwc, w_krsc):
    """numpy interpreter of the dgrad plan: exactly the gather the igemm kernel performs per class."""
    N, Cc, H, W, K = dd.N, dd.C, dd.H, dd.W, dd.K
    P, Q = dy_nhwc.shape[1:3]
    sh, sw = dd.stride_h, dd.stride_w
    classes = dgrad_plan(dd)
    assert len(classes) == sh * sw
    total = L.load().cvhip_conv2d_dgrad_weight_elems(C.byref(dd))
    wimg = np.zeros(total, dtype=np.float64)
    # weight image: per class [C][taps][K] at w_off
    for q, cl in enumerate(classes):
        T_ = cl["TR"] * cl["TS"]
        for i in range(cl["TR"]):
            for j in range(cl["TS"]):
                r, s = cl["r0"] + i * cl["r_step"], cl["s0"] + j * cl["s_step"]
                blk = w_krsc[:, r, s, :].T  # (C, K)
                for c in range(Cc):
                    o = cl["w_off"] + (c * T_ + i * cl["TS"] + j) * K
                    wimg[o:o + K] = blk[c]
    assert sum(Cc * cl["TR"] * cl["TS"] * K for cl in classes) == total
    dx = np.zeros((N, H, W, Cc))
    qi = 0
    for ph in range(sh):
        for pw in range(sw):
            cl = classes[qi]
            qi += 1
            T_ = cl["TR"] * cl["TS"]
            OHi = (H - ph + sh - 1) // sh if ph < H else 0
            OWi = (W - pw + sw - 1) // sw if pw < W else 0
            wq = wimg[cl["w_off"]:cl["w_off"] + Cc * T_ * K].reshape(Cc, T_, K) if T_ else None
            for hh in range(OHi):
                for ww in range(OWi):
                    acc = np.zeros((N, Cc))
                    for i in range(cl["TR"]):
                        ih = hh + cl["dh0"] + i * cl["dh_step"]
                        if not (0 <= ih < P):
                            continue
                        for j in range(cl["TS"]):
                            iw = ww + cl["dw0"] + j * cl["dw_step"]
                            if not (0 <= iw < Q):
                                continue
                            acc += dy_nhwc[:, ih, iw, :] @ wq[:, i * cl["TS"] + j, :].T
                    dx[:, hh * sh + ph, ww * sw + pw, :] = acc
    return dx


@pytest.mark.parametrize("H,W,R,S,stride,pad,dil", [
    (8, 10, 3, 3, (1, 1), (1, 1), (1, 1)),
    (8, 10, 3, 3, (2, 2), (1, 1), (1, 1)),
    (9, 11, 3, 3, (2, 2), (1, 1), (1, 1)),   # odd sizes: parity classes of unequal extent
    (12, 12, 6, 6, (2, 2), (2, 2), (1, 1)),  # YOLOv5 stem geometry
    (8, 8, 1, 1, (2, 2), (0, 0), (1, 1)),    # ResNet downsample: three empty classes must write zeros
    (10, 10, 3, 3, (1, 1), (2, 2), (2, 2)),  # dilation
    (11, 9, 3, 5, (2, 1), (1, 2), (1, 1)),   # asymmetric
    (13, 13, 5, 5, (3, 3), (2, 2), (1, 1)),
    (12, 12, 3, 3, (2, 2), (2, 2), (2, 2)),  # stride 2 + dilation 2: only one parity per axis has taps
])
def test_dgrad_plan_interpreted_matches_torch(H, W, R, S, stride, pad, dil):
    torch.manual_seed(0)
    N, Cc, K = 2, 8, 8
    x = torch.randn(N, Cc, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(K, Cc, R, S, dtype=torch.float64)
    y = F.conv2d(x, w, stride=stride, padding=pad, dilation=dil)
    dy = torch.randn_like(y)
    (gx,) = torch.autograd.grad(y, x, dy)
    dd = desc(N, Cc, H, W, K, R, S, stride, pad, dil)
    got = interpret_dgrad(dd, dy.permute(0, 2, 3, 1).numpy(), w.permute(0, 2, 3, 1).numpy())
    np.testing.assert_allclose(got, gx.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-10, atol=1e-10)


def test_div31_constants_divide_exactly():
    """conv_plan.h div31_consts / fast_div31: q = umulhi(n, mul) >> shift must equal n // d for every 0 <= n < 2^31 the kernels
    can meet (pixel indices) — checked at the edges of every quotient step near 2^31, at small n, and on random draws."""
    import random
    lib = L.load()
    rng = random.Random(1029)
    ds = [1, 2, 3, 5, 7, 20, 25, 40, 80, 160, 320, 400, 1600, 6400, 25600, 102400, 409600, 1 << 16, (1 << 16) + 1, 999983, (1 << 30) - 1, 1 << 30, (1 << 31) - 1]
    ds += [rng.randrange(1, 1 << 22) for _ in range(200)]
    for d in ds:
        mul, sh = C.c_uint32(), C.c_uint32()
        assert lib.cvhip_div31_consts(d, C.byref(mul), C.byref(sh)) == 0
        m, s = mul.value, sh.value
        assert (m == 0) == (d == 1)
        top = (1 << 31) - 1
        ns = [0, 1, d - 1, d, d + 1, top, top - 1, (top // d) * d, max((top // d) * d - 1, 0)]
        ns += [rng.randrange(0, 1 << 31) for _ in range(300)] + [k * d + o for k in (1, 2, 1000, top // d - 1) for o in (-1, 0, 1) if 0 <= k * d + o <= top]
        for n in ns:
            q = n if m == 0 else ((n * m) >> 32) >> s
            assert q == n // d, (d, n, q, n // d, m, s)
    assert lib.cvhip_div31_consts(0, C.byref(mul), C.byref(sh)) == L.ERR_INVALID


def test_default_path_kernels_do_not_spill():
    """build.py keeps the compiler's per-kernel resource remarks (csrc/_obj/*.usage.txt). A tuned kernel that starts to spill
    registers to scratch still passes every parity test — it is just 30-80 % slower (round 3: runtime-flag tail sums in
    bwd1x1_kernel<128,128>, 104 spilled VGPRs). The few kernels allowed to spill are listed explicitly, and every entry must still
    match a kernel of the build."""
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(here, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    rows = ru.table()
    if not rows:
        pytest.skip("no usage files (library was not built by cvpytorch_amd.build in this tree)")
    allowed = (
        r"stem_fprop_kernelILi1ELi13ELb0ELb1E",                 # fused-epilogue instance of the 7x7 stride-1 stem (inference only)
        r"conv_patch_kernelILi128ELi32ELi1E",                   # prologue form, 128 x 64 wave tiles: the values only the per-chunk in-place
                                                                # transform uses (its constants' addresses, ownership mask) are parked in
                                                                # scratch across the K loop — 16 dwords read once per 32-channel chunk
    )
    bad = []
    for obj, k, d in rows:
        sc = d.get("ScratchSize [bytes/lane]", 0)
        if sc > 32 and not any(re.search(a, k) for a in allowed):
            bad.append((obj, k, sc))
    assert not bad, bad
    stale = [a for a in allowed if not any(re.search(a, k) for _, k, _ in rows)]
    assert not stale, "allowed-spill entries that match no kernel of the build: %s" % stale
