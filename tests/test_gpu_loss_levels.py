"""The multi-level entries of the fused YOLOv5 loss (cvhip_yolov5_loss_fwd_levels / _bwd_levels: one launch per stage for the whole
pyramid, one workspace) against the per-level entries (cvhip_yolov5_loss_level_fwd / _level_bwd_bias) on the same maps and targets.
Every level keeps its arithmetic, its partial-row layout and its reduction order, so everything is compared BITWISE: the four sums of
every level, total and stats of the finalize, every gradient map, every block of bias partial rows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cvpytorch_amd import lib as L
from test_gpu_modules import dev

N, A, NC = 2, 3, 3
NO = NC + 5
T = 16
ANCHOR_FRAC = ((0.15, 0.15), (0.30, 0.25), (0.10, 0.30))   # anchors as fractions of the map: the ratio test is the same on every level


def _targets():
    """16 rows: cells claimed by several targets (winner conflicts, lists of duplicates), boxes on the border (index clamp), targets
    that fail the ratio test on some anchors, and padded rows (img < 0 with zero boxes, and all-zero rows)."""
    t = torch.zeros(T, 6)
    t[0] = torch.tensor([0, 0, 0.52, 0.47, 0.20, 0.25])
    t[1] = torch.tensor([0, 1, 0.521, 0.471, 0.22, 0.24])     # same cell as row 0 on every level
    t[2] = torch.tensor([0, 2, 0.523, 0.469, 0.18, 0.26])     # and a third
    t[3] = torch.tensor([0, 1, 0.30, 0.80, 0.12, 0.30])
    t[4] = torch.tensor([1, 0, 1.0, 0.999, 0.30, 0.30])       # right / bottom border
    t[5] = torch.tensor([1, 2, 0.0, 0.0, 0.20, 0.20])         # top-left corner
    t[6] = torch.tensor([1, 1, 0.999, 0.001, 0.40, 0.10])
    t[7] = torch.tensor([1, 0, 0.26, 0.74, 0.15, 0.15])
    t[8] = torch.tensor([1, 2, 0.26, 0.74, 0.28, 0.27])       # same centre as row 7, other size
    t[9] = torch.tensor([0, 0, 0.75, 0.25, 0.90, 0.90])       # too large for every anchor
    t[10] = torch.tensor([0, 2, 0.0625, 0.9375, 0.10, 0.28])
    t[11] = torch.tensor([1, 1, 0.51, 0.51, 0.16, 0.14])
    t[12] = torch.tensor([-1, 0, 0.5, 0.5, 0.5, 0.5])         # padding
    t[13] = torch.tensor([-1, 0, 0.5, 0.5, 0.5, 0.5])
    # rows 14, 15 stay all-zero: image 0, class 0, a zero box — never selected (ratio test), still walked by every stage
    return t.to(dev())


def _desc(H, W, ld):
    d = L.YoloLossDesc(N, A, NO, H, W, ld, T, 4.0)
    for a, (fw, fh) in enumerate(ANCHOR_FRAC):
        d.anchors[2 * a], d.anchors[2 * a + 1] = fw * W, fh * H
    return d


def _run(sizes, ld):
    """-> (per-level results, multi-level results), each (sums, total, stats, [draw], [bias rows])"""
    g = torch.Generator().manual_seed(11 + 100 * len(sizes) + ld)
    nl = len(sizes)
    K = A * NO
    tg = _targets()
    raws = [torch.randn(N, H, W, ld, generator=g).to(torch.bfloat16).to(dev()) for H, W in sizes]
    descs = (L.YoloLossDesc * nl)()
    for i, (H, W) in enumerate(sizes):
        descs[i] = _desc(H, W, ld)
    gout = torch.tensor([0.75], dtype=torch.float32, device=dev())
    ncell = torch.tensor([float(N * A * H * W) for H, W in sizes], dtype=torch.float32, device=dev())
    balance = torch.tensor([4.0, 1.0, 0.4, 0.1][:nl], dtype=torch.float32, device=dev())
    k_box, k_cls = 0.05 * N, 0.5 * N / NC
    k_obj = [1.0 * b * N / (N * A * H * W) for b, (H, W) in zip((4.0, 1.0, 0.4, 0.1), sizes)]
    lib = L.load()

    def outputs():
        sums = torch.full((nl, 4), -7.0, dtype=torch.float32, device=dev())
        draws = [torch.full((N, H, W, ld), 3.0, dtype=torch.bfloat16, device=dev()) for H, W in sizes]
        bps = [torch.zeros((L.YOLO_BIAS_ROWS + L.REDUCE_SCRATCH_ROWS, 2, K), dtype=torch.float32, device=dev()) for _ in sizes]
        return sums, draws, bps

    def finish(sums, draws, bps):
        total = torch.empty(1, dtype=torch.float32, device=dev())
        stats = torch.empty(3, dtype=torch.float32, device=dev())
        L.call("cvhip_yolov5_loss_finalize", sums.data_ptr(), nl, ncell.data_ptr(), balance.data_ptr(), 0.05, 1.0, 0.5, NC, float(N),
               total.data_ptr(), stats.data_ptr(), None)
        torch.cuda.synchronize()
        return sums.cpu(), total.cpu(), stats.cpu(), [d.cpu() for d in draws], [b[:L.YOLO_BIAS_ROWS, 0].cpu() for b in bps]

    # per level
    sums, draws, bps = outputs()
    for i in range(nl):
        d = descs[i]
        nb = lib.cvhip_yolov5_loss_workspace_bytes(C.byref(d))
        assert nb > 0
        ws = torch.empty(int(nb), dtype=torch.uint8, device=dev())
        L.call("cvhip_yolov5_loss_level_fwd", C.byref(d), raws[i].data_ptr(), tg.data_ptr(), ws.data_ptr(), sums[i].data_ptr(), None)
        L.call("cvhip_yolov5_loss_level_bwd_bias", C.byref(d), raws[i].data_ptr(), tg.data_ptr(), ws.data_ptr(), sums[i].data_ptr(),
               gout.data_ptr(), k_box, k_cls, k_obj[i], draws[i].data_ptr(), bps[i].data_ptr(), None)
    per_level = finish(sums, draws, bps)

    # all levels at once
    sums, draws, bps = outputs()
    nb = lib.cvhip_yolov5_loss_workspace_bytes_levels(descs, nl)
    assert nb == sum(lib.cvhip_yolov5_loss_workspace_bytes(C.byref(descs[i])) for i in range(nl))
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev())
    vp = C.c_void_p * nl
    L.call("cvhip_yolov5_loss_fwd_levels", descs, nl, vp(*[r.data_ptr() for r in raws]), tg.data_ptr(), ws.data_ptr(), sums.data_ptr(), None)
    L.call("cvhip_yolov5_loss_bwd_levels", descs, nl, vp(*[r.data_ptr() for r in raws]), tg.data_ptr(), ws.data_ptr(), sums.data_ptr(),
           gout.data_ptr(), k_box, k_cls, (C.c_float * nl)(*k_obj), vp(*[d.data_ptr() for d in draws]), vp(*[b.data_ptr() for b in bps]), None)
    return per_level, finish(sums, draws, bps)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


LEVEL_SETS = [((8, 8), (4, 4), (2, 2)), ((6, 10), (3, 5)), ((8, 8),), ((8, 8), (4, 4), (2, 2), (1, 1))]


@pytest.mark.parametrize("ld", [32, 28], ids=["ld32-vector", "ld28-two-pass"])
@pytest.mark.parametrize("sizes", LEVEL_SETS, ids=["8-4-2", "6x10-3x5", "one-level", "four-levels"])
def test_levels_entries_equal_per_level_entries_bitwise(sizes, ld):
    """ld = 32: A*NO = 24 channels padded to a multiple of 8 (the one-pass vector fill of the gradient map); ld = 28: not a multiple of
    8, every level takes the zero-fill + objectness two-pass form inside the multi-level call"""
    (s0, t0, st0, d0, b0), (s1, t1, st1, d1, b1) = _run(sizes, ld)
    assert float(s0[0, 0]) >= 3.0, "the case matches targets (duplicates included) on the finest level"
    assert torch.isfinite(s0).all() and torch.isfinite(t0).all()
    assert torch.equal(_bits(s0), _bits(s1)), (s0, s1)
    assert torch.equal(_bits(t0), _bits(t1)) and torch.equal(_bits(st0), _bits(st1)), (t0, t1, st0, st1)
    for i, (a, b) in enumerate(zip(d0, d1)):
        assert float(a.float().abs().max()) > 0 and not bool((a == 3.0).all())
        assert torch.equal(_bits(a), _bits(b)), ("gradient map of level %d" % i, int((_bits(a) != _bits(b)).sum()))
    for i, (a, b) in enumerate(zip(b0, b1)):
        assert float(a.abs().max()) > 0
        assert torch.equal(_bits(a), _bits(b)), ("bias rows of level %d" % i, int((_bits(a) != _bits(b)).sum()))


def test_levels_entries_refuse_bad_level_counts():
    d = (L.YoloLossDesc * 1)()
    d[0] = _desc(4, 4, 32)
    lib = L.load()
    assert lib.cvhip_yolov5_loss_workspace_bytes_levels(d, 0) == L.ERR_INVALID
    assert lib.cvhip_yolov5_loss_workspace_bytes_levels(d, L.YOLO_MAX_LEVELS + 1) == L.ERR_INVALID
