"""SPPF's pooling chain in one launch per direction (cvhip_sppf_chain_fwd / _bwd) against the three-launch chain it replaces: three
cvhip_maxpool2d_fwd calls on the slices of one (N, H, W, 4c) buffer, and the in-place walk of three accumulate-form cvhip_maxpool2d_bwd
calls. Values, arg-max bytes and the slice-0 gradient are compared BITWISE; the inputs carry exact ties, -inf and NaN."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cvpytorch_amd import lib as L
from test_gpu_modules import dev

N = 3


def _bits(t):
    return t.contiguous().view(torch.int16)


def _input(c, H, W, seed):
    """slice 0 of an (N, H, W, 4c) buffer: small integers (most windows hold exact ties), -inf and NaN sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, H, W, c), generator=g).float()
    r = torch.rand(N, H, W, c, generator=g)
    x[r < 0.06] = float("-inf")
    x[r > 0.97] = float("nan")
    x[0, 0, 0, 0] = float("-inf")          # a corner window
    x[N - 1, H - 1, W - 1, c - 1] = float("nan")
    buf = torch.full((N, H, W, 4 * c), 77.0, dtype=torch.bfloat16)
    buf[..., :c] = x.to(torch.bfloat16)
    return buf.to(dev())


def _three_fwd(buf, c, H, W, k):
    buf = buf.clone()
    idx = torch.full((3, N, H, W, c), 255, dtype=torch.uint8, device=buf.device)
    for j in range(3):
        L.call("cvhip_maxpool2d_fwd", buf.data_ptr() + j * c * 2, 4 * c, buf.data_ptr() + (j + 1) * c * 2, 4 * c, idx[j].data_ptr(),
               N, c, H, W, k, 1, k // 2, None)
    torch.cuda.synchronize()
    return buf, idx


def _three_bwd(d, idx, c, H, W, k):
    d = d.clone()
    for j in (2, 1, 0):
        L.call("cvhip_maxpool2d_bwd", d.data_ptr() + (j + 1) * c * 2, 4 * c, idx[j].data_ptr(), d.data_ptr() + j * c * 2, 4 * c,
               N, c, H, W, k, 1, k // 2, 1, None)
    torch.cuda.synchronize()
    return d


def _compare(c, H, W, k, seed):
    x = _input(c, H, W, seed)
    ref, ref_idx = _three_fwd(x, c, H, W, k)
    got = x.clone()
    got_idx = torch.full((3, N, H, W, c), 255, dtype=torch.uint8, device=x.device)
    L.call("cvhip_sppf_chain_fwd", got.data_ptr(), 4 * c, got_idx.data_ptr(), N, c, H, W, k, None)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got[..., :c]), _bits(x[..., :c])), "slice 0 is read only"
    for j in (1, 2, 3):
        a, b = _bits(ref[..., j * c:(j + 1) * c]), _bits(got[..., j * c:(j + 1) * c])
        assert torch.equal(a, b), ("values of stage %d" % j, int((a != b).sum()))
    assert torch.equal(ref_idx, got_idx), ("arg-max bytes", int((ref_idx != got_idx).sum()))
    assert int(ref_idx.max()) < k * k
    assert bool(torch.isnan(ref[..., c:].float()).any()), "a NaN wins every window that holds it"

    g = torch.Generator().manual_seed(seed + 1)
    d = torch.randn(N, H, W, 4 * c, generator=g).to(torch.bfloat16).to(dev())
    dref = _three_bwd(d, ref_idx, c, H, W, k)
    dgot = d.clone()
    L.call("cvhip_sppf_chain_bwd", dgot.data_ptr(), 4 * c, ref_idx.data_ptr(), N, c, H, W, k, None)
    torch.cuda.synchronize()
    a, b = _bits(dref[..., :c]), _bits(dgot[..., :c])
    assert torch.equal(a, b), ("slice-0 gradient", int((a != b).sum()))
    assert not torch.equal(a, _bits(d[..., :c])), "the pools' gradient reached slice 0"
    assert torch.equal(_bits(dgot[..., 3 * c:]), _bits(d[..., 3 * c:])), "slice 3 of the incoming gradient is read only"


@pytest.mark.parametrize("H,W", [(5, 7), (20, 20), (1, 3)], ids=["5x7", "20x20", "1x3"])
@pytest.mark.parametrize("c", [8, 40], ids=["c8", "c40-partial-group"])
def test_sppf_chain_equals_three_launch_chain_bitwise(c, H, W):
    """k = 5 (the instantiated size): c = 8 is one channel vector in a block of four, c = 40 five vectors = one full group and a partial
    one; 20 x 20 is SPPF's map in YOLOv5-s at 640, 5 x 7 a map smaller than two windows, 1 x 3 a map smaller than one"""
    _compare(c, H, W, 5, 3 + c + H)


@pytest.mark.parametrize("c,H,W,k", [(8, 5, 7, 3), (12, 6, 5, 5)], ids=["k3-not-instantiated", "c12-not-a-multiple-of-8"])
def test_sppf_chain_falls_back_to_the_three_launches(c, H, W, k):
    """shapes the one-launch kernels do not take: the entry points run the three single-pool launches themselves — same results"""
    _compare(c, H, W, k, 9)
