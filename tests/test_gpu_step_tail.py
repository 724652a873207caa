"""cvhip_train_step_tail — EMA of the floating-point buffers, the step counters' add and the zero fill of two ranges in one launch —
against the four calls it replaces (cvhip_ema_update, cvhip_i64_add, 2 x cvhip_zero_fill): bitwise, and nothing outside the ranges moves."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cvpytorch_amd import lib as L
from test_gpu_modules import dev


def _state(seed, n_ema, n_cnt, words_a, words_b, pad):
    g = torch.Generator().manual_seed(seed)
    ema = torch.randn(n_ema, generator=g).to(dev())
    src = torch.randn(n_ema, generator=g).to(dev())
    cnt = torch.randint(0, 1 << 40, (max(n_cnt, 1),), generator=g, dtype=torch.int64).to(dev())
    # the ranges sit `pad` words into buffers of random bits, with as many guard words behind them
    a = torch.randint(-2 ** 31, 2 ** 31 - 1, (words_a + 2 * pad + 8,), generator=g, dtype=torch.int32).to(dev())
    b = torch.randint(-2 ** 31, 2 ** 31 - 1, (words_b + 2 * pad + 8,), generator=g, dtype=torch.int32).to(dev())
    dyn = torch.tensor([0.9973, 1.0], dtype=torch.float32, device=dev())
    return ema, src, cnt, a, b, dyn


@pytest.mark.parametrize("n_ema,n_cnt,words_a,words_b,pad", [(1000, 7, 4096 + 4, 260, 0), (1000, 7, 4099, 257, 1), (0, 0, 64, 0, 0), (333, 0, 0, 0, 0),
                                                              (70000, 300, 300000, 1028, 4)],
                         ids=["16-byte-ranges", "word-ranges", "fill-only", "ema-only", "several-blocks"])
def test_step_tail_equals_the_four_calls(n_ema, n_cnt, words_a, words_b, pad):
    ref = _state(5, n_ema, n_cnt, words_a, words_b, pad)
    got = [t.clone() for t in ref]
    ema, src, cnt, a, b, dyn = ref
    if n_ema:
        L.call("cvhip_ema_update", ema.data_ptr(), src.data_ptr(), n_ema, 0.0, dyn.data_ptr(), None)
    if n_cnt:
        L.call("cvhip_i64_add", cnt.data_ptr(), n_cnt, 1, None)
    L.call("cvhip_zero_fill", a.data_ptr() + 4 * pad, 4 * words_a, None)
    L.call("cvhip_zero_fill", b.data_ptr() + 4 * pad, 4 * words_b, None)
    ema2, src2, cnt2, a2, b2, dyn2 = got
    L.call("cvhip_train_step_tail", ema2.data_ptr() if n_ema else None, src2.data_ptr() if n_ema else None, n_ema, 0.0, dyn2.data_ptr(),
           cnt2.data_ptr() if n_cnt else None, n_cnt, 1, a2.data_ptr() + 4 * pad if words_a else None, 4 * words_a,
           b2.data_ptr() + 4 * pad if words_b else None, 4 * words_b, None)
    torch.cuda.synchronize()
    assert torch.equal(ema.view(torch.int32), ema2.view(torch.int32))
    assert torch.equal(cnt, cnt2)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    if words_a:
        assert int(a2[pad:pad + words_a].abs().max()) == 0 and int(a2[pad + words_a:].abs().max()) != 0
    if n_ema:
        ema0 = _state(5, n_ema, n_cnt, words_a, words_b, pad)[0]
        assert not torch.equal(ema2, ema0) and torch.isfinite(ema2).all()
