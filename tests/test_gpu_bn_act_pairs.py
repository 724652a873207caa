"""The vector paths of csrc/bn_act.hip (pair-wise math, block-relative 32-bit or 64-bit addressing) against an fp64 evaluation of
the same formulas on the same 16-bit inputs, through the C ABI, for both storage precisions and every activation id.

Entry points: cvhip_bn_act_bwd_partial, cvhip_bn_act_bwd_sums_acc, cvhip_bn_tail_bwd_sums_acc, cvhip_bn_act_fwd,
cvhip_bn_add_act_fwd, cvhip_bn_act_fwd_acc, cvhip_bn_act_fwd_acc_lazyres, cvhip_bn_act_bwd_apply, cvhip_bn_act_bwd_apply_acc.

Shapes: C = 8 (one 16-byte vector), 24 (3 column vectors: 85 rows per pass, one idle thread), 136, 2056 (more than 256 column
vectors: a second column pass of the reduction); M = 1, 67, 4 * rows-per-pass + 1, 1500 (partial last trips, trips that are fully
masked for a wave); row pitch C and C + 8; and one pair of shapes on a really allocated > 2 GiB buffer whose pitch makes a block's
rows span more than 2^31 bytes, so that the kernels' 64-bit-address instances run. Outputs are prefilled with NaN.

Bounds (none of them tuned):
  * a stored 16-bit value:  |out - ref| <= ulp16 * sum|terms of the final expression| + smallest normal + inner, with ulp16 = 2^-7
    (bf16) or 2^-10 (fp16). `inner` is the effect of the fp32 error of the pre-activation u = y*scale + shift (+ residual), which the
    activation or its derivative may amplify without bound at a kink (ReLU' jumps at 0, h-swish' at +-3): the expression is evaluated
    at u - d and u + d with d = 2^-22 * (|y*scale| + |shift| + |residual|) (four fp32 roundings of the terms of u) and the
    difference is allowed on top. In the derivatives the sigmoid's own error counts too (act_d_spread).
  * the lazy residual is rounded to 16 bits before it is added, so it may land on the neighbouring 16-bit value: one more ulp16 * |r|.
  * an fp32 partial sum, or the fp64 accumulator it is added to:  |sum - ref| <= (n + 8) * 2^-24 * sum|term| + inner, with n the number
    of terms one fp32 chain adds (rows per block / rows per pass, rounded up).
  * the residual-tail pass stores du and sums what it stored: du is checked as a stored value, the sums against the stored du.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from cvpytorch_amd import lib as L

F64 = torch.float64
AP = float(torch.tensor(0.1, dtype=torch.float32))  # the activation parameter as the kernels receive it
EPS, MOM = 1e-3, 0.03
ACTS = [L.ACT_NONE, L.ACT_RELU, L.ACT_SILU, L.ACT_LEAKY, L.ACT_SIGMOID, L.ACT_HSWISH]
TAIL_ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_LEAKY)
LAZY_ACTS = (L.ACT_RELU, L.ACT_SILU, L.ACT_LEAKY)
EW_ACC_MAX_C = 2048
PRECS = {"bf16": (torch.bfloat16, 2.0 ** -7, 2.0 ** -126), "fp16": (torch.float16, 2.0 ** -10, 2.0 ** -14)}


def dev():
    return torch.device("cuda:0")


def rows_per_pass(C):
    return 256 // min((C + 7) // 8, 256)


def act_f(u, act):
    if act == L.ACT_RELU:
        return u.clamp_min(0)
    if act == L.ACT_SILU:
        return u * torch.sigmoid(u)
    if act == L.ACT_LEAKY:
        return torch.where(u > 0, u, u * AP)
    if act == L.ACT_SIGMOID:
        return torch.sigmoid(u)
    if act == L.ACT_HSWISH:
        return u * (u + 3).clamp(0, 6) / 6
    return u


def act_d(u, act, rel=0.0):
    """act'(u); rel: a relative error put on the sigmoid inside it"""
    one, zero = torch.ones_like(u), torch.zeros_like(u)
    if act == L.ACT_RELU:
        return torch.where(u > 0, one, zero)
    if act == L.ACT_SILU:
        s = torch.sigmoid(u) * (1 + rel)
        return s * (1 + u * (1 - s))
    if act == L.ACT_LEAKY:
        return torch.where(u > 0, one, one * AP)
    if act == L.ACT_SIGMOID:
        s = torch.sigmoid(u) * (1 + rel)
        return s * (1 - s)
    if act == L.ACT_HSWISH:
        return torch.where(u <= -3, zero, torch.where(u >= 3, one, (2 * u + 3) / 6))
    return one


def spread(f, u, d):
    """|f(u + d) - f(u - d)|: what an error of d in u can do to f(u), kinks included"""
    return (f(u + d) - f(u - d)).abs()


def act_d_spread(u, act, d):
    """what the fp32 evaluation can do to act'(u): an error of d in u, and the sigmoid's own error — v_exp_f32 and v_rcp_f32 are good
    to 1 ulp each and 1 + e rounds once, 2^-22 relative on s in all, which 1 - s amplifies without bound as s -> 1"""
    return spread(lambda v: act_d(v, act), u, d) + (act_d(u, act, 2.0 ** -22) - act_d(u, act, -2.0 ** -22)).abs()


class Case:
    """The operands of one shape as [M, C] views of pitch ld, and a factory for NaN-filled outputs of the same layout."""

    def __init__(self, prec, M, C, ld, views=None):
        self.prec, self.M, self.C, self.ld = prec, M, C, ld
        self.dt, self.ulp, self.tiny = PRECS[prec]
        d = dev()
        g = torch.Generator(device=d).manual_seed(1000 * C + M + ld)
        rnd = lambda s, o: (torch.randn(M, C, generator=g, device=d) * s + o).to(self.dt)
        vals = {"dz": rnd(0.1, 0.0), "y": rnd(1.5, 0.2), "res": rnd(1.1, -0.2), "zsaved": rnd(1.0, 0.3)}
        self._views = views
        self._bufs = []
        for k, v in vals.items():
            t = self._alloc(k)
            t.copy_(v)
            setattr(self, k, t)
        ch = lambda s, o: (torch.randn(C, generator=g, device=d) * s + o).float().contiguous()
        self.scale, self.shift = ch(0.2, 1.0), ch(0.3, 0.0)
        self.mean, self.invstd = ch(0.3, 0.2), (torch.rand(C, generator=g, device=d) + 0.5).float().contiguous()
        self.gamma, self.beta = ch(0.2, 1.0), ch(0.3, 0.0)
        self.rscale, self.rshift = ch(0.2, 1.0), ch(0.3, 0.0)
        self.dgamma, self.dbeta = ch(2.0, 0.0), ch(2.0, 0.0)

    def _alloc(self, name):
        if self._views is not None:
            return self._views[name]
        buf = torch.full((self.M, self.ld), float("nan"), dtype=self.dt, device=dev())
        self._bufs.append(buf)
        return buf[:, :self.C]

    def out(self):
        if self._views is not None:
            t = self._views["out"]
            t.fill_(float("nan"))
            return t, None
        buf = torch.full((self.M, self.ld), float("nan"), dtype=self.dt, device=dev())
        return buf[:, :self.C], buf

    def check_stored(self, what, out, buf, ref, terms, inner):
        tol = self.ulp * terms + self.tiny + inner
        err = (out.double() - ref).abs()
        bad = ~(err <= tol)  # a NaN left in the output is bad
        worst = float((err / tol).nan_to_num(nan=float("inf")).max())
        print("%s %s M=%d C=%d ld=%d: worst |err|/bound %.3f" % (what, self.prec, self.M, self.C, self.ld, worst))
        assert not bool(bad.any()), (what, self.prec, self.M, self.C, self.ld, worst)
        if buf is not None and self.ld > self.C:
            assert bool(buf[:, self.C:].isnan().all()), (what, "wrote outside its columns")


def check_sums(what, cs, got, ref, absum, inner, n):
    tol = (n + 8) * 2.0 ** -24 * absum + inner
    err = (got.double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    print("%s %s M=%d C=%d ld=%d n=%d: worst |err|/bound %.3f" % (what, cs.prec, cs.M, cs.C, cs.ld, n, worst))
    assert bool((err <= tol).all()), (what, cs.prec, cs.M, cs.C, cs.ld, worst)


def run_reductions(cs, act):
    M, C, ld = cs.M, cs.C, cs.ld
    d = dev()
    y, dz = cs.y.double(), cs.dz.double()
    sc, sh, mu, is_ = (t.double() for t in (cs.scale, cs.shift, cs.mean, cs.invstd))
    u = y * sc + sh
    du_d = 2.0 ** -22 * ((y * sc).abs() + sh.abs())
    xh = (y - mu) * is_
    t1 = dz * act_d(u, act)
    t2 = t1 * xh
    k1 = dz.abs() * act_d_spread(u, act, du_d)
    k2 = k1 * xh.abs()
    grid = L.load().cvhip_colreduce_rows(M, C)
    rpb = -(-M // grid)
    n = -(-rpb // rows_per_pass(C))

    def per_block(t):
        pad = torch.zeros(grid * rpb - M, C, dtype=F64, device=d)
        return torch.cat([t, pad]).view(grid, rpb, C).sum(1)

    # fp32 partial rows [grid][2][C]
    partial = torch.full((grid, 2, C), float("nan"), dtype=torch.float32, device=d)
    L.call("cvhip_bn_act_bwd_partial", dz_ptr(cs.dz), ld, dz_ptr(cs.y), ld, M, C, cs.scale.data_ptr(), cs.shift.data_ptr(), cs.mean.data_ptr(),
           cs.invstd.data_ptr(), act, AP, partial.data_ptr(), None)
    check_sums("bwd_partial s1", cs, partial[:, 0], per_block(t1), per_block(t1.abs()), per_block(k1), n)
    check_sums("bwd_partial s2", cs, partial[:, 1], per_block(t2), per_block(t2.abs()), per_block(k2), n)
    # fp64 accumulator [shards][2][acc_ld]; the columns behind C must stay untouched
    acc_ld = C + 8
    acc = torch.zeros(L.BN_ACC_SHARDS, 2, acc_ld, dtype=F64, device=d)
    acc[:, :, C:] = float("nan")
    L.call("cvhip_bn_act_bwd_sums_acc", dz_ptr(cs.dz), ld, dz_ptr(cs.y), ld, M, C, cs.scale.data_ptr(), cs.shift.data_ptr(), cs.mean.data_ptr(),
           cs.invstd.data_ptr(), act, AP, acc.data_ptr(), acc_ld, None)
    assert bool(acc[:, :, C:].isnan().all())
    s = acc[:, :, :C].sum(0)
    check_sums("bwd_sums_acc s1", cs, s[0], t1.sum(0), t1.abs().sum(0), k1.sum(0), n)
    check_sums("bwd_sums_acc s2", cs, s[1], t2.sum(0), t2.abs().sum(0), k2.sum(0), n)
    # the residual tail: du = dz * act'(z) from the saved output, stored, and summed as stored
    acc = torch.zeros(L.BN_ACC_SHARDS, 2, acc_ld, dtype=F64, device=d)
    du, du_buf = cs.out()
    st = L.fn("cvhip_bn_tail_bwd_sums_acc")(dz_ptr(cs.dz), ld, dz_ptr(cs.zsaved), ld, dz_ptr(cs.y), ld, dz_ptr(du), ld, M, C, cs.mean.data_ptr(),
                                            cs.invstd.data_ptr(), act, AP, acc.data_ptr(), acc_ld, None)
    if act not in TAIL_ACTS:
        assert st == L.ERR_UNSUPPORTED
        return
    L.check(st, "cvhip_bn_tail_bwd_sums_acc")
    ref = dz * act_d(cs.zsaved.double(), act)  # z is a 16-bit value: its sign is the same in every precision, no kink term
    cs.check_stored("tail du", du, du_buf, ref, ref.abs(), 0.0)
    dus = du.double()
    s = acc[:, :, :C].sum(0)
    check_sums("tail s1", cs, s[0], dus.sum(0), dus.abs().sum(0), 0.0, n)
    check_sums("tail s2", cs, s[1], (dus * xh).sum(0), (dus * xh).abs().sum(0), 0.0, n)


def dz_ptr(t):
    return t.data_ptr()


def run_forward(cs, act):
    M, C, ld = cs.M, cs.C, cs.ld
    d = dev()
    y, r = cs.y.double(), cs.res.double()
    f = lambda v: act_f(v, act)

    def ref_fwd(sc, sh, mode, extra_d=0.0):
        """mode 0: no residual, 1: after the activation, 2: before it. -> (ref, terms, inner)"""
        u = y * sc + sh + (r if mode == 2 else 0.0)
        dd = 2.0 ** -22 * ((y * sc).abs() + sh.abs() + (r.abs() if mode == 2 else 0.0)) + extra_d
        a = f(u)
        ref = a + (r if mode == 1 else 0.0)
        return ref, a.abs() + (r.abs() if mode == 1 else 0.0), spread(f, u, dd)

    sc, sh = cs.scale.double(), cs.shift.double()
    for mode, name in ((0, "cvhip_bn_act_fwd"), (1, "cvhip_bn_act_fwd"), (2, "cvhip_bn_add_act_fwd")):
        z, zb = cs.out()
        L.call(name, cs.y.data_ptr(), ld, z.data_ptr(), ld, M, C, cs.scale.data_ptr(), cs.shift.data_ptr(), act, AP,
               cs.res.data_ptr() if mode else None, ld if mode else 0, None)
        cs.check_stored("%s(res %d)" % (name, mode), z, zb, *ref_fwd(sc, sh, mode))

    # the accumulator forms derive scale / shift in their prologue from (sum y, sum y^2)
    acc = torch.zeros(L.BN_ACC_SHARDS, 2, C, dtype=F64, device=d)
    acc[3, 0] = y.sum(0)
    acc[7, 1] = (y * y).sum(0)
    m = acc[:, 0].sum(0) / M
    var = (acc[:, 1].sum(0) / M - m * m).clamp_min(0)
    g, b = cs.gamma.double(), cs.beta.double()
    sc_a = g / torch.sqrt(var + EPS)
    sh_a = b - m * sc_a
    # scale and shift are fp32 products of fp32 roundings of these: their error reaches u as well
    extra = 2.0 ** -22 * (b.abs() + (m * sc_a).abs())

    def stats():
        st4 = torch.full((4, C), float("nan"), dtype=torch.float32, device=d)
        rm = torch.full((C,), 0.5, dtype=torch.float32, device=d)
        rv = torch.full((C,), 2.0, dtype=torch.float32, device=d)
        return st4, rm, rv

    def head(z, st4, rm, rv):
        return (cs.y.data_ptr(), ld, z.data_ptr(), ld, M, C, acc.data_ptr(), C, M, cs.gamma.data_ptr(), cs.beta.data_ptr(), rm.data_ptr(),
                rv.data_ptr(), MOM, EPS, st4[0].data_ptr(), st4[1].data_ptr(), st4[2].data_ptr(), st4[3].data_ptr(), act, AP)

    def check_stats(st4, rm):
        for got, ref, mag in ((st4[0], m, m.abs()), (st4[1], 1 / torch.sqrt(var + EPS), 1 / torch.sqrt(var + EPS)), (st4[2], sc_a, sc_a.abs()),
                              (st4[3], sh_a, b.abs() + (m * sc_a).abs()), (rm, (1 - MOM) * 0.5 + MOM * m, 0.5 + m.abs())):
            assert bool(((got.double() - ref).abs() <= 2.0 ** -21 * mag + 1e-30).all())  # a handful of fp32 roundings each

    for mode in (0, 1, 2):
        z, zb = cs.out()
        st4, rm, rv = stats()
        st = L.fn("cvhip_bn_act_fwd_acc")(*head(z, st4, rm, rv), cs.res.data_ptr() if mode else None, ld if mode else 0, int(mode == 2), None)
        if C > EW_ACC_MAX_C:
            assert st == L.ERR_UNSUPPORTED
            continue
        L.check(st, "cvhip_bn_act_fwd_acc")
        cs.check_stored("cvhip_bn_act_fwd_acc(res %d)" % mode, z, zb, *ref_fwd(sc_a, sh_a, mode, extra))
        check_stats(st4, rm)

    z, zb = cs.out()
    st4, rm, rv = stats()
    st = L.fn("cvhip_bn_act_fwd_acc_lazyres")(*head(z, st4, rm, rv), cs.res.data_ptr(), ld, cs.rscale.data_ptr(), cs.rshift.data_ptr(), None)
    if C > EW_ACC_MAX_C or act not in LAZY_ACTS:
        assert st == L.ERR_UNSUPPORTED
        return
    L.check(st, "cvhip_bn_act_fwd_acc_lazyres")
    rs, rh = cs.rscale.double(), cs.rshift.double()
    ur = r * rs + rh
    lazy = f(ur).to(cs.dt).double()  # rounded as the stand-alone pass stores it
    u = y * sc_a + sh_a
    a = f(u)
    inner = spread(f, u, 2.0 ** -22 * ((y * sc_a).abs() + sh_a.abs()) + extra) + spread(f, ur, 2.0 ** -22 * ((r * rs).abs() + rh.abs()))
    cs.check_stored("cvhip_bn_act_fwd_acc_lazyres", z, zb, a + lazy, a.abs() + 2 * lazy.abs(), inner)
    check_stats(st4, rm)


def run_backward_apply(cs, act):
    M, C, ld = cs.M, cs.C, cs.ld
    d = dev()
    y, dz = cs.y.double(), cs.dz.double()
    sc, sh, mu, is_ = (t.double() for t in (cs.scale, cs.shift, cs.mean, cs.invstd))
    u = y * sc + sh
    dd = 2.0 ** -22 * ((y * sc).abs() + sh.abs())
    du = dz * act_d(u, act)
    xh = (y - mu) * is_
    inner = (sc * dz).abs() * act_d_spread(u, act, dd)

    def ref(s1, s2):
        return sc * (du - s1 / M - xh * s2 / M), (sc * du).abs() + (sc * s1 / M).abs() + (sc * xh * s2 / M).abs(), inner

    common = (cs.dz.data_ptr(), ld, cs.y.data_ptr(), ld)
    consts = (cs.scale.data_ptr(), cs.shift.data_ptr(), cs.mean.data_ptr(), cs.invstd.data_ptr())
    dy, dyb = cs.out()
    L.call("cvhip_bn_act_bwd_apply", *common, dy.data_ptr(), ld, M, C, *consts, cs.dgamma.data_ptr(), cs.dbeta.data_ptr(), act, AP, None)
    cs.check_stored("cvhip_bn_act_bwd_apply", dy, dyb, *ref(cs.dbeta.double(), cs.dgamma.double()))
    # without batch statistics (a frozen BatchNorm): dy = scale * du
    dy, dyb = cs.out()
    L.call("cvhip_bn_act_bwd_apply", *common, dy.data_ptr(), ld, M, C, cs.scale.data_ptr(), cs.shift.data_ptr(), None, None, None, None, act, AP, None)
    cs.check_stored("cvhip_bn_act_bwd_apply(no stats)", dy, dyb, sc * du, (sc * du).abs(), inner)
    # the accumulator form: (sum du, sum du*xhat) spread over the shards
    acc = torch.zeros(L.BN_ACC_SHARDS, 2, C, dtype=F64, device=d)
    acc[1, 0], acc[12, 0] = cs.dbeta.double() * 0.75, cs.dbeta.double() * 0.25
    acc[5, 1], acc[6, 1] = cs.dgamma.double() * 0.5, cs.dgamma.double() * 0.5
    s1, s2 = acc[:, 0].sum(0), acc[:, 1].sum(0)
    dy, dyb = cs.out()
    dg = torch.full((C,), float("nan"), dtype=torch.float32, device=d)
    db = torch.full((C,), float("nan"), dtype=torch.float32, device=d)
    st = L.fn("cvhip_bn_act_bwd_apply_acc")(*common, dy.data_ptr(), ld, M, C, *consts, acc.data_ptr(), C, dg.data_ptr(), db.data_ptr(), 0, act, AP, None)
    if C > EW_ACC_MAX_C:
        assert st == L.ERR_UNSUPPORTED
        return
    L.check(st, "cvhip_bn_act_bwd_apply_acc")
    cs.check_stored("cvhip_bn_act_bwd_apply_acc", dy, dyb, *ref(s1, s2))
    assert bool(((dg.double() - s2).abs() <= 2.0 ** -24 * s2.abs()).all()) and bool(((db.double() - s1).abs() <= 2.0 ** -24 * s1.abs()).all())


SHAPES = [(C, M, C + pad) for C in (8, 24, 136, 2056) for M in (1, 67, 4 * rows_per_pass(C) + 1, 1500) for pad in (0, 8)]


@functools.lru_cache(maxsize=None)
def small_case(prec, C, M, ld):
    return Case(prec, M, C, ld)


@pytest.fixture(params=["bf16", "fp16"])
def prec(request):
    L.set_precision(request.param)
    try:
        yield request.param
    finally:
        L.set_precision("bf16")


@pytest.mark.parametrize("act", ACTS)
def test_reductions(prec, act):
    for C, M, ld in SHAPES:
        run_reductions(small_case(prec, C, M, ld), act)
    torch.cuda.synchronize()


@pytest.mark.parametrize("act", ACTS)
def test_forward_apply(prec, act):
    for C, M, ld in SHAPES:
        run_forward(small_case(prec, C, M, ld), act)
    torch.cuda.synchronize()


@pytest.mark.parametrize("act", ACTS)
def test_backward_apply(prec, act):
    for C, M, ld in SHAPES:
        run_backward_apply(small_case(prec, C, M, ld), act)
    torch.cuda.synchronize()


# ---- 64-bit addressing: one block's rows span more than 2^31 bytes --------------------------------------------------------------
# C = 8. Reductions run M = 64 rows in ONE block (cvhip_colreduce_rows(64, 8) = 1) at a pitch of 2^24 + 8 elements: 64 rows * 2 *
# (2^24 + 8) bytes > 2^31. The elementwise passes run M = 1100 rows in one block (16 rows per thread * 256 rows per pass = 4096 rows
# per block: two trips, the second partial) at a pitch of 2^20 + 8 elements: 1100 * 2 * (2^20 + 8) bytes > 2^31. Every operand and
# output lives in the same really allocated buffer at its own column offset, so each of them needs the 64-bit form.
BIG_RED = (64, (1 << 24) + 8)
BIG_EW = (1100, (1 << 20) + 8)


@functools.lru_cache(maxsize=None)
def big_buffer():
    need = max(M * ld for M, ld in (BIG_RED, BIG_EW))
    return torch.empty(need, dtype=torch.int16, device=dev())


def big_case(prec, M, ld):
    assert M * ld * 2 > (1 << 31) and (M - 1) * ld + 5 * 8 <= big_buffer().numel()
    raw = big_buffer().view(PRECS[prec][0])
    views = {k: torch.as_strided(raw, (M, 8), (ld, 1), storage_offset=8 * i) for i, k in enumerate(("dz", "y", "res", "zsaved", "out"))}
    return Case(prec, M, 8, ld, views)


@pytest.mark.parametrize("act", ACTS)
def test_rows_spanning_2gib(prec, act):
    assert L.load().cvhip_colreduce_rows(BIG_RED[0], 8) == 1
    run_reductions(big_case(prec, *BIG_RED), act)
    cs = big_case(prec, *BIG_EW)
    run_forward(cs, act)
    run_backward_apply(cs, act)
    torch.cuda.synchronize()
