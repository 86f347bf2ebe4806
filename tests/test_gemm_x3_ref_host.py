"""Host checks of tests/gemm_x3_ref.py, the yardsticks of compute = A3T_BF16X3: the split is exact on 16-bit integers, the
three-product sum on integer operands is the full product minus sum lo_a lo_b, the error bound holds for the float64 emulation
on Gaussian operands, and the plan routes the mode (a3t_gemm_plan is host code)."""
import numpy as np
import pytest
import torch

import gemm_ref as G
import gemm_x3_ref as X
from a3t_amd._lib import BF16, BF16X3, F32


def test_split_is_exact_on_16_bit_integers():
    x = torch.arange(-(1 << 16) + 1, 1 << 16, dtype=torch.float32)
    hi, lo = X.split(x)
    assert torch.equal(hi + lo, x)
    assert torch.equal(hi.to(torch.bfloat16).float(), hi) and torch.equal(lo.to(torch.bfloat16).float(), lo)
    inexact = (lo != 0) & (x.abs() <= X.WIDE)
    assert int(inexact.sum()) >= 200          # (the odd integers of 257 .. 511, both signs, at the least)
    assert not lo[x.abs() <= 256].any()


def test_split_of_real_and_non_finite_values():
    x = torch.randn(1 << 16, generator=torch.Generator().manual_seed(0)) * 37.0
    hi, lo = X.split(x)
    # two roundings to 8 significand bits (unit roundoff 2^-8 each): 16 bits are kept
    res = (x.double() - hi.double() - lo.double()).abs() / x.double().abs()
    print(f"split residual / |x|: max {float(res.max()):.3e} (2^-16 = {2.0 ** -16:.3e}), rms {float(res.pow(2).mean().sqrt()):.3e}")
    assert float(res.max()) <= 2.0 ** -16
    big = torch.tensor([float("inf"), -float("inf"), 3.4e38, float("nan"), 1.0])
    hi, lo = X.split(big)
    assert torch.isinf(hi[:3]).all() and torch.isnan(hi[3]) and not lo.any()


@pytest.mark.parametrize("wide", ["A", "B", "AB"])
def test_three_products_on_integers_are_the_full_product_minus_lo_lo(wide):
    """numpy, float64: hi x hi + hi x lo + lo x hi == a b - lo_a lo_b element by element, so with one side bf16-exact the three
    products ARE the full product, and with both wide the missing term is exactly sum lo_a lo_b (not 0 on the wide fill)."""
    gen = torch.Generator().manual_seed(3)
    M, N, K = 33, 17, 64
    A = X.wide_fill(M * K, X.WIDE, gen).view(M, K) if "A" in wide else torch.randint(-3, 4, (M, K), generator=gen).float()
    B = X.wide_fill(N * K, X.WIDE, gen).view(N, K) if "B" in wide else torch.randint(-3, 4, (N, K), generator=gen).float()
    (ah, al), (bh, bl) = X.split(A), X.split(B)
    a, b = A.double().numpy(), B.double().numpy()
    three = (al.double().numpy() @ bh.double().numpy().T + ah.double().numpy() @ bl.double().numpy().T +
             ah.double().numpy() @ bh.double().numpy().T)
    lolo = al.double().numpy() @ bl.double().numpy().T
    assert np.array_equal(three, a @ b.T - lolo)
    assert np.array_equal(three, X.x3_emulate(A, B).numpy())
    assert bool(np.any(lolo)) == (wide == "AB")
    assert float((np.abs(a) @ np.abs(b).T).max()) < G.EXACT


@pytest.mark.parametrize("K", [40, 1152])
def test_bound_holds_for_the_emulation_on_gaussian_operands(K):
    gen = torch.Generator().manual_seed(K)
    A, B = torch.randn(129, K, generator=gen), torch.randn(33, K, generator=gen)
    full = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    err = (X.x3_emulate(A, B) - full).abs()
    # the emulation has no accumulation error: the dropped terms alone, held to the 2^-16 mag of x3_bound
    ratio = float((err / (2.0 ** -16 * mag)).max())
    print(f"K = {K}: dropped terms / (2^-16 mag) = {ratio:.3f}, / x3_bound = {float((err / X.x3_bound(K, mag)).max()):.3f}")
    assert ratio <= 1.0 and bool((err <= X.x3_bound(K, mag)).all())
    assert float(err.max()) > 0


def test_cases_keep_every_accumulated_sum_below_2_24():
    """the exact GPU cases: with the wide fills the sums of |terms| stay below 2^24, so any accumulation order is exact"""
    for wide, K in (("A", 1152), ("B", 1152), ("AB", 64)):
        case = X.x3_case(f"wide {wide}", 5, 33, 33, K, "NT", wide)
        exp, worst = X.x3_expected(case)
        assert worst < G.EXACT, (wide, worst)
        t = case.place("cpu")[0]
        full = case.reference(t).C
        assert torch.equal(exp, full) == (wide != "AB")
        A = t["A"][:33 * K].view(33, K)
        assert int((X.split(A)[1] != 0).sum()) > 0 if "A" in wide else not X.split(A)[1].any()


def _plan(case):
    from a3t_amd import ops
    return case.call(ops.gemm_plan, case.place("cpu")[0])


def test_plan_routes_bf16x3_and_refuses_what_f32_refuses():
    """aligned descriptors of every layout plan gemm_bf16x3_kernel, unaligned ones the fp32 kernel; over the whole fp32 table
    BF16X3 accepts exactly what F32 accepts; colsum, a sign mask and bf16 operands are refused."""
    f32 = lambda name: name is not None and name.startswith("gemm_f32_kernel<")
    for ly, ak, bk in (("NT", "true", "true"), ("NN", "true", "false"), ("TN", "false", "false")):
        x3 = f"gemm_bf16x3_kernel<{ak}, {bk}>"
        assert _plan(G.build("aligned", 1, 136, 72, 40, ly, compute=BF16X3)) == x3
        assert f32(_plan(G.build("12-byte pointer", 1, 136, 72, 40, ly, compute=BF16X3, offs=(3, 0, 0))))
        if ly == "TN":      # no operand is k-contiguous: any K is inside the contract, the row strides are held to 4 elements
            assert _plan(G.build("K 13", 1, 136, 72, 13, ly, compute=BF16X3)) == x3
            assert f32(_plan(G.build("a_cs % 4", 1, 136, 72, 40, ly, compute=BF16X3, a_ld=138)))
        else:
            assert f32(_plan(G.build("K 13", 1, 136, 72, 13, ly, compute=BF16X3, a_ld=16, b_ld=16 if ly == "NT" else 72)))
            assert f32(_plan(G.build("a_rs % 8", 1, 136, 72, 40, ly, compute=BF16X3, a_ld=44)))
    for case in G.f32_fixed_cases():
        as_f32 = _plan(case)
        case.kw["compute"] = BF16X3
        x3 = _plan(case)
        assert (as_f32 is None) == (x3 is None), case
        assert x3.startswith("gemm_bf16x3_kernel<") or x3 == as_f32, (case, as_f32, x3)
    assert _plan(G.build("colsum", 1, 136, 72, 40, "NT", compute=BF16X3, colsum=True)) is None
    assert _plan(G.build("sign mask", 1, 136, 72, 40, "TN", compute=BF16X3, signmask=True)) is None
    assert _plan(G.build("bf16 A", 1, 136, 72, 40, "NT", compute=BF16X3, dt=("bf16", "f32", "f32"))) is None
    assert _plan(G.build("bf16 B", 1, 136, 72, 40, "NT", compute=BF16X3, dt=("f32", "bf16", "f32"))) is None
    assert _plan(G.build("bf16 compute unchanged", 1, 136, 72, 40, "NT", compute=BF16, dt=G.BB)).startswith("gemm_bf16_glds_kernel<")
    assert _plan(G.build("f32 unchanged", 1, 136, 72, 40, "NT", compute=F32)) == "gemm_f32_kernel<true, true, true>"
