"""CPU yardsticks of compute = A3T_BF16X3 (three bf16 MFMA products per fp32 product; csrc/gemm.hip: gemm_bf16x3_kernel).

  * split(x): hi = bf16(x), lo = bf16(x - hi), both round to nearest even (torch's bfloat16 casts), lo = 0 where hi is not
    finite -- the split the kernel's loaders make.
  * wide integer fills: integers up to 511 need nine significand bits, so most of those above 256 are NOT bf16-exact and
    their lo is not 0, while every hi x hi, hi x lo and lo x hi product and every partial sum below 2^24 is still an exact
    fp32 integer.  A kernel that drops, doubles or misreads one of the three terms cannot EQUAL the references below.
  * x3_bound: the error bound of the three-product sum on real operands.
Not a test module: tests/test_gemm_x3_ref_host.py and tests/test_gpu_gemm_x3.py import it."""
import torch

import gemm_ref as G
from a3t_amd._lib import BF16X3

WIDE = 511                      # |a| <= 511: hi has 8 significand bits, lo the ninth


def split(x):
    """(hi, lo) of an fp32 tensor, both fp32 tensors holding bf16 values."""
    x = x.to(torch.float32)
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)         # (x - hi is exact in fp32)
    return hi, torch.where(torch.isfinite(hi), lo, torch.zeros_like(lo))


def x3_emulate(A, B):
    """The three-product sum of A [M][K] x B [N][K]^T in float64 (every product and sum exact there for the sizes used)."""
    (ah, al), (bh, bl) = (tuple(t.double() for t in split(A)), tuple(t.double() for t in split(B)))
    return al @ bh.t() + ah @ bl.t() + ah @ bh.t()


def x3_bound(K, mag):
    """The bound the tests hold the three-product sum to on Gaussian operands: |sum in fp32 - exact| <= (2^-16 + 3 K 2^-23) mag,
    mag = sum_k |a_k||b_k|.  First term: what is dropped -- lo_a lo_b and the two split residuals x - hi - lo.  Each of the
    three is at most 2^-16 |a||b| for a single product (bf16 rounds to 8 significand bits, unit roundoff 2^-8, twice), so a sum
    whose every dropped term had the largest size and the same sign could reach 3 * 2^-16 mag; the dropped terms of real
    operands are signed and mostly far smaller (rms ~ 2^-18 |a||b| each), and their sum over k is held to 2^-16 mag, a third of
    that worst case.  Second term: the products are exact in fp32 and the 3 K accumulation steps are each within 2^-23 of the
    running sum (twice the RNE unit: the MFMA's internal order is covered).  The tests print the measured share of it."""
    return (2.0 ** -16 + 3 * K * 2.0 ** -23) * mag


def wide_max(K, other_max):
    """the largest magnitude <= 511, halved as gemm_ref.build narrows its range, with K * wide * other < 2^24"""
    m = WIDE
    while K * m * other_max >= G.EXACT:
        m //= 2
    assert m > 256, "the range no longer holds values that are not bf16-exact"
    return m


def wide_fill(n, amax, gen):
    """n integers in [-amax, amax], every second one drawn from the magnitudes above 256 (where odd integers are not
    bf16-exact), as fp32"""
    v = torch.randint(-amax, amax + 1, (n,), generator=gen)
    big = torch.randint(257, amax + 1, (n,), generator=gen) * (2 * torch.randint(0, 2, (n,), generator=gen) - 1)
    return torch.where(torch.arange(n) % 2 == 0, big, v).to(torch.float32)


def x3_case(name, seed, M, N, K, layout, wide, **kw):
    """A gemm_ref case in BF16X3 compute with zeroed C and `wide` in ('A', 'B', 'AB'): those operands refilled with wide
    integers (the other keeps gemm_ref's +-3 fill)."""
    case = G.build(name, seed, M, N, K, layout, compute=BF16X3, **kw)
    gen = torch.Generator().manual_seed(seed + 77)
    both = len(wide) == 2
    for nm in wide:
        buf, off = case.bufs[nm]
        case.bufs[nm] = (wide_fill(buf.numel(), WIDE if both else wide_max(K, 3), gen), off)
    case.bufs["C"] = (torch.zeros_like(case.bufs["C"][0]), case.bufs["C"][1])
    return case


def x3_expected(case):
    """float64 image of C (from the descriptor's pointer on) after a plain-store case ran in BF16X3 on integer operands: the
    full product minus sum_k lo_a lo_b (0 where one side is bf16-exact); and the largest sum_k of the |terms| an accumulator
    sees (the caller checks it against 2^24)."""
    assert not any(k in case.kw for k in ("alpha", "act", "acc", "splitk", "drop", "second")) and "bias" not in case.bufs
    t, base = case.place("cpu")
    assert not base["C"].any()
    ref = case.reference(t)
    offs = {nm: case.bufs[nm][1] for nm in ("A", "B")}
    (ah, al), (bh, bl) = ([x[offs[nm]:] for x in split(base[nm])] for nm in ("A", "B"))     # (tail views, like t: indices may be negative)
    lolo = G.reference(case.kw, al, bl, t["C"])
    mags = [G.reference(case.kw, x.abs(), y.abs(), t["C"]).C for x, y in ((al, bh), (ah, bl), (ah, bh))]
    return ref.C - lolo.C, float(sum(mags).max())
