"""compute = A3T_BF16X3 on the GPU (csrc/gemm.hip: gemm_bf16x3_kernel, three bf16 MFMA products per fp32 product; yardsticks in
tests/gemm_x3_ref.py, checked on the host by tests/test_gemm_x3_ref_host.py).

  1. the descriptor space: every table the fp32 kernel is held to (tests/gemm_ref.py), built with compute = BF16X3, EQUALS the
     interpreter -- the +-3 fills are bf16-exact, so lo = 0 and this holds indexing, taps, masks, split K and the epilogues;
  2. routes: the new kernel on aligned descriptors, the fp32 kernel on unaligned ones, A3T_EINVAL for what fp32 refuses;
  3. the lo path: integer operands that are NOT bf16-exact, equality again (one side wide: the full product; both wide: the
     full product minus sum lo_a lo_b);
  4. Gaussian operands against float64 within x3_bound."""
import collections

import pytest
import torch

import gemm_ref as G
import gemm_x3_ref as X
from a3t_amd._lib import ACC_ADD, ACC_ATOMIC, ACC_SOLE, ACT_RELU, BF16X3

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = "gemm_bf16x3_kernel<"


def _env():
    from a3t_amd import _lib, ops
    return ops, _lib.load()


def _launch(case, ops, lib):
    """runs the case; planned name == launched name; returns (name, C's whole buffer on the host, the operands untouched)"""
    t, base = case.place(DEV)
    planned = case.call(ops.gemm_plan, t)
    assert planned is not None, case
    case.call(ops.gemm, t)
    torch.cuda.synchronize()
    launched = lib.a3t_gemm_last_kernel().decode()
    assert planned == launched, (case, planned, launched)
    for nm in ("A", "B", "bias", "R", "S"):
        if nm in base:
            assert torch.equal(base[nm].cpu().view(torch.uint8), case.bufs[nm][0].view(torch.uint8)), (case, nm)     # (bytes: a NaN is itself)
    return launched, base["C"].cpu()


def _equal(case, launched, got, exp_tail):
    """C's whole buffer (the sentinels in front of, between and behind the tiles included) against the expected image"""
    buf, off = case.bufs["C"]
    exp = buf.clone()
    exp[off:] = exp_tail.to(buf.dtype)
    if not torch.equal(got, exp):
        bad = (got.double() != exp.double()).nonzero().flatten()
        d = (got.double() - exp.double())[bad]
        raise AssertionError(f"{case}\n{launched}: {bad.numel()} of {exp.numel()} elements differ, first at flat {bad[:8].tolist()}: "
                             f"got {got[bad[:8]].tolist()} expected {exp[bad[:8]].tolist()}; |diff| max {float(d.abs().max())}")


def _keep(case, ops, t_len):
    ones = torch.ones(t_len, device=DEV)
    y = torch.empty_like(ones)
    ops.dropout(ones, y, case.kw["drop"][0], case.kw["drop"][1])
    return y.cpu()


# ---- 1. the descriptor space -------------------------------------------------------------------------------------------------
GROUPS = {"NT": lambda: G.f32_shape_cases("NT"), "NN": lambda: G.f32_shape_cases("NN"), "TN": lambda: G.f32_shape_cases("TN"),
          "strides": G.f32_stride_cases, "conv": G.f32_conv_cases, "accumulate": G.f32_acc_cases, "epilogue": G.f32_epilogue_cases}


@pytest.mark.parametrize("group", list(GROUPS))
def test_f32_tables_in_bf16x3_equal_the_interpreter(group):
    ops, lib = _env()
    seen = collections.Counter()
    for case in GROUPS[group]():
        case.kw["compute"] = BF16X3
        launched, got = _launch(case, ops, lib)
        seen[launched.split("<")[0]] += 1
        host = case.place("cpu")[0]
        keep = _keep(case, ops, host["C"].numel()) if "drop" in case.kw else None
        _equal(case, launched, got, case.reference(host, keep=keep).C)
    print("bf16x3", group, dict(seen))
    assert set(seen) <= {"gemm_bf16x3_kernel", "gemm_f32_kernel"}, seen
    # (no descriptor of the accumulate table is inside the new kernel's alignment contract: the aligned twins are below)
    assert seen["gemm_bf16x3_kernel"] > 0 or group == "accumulate", seen


def _aligned_cases():
    """split K, the accumulate modes, token shifts and the epilogue terms of the fp32 tables on shapes inside the new kernel's
    contract (k-contiguous strides and extents multiples of 8, row-contiguous ones multiples of 4): K = 136 is 5 K-tiles of 32
    with a tail of 8, so 5 splits take one tile each and 2 splits 3 + 2; K = 104 is 4 tiles, so the last of 5 splits is EMPTY"""
    c, s = [], 7000
    ld = {"NT": {}, "NN": dict(b_ld=40), "TN": dict(a_ld=132, b_ld=40)}
    for ly in ("NT", "NN", "TN"):
        for acc in (ACC_ADD, ACC_ATOMIC, ACC_SOLE):
            for splitk in ((1,) if acc == ACC_ADD else (1, 2, 5)):
                s += 1
                K = (136, 104, 96)[s % 3] if splitk == 5 else (40, 136)[s % 2]
                c.append(G.build(f"{ly} acc {acc} splitk {splitk} K{K}", s, 129, 40, K, ly, compute=BF16X3, acc=acc, splitk=splitk,
                                 alpha=G.POW2[s % 4], bias=s % 2 == 0, R=s % 3 == 0, S=(None, "f32", "bf16")[s % 3], **ld[ly]))
        for S in ("f32", "bf16"):
            s += 1
            c.append(G.build(f"{ly} bias relu S {S} alpha R", s, 129, 136, 24, ly, compute=BF16X3, bias=True, act=ACT_RELU, S=S,
                             alpha=G.POW2[1 + s % 3], R=True, c_ld=140, offs=(0, 0, 3), **dict(ld[ly], **({"b_ld": 136} if ly != "NT" else {}))))
        s += 1
        c.append(G.build(f"{ly} bf16 C add", s, 129, 40, 40, ly, compute=BF16X3, dt=("f32", "f32", "bf16"), acc=ACC_ADD, bias=True, alpha=0.5,
                         **ld[ly]))
    for kshift in (-2, 0, 3, 50, -50):
        s += 1
        c.append(G.build(f"kshift {kshift}", s, 37, 40, 150, "TN", compute=BF16X3, a_ld=40, Tseq=50, kshift=kshift, acc=ACC_ATOMIC, splitk=2,
                         alpha=G.POW2[s % 4]))
    c.append(G.build("dropout", s + 1, 129, 40, 24, "NT", compute=BF16X3, drop=(0.5, 4321), bias=True, alpha=0.5))
    c.append(G.build("batch 6/3", s + 2, 37, 136, 16, "NN", compute=BF16X3, batch=6, batch_inner=3, a_bs="swap", b_bs="dense", c_bs="swap", bs_gap=8))
    c.append(G.build("shared B (0, dk)", s + 3, 37, 16, 40, "NN", compute=BF16X3, b_ld=48, batch=6, batch_inner=3, b_bs=(0, 16)))
    c.append(G.build("overlap hop 8", s + 4, 200, 37, 16, "NT", compute=BF16X3, a_ld=8))
    c.append(G.build("conv data gradient", s + 5, 150, 8, 3 * 16, "NN", compute=BF16X3, taps=3, pad=1, dil=2, Tseq=50))
    c.append(G.build("conv k5 dilated epilogue", s + 6, 21, 37, 5 * 8, "NT", compute=BF16X3, taps=5, pad=4, dil=2, Tseq=7, bias=True,
                     act=ACT_RELU, S="bf16", alpha=0.5, R=True))
    return c


def test_aligned_accumulate_and_epilogue_cases_run_on_the_new_kernel_and_equal_the_interpreter():
    ops, lib = _env()
    seen = collections.Counter()
    for case in _aligned_cases():
        launched, got = _launch(case, ops, lib)
        assert launched.startswith(X3), (case, launched)
        seen[launched] += 1
        host = case.place("cpu")[0]
        keep = _keep(case, ops, host["C"].numel()) if "drop" in case.kw else None
        _equal(case, launched, got, case.reference(host, keep=keep).C)
    print("bf16x3 aligned", dict(seen))
    assert len(seen) == 3, seen


def test_the_tables_cover_all_three_instantiations():
    ops, _ = _env()
    names = set()
    for case in G.f32_fixed_cases():
        case.kw["compute"] = BF16X3
        names.add(case.call(ops.gemm_plan, case.place("cpu")[0]))
    assert {X3 + "true, true>", X3 + "true, false>", X3 + "false, false>"} <= names, names


# ---- 2. routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ly,name", [("NT", X3 + "true, true>"), ("NN", X3 + "true, false>"), ("TN", X3 + "false, false>")])
def test_routes(ly, name):
    """aligned: the new kernel; K = 13, a 12-byte-offset pointer, a leading stride of A outside the granule: the fp32 kernel
    (for TN no operand is k-contiguous, so K = 13 stays inside the contract and runs on the new kernel).  All of them run and
    equal the interpreter."""
    ops, lib = _env()
    b = lambda nm, K=40, **k: G.build(f"{ly} {nm}", 11, 136, 72, K, ly, compute=BF16X3, **k)
    k13 = b("K 13", 13) if ly == "TN" else b("K 13", 13, a_ld=16, b_ld=16 if ly == "NT" else 72)
    table = [(b("aligned"), True), (k13, ly == "TN"), (b("12-byte pointer", offs=(3, 0, 0)), False),
             (b("A stride", a_ld=138 if ly == "TN" else 44), False)]
    for case, x3 in table:
        launched, got = _launch(case, ops, lib)
        assert launched == name if x3 else launched.startswith("gemm_f32_kernel<"), (case, launched)
        _equal(case, launched, got, case.reference(case.place("cpu")[0]).C)


def test_refused_descriptors_stay_refused():
    """what A3T_F32 refuses -- column sums, a sign mask on A, bf16 storage of A or of B -- A3T_BF16X3 refuses with A3T_EINVAL and
    writes nothing"""
    from a3t_amd._lib import A3TLibraryError
    ops, lib = _env()
    bad = [G.build("colsum", 1, 136, 72, 40, "NT", compute=BF16X3, colsum=True),
           G.build("sign mask", 1, 136, 72, 40, "TN", compute=BF16X3, signmask=True),
           G.build("bf16 A", 1, 136, 72, 40, "NT", compute=BF16X3, dt=("bf16", "f32", "f32")),
           G.build("bf16 B", 1, 136, 72, 40, "NN", compute=BF16X3, dt=("f32", "bf16", "f32"))]
    for case in bad:
        t, base = case.place(DEV)
        assert case.call(ops.gemm_plan, t) is None, case
        with pytest.raises(A3TLibraryError) as e:
            case.call(ops.gemm, t)
        assert "rc=-22" in str(e.value), e.value         # A3T_EINVAL
        torch.cuda.synchronize()
        assert torch.equal(base["C"].cpu(), case.bufs["C"][0])


# ---- 3. the lo path, exactly --------------------------------------------------------------------------------------------------
DIMS = (1, 33, 128, 129)


def _lo_cases(wide, Ks):
    """every M and every N of DIMS with every K, walking N against M; plus a conv (3 taps, the utterance boundary Tseq = 50 inside
    the 128-row tile) and a batched case with batch_inner = 2"""
    out = []
    for ki, K in enumerate(Ks):
        for mi, M in enumerate(DIMS):
            N = DIMS[(mi + ki + 1) % 4]
            ly = ("NT", "NN", "TN")[(mi + ki) % 3]
            # the row-contiguous operands keep their 4-element granule: strides rounded up to a multiple of 4
            ld = {}
            if ly == "TN":
                ld = dict(a_ld=(M + 3) // 4 * 4, b_ld=(N + 3) // 4 * 4)
            elif ly == "NN":
                ld = dict(b_ld=(N + 3) // 4 * 4)
            out.append(X.x3_case(f"{wide} wide {ly} {M}x{N}x{K}", 100 * ki + mi, M, N, K, ly, wide, **ld))
    Kc = 24 if len(wide) == 1 else 16
    out.append(X.x3_case(f"{wide} wide conv", 900, 150, 33, 3 * Kc, "NT", wide, taps=3, pad=1, dil=1, Tseq=50))
    out.append(X.x3_case(f"{wide} wide batched", 901, 33, 129, Ks[-1] if len(wide) == 2 else 40, "NT", wide, batch=4, batch_inner=2,
                         a_bs="swap", c_bs="swap", bs_gap=8))
    return out


@pytest.mark.parametrize("wide", ["A", "B", "AB"])
def test_wide_integer_operands_exactly(wide):
    """(a) A wide (|a| <= 511, not bf16-exact), B in +-3; (b) the roles swapped: one side is bf16-exact, the three products are the
    full product and C EQUALS the integer reference.  (c) both wide at K = 64: C EQUALS reference - sum_k lo_a lo_b.  A term
    that is missing, doubled or read from the wrong image breaks one of the three."""
    ops, lib = _env()
    n_lo = 0
    for case in _lo_cases(wide, (64,) if wide == "AB" else (8, 32, 40, 72, 1152)):
        exp, worst = X.x3_expected(case)
        assert worst < G.EXACT, (case, worst)
        launched, got = _launch(case, ops, lib)
        assert launched.startswith(X3), (case, launched)
        _equal(case, launched, got, exp)
        if wide == "AB":
            n_lo += int((exp != case.reference(case.place("cpu")[0]).C).sum())
    assert (n_lo > 0) == (wide == "AB")        # (c) is not (a): the lo x lo term it lacks is there to be missed


def test_non_finite_operands_stay_in_their_rows():
    """an infinity, a NaN and a finite value that rounds to infinity in bf16, each in one row of A: those rows come out non-finite
    (not always fp32's infinity: inf x lo_b is NaN where lo_b = 0), every other row stays exact"""
    ops, lib = _env()
    case = G.build("non-finite", 5, 33, 40, 40, "NT", compute=BF16X3)
    A, off = case.bufs["A"]
    A[off + 3 * 40 + 7] = float("inf")
    A[off + 5 * 40 + 39] = float("nan")
    A[off + 9 * 40 + 1] = 3.4e38
    launched, got = _launch(case, ops, lib)
    assert launched.startswith(X3)
    C = got[case.bufs["C"][1]:][:33 * 40].view(33, 40)
    assert not torch.isfinite(C[[3, 5, 9]]).any() and bool(torch.isnan(C[5]).all())
    rest = [m for m in range(33) if m not in (3, 5, 9)]
    host = case.place("cpu")[0]
    host["A"][3 * 40 + 7] = host["A"][5 * 40 + 39] = host["A"][9 * 40 + 1] = 0.0
    assert torch.equal(C[rest].double(), case.reference(host).C[:33 * 40].view(33, 40)[rest])


# ---- 4. real operands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [40, 1152])
@pytest.mark.parametrize("ly", ["NT", "NN", "TN"])
def test_gaussian_operands_within_the_bound(ly, K):
    ops, lib = _env()
    case = G.build(f"gauss {ly} K{K}", 40 + K, 129, 136, K, ly, compute=BF16X3, values="gauss", a_ld=132 if ly == "TN" else None)
    case.bufs["C"] = (torch.zeros_like(case.bufs["C"][0]), case.bufs["C"][1])
    launched, got = _launch(case, ops, lib)
    assert launched.startswith(X3), launched
    ref = case.reference(case.place("cpu")[0])
    err = (got.double()[case.bufs["C"][1]:] - ref.C).abs()
    bound = X.x3_bound(K, ref.mag)
    touched = ref.mag > 0
    ratio = float((err[touched] / bound[touched]).max())
    print(f"{launched} K = {K}: worst |err| / bound = {ratio:.4f} (|err| max {float(err.max()):.3e})")
    assert ratio <= 1.0, (case, ratio)
    assert not err[~touched].any()
