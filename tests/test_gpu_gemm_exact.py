"""Exact integer-operand sweep of the a3t_gemm descriptor space on the GPU (tests/gemm_ref.py holds the interpreter and the case
tables; tests/test_gemm_ref_host.py checks both on the host).  With small integer operands and power-of-two scales every product
and partial sum is exact in fp32 and in bf16-in / fp32-accumulate, whatever the accumulation order: C, the rest of C's buffer and
the fused column sums must EQUAL the float64 reference.  Two fp32 tests on Gaussian operands hold the rounding behaviour."""
import collections

import pytest
import torch

import gemm_ref as G
from a3t_amd._lib import ACC_ADD, ACC_ATOMIC, ACC_SOLE, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, BF16, F32

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _env():
    from a3t_amd import _lib, ops
    return ops, _lib.load()


def _where(case, bad):
    """the first mismatching elements as (batch element, row, column) of the descriptor, or the flat offset outside C's tiles"""
    kw, out = case.kw, []
    bi, c_bs = max(1, kw.get("batch_inner", 1)), kw.get("c_bs", (0, 0))
    for i in bad[:12].tolist():
        i -= case.bufs["C"][1]
        hit = None
        for z in range(max(1, kw.get("batch", 1))):
            r = i - (z // bi) * c_bs[0] - (z % bi) * c_bs[1]
            if r >= 0 and r // kw["c_rs"] < kw["M"] and r % kw["c_rs"] < kw["N"]:
                hit = (z, r // kw["c_rs"], r % kw["c_rs"])
        out.append(hit if hit else f"flat {i}")
    return out


def _run(case, ops, lib, seen=None):
    """runs one case: planned name == launched name, C's whole buffer (sentinels around and between the tiles included), the
    column sums and the untouched operands against the interpreter; returns the launched kernel's name"""
    t, base = case.place(DEV)
    keep = None
    if "drop" in case.kw:       # the keep mask of the stand-alone kernel: same key, same linear index (test_dropout_statistics_replay_and_gemm_epilogue)
        ones = torch.ones(t["C"].numel(), device=DEV)
        y = torch.empty_like(ones)
        ops.dropout(ones, y, case.kw["drop"][0], case.kw["drop"][1])
        keep = y.cpu()
    planned = case.call(ops.gemm_plan, t)
    assert planned is not None, case
    case.call(ops.gemm, t)
    torch.cuda.synchronize()
    launched = lib.a3t_gemm_last_kernel().decode()
    assert planned == launched, (case, planned, launched)
    if seen is not None:
        seen[launched] += 1
    host, _ = case.place("cpu")
    ref = case.reference(host, keep=keep)
    buf, off = case.bufs["C"]
    exp = buf.clone()
    exp[off:] = ref.C.to(buf.dtype)
    got = base["C"].cpu()
    if not torch.equal(got, exp):
        bad = (got.double() != exp.double()).nonzero().flatten()
        d = (got.double() - exp.double())[bad]
        raise AssertionError(f"{case}\n{launched}: {bad.numel()} of {exp.numel()} elements differ, first at (z, m, n) {_where(case, bad)}: "
                             f"got {got[bad[:12]].tolist()} expected {exp[bad[:12]].tolist()}; |diff| max {float(d.abs().max())}")
    for nm in ("A", "B", "bias", "R", "S", "A2", "B2"):
        if nm in base:
            assert torch.equal(base[nm].cpu(), case.bufs[nm][0]), (case, nm)
    if ref.colsum is not None:
        assert torch.equal(G.folded(case, base["colsum"]), ref.colsum), (case, launched, G.folded(case, base["colsum"]), ref.colsum)
        if ref.colsum2 is not None:
            assert torch.equal(G.folded(case, base["colsum2"]), ref.colsum2), (case, launched)
    return launched


F32_GROUPS = {"NT": lambda: G.f32_shape_cases("NT"), "NN": lambda: G.f32_shape_cases("NN"), "TN": lambda: G.f32_shape_cases("TN"),
              "strides": G.f32_stride_cases, "conv": G.f32_conv_cases, "accumulate": G.f32_acc_cases, "epilogue": G.f32_epilogue_cases}


@pytest.mark.parametrize("group", list(F32_GROUPS))
def test_f32_fixed_table_exact(group):
    ops, lib = _env()
    seen = collections.Counter()
    for case in F32_GROUPS[group]():
        _run(case, ops, lib, seen)
    assert all(k.startswith("gemm_f32_kernel<") for k in seen), seen
    print("fp32", group, dict(seen))


def test_f32_random_descriptors_exact_and_all_six_instantiations():
    ops, lib = _env()
    seen = collections.Counter()
    for case in G.draws(101, 40, F32):
        if case.call(ops.gemm_plan, case.place()[0]) is None:      # (at most 4 of 40: test_gemm_ref_host.py)
            with pytest.raises(Exception):
                case.call(ops.gemm, case.place(DEV)[0])
            continue
        _run(case, ops, lib, seen)
    want = {f"gemm_f32_kernel<{a}, {b}, {v}>" for a, b in (("true", "true"), ("true", "false"), ("false", "false")) for v in ("true", "false")}
    assert set(seen) == want, seen
    print("fp32 draws", dict(seen))


# one shape per instantiation, K <= 128 (beyond ~500 the bound's margin over bf16-rounded operands is gone)
PRECISION = [("NT", 200, 129, 96, {}), ("NT", 129, 200, 33, {}), ("NN", 130, 136, 128, {}), ("NN", 127, 37, 17, {}),
             ("TN", 136, 200, 128, dict(a_ld=136)), ("TN", 37, 129, 97, {})]


@pytest.mark.parametrize("act", [ACT_NONE, ACT_TANH, ACT_SWISH])
def test_f32_precision_bound(act):
    """|got - ref64| <= (K + 8) 2^-23 mag with mag = |alpha| (sum |a||b| + |bias|) + |R| + |C_old|: the accumulation bound gamma_K,
    doubled for unfused products and the epilogue's three roundings.  tanh / swish add the project's tolerance for those activations
    (atol 2e-5, rtol 1e-4) to 1.1 x the bound."""
    ops, lib = _env()
    names = set()
    for i, (ly, M, N, K, extra) in enumerate(PRECISION):
        case = G.build(f"gauss {ly} {M}x{N}x{K}", 900 + i, M, N, K, ly, values="gauss", bias=True, R=True, alpha=0.7, acc=ACC_ADD, **extra)
        if act != ACT_NONE:
            case.kw["act"] = act
        t, base = case.place(DEV)
        case.call(ops.gemm, t)
        torch.cuda.synchronize()
        name = lib.a3t_gemm_last_kernel().decode()
        names.add(name)
        ref = case.reference(case.place("cpu")[0])
        off = case.bufs["C"][1]
        err = (base["C"].cpu().double()[off:] - ref.C).abs()
        bound = (K + 8) * 2.0 ** -23 * ref.mag
        touched = ref.mag > 0
        if act != ACT_NONE:
            bound = 1.1 * bound + 2e-5 + 1e-4 * ref.C.abs()
        ratio = float((err[touched] / bound[touched]).max())
        print(f"precision act {act} {name}: max error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (case, name, ratio)
        assert torch.equal(err[~touched], torch.zeros_like(err[~touched]))
    assert len(names) == 6, names


@pytest.mark.parametrize("ly,K,lds", [("NT", 32, {}), ("NT", 33, {}), ("NN", 32, dict(b_ld=204)), ("NN", 33, dict(b_ld=203)),
                                      ("TN", 32, dict(a_ld=204, b_ld=204)), ("TN", 33, dict(a_ld=203, b_ld=203))])
def test_f32_tile_position_invariance(ly, K, lds):
    """Copies of one A row at m = 5, 127, 128, 133, M - 1 give bit-identical C rows, copies of one B row across N bit-identical
    columns: every element's sum visits k in the same order, so a difference is a loader or edge-tile fault."""
    ops, lib = _env()
    M = N = 203
    case = G.build(f"positions {ly}", 77, M, N, K, ly, values="gauss", bias=False, **lds)
    kw = case.kw
    pos = (5, 127, 128, 133, M - 1)
    A, B = case.bufs["A"][0], case.bufs["B"][0]
    k = torch.arange(K)
    for p in pos[1:]:
        A[p * kw["a_rs"] + k * kw["a_cs"]] = A[pos[0] * kw["a_rs"] + k * kw["a_cs"]]
        B[p * kw["b_rs"] + k * kw["b_cs"]] = B[pos[0] * kw["b_rs"] + k * kw["b_cs"]]
    t, base = case.place(DEV)
    case.call(ops.gemm, t)
    torch.cuda.synchronize()
    assert lib.a3t_gemm_last_kernel().decode() == f"gemm_f32_kernel<{'false' if ly == 'TN' else 'true'}, {'true' if ly == 'NT' else 'false'}, " \
                                                  f"{'true' if K == 32 else 'false'}>"
    C = base["C"].cpu()[:M * N].view(M, N)
    assert float(C.abs().max()) > 0
    for p in pos[1:]:
        assert torch.equal(C[p], C[pos[0]]), (ly, K, p, (C[p] != C[pos[0]]).nonzero().flatten()[:8])
        assert torch.equal(C[:, p], C[:, pos[0]]), (ly, K, p, (C[:, p] != C[:, pos[0]]).nonzero().flatten()[:8])


# ---- bf16 compute ----------------------------------------------------------------------------------------------------------------
ROUTES = ["glds", "8p", "8p_tn", "8p_tn3", "pn", "tt", "legacy"]


@pytest.mark.parametrize("route", ROUTES)
def test_bf16_route_exact(route):
    ops, lib = _env()
    mode, cases, prefix = G.bf16_route_table()[ROUTES.index(route)]
    seen = collections.Counter()
    old = G.set_modes(lib, G.MODES[mode])
    try:
        for case in cases:
            _run(case, ops, lib, seen)
    finally:
        G.set_modes(lib, old)
    assert all(k.startswith(prefix + "<") for k in seen), seen
    print("bf16", route, dict(seen))
    if route == "glds":
        assert len(seen) >= 8, seen
    elif route == "legacy":
        assert len({tuple(k.split(",")[:2]) for k in seen}) >= 3, seen
    elif route == "tt":
        assert any(k.endswith("true>") for k in seen) and any(k.endswith("false>") for k in seen), seen
    else:
        assert {prefix + "<false>", prefix + "<true>"} == set(seen), seen


@pytest.mark.parametrize("mode", list(G.MODES))
def test_bf16_random_descriptors_exact(mode):
    ops, lib = _env()
    seen = collections.Counter()
    old = G.set_modes(lib, G.MODES[mode])
    try:
        for case in G.draws(202, 40, BF16):
            if case.call(ops.gemm_plan, case.place()[0]) is None:      # (at most 4 of 40: test_gemm_ref_host.py)
                with pytest.raises(Exception):
                    case.call(ops.gemm, case.place(DEV)[0])
                continue
            _run(case, ops, lib, seen)
    finally:
        G.set_modes(lib, old)
    print("bf16 draws", mode, dict(seen))


def test_rejected_descriptors_raise():
    """what a3t_gemm_plan rejects, a3t_gemm refuses: a non-linear activation under split K (each split would apply it to its partial
    sum), atomics on bf16 C, column sums in fp32 compute, [k][m] x [n][k]"""
    from a3t_amd._lib import A3TLibraryError
    ops, lib = _env()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    bad = []
    for compute, dt in ((F32, torch.float32), (BF16, torch.bfloat16)):
        A, B = z(128, 256, dt=dt), z(128, 256, dt=dt)
        for act in (ACT_RELU, ACT_TANH, ACT_SWISH):
            for acc in (ACC_ATOMIC, ACC_SOLE):
                bad.append(((A, B, z(128, 128), 128, 128, 256, 256, 1, 256, 1, 128), dict(acc=acc, splitk=2, act=act, compute=compute)))
                bad.append(((A, B, z(128, 128), 128, 128, 256, 1, 128, 1, 128, 128), dict(acc=acc, splitk=4, act=act, compute=compute)))
        bad.append(((A, B, z(128, 128, dt=torch.bfloat16), 128, 128, 256, 256, 1, 256, 1, 128), dict(acc=ACC_ATOMIC, compute=compute)))
        bad.append(((A, B, z(128, 128), 128, 128, 256, 1, 128, 256, 1, 128), dict(compute=compute)))
        bad.append(((A, B, z(128, 128), 128, 128, 256, 256, 1, 256, 1, 128), dict(splitk=2, compute=compute)))
    bad.append(((z(128, 256), z(128, 256), z(128, 128), 128, 128, 256, 256, 1, 256, 1, 128), dict(colsum=z(128), compute=F32)))
    for args, kw in bad:
        C = args[2]
        C.fill_(5.0)
        assert ops.gemm_plan(*args, **kw) is None, kw
        with pytest.raises(A3TLibraryError):
            ops.gemm(*args, **kw)
        torch.cuda.synchronize()
        assert bool((C == 5.0).all())
    # the linear forms stay legal
    A, B, C = z(128, 256), z(128, 256), z(128, 128)
    ops.gemm(A, B, C, 128, 128, 256, 256, 1, 256, 1, 128, acc=ACC_ATOMIC, splitk=2, compute=F32)
    ops.gemm(A, B, C, 128, 128, 256, 256, 1, 256, 1, 128, act=ACT_RELU, compute=F32)
    torch.cuda.synchronize()
