"""Host checks of the GEMM descriptor interpreter (tests/gemm_ref.py) and of the case tables the GPU sweeps run: the interpreter
against torch in float64 on integer inputs (equality), the routes a3t_gemm_plan gives the tables, and two refusals.  No GPU."""
import collections
import ctypes

import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
from a3t_amd import _lib, ops
from a3t_amd._lib import ACC_ADD, ACC_ATOMIC, ACC_SOLE, ACC_STORE, ACT_RELU, ACT_TANH, BF16, F32


def _ints(*shape, seed=0, hi=3, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=g).to(dtype)


def _kw(M, N, K, a_rs, a_cs, b_rs, b_cs, c_rs, **k):
    return dict(M=M, N=N, K=K, a_rs=a_rs, a_cs=a_cs, b_rs=b_rs, b_cs=b_cs, c_rs=c_rs, **k)


def test_reference_linear_three_layouts_and_epilogue():
    M, N, K = 37, 29, 17
    x, W, b, R, S, C0 = _ints(M, K, seed=1), _ints(N, K, seed=2), _ints(N, seed=3, hi=8), _ints(M, N, seed=4, hi=8), _ints(M, N, seed=5), \
        _ints(M, N, seed=6, hi=8)
    lin = F.linear(x, W, b)
    z = torch.zeros(M, N, dtype=torch.float64)
    r = G.reference(_kw(M, N, K, K, 1, K, 1, N), x, W, z, bias=b)
    assert torch.equal(r.C, lin)
    assert torch.equal(G.reference(_kw(M, N, K, K, 1, 1, N, N), x, W.t().contiguous(), z, bias=b).C, lin)             # B [k][n]
    assert torch.equal(G.reference(_kw(M, N, K, 1, M, 1, N, N), x.t().contiguous(), W.t().contiguous(), z, bias=b).C, lin)   # A [k][m]
    # mag = sum |a||b| + |bias|
    assert torch.equal(r.mag, x.abs() @ W.abs().t() + b.abs())
    # alpha * mask_S(relu(. + bias)) + R, accumulated onto C
    exp = C0 + (-2.0 * torch.where(S > 0, torch.relu(lin), z) + R)
    for acc in (ACC_ADD, ACC_ATOMIC, ACC_SOLE):
        got = G.reference(_kw(M, N, K, K, 1, K, 1, N, alpha=-2.0, act=ACT_RELU, acc=acc), x, W, C0, bias=b, R=R, S=S)
        assert torch.equal(got.C, exp)
    # split K changes nothing (linear epilogue); a non-linear one is refused, as is a plain store
    got = G.reference(_kw(M, N, K, K, 1, K, 1, N, alpha=0.5, acc=ACC_SOLE, splitk=3), x, W, C0, bias=b, R=R, S=S)
    assert torch.equal(got.C, C0 + 0.5 * torch.where(S > 0, lin, z) + R)
    for bad in (dict(act=ACT_RELU, acc=ACC_ATOMIC), dict(acc=ACC_STORE), dict(acc=ACC_ADD)):
        with pytest.raises(ValueError):
            G.reference(_kw(M, N, K, K, 1, K, 1, N, splitk=2, **bad), x, W, C0)
    # dropout: keep mask by linear index in C, p = 0.5
    keep = (_ints(M, N, seed=7, hi=1) > 0).double()
    got = G.reference(_kw(M, N, K, K, 1, K, 1, N, drop=(0.5, 1)), x, W, z, bias=b, keep=keep)
    assert torch.equal(got.C, keep * lin * 2.0)
    # tanh is applied before the mask and alpha
    got = G.reference(_kw(M, N, K, K, 1, K, 1, N, act=ACT_TANH, alpha=0.5), x, W, z, bias=b)
    assert torch.equal(got.C, 0.5 * torch.tanh(lin))
    # bf16 C: one rounding of the fp32 sum; ADD is formed in fp32 and rounded once
    big = 40.0 * lin + 0.0
    C16 = _ints(M, N, seed=8, hi=300).to(torch.bfloat16)
    got = G.reference(_kw(M, N, K, K, 1, K, 1, N, alpha=40.0), x, W, C16, bias=b)
    assert torch.equal(got.C, big.to(torch.bfloat16).double())
    got = G.reference(_kw(M, N, K, K, 1, K, 1, N, alpha=40.0, acc=ACC_ADD), x, W, C16, bias=b)
    assert torch.equal(got.C, (big + C16.double()).to(torch.bfloat16).double())
    assert not torch.equal(got.C, (big.to(torch.bfloat16).double() + C16.double()).to(torch.bfloat16).double())   # (two roundings differ)


def test_reference_strided_slice_of_c_leaves_the_rest():
    M, N, K = 9, 5, 4
    x, W = _ints(M, K, seed=1), _ints(N, K, seed=2)
    wide = torch.full((M, 12), 77.0, dtype=torch.float64)
    got = G.reference(_kw(M, N, K, K, 1, K, 1, 12), x, W, wide.view(-1)[3:]).C
    exp = wide.clone()
    exp[:, 3:3 + N] = x @ W.t()
    assert torch.equal(got, exp.view(-1)[3:])
    with pytest.raises(AssertionError):       # reads beyond A
        G.reference(_kw(M + 1, N, K, K, 1, K, 1, 12), x, W, torch.zeros(200, dtype=torch.float64))


@pytest.mark.parametrize("taps,dil,pad", [(3, 1, 1), (3, 2, 1), (3, 1, 0), (3, 2, 2), (5, 1, 2), (5, 2, 1), (5, 2, 3), (5, 1, 4), (3, 4, 1)])
@pytest.mark.parametrize("T", [1, 3, 7, 20])
def test_reference_conv_forward_data_gradient_weight_gradient(taps, dil, pad, T):
    Bn, Cin, Cout = 3, 4, 5
    M = Bn * T
    x = _ints(Bn, T, Cin, seed=1).requires_grad_(True)
    Wt = _ints(Cout, Cin, taps, seed=2).requires_grad_(True)        # torch layout; the project keeps W[n][tap][c]
    bias = _ints(Cout, seed=3, hi=8)
    dy = _ints(Bn, T, Cout, seed=4)
    # out[t] = sum_tap W[tap] x[t + (tap - pad) dil], zeros outside the utterance: asymmetric padding for pad != (taps - 1) / 2
    xp = F.pad(x.transpose(1, 2), (pad * dil, (taps - 1 - pad) * dil))
    y = F.conv1d(xp, Wt, bias, dilation=dil).transpose(1, 2)
    assert y.shape == (Bn, T, Cout)
    y.backward(dy)
    Wk = Wt.detach().permute(0, 2, 1).contiguous()
    xf, dyf = x.detach().reshape(M, Cin), dy.reshape(M, Cout)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    got = G.reference(_kw(M, Cout, taps * Cin, Cin, 1, taps * Cin, 1, Cout, b_ts=Cin, taps=taps, pad=pad, dil=dil, Tseq=T), xf, Wk, z(M, Cout),
                      bias=bias)
    assert torch.equal(got.C, y.detach().reshape(M, Cout))
    # data gradient: the same loader on dy, taps back to front (ops.conv_bwd_data)
    Wv = Wk.view(-1)[(taps - 1) * Cin:]
    got = G.reference(_kw(M, Cin, taps * Cout, Cout, 1, 1, taps * Cin, Cin, b_ts=-Cin, taps=taps, pad=taps - 1 - pad, dil=dil, Tseq=T), dyf, Wv,
                      z(M, Cin))
    assert torch.equal(got.C, x.grad.reshape(M, Cin))
    # weight gradient, one token-shifted reduction per tap (ops.conv_bwd_weight) ...
    dWk = z(Cout, taps, Cin)
    for tap in range(taps):
        flat = dWk.view(-1)[tap * Cin:]
        flat.copy_(G.reference(_kw(Cout, Cin, M, 1, Cout, 1, Cin, taps * Cin, Tseq=T, kshift=(tap - pad) * dil, acc=ACC_ATOMIC, splitk=2), dyf, xf,
                               flat.clone()).C)
    assert torch.equal(dWk, Wt.grad.permute(0, 2, 1))
    # ... and all taps in one launch: output columns (tap, c)
    got = G.reference(_kw(Cout, taps * Cin, M, 1, Cout, 1, Cin, taps * Cin, taps=taps, pad=pad, dil=dil, Tseq=T, acc=ACC_SOLE), dyf, xf,
                      z(Cout, taps * Cin))
    assert torch.equal(got.C, Wt.grad.permute(0, 2, 1).reshape(Cout, taps * Cin))


def test_reference_batched_attention_forms():
    Bn, H, T, dk = 2, 3, 5, 4
    d = H * dk
    q, k, v = _ints(Bn, T, H, dk, seed=1), _ints(Bn, T, H, dk, seed=2), _ints(Bn, T, H, dk, seed=3)
    p = _ints(Bn, H, T, T, seed=4)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    b2 = dict(batch=Bn * H, batch_inner=H)
    # scores: q k^T per (b, h), operands strided through the [B][T][H][dk] projections
    got = G.reference(_kw(T, T, dk, d, 1, d, 1, T, a_bs=(T * d, dk), b_bs=(T * d, dk), c_bs=(H * T * T, T * T), alpha=0.5, **b2), q, k, z(Bn, H, T, T))
    assert torch.equal(got.C, 0.5 * torch.einsum("bihd,bjhd->bhij", q, k))
    # context: probs v, B [k][n], C written head by head into [B][T][H][dk]
    got = G.reference(_kw(T, dk, T, T, 1, 1, d, d, a_bs=(H * T * T, T * T), b_bs=(T * d, dk), c_bs=(T * d, dk), **b2), p, v, z(Bn, T, H, dk))
    assert torch.equal(got.C, torch.einsum("bhij,bjhd->bihd", p, v))
    # dV = probs^T dctx, A [k][m]; signed probabilities read as zero; column sums per head over the batch
    cs_len = (H - 1) * 8 + dk
    got = G.reference(_kw(T, dk, T, 1, T, 1, d, d, a_bs=(H * T * T, T * T), b_bs=(T * d, dk), c_bs=(T * d, dk), a_signmask=True, colsum_len=cs_len,
                          colsum_bs1=8, colsum_scale=0.5, **b2), p, v, z(Bn, T, H, dk))
    exp = torch.einsum("bhij,bihd->bjhd", p.clamp(min=0), v)
    assert torch.equal(got.C, exp)
    for h in range(H):
        assert torch.equal(got.colsum[h * 8:h * 8 + dk], 0.5 * exp[:, :, h].sum((0, 1)))
    # a key / value tensor shared by the heads: b_bs = (T dk, 0)
    ks = _ints(Bn, T, dk, seed=5)
    got = G.reference(_kw(T, T, dk, d, 1, dk, 1, T, a_bs=(T * d, dk), b_bs=(T * dk, 0), c_bs=(H * T * T, T * T), **b2), q, ks, z(Bn, H, T, T))
    assert torch.equal(got.C, torch.einsum("bihd,bjd->bhij", q, ks))
    # two products in one launch, the second with its own row stride; each product's share of the column sums
    a2 = _ints(Bn * H, T, T + 3, seed=6)
    kk = _ints(Bn * H, T, dk, seed=7)
    pp = _ints(Bn * H, T, dk, seed=8)
    sec = dict(b2_cs=dk, b2_bs=(H * T * dk, T * dk), a2_rs=T + 3)
    a1 = _ints(Bn * H, T, T + 3, seed=9)
    got = G.reference(_kw(T, dk, T, T + 3, 1, 1, dk, dk, a_bs=(H * T * (T + 3), T * (T + 3)), b_bs=(H * T * dk, T * dk), c_bs=(H * T * dk, T * dk), alpha=2.0,
                          second=sec, colsum_len=dk, **b2), a1, kk, z(Bn * H, T, dk), A2=a2, B2=pp)
    e1, e2 = 2.0 * a1[:, :, :T] @ kk, 2.0 * a2[:, :, :T] @ pp
    assert torch.equal(got.C, e1 + e2)
    assert torch.equal(got.colsum, e1.sum((0, 1))) and torch.equal(got.colsum2, e2.sum((0, 1)))


@pytest.mark.parametrize("hop,n_fft", [(3, 16), (4, 16), (1, 5), (7, 4)])
def test_reference_overlapping_rows_are_unfold(hop, n_fft):
    x = _ints(2, 61, seed=1)
    Wb = _ints(6, n_fft, seed=2)
    Fr = 1 + (61 - n_fft) // hop
    got = G.reference(_kw(Fr, 6, n_fft, hop, 1, n_fft, 1, 6, batch=2, a_bs=(61, 0), c_bs=(Fr * 6, 0)), x, Wb, torch.zeros(2, Fr, 6, dtype=torch.float64))
    assert torch.equal(got.C, x.unfold(1, n_fft, hop) @ Wb.t())


# ---- the case tables -----------------------------------------------------------------------------------------------------------
F32_NAMES = [f"gemm_f32_kernel<{a}, {b}, {v}>" for a, b in (("true", "true"), ("true", "false"), ("false", "false")) for v in ("true", "false")]
DRAWS = {F32: (101, 40), BF16: (202, 40)}


def _plan(case):
    t, _ = case.place()
    return case.call(ops.gemm_plan, t)


def _check_exact_range(case):
    """every case is interpretable (no access outside a buffer: the kernels run on exactly these) and stays below 2^24"""
    t, _ = case.place()
    keep = torch.ones_like(t["C"], dtype=torch.float32) if "drop" in case.kw else None
    r = case.reference(t, keep=keep)
    unit = min(1.0, abs(case.kw.get("alpha", 1.0)))
    assert float(r.mag.max()) / unit < G.EXACT, case
    if r.colsum is not None:
        assert float(r.colsum.abs().max()) / (unit * min(1.0, abs(case.kw.get("colsum_scale", 1.0)))) < G.EXACT, case


def test_f32_table_and_draws_reach_every_instantiation():
    fixed = G.f32_fixed_cases()
    seen = collections.Counter(_plan(c) for c in fixed)
    assert seen[None] == 0, [c for c in fixed if _plan(c) is None]
    assert all(seen[n] >= 3 for n in F32_NAMES) and set(seen) == set(F32_NAMES), seen
    drawn = G.draws(*DRAWS[F32], F32)
    plans = [_plan(c) for c in drawn]
    assert plans.count(None) <= len(drawn) // 10, plans
    print("fp32 fixed", dict(seen), "draws", dict(collections.Counter(plans)))
    for c in fixed + drawn:
        _check_exact_range(c)


def test_bf16_route_table_and_draws():
    lib = _lib.load()
    seen = collections.Counter()
    for mode, cases, prefix in G.bf16_route_table():
        old = G.set_modes(lib, G.MODES[mode])
        try:
            for c in cases:
                name = _plan(c)
                assert name is not None and name.startswith(prefix + "<"), (mode, c, name)
                seen[name] += 1
        finally:
            G.set_modes(lib, old)
        for c in cases:
            _check_exact_range(c)
    fam = lambda p, **has: sum(v for k, v in seen.items() if k.startswith(p) and all((s in k) == on for s, on in has.items()))
    assert len([k for k in seen if k.startswith("gemm_bf16_glds_kernel<")]) >= 8, seen
    for p in ("gemm_bf16_8p_kernel<", "gemm_bf16_8p_tn_kernel<", "gemm_bf16_8p_tn3_kernel<", "gemm_bf16_pn_kernel<false>", "gemm_bf16_pn_kernel<true>",
              "gemm_bf16_glds_kernel<"):
        assert fam(p) >= 3, (p, seen)
    dual = sum(v for k, v in seen.items() if k.startswith("gemm_bf16_tt_kernel<") and k.endswith("true>"))
    assert dual >= 3 and fam("gemm_bf16_tt_kernel<") - dual >= 3, seen
    legacy = [k for k in seen if k.startswith("gemm_bf16_kernel<")]
    assert len({k.split(",")[0] + k.split(",")[1] for k in legacy}) >= 3 and fam("gemm_bf16_kernel<") >= 3, seen
    print("bf16 fixed", dict(seen))
    # the random draws, under every mode setting
    drawn = G.draws(*DRAWS[BF16], BF16)
    for c in drawn:
        _check_exact_range(c)
    for mode, modes in G.MODES.items():
        old = G.set_modes(lib, modes)
        try:
            plans = [_plan(c) for c in drawn]
        finally:
            G.set_modes(lib, old)
        assert plans.count(None) <= len(drawn) // 10, (mode, [c for c, p in zip(drawn, plans) if p is None])
        print("bf16 draws", mode, "rejected", plans.count(None), dict(collections.Counter(plans)))


def test_generator_refuses_what_it_cannot_bound():
    with pytest.raises(RuntimeError):
        G.build("too long", 0, 8, 8, 1 << 25, "NT")
    c = G.build("narrowed", 0, 8, 8, 1 << 21, "NT")       # K * 3 * 3 > 2^24: the ranges shrink until the sums fit
    assert float(c.bufs["A"][0].abs().max()) * float(c.bufs["B"][0].abs().max()) * (1 << 21) + 16 < G.EXACT


@pytest.mark.parametrize("compute", [F32, BF16])
def test_plan_refuses_a_nonlinear_activation_with_split_k(compute):
    """every split runs the epilogue on its partial sum: act(a) + act(b) != act(a + b)"""
    dt = torch.float32 if compute == F32 else torch.bfloat16
    A, B, C = torch.zeros(128, 256, dtype=dt), torch.zeros(128, 256, dtype=dt), torch.zeros(128, 128)
    for ly in ((256, 1, 256, 1), (1, 128, 1, 128)):
        for acc in (ACC_ATOMIC, ACC_SOLE):
            assert ops.gemm_plan(A, B, C, 128, 128, 256, *ly, 128, acc=acc, splitk=2, compute=compute) is not None
            assert ops.gemm_plan(A, B, C, 128, 128, 256, *ly, 128, acc=acc, splitk=1, act=ACT_RELU, compute=compute) is not None
            for act in (ACT_RELU, ACT_TANH, _lib.ACT_SWISH):
                assert ops.gemm_plan(A, B, C, 128, 128, 256, *ly, 128, acc=acc, splitk=2, act=act, compute=compute) is None


def test_logmel_refusals():
    """reflect padding needs pad < N (a3t_reflect_pad answers before it launches anything); the constructor takes the recipe's STFT
    variant only"""
    from a3t_amd.features import LogMelFbank
    lib = _lib.load()
    x, out = torch.zeros(1, 8), torch.zeros(1, 64)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for pad in (8, 9, 20):
        assert lib.a3t_reflect_pad(P(x), P(out), 1, 8, pad, 64, None) == -22
        with pytest.raises(_lib.A3TLibraryError):
            _lib.check(lib.a3t_reflect_pad(P(x), P(out), 1, 8, pad, 64, None), "reflect_pad")
    assert lib.a3t_reflect_pad(P(x), P(out), 1, 8, 3, 13, None) == -22       # row shorter than N + 2 pad
    for bad in (dict(window="hamming"), dict(center=False), dict(normalized=True), dict(onesided=False), dict(htk=True)):
        with pytest.raises(NotImplementedError):
            LogMelFbank(device="cpu", **bad)
    assert LogMelFbank(n_fft=255, win_length=255, hop_length=85, n_mels=20, device="cpu").output_size() == 20
