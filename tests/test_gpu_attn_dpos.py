"""a3t_attn_bwd_dpos (csrc/attn_dpos.hip): the gradient of linear_pos' output as a streaming product over groups of batch elements + a
fold in fixed order, against the float64 sum over the bf16-rounded operands and against the path it replaces (the 128-row GEMM with
fp32 atomics + cast_bf16).

Bound (the convention of tests/rowkernel_ref.py): |got - ref| <= (L + 8) 2^-23 mag + 2^-8 |ref|, L = B T + groups (the longest fp32
addition chain of an output: B T products in the MFMA accumulators of one workgroup after another, then the groups in the fold),
mag the same sum over absolute values, the last term the bf16 store.  The optional fp32 output is held to the first term alone.
The path it replaces is held to the same bound of the same reference, and to twice the bound against the new output (each of the two
rounds an fp32 sum of its own to bf16; two values inside one bound of a reference are inside two of each other, no closer).

Every operand lies inside a buffer whose surroundings are NaN, and the workspace starts as NaN: a read past an extent or a float of
the workspace that nobody wrote shows up in the output.
"""
import math

import numpy as np
import pytest
import torch

from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
EINVAL = -22
# (B, H, T, dk): one tile, K tail 40 % 32, odd B | three column blocks | two column blocks | more than one row tile at every tile
# height the kernel can be built with, last tile nearly empty | dk = 96 | groups of TWO batch elements (the hand-over inside a
# workgroup, the ring of stages spanning three elements), last group short | the same with several K-tiles per element
CASES = [(3, 2, 40, 32), (5, 1, 72, 192), (2, 2, 136, 128), (3, 2, 328, 64), (4, 2, 168, 96), (141, 2, 40, 32), (129, 2, 136, 128)]
PAD = 4096


def _poisoned(n, head, dtype=torch.bfloat16):
    """n elements `head` elements into a buffer of NaNs (head 8: 16-byte aligned, head 9: 2-byte aligned)."""
    buf = torch.full((head + n + PAD,), float("nan"), device=DEV, dtype=dtype)
    return buf, buf[head:head + n]


def _operands(B, H, T, dk, form, seed, border=False):
    """dbd as the stored matrix (row stride T, base 2-byte aligned) or as the view of dS (row stride T + 1, T zeros in front of every
    block: tests/test_gpu_attn_fused.py, test_compact_dbd_matrix_read_as_a_view_of_ds), and qv.  Returns the device operands, their
    strides and the float64 CPU copies of what the kernel is to read."""
    g = torch.Generator().manual_seed(seed)
    d, M = H * dk, B * T
    vals = (torch.randn(B * H, T * T, generator=g) * 0.25).bfloat16()
    qvv = torch.randn(M, d, generator=g).bfloat16()
    if border:      # NaN-free but large (|x| up to 2^6) in the last row and the last column of every block
        big = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * 64.0).bfloat16()
        v3 = vals.view(B * H, T, T)
        v3[:, T - 1, :] = big(B * H, T)
        v3[:, :, T - 1] = big(B * H, T)
        q4 = qvv.view(B, T, H, dk)
        q4[:, T - 1] = big(B, H, dk)
        q4[:, :, :, dk - 1] = big(B, T, H)
    keep = []
    if form == "stored":
        buf, dbd = _poisoned(B * H * T * T, 9)
        dbd.copy_(vals.view(-1).to(DEV))
        rs, bs = T, (H * T * T, T * T)
        mat = vals.view(B, H, T, T).double()
    else:
        bsv = T + T * T
        buf, flat = _poisoned(B * H * bsv, 8)
        flat.zero_()
        flat.view(B * H, bsv)[:, T:] = vals.to(DEV)
        dbd = flat[1:]
        rs, bs = T + 1, (H * bsv, bsv)
        mat = torch.as_strided(flat.cpu(), (B * H, T, T), (bsv, T + 1, 1), storage_offset=1).reshape(B, H, T, T).double()
    keep.append(buf)
    qbuf, qv = _poisoned(M * d, 8)
    qv = qv.view(M, d)
    qv.copy_(qvv.to(DEV))
    keep.append(qbuf)
    return dbd, rs, bs, qv, mat, qvv.double().view(B, T, H, dk), keep


def _reference(mat, q4):
    """ref[r, h, n] = sum_b sum_i dbd[b, h, i, r] qv[b, i, h, n] in float64, and the same sum over absolute values."""
    B, H, T, _ = mat.shape
    dk = q4.shape[3]
    ref, mag = torch.zeros(T, H, dk, dtype=torch.float64), torch.zeros(T, H, dk, dtype=torch.float64)
    for h in range(H):
        a = mat[:, h].reshape(B * T, T).t()
        b = q4[:, :, h].reshape(B * T, dk)
        ref[:, h] = a @ b
        mag[:, h] = a.abs() @ b.abs()
    return ref.reshape(T, H * dk), mag.reshape(T, H * dk)


def _run(ops, dbd, rs, bs, qv, B, H, T, dk, want32=True):
    d = H * dk
    n = ops.attn_bwd_dpos_ws(B, H, T, dk)
    ws = torch.full((n,), float("nan"), device=DEV)
    out16 = torch.full((T, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    out32 = torch.full((T, d), float("nan"), device=DEV) if want32 else None
    ops.attn_bwd_dpos(dbd, qv, ws, out16, B, H, T, rs, bs, dP=out32)
    torch.cuda.synchronize()
    return out16, out32


def _old_path(ops, dbd, rs, bs, qv, B, H, T, dk, form):
    from a3t_amd._lib import ACC_ATOMIC, BF16
    d = H * dk
    if form == "stored":        # (the GEMM takes a dense operand from a 16-byte aligned base only)
        dbd = dbd.clone()
    dP = torch.zeros(T, d, device=DEV)
    ops.gemm(dbd, qv, dP, T, dk, T, 1, rs, 1, d, d, batch=B * H, batch_inner=H, a_bs=bs, b_bs=(T * d, dk), c_bs=(0, dk),
             acc=ACC_ATOMIC, compute=BF16, a_view=form == "view")
    old16 = torch.empty(T, d, device=DEV, dtype=torch.bfloat16)
    ops.cast_bf16(dP, old16)
    torch.cuda.synchronize()
    return old16


def _check(tag, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{tag}: max |err| {float(err.max()):.3e}, max err / bound {worst:.3f}")
    assert torch.isfinite(got).all(), tag
    assert bool((err <= bound).all()), (tag, worst)


@pytest.mark.parametrize("form", ["stored", "view"])
@pytest.mark.parametrize("B,H,T,dk", CASES)
def test_dpos_against_float64_and_the_atomic_path(B, H, T, dk, form):
    from a3t_amd import ops
    plan = ops.attn_bwd_dpos_plan(B, H, T, dk)
    assert plan is not None
    groups = -(-B // plan[2])
    dbd, rs, bs, qv, mat, q4, keep = _operands(B, H, T, dk, form, seed=T * 7 + dk + B)
    ref, mag = _reference(mat, q4)
    first = (B * T + groups + 8) * EPS * mag
    bound = first + 2.0 ** -8 * ref.abs()
    out16, out32 = _run(ops, dbd, rs, bs, qv, B, H, T, dk)
    assert float(ref.abs().max()) > 0
    _check("fp32 output", out32, ref, first)
    _check("bf16 output", out16, ref, bound)
    assert torch.equal(out16, out32.bfloat16()), "the bf16 output is the rounded fp32 sum"
    # the path this replaces, on the same inputs: inside the same bound of the reference, hence within twice the bound of the new
    # output (two values that each round an fp32 sum of their own to bf16 can lie one bf16 step apart)
    old16 = _old_path(ops, dbd, rs, bs, qv, B, H, T, dk, form)
    _check("atomic path", old16, ref, bound)
    _check("atomic path against the new output", old16, out16.double().cpu(), 2 * bound)
    # determinism: a second launch gives the same bits, bf16 and fp32
    again16, again32 = _run(ops, dbd, rs, bs, qv, B, H, T, dk)
    assert torch.equal(again16, out16) and torch.equal(again32, out32)
    # without the optional fp32 output
    only16, _ = _run(ops, dbd, rs, bs, qv, B, H, T, dk, want32=False)
    assert torch.equal(only16, out16)


@pytest.mark.parametrize("form", ["stored", "view"])
def test_dpos_large_values_on_the_borders_of_every_block(form):
    """|x| up to 2^6 in the last row and the last column of every dbd block and of every (batch element, head) block of qv: a
    fragment, a K tail or a tile edge that drops or doubles the border moves the output far beyond the bound."""
    from a3t_amd import ops
    B, H, T, dk = 3, 2, 328, 64
    groups = -(-B // ops.attn_bwd_dpos_plan(B, H, T, dk)[2])
    dbd, rs, bs, qv, mat, q4, keep = _operands(B, H, T, dk, form, seed=11, border=True)
    assert float(mat.abs().max()) > 32 and float(q4.abs().max()) > 32 and bool(torch.isfinite(mat).all())
    ref, mag = _reference(mat, q4)
    first = (B * T + groups + 8) * EPS * mag
    out16, out32 = _run(ops, dbd, rs, bs, qv, B, H, T, dk)
    _check("fp32 output", out32, ref, first)
    _check("bf16 output", out16, ref, first + 2.0 ** -8 * ref.abs())


def test_dpos_reads_nothing_past_the_last_batch_element():
    """qv is a view of the first B T rows of a larger tensor whose further rows hold a sentinel (here NaN; so do the elements in front
    of and behind dbd): with the K tail 72 % 32 in the last batch element of a short last group, nothing past the extents is read."""
    from a3t_amd import ops
    B, H, T, dk = 5, 1, 72, 192
    d = H * dk
    g = torch.Generator().manual_seed(3)
    big = torch.full((B * T + 64, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    qvv = torch.randn(B * T, d, generator=g).bfloat16()
    big[:B * T] = qvv.to(DEV)
    qv = big[:B * T]
    dbd, rs, bs, _, mat, _, keep = _operands(B, H, T, dk, "view", seed=5)
    ref, mag = _reference(mat, qvv.double().view(B, T, H, dk))
    groups = -(-B // ops.attn_bwd_dpos_plan(B, H, T, dk)[2])
    out16, out32 = _run(ops, dbd, rs, bs, qv, B, H, T, dk)
    _check("fp32 output", out32, ref, (B * T + groups + 8) * EPS * mag)
    assert bool(torch.isnan(big[B * T:]).all())


def test_dpos_refusals_leave_the_output_untouched():
    from a3t_amd import _lib
    lib = _lib.load()
    P = lambda t: None if t is None else t.data_ptr()
    ws = torch.zeros(1 << 16, device=DEV)

    def call(B, H, T, dk, qv_shift=0):
        d = H * dk
        dbd = torch.zeros(B * H * T * T + 8, device=DEV, dtype=torch.bfloat16)
        qv = torch.zeros(B * T * d + 8, device=DEV, dtype=torch.bfloat16)
        out = torch.full((T, d), 3.0, device=DEV, dtype=torch.bfloat16)
        rc = lib.a3t_attn_bwd_dpos(P(dbd), P(qv) + qv_shift, P(ws), P(out), None, B, H, T, dk, T, H * T * T, T * T,
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, bool((out == 3.0).all())

    assert call(2, 2, 44, 32) == (EINVAL, True)
    assert call(2, 2, 40, 160) == (EINVAL, True)
    assert call(2, 2, 40, 32, qv_shift=2) == (EINVAL, True)
    rc, untouched = call(2, 2, 40, 32)
    assert rc == 0 and not untouched, "the same call with an aligned qv is taken"


def test_engine_step_with_and_without_the_streaming_dpos(monkeypatch):
    """One training step of a tiny Conformer (2 + 2 blocks, d = 64, H = 2, B = 3, T = 32 + 8, bf16, dropout on) as shipped, and the same
    step with ops.attn_bwd_dpos_plan answering "not taken" (the atomic GEMM + cast_bf16 of before).  Only the gradients of linear_pos
    may differ.  Their bound, composed: both steps hand a bf16 dP16 to the weight gradient gW[o][c] = sum_r dP16[r][o] pos[r][c]; each
    dP16 lies within bnd[r][o] = (L + 8) 2^-23 mag + 2^-8 |ref| of the exact sum over its bf16 operands (the bound of this file, L = B T
    + groups; mag and ref are formed in float64 from the operands the shipped step hands to the new kernel), so the two differ by at
    most 2 bnd; that goes linearly through the sum over the T rows against |pos|, and each of the two weight-gradient sums adds its
    own fp32 accumulation error over T terms in whatever order, (T + 8) 2^-23 sum_r |dP16[r][o]| |pos[r][c]|:
        |gW_new - gW_old| <= sum_r 2 bnd[r][o] |pos[r][c]| + 2 (T + 8) 2^-23 sum_r |dP16[r][o]| |pos[r][c]|.
    Every other gradient that a GEMM makes (all matrices) must be bit-equal.  The gradients that kernels untouched here finish with fp32
    atomics in hardware order (1-D tensors, depthwise taps, the embedding scatter-adds) do not repeat their bits between two runs of
    the unchanged step, so they are held to the order-of-summation bound written at their branch below instead."""
    from a3t_amd import ops
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    B, Tm, Tp, H, dm = 3, 32, 8, 2, 64
    T, dk = Tm + Tp, dm // H
    kw = dict(adim=dm, heads=H, ff=128, enc_blocks=2, dec_blocks=2, postnet_layers=2, postnet_chans=32)
    oc = O.A3TConfig(**kw)
    c = A3TConfig(vocab=oc.vocab, dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.2, postnet_dropout_rate=0.5, **kw)
    state = O.procedural_state(O.param_shapes(oc), 5)
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(oc, B=B, T_mel=Tm, T_phn=Tp, seed=9).items()}
    real_plan, real_dpos, real_wgrad = ops.attn_bwd_dpos_plan, ops.attn_bwd_dpos, ops.linear_bwd_weight
    assert real_plan(B, H, T, dk) is not None
    groups = -(-B // real_plan(B, H, T, dk)[2])
    seen, bounds = [], {}

    def dpos_spy(dbd, qv, ws, dP16, B_, H_, T_, rs, bs, dP=None):
        real_dpos(dbd, qv, ws, dP16, B_, H_, T_, rs, bs, dP=dP)
        torch.cuda.synchronize()
        mat = torch.as_strided(dbd.cpu(), (B_, H_, T_, T_), (bs[0], bs[1], rs, 1)).double()
        ref, mag = _reference(mat, qv.cpu().double().view(B_, T_, H_, qv.shape[1] // H_))
        seen.append((dP16.data_ptr(), (B_ * T_ + groups + 8) * EPS * mag + 2.0 ** -8 * ref.abs(), dP16.double().cpu()))

    def wgrad_spy(x, y, gw, *a, **k):
        if seen and seen[-1][0] == x.data_ptr() and len(seen[-1]) == 3:
            _, bnd, dp = seen[-1]
            pa = y.double().cpu().abs()
            seen[-1] = seen[-1] + (None,)
            bounds[gw.data_ptr()] = (2 * bnd).t() @ pa + 2 * (T + 8) * EPS * (dp.abs().t() @ pa)
        real_wgrad(x, y, gw, *a, **k)

    real_embed = ops.embed_finish_bwd
    scatter = {}        # data_ptr of a gradient a3t_embed_finish_bwd scatter-adds -> per-column sum of |terms| (an upper bound)

    def embed_spy(dxs, e, text, spos, tpos, de, demb, dseg, B_, Tm_, Tp_, D, V, nseg, xscale, drop=(0.0, 0)):
        torch.cuda.synchronize()
        m = dxs.double().cpu().reshape(-1, D).abs().sum(0) / (1.0 - drop[0]) * max(1.0, xscale)
        for t in (demb, dseg):
            if t is not None:
                scatter[t.data_ptr()] = scatter.get(t.data_ptr(), 0) + m
        real_embed(dxs, e, text, spos, tpos, de, demb, dseg, B_, Tm_, Tp_, D, V, nseg, xscale, drop=drop)

    res = {}
    for mode in ("shipped", "atomic"):
        if mode == "atomic":
            monkeypatch.setattr(ops, "attn_bwd_dpos_plan", lambda *a: None)
        else:
            monkeypatch.setattr(ops, "attn_bwd_dpos", dpos_spy)
            monkeypatch.setattr(ops, "linear_bwd_weight", wgrad_spy)
            monkeypatch.setattr(ops, "embed_finish_bwd", embed_spy)
        store = ParamStore(c, DEV)
        store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
        eng = MLMEngine(c, store, compute="bf16", training=True, dropout=True)
        loss = float(eng.forward(batch)["loss"])
        store.zero_grad()
        n_seen = len(seen)
        eng.backward()
        torch.cuda.synchronize()
        assert len(seen) - n_seen == (4 if mode == "shipped" else 0), (mode, len(seen))
        res[mode] = (loss, {k: v.clone() for k, v in store.g.items()}, {k: v.data_ptr() for k, v in store.g.items()})
        monkeypatch.setattr(ops, "attn_bwd_dpos", real_dpos)
        monkeypatch.setattr(ops, "linear_bwd_weight", real_wgrad)
        monkeypatch.setattr(ops, "embed_finish_bwd", real_embed)
    (l1, g1, ptr1), (l0, g0, _) = res["shipped"], res["atomic"]
    assert l0 == l1 and math.isfinite(l1)
    npos, bad = 0, []
    for k in g1:
        err = (g1[k].double().cpu() - g0[k].double().cpu()).abs()
        if k.endswith(".wpos"):
            npos += 1
            bnd = bounds[ptr1[k]]
            assert err.shape == bnd.shape and float(g1[k].abs().max()) > 0
            print(f"{k}: max |diff| {float(err.max()):.3e}, max diff / bound {float((err / bnd.clamp_min(1e-300)).max()):.3f}")
            if not bool((err <= bnd).all()):
                bad.append(k)
        elif ptr1[k] in scatter:
            # the scatter-adds of a3t_embed_finish_bwd (segment and token embeddings: fp32 atomics in the order the hardware takes them,
            # a kernel and an input this change does not touch) do not repeat their bits from one run of the SAME step to the next, so
            # bit equality cannot be asked of them: each of the two sums of at most B T terms lies within (B T + 8) 2^-23 of the
            # column's sum of |terms| (from the kernel's own input, as the shipped step hands it over) of the exact sum
            bnd = 2 * (B * T + 8) * EPS * scatter[ptr1[k]]
            print(f"{k} (atomic scatter-add): max |diff| {float(err.max()):.3e}, max bound {float(bnd.max()):.3e}")
            if not bool((err.reshape(-1, bnd.numel()) <= bnd).all()):
                bad.append(k)
        elif g1[k].dim() == 1 or k.endswith(".dw"):
            # biases, LayerNorm / BatchNorm gains and the depthwise taps: column sums over the B T rows that their kernels finish with fp32
            # atomics in hardware order -- three runs of the unchanged step differ in some forty of them by an ulp or two (max |diff|
            # 2e-9 .. 4e-6 on values of 0.1 .. 23), so bit equality cannot be asked here either.  Two orders of N = B T terms differ by at
            # most 2 (N + 8) 2^-23 mag; mag is not visible outside those kernels, the tensor's largest |sum| stands in for it.
            # (the depthwise bias sits in front of a BatchNorm: its gradient sum_r dz[r][c] is zero in exact arithmetic, what is stored
            #  is rounding alone and says nothing about mag; its sibling dw[c][k] = sum_r dz[r][c] x[r + k][c] sums the same dz against
            #  inputs of order one and stands in for it)
            scale = g0[k[:-3] + ".dw"] if k.endswith(".cnv.db") else g0[k]
            tol = 2 * (B * T + 8) * EPS * float(scale.abs().max())
            if float(err.max()) > tol:
                print(f"{k} (atomic column sum): max |diff| {float(err.max()):.3e} > {tol:.3e}")
                bad.append(k)
        elif not torch.equal(g1[k], g0[k]):
            print(f"{k}: NOT bit-equal, max |diff| {float(err.max()):.3e} of max {float(g0[k].abs().max()):.3e}")
            bad.append(k)
    assert not bad, bad
    assert npos == 4
