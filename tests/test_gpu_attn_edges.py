"""The fused attention forward (a3t_attn_fwd / a3t_attn_fwd_train) at its short-sequence edge and on its 16-query kernel alone,
against the float64 forward of tests/attn_ref.py.

* T ladder: T in {8 .. 128} x d_k in {32, 192}, B = 2, H = 2, one ragged row.  The existing forward tests stop at T = 40; below
  T = 32 every key / value / band tile is mostly zero fill (buffer range checks, the zero page) and a 128-query block has waves
  without a single query.  Assertions: the two of test_fused_forward_matches_exact_formula_and_materialised_path (1.2e-2 of the
  scale; no worse than 1.5 x the materialised path, floor 6e-3) and its log-sum-exp assertions; probs * rowscale against the float64
  softmax at 6e-3 (test_training_forward_saves_probabilities_...); with dropout the dropped copy / the sign tags against the
  counter generator restated in tests/stepkernel_ref.py; guard bands around ctx, lse, probs, probs_drop and rowscale.
* More than 2^16 (b, h, query block) workgroups: launch_fwd16 then starts the rescaling 16-query kernel alone, and refuses to
  save probabilities (rc = -22).
"""
import math

import numpy as np
import pytest
import torch

import attn_ref as A
import stepkernel_ref as SK
from test_gpu_attn_fused import _inputs, _materialised
from test_gpu_rowkernel_paths import Bands

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


def _check_ctx_lse(tag, ctx, lse, ref, rlse, err_mat_of, tol=1.2e-2, floor=6e-3):
    scale = max(1.0, float(ref.abs().max()))
    err = float((ctx.to(F64) - ref).abs().max()) / scale
    err_mat = err_mat_of(scale)
    print(f"[{tag}] fused max err {err:.2e}, materialised {err_mat:.2e} (of scale {scale:.2f})")
    assert bool(torch.isfinite(ctx.float()).all())
    assert err < tol, err
    assert err <= max(1.5 * err_mat, floor), (err, err_mat)
    valid = torch.isfinite(rlse)
    l = lse.to(F64)
    assert bool(torch.isinf(l[~valid]).all()) and bool((l[~valid] > 0).all())
    assert float((l[valid] - rlse[valid]).abs().max()) < 2e-3


@pytest.mark.parametrize("dk", A.LADDER_DK)
@pytest.mark.parametrize("T", A.LADDER_T)
def test_short_sequence_ladder_against_float64(T, dk):
    from a3t_amd import ops
    B, H = 2, 2
    d = H * dk
    lengths = [T, max(1, (5 * T) // 8 - 3)]
    qkv, qu, qv, P, keymask = _inputs(B, H, T, dk, seed=17 * T + dk, lengths=lengths)
    scale = 1.0 / math.sqrt(dk)
    ref, pr, rlse = A.ref_fwd(qkv, qu, qv, P, keymask, B, H, T, dk)
    mat, _, _ = _materialised(qkv, qu, qv, P, keymask, B, H, T, dk, (0.0, 0))
    torch.cuda.synchronize()
    plain_mat = lambda s: float((mat.to(F64) - ref).abs().max()) / s
    tag = f"T{T} dk{dk}"
    bands = Bands()
    outs = lambda two: (bands.out((B * T, d), torch.bfloat16), bands.out((B, H, T), torch.float32),
                        bands.out((B, H, T, T), torch.bfloat16), bands.out((B, H, T, T), torch.bfloat16) if two else None,
                        bands.out((B, H, T), torch.float32))
    # ---- a3t_attn_fwd
    ctx, lse, _, _, _ = outs(False)
    ops.attn_fwd(qu, qv, qkv, P, keymask, ctx, lse, B, H, T, scale)
    bands.intact()
    _check_ctx_lse(tag + " fwd", ctx, lse, ref, rlse, plain_mat)
    # ---- a3t_attn_fwd_train without dropout
    ctx, lse, probs, _, rs = outs(False)
    ops.attn_fwd_train(qu, qv, qkv, P, keymask, ctx, lse, probs, None, rs, B, H, T, scale)
    bands.intact()
    _check_ctx_lse(tag + " train", ctx, lse, ref, rlse, plain_mat)
    valid = torch.isfinite(rlse)

    def check_probs(what, probs, rs):
        got = probs.abs().to(F64) * rs.to(F64)[..., None]
        assert bool(torch.isfinite(got).all())
        err = float((got - pr).abs().max())
        print(f"[{tag} {what}] normalised saved probabilities: max err {err:.2e}")
        assert err < 6e-3, err                              # bf16 probabilities (relative 2^-9) of rows that sum to 1
        assert float(rs[~valid].abs().max() if bool((~valid).any()) else 0.0) == 0.0
    check_probs("train", probs, rs)
    assert not bool((probs.view(torch.int16) < 0).any())
    # ---- with dropout: a dropped copy, and the sign-tagged single tensor
    drop = (0.2, 0x1234567)
    keep = torch.from_numpy(SK.keep(drop[1], np.arange(B * H * T * T, dtype=np.int64), drop[0])).view(B, H, T, T).to(DEV)
    dinv = float(SK.drop_inv(drop[0]))
    refd, _, _ = A.ref_fwd(qkv, qu, qv, P, keymask, B, H, T, dk, keep=keep, dinv=dinv)
    matd, _, _ = _materialised(qkv, qu, qv, P, keymask, B, H, T, dk, drop)
    torch.cuda.synchronize()
    drop_mat = lambda s: float((matd.to(F64) - refd).abs().max()) / s
    for two in (True, False):
        what = "train+copy" if two else "train+signs"
        ctx, lse, probs, pdrop, rs = outs(two)
        ops.attn_fwd_train(qu, qv, qkv, P, keymask, ctx, lse, probs, pdrop, rs, B, H, T, scale, drop=drop)
        bands.intact()
        # (the numbers of test_fused_forward_dropout_uses_the_same_mask_as_the_materialised_path)
        _check_ctx_lse(f"{tag} {what}", ctx, lse, refd, rlse, drop_mat, tol=1.5e-2, floor=8e-3)
        check_probs(what, probs, rs)
        nz = (probs.view(torch.int16) & 0x7fff) != 0
        if two:
            assert not bool((probs.view(torch.int16) < 0).any())
            want = probs.float() * keep * dinv
            rel = float(((pdrop.float() - want).abs() / (want.abs() + 1e-20)).max())
            assert rel < 1e-2, rel                          # same mask; one more bf16 rounding
            assert torch.equal((pdrop.view(torch.int16) == 0) & nz, ~keep & nz)
        else:
            assert torch.equal((probs.view(torch.int16) < 0) & nz, ~keep & nz), "sign = dropped"


def test_more_than_65536_blocks_run_the_16_query_kernel_alone():
    """B H ceil(T/128) = 65537 workgroups: no overflow flag per block is left, so launch_fwd16 skips the 32-query kernel and the
    rescaling 16-query kernel computes every block; saving probabilities is refused."""
    from a3t_amd import ops
    B, H, T, dk = 65537, 1, 8, 32
    d = H * dk
    g = torch.Generator(device=DEV).manual_seed(65537)
    mk = lambda *s, sc=1.0: (torch.randn(*s, device=DEV, generator=g) * sc).bfloat16()
    qkv = mk(B * T, 3 * d)
    qu = (qkv[:, :d].float() + mk(1, d, sc=0.3).float()).bfloat16().contiguous()
    qv = (qkv[:, :d].float() + mk(1, d, sc=0.3).float()).bfloat16().contiguous()
    P = mk(T, d)
    keymask = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    keymask[1, 3:] = 0
    keymask[2] = 0
    keymask[B - 1, 5:] = 0
    scale = 1.0 / math.sqrt(dk)
    bands = Bands()
    ctx, lse = bands.out((B * T, d), torch.bfloat16), bands.out((B, H, T), torch.float32)
    ops.attn_fwd(qu, qv, qkv, P, keymask, ctx, lse, B, H, T, scale)
    bands.intact()
    ref, _, rlse = A.ref_fwd(qkv, qu, qv, P, keymask, B, H, T, dk)
    sc = max(1.0, float(ref.abs().max()))
    err = float((ctx.to(F64) - ref).abs().max()) / sc
    print(f"[B{B} T{T} dk{dk}] 16-query kernel alone: max err {err:.2e} (of scale {sc:.2f})")
    assert bool(torch.isfinite(ctx.float()).all()) and err < 1.2e-2, err
    valid = torch.isfinite(rlse)
    l = lse.to(F64)
    assert int((~valid).sum()) == T and bool(torch.isinf(l[~valid]).all()) and bool((l[~valid] > 0).all())
    assert float((l[valid] - rlse[valid]).abs().max()) < 2e-3
    assert not bool(ctx.view(B, T, d)[2].any())
    probs = bands.out((4, T), torch.bfloat16)               # (never written: the call is refused before any launch)
    rs = bands.out((4, T), torch.float32)
    with pytest.raises(Exception, match="rc=-22"):
        ops.attn_fwd_train(qu, qv, qkv, P, keymask, ctx, lse, probs, None, rs, B, H, T, scale)
    bands.intact()
