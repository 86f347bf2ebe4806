"""The band-free instantiations of the fused attention forward (a3t_attn_fwd_plain / a3t_attn_fwd_train_plain: scores q k^T * scale,
a transformer model's MultiHeadedAttention).  The exact yardstick: the existing kernels fed qu = qv = q and an all-zero positional
table compute the same scores (every band term is + 0.0f), so every output must equal that launch bit for bit.  Then the float64
formula with the bounds of tests/test_gpu_attn_fused.py, whose shapes and helpers these tests import, and the engine's fused
training step against its materialised one."""
import math

import numpy as np
import pytest
import torch

import test_gpu_attn_fused as F
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = F.CASES


def _plain_inputs(B, H, T, dk, seed, lengths=None):
    """(qkv, q as a tensor of its own, zero table, keymask): q is what the zero-table launch is handed as qu and qv."""
    qkv, _, _, P, keymask = F._inputs(B, H, T, dk, seed, lengths)
    d = H * dk
    return qkv, qkv[:, :d].contiguous(), torch.zeros_like(P), keymask


def _bufs(B, H, T, d, train, two):
    ctx = torch.full((B * T, d), 7.0, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(B, H, T, device=DEV)
    if not train:
        return [ctx, lse]
    probs = torch.full((B, H, T, T), 9.0, device=DEV, dtype=torch.bfloat16)
    pdrop = torch.full((B, H, T, T), 9.0, device=DEV, dtype=torch.bfloat16) if two else None
    return [ctx, lse, probs, pdrop, torch.full((B, H, T), -1.0, device=DEV)]


def _run_plain(qkv, keymask, B, H, T, dk, train, drop=(0.0, 0), two=False):
    from a3t_amd import ops
    o = _bufs(B, H, T, H * dk, train, two)
    if train:
        ops.attn_fwd_train_plain(qkv, keymask, *o, B, H, T, 1.0 / math.sqrt(dk), drop=drop)
    else:
        ops.attn_fwd_plain(qkv, keymask, *o, B, H, T, 1.0 / math.sqrt(dk), drop=drop)
    torch.cuda.synchronize()
    return o


def _run_zero_table(qkv, q, Z, keymask, B, H, T, dk, train, drop=(0.0, 0), two=False):
    from a3t_amd import ops
    o = _bufs(B, H, T, H * dk, train, two)
    if train:
        ops.attn_fwd_train(q, q, qkv, Z, keymask, *o, B, H, T, 1.0 / math.sqrt(dk), drop=drop)
    else:
        ops.attn_fwd(q, q, qkv, Z, keymask, *o, B, H, T, 1.0 / math.sqrt(dk), drop=drop)
    torch.cuda.synchronize()
    return o


def _same_bits(a, b):
    """bit for bit, also where both hold an infinity or a signed zero (lse of a fully masked row, a dropped zero probability)"""
    if a is None or b is None:
        return a is None and b is None
    wa = a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32)
    wb = b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)
    return bool(torch.equal(wa, wb))


# (train, dropout probability, two saved tensors): forward only; training; training with the dropped copy; with the sign-tagged tensor
MODES = [(False, 0.0, False), (False, 0.2, False), (True, 0.0, False), (True, 0.2, True), (True, 0.2, False)]


@pytest.mark.parametrize("train,drop_p,two", MODES)
@pytest.mark.parametrize("B,H,T,dk,lengths", CASES)
def test_band_free_forward_equals_the_zero_table_launch_bit_for_bit(B, H, T, dk, lengths, train, drop_p, two):
    qkv, q, Z, keymask = _plain_inputs(B, H, T, dk, seed=T + dk, lengths=lengths)
    drop = (drop_p, 0x9E3779B1) if drop_p else (0.0, 0)
    got = _run_plain(qkv, keymask, B, H, T, dk, train, drop, two)
    ref = _run_zero_table(qkv, q, Z, keymask, B, H, T, dk, train, drop, two)
    names = ["ctx", "lse", "probs", "pdrop", "rowscale"]
    for n, a, b in zip(names, got, ref):
        assert _same_bits(a, b), n
    if train and drop_p and not two:      # the mask rides on the sign bits: some, not all, of a full row's probabilities are tagged
        neg = torch.signbit(got[2][0, 0, 0].float())
        assert 0 < int(neg.sum()) < T


@pytest.mark.parametrize("B,H,T,dk,lengths", CASES)
def test_band_free_forward_matches_the_float64_formula(B, H, T, dk, lengths):
    """Bounds of test_fused_forward_matches_exact_formula_and_materialised_path: 1.2e-2 of scale, no worse than
    max(1.5 x materialised, 6e-3), lse within 2e-3."""
    qkv, q, Z, keymask = _plain_inputs(B, H, T, dk, seed=T + dk, lengths=lengths)
    ctx, lse = _run_plain(qkv, keymask, B, H, T, dk, False)
    ref, _, rlse = F._exact(qkv, q, q, Z, keymask, B, H, T, dk)
    got = ctx.float().cpu().double()
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max()) / scale
    mat, _, _ = F._materialised(qkv, q, q, Z, keymask, B, H, T, dk, (0.0, 0))
    err_mat = float((mat.float().cpu().double() - ref).abs().max()) / scale
    print(f"[B{B} H{H} T{T} dk{dk}] band-free max err {err:.2e}, materialised {err_mat:.2e} (of scale {scale:.2f})")
    assert err < 1.2e-2, err
    assert err <= max(1.5 * err_mat, 6e-3)
    valid = torch.isfinite(rlse)
    l = lse.cpu().double()
    assert bool(torch.isinf(l[~valid]).all()) and bool((l[~valid] > 0).all())
    assert float((l[valid] - rlse[valid]).abs().max()) < 2e-3


@pytest.mark.parametrize("B,H,T,dk,lengths", CASES[:4])
def test_band_free_dropout_uses_the_mask_of_the_materialised_path(B, H, T, dk, lengths):
    """Dropout 0.2 against the float64 formula under the mask a3t_softmax_plain_fwd draws (bounds of
    test_fused_forward_dropout_uses_the_same_mask_as_the_materialised_path)."""
    from a3t_amd import ops
    from a3t_amd._lib import BF16
    qkv, q, Z, keymask = _plain_inputs(B, H, T, dk, seed=3 * T + dk, lengths=lengths)
    d = H * dk
    drop = (0.2, 0x9E3779B1)
    ctx, _ = _run_plain(qkv, keymask, B, H, T, dk, False, drop)
    # the materialised path of a transformer block: q k^T, a3t_softmax_plain_fwd, probs @ V
    ac = torch.empty(B, H, T, T, device=DEV, dtype=torch.bfloat16)
    qb, zb = (T * 3 * d, dk), (H * T * T, T * T)
    ops.gemm(qkv, qkv.view(-1)[d:], ac, T, T, dk, 3 * d, 1, 3 * d, 1, T, batch=B * H, batch_inner=H, a_bs=qb, b_bs=qb, c_bs=zb,
             compute=BF16)
    probs, pdrop = torch.empty_like(ac), torch.empty_like(ac)
    ops.softmax_plain_fwd(ac, keymask, probs, B, H, T, 1.0 / math.sqrt(dk), probs_drop=pdrop, drop=drop)
    mat = torch.empty(B * T, d, device=DEV, dtype=torch.bfloat16)
    ops.gemm(pdrop, qkv.view(-1)[2 * d:], mat, T, dk, T, T, 1, 1, 3 * d, d, batch=B * H, batch_inner=H, a_bs=zb, b_bs=qb,
             c_bs=(T * d, dk), compute=BF16)
    torch.cuda.synchronize()
    _, pr, _ = F._exact(qkv, q, q, Z, keymask, B, H, T, dk)
    keep = (pdrop.float().cpu() != 0) | (probs.float().cpu() == 0)
    v = qkv[:, 2 * d:].double().cpu().view(B, T, H, dk).transpose(1, 2)
    ref = ((pr * keep / (1.0 - drop[0])) @ v).transpose(1, 2).reshape(B * T, d)
    scale = max(1.0, float(ref.abs().max()))
    err = float((ctx.float().cpu().double() - ref).abs().max()) / scale
    err_mat = float((mat.float().cpu().double() - ref).abs().max()) / scale
    print(f"[B{B} H{H} T{T} dk{dk}] dropout: band-free {err:.2e}, materialised {err_mat:.2e}")
    assert err < 1.5e-2 and err <= max(1.5 * err_mat, 8e-3)


@pytest.mark.parametrize("B,H,T,dk,lengths", CASES[:4])
def test_band_free_training_save_with_the_mask_in_the_sign_bits(B, H, T, dk, lengths):
    """|probs| * rowscale = the exact softmax to bf16 accuracy (6e-3, as the two-tensor save), the sign bits are the mask of the
    materialised path, ctx / lse are the forward-only launch's."""
    from a3t_amd import ops
    qkv, q, Z, keymask = _plain_inputs(B, H, T, dk, seed=5 * T + dk, lengths=lengths)
    drop = (0.2, 0x1234567)
    ctx, lse, probs, _, rs = _run_plain(qkv, keymask, B, H, T, dk, True, drop, two=False)
    ctx2, lse2 = _run_plain(qkv, keymask, B, H, T, dk, False, drop)
    assert _same_bits(lse, lse2)
    # (the sign-tagged save multiplies the accumulators by 1 / (1 - p) once, the forward-only kernel its probabilities: one bf16 ulp)
    assert float((ctx.float() - ctx2.float()).abs().max()) <= 2.0 ** -7 * max(1.0, float(ctx2.float().abs().max()))
    _, pr, rlse = F._exact(qkv, q, q, Z, keymask, B, H, T, dk)
    got = probs.float().abs().cpu().double() * rs.cpu().double()[..., None]
    assert bool(torch.isfinite(got).all()) and float((got - pr).abs().max()) < 6e-3
    valid = torch.isfinite(rlse)
    assert float(rs.cpu()[~valid].abs().max() if (~valid).any() else 0.0) == 0.0
    one, keepf = torch.ones(B * H * T * T, device=DEV), torch.empty(B * H * T * T, device=DEV)
    ops.dropout(one, keepf, drop[0], drop[1])                      # the counter RNG over the score index (b, h, i, j)
    dropped = (keepf == 0).view(B, H, T, T)
    live = (probs.float().abs() > 0)
    assert bool((torch.signbit(probs.float())[live] == dropped[live]).all())


@pytest.mark.parametrize("train", [False, True])
def test_band_free_overflow_redo_stays_exact(train):
    """The scenario of test_fixed_reference_maximum_overflow_falls_back_and_stays_exact (the keys of the second half of one utterance
    scaled by 40), its bounds, and the zero-table launch bit for bit through the redo."""
    B, H, T, dk = 2, 2, 328, 64
    qkv, q, Z, keymask = _plain_inputs(B, H, T, dk, seed=99)
    d = H * dk
    qkv = qkv.clone()
    kview = qkv.view(B, T, 3 * d)
    kview[1, 200:, d:2 * d] = (kview[1, 200:, d:2 * d].float() * 40.0).bfloat16()
    q = qkv[:, :d].contiguous()
    got = _run_plain(qkv, keymask, B, H, T, dk, train)
    ref, pr, rlse = F._exact(qkv, q, q, Z, keymask, B, H, T, dk)
    assert float(rlse.max()) > 100.0
    ctx = got[0].float().cpu().double()
    assert bool(torch.isfinite(ctx).all())
    scale = max(1.0, float(ref.abs().max()))
    assert float((ctx - ref).abs().max()) / scale < 2e-2
    assert float((got[1].cpu().double() - rlse).abs().max()) < 2e-2
    if train:
        pn = got[2].float().cpu().double() * got[4].cpu().double()[..., None]
        assert bool(torch.isfinite(pn).all()) and float((pn - pr).abs().max()) < 8e-3
    old = _run_zero_table(qkv, q, Z, keymask, B, H, T, dk, train)
    for a, b in zip(got, old):
        assert _same_bits(a, b)


@pytest.mark.parametrize("train,drop_p", [(False, 0.0), (True, 0.0), (True, 0.2)])
def test_band_free_key_split_equals_the_unsplit_launch(train, drop_p):
    """(16, 2, 1120, 64): 288 blocks = 256 + 32 on 256 CUs, the tail runs as 4 key ranges.  As
    test_key_split_tail_blocks_equal_the_unsplit_launch defines equal: saved probabilities bit for bit, ctx within a bf16 ulp, lse and
    rowscale within 1e-5 (the fp32 summation order)."""
    B, H, T, dk = 16, 2, 1120, 64
    qkv, q, Z, keymask = _plain_inputs(B, H, T, dk, seed=7 + B)
    drop = (drop_p, 4242) if drop_p else (0.0, 0)
    got = _run_plain(qkv, keymask, B, H, T, dk, train, drop, two=bool(drop_p))
    old = F._split_off()
    try:
        ref = _run_plain(qkv, keymask, B, H, T, dk, train, drop, two=bool(drop_p))
    finally:
        F._split_restore(old)
    assert old == 1
    assert bool(torch.isfinite(got[0].float()).all())
    assert float((got[0].float() - ref[0].float()).abs().max()) <= 2.0 ** -7 * max(1.0, float(ref[0].float().abs().max()))
    assert float((got[1] - ref[1]).abs().max()) < 1e-5
    if train:
        assert float(((got[4] - ref[4]).abs() / ref[4].abs().clamp_min(1e-30)).max()) < 1e-5
        assert torch.equal(got[2], ref[2])
        if drop_p:
            assert torch.equal(got[3], ref[3])


def test_entry_points_refuse_what_the_kernels_cannot_run():
    from a3t_amd import _lib, ops
    B, H, T, dk = 1, 2, 40, 16                      # d_k = 16 is outside attn_shape_ok
    qkv = torch.zeros(B * T, 3 * H * dk, device=DEV, dtype=torch.bfloat16)
    km = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    ctx, lse = torch.zeros(B * T, H * dk, device=DEV, dtype=torch.bfloat16), torch.zeros(B, H, T, device=DEV)
    with pytest.raises(_lib.A3TLibraryError):
        ops.attn_fwd_plain(qkv, km, ctx, lse, B, H, T, 0.25)
    with pytest.raises(ValueError):
        ops.attn_fwd_plain(qkv.float(), km, ctx, lse, B, H, T, 0.25)
    assert not ops.attn_fused_supported(dk, T) and ops.attn_fused_supported(32, 136)


# ---------------------------------------------------------------- the engine on the fused kernels
def _model64(seed=3, **kw):
    """A restated transformer model at adim 64, 2 heads (d_k = 32: inside the fused kernels' shapes), T_mel = 120, T_phn = 16
    (T = 136, two query blocks) with a row of 97 valid keys."""
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.config import A3TConfig
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    c = A3TConfig(adim=64, heads=2, ff=128, ff_kernel=3, enc_blocks=2, dec_blocks=1, postnet_layers=2, postnet_chans=16, vocab=40,
                  block="transformer", scaled_pos=True, **kw)
    store = ParamStore(c, DEV)
    xavier_init_(store, seed=seed, bn_gamma=1.0)
    store.p["emb.alpha_s"].fill_(1.3)
    store.p["emb.alpha_t"].fill_(0.7)
    batch = synthetic_batch(c, 3, 120, 16, seed=21, device=DEV)
    batch["speech_mask"][1, ..., 85:] = False           # 85 + 12 = 97 valid keys in row 1
    batch["text_mask"][1, ..., 12:] = False
    batch["masked_position"][1, 85:] = False
    return c, store, batch


def _step(eng, store, batch):
    store.zero_grad()
    loss = float(eng.forward(batch)["loss"])
    eng.backward()
    torch.cuda.synchronize()
    return loss, store.grad.clone()


def test_bf16_engine_on_the_fused_kernels_tracks_fp32():
    """The project's bf16 bounds (loss 1e-2, gradient cosine >= 0.99) with every block on the band-free fused training forward
    (fused_attn_train = 2 lifts the 64-workgroup threshold, as the parity fixtures do), and the forward-only pass on a3t_attn_fwd_plain."""
    from a3t_amd.conformer import EngineOptions
    from a3t_amd.engine import MLMEngine
    c, store, batch = _model64()
    eng = MLMEngine(c, store, compute="bf16", training=True, dropout=False, options=EngineOptions(fused_attn_train=2))
    l16, g16 = _step(eng, store, batch)
    assert eng.attn_path == {"enc.0": "train", "enc.1": "train", "dec.0": "train"}, eng.attn_path
    assert eng.block_dims == {"enc.0": (3, 136), "enc.1": (3, 136), "dec.0": (3, 136)}
    assert all(f"{b}.mha.rs" in eng.sv for b in eng.attn_path)
    e32 = MLMEngine(c, store, compute="f32", training=True, dropout=False)
    l32, g32 = _step(e32, store, batch)
    assert set(e32.attn_path.values()) == {"mat"}
    cos = float(torch.nn.functional.cosine_similarity(g16, g32, dim=0))
    print(f"bf16 (fused) against fp32: loss {l16:.6f} / {l32:.6f}, gradient cosine {cos:.6f}")
    assert abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert bool(torch.isfinite(g16).all()) and cos >= 0.99, cos
    # forward only: a3t_attn_fwd_plain, nothing kept; the same mel to bf16 accuracy as the materialised forward
    ef = MLMEngine(c, store, compute="bf16", training=False, options=EngineOptions(fused_attn="fwd"))
    out_f = ef.forward(batch, need_grad=False)["after"].float().clone()
    assert set(ef.attn_path.values()) == {"fwd"} and ef.sv["enc.0.mha"] is None
    em = MLMEngine(c, store, compute="bf16", training=False, options=EngineOptions(fused_attn="0"))
    out_m = em.forward(batch, need_grad=False)["after"].float()
    assert set(em.attn_path.values()) == {"mat"}
    assert float((out_f - out_m).abs().max()) < 3e-2 * float(out_m.abs().max())


@pytest.mark.parametrize("bwd_ds", [False, True])
@pytest.mark.parametrize("dropout", [False, True])
def test_engine_training_step_on_the_fused_forward_matches_the_materialised_step(dropout, bwd_ds):
    """test_engine_training_step_with_the_fused_forward_matches_the_materialised_step on the transformer model, its criteria: the
    same dropout masks, loss within 5e-3, every parameter gradient with cosine >= 0.985 and norm ratio in (0.93, 1.07)."""
    from a3t_amd.conformer import EngineOptions
    from a3t_amd.engine import MLMEngine
    rates = dict(dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.2, postnet_dropout_rate=0.5)
    res = {}
    for fused in (0, 2):
        c, store, batch = _model64(**rates)
        eng = MLMEngine(c, store, compute="bf16", training=True, dropout=dropout,
                        options=EngineOptions(fused_attn_train=fused, attn_bwd_ds=bwd_ds))
        loss = float(eng.forward(batch)["loss"])
        assert set(eng.attn_path.values()) == ({"train"} if fused else {"mat"})
        assert sum(k.endswith(".rs") for k in eng.sv) == (3 if fused else 0)
        if fused and dropout:      # one saved tensor exactly when the one-launch score gradients read it
            assert all(bool(eng.sv[f"{b}.mha.signed"]) == bwd_ds for b in eng.attn_path)
        store.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        res[fused] = (loss, store.state_dict(grads=True))
    (l0, g0), (l1, g1) = res[0], res[2]
    print(f"loss materialised {l0:.5f} fused-forward {l1:.5f}")
    assert abs(l0 - l1) < 5e-3 * abs(l0), (l0, l1)
    bad = []
    for k in g0:
        a, b_ = g1[k].double().flatten(), g0[k].double().flatten()
        nb = float(b_.norm())
        if nb < 1e-6 or k.endswith("linear_k.bias"):
            continue
        cos = float((a * b_).sum() / (a.norm() * b_.norm() + 1e-30))
        ratio = float(a.norm()) / nb
        if cos < 0.985 or not (0.93 < ratio < 1.07):
            bad.append((k, round(cos, 4), round(ratio, 4)))
    assert not bad, bad[:10]
