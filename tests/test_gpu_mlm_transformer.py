"""The transformer MLM model (`encoder: transformer`: plain attention, absolute positions) on the device: the softmax pair without a
positional term and the absolute-position prologue kernels against float64 and against the existing kernels bit for bit; the fp32
engine against the reference's own records (tests/golden/mlm_transformer*.npz), bf16 and bf16x3 against fp32, dropout steps, the
overlapped all-reduce hooks, checkpoints and the speech editor."""
import argparse
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import mlm_transformer_ref as R
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
CASES = R.CASES


def _f(x):
    return float(np.asarray(x).reshape(-1)[0])


def _dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _task_args(case, dropout=False, **enc_extra):
    oc, o = O.tiny_config(), R.options(case)
    ffn = dict(positionwise_layer_type=o["positionwise_layer_type"], positionwise_conv_kernel_size=o["positionwise_conv_kernel_size"])
    enc = dict(input_layer=o["input_layer"], attention_dim=oc.adim, attention_heads=oc.heads, linear_units=oc.ff,
               num_blocks=o["enc_blocks"], dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.2,
               selfattention_layer_type="selfattn", **ffn)
    enc.update(enc_extra)
    decc = dict(attention_dim=oc.adim, attention_heads=oc.heads, linear_units=oc.ff, num_blocks=oc.dec_blocks,
                selfattention_layer_type="selfattn", **ffn)
    mc = dict(lsm_weight=0.1, mean_phn_span=8, mlm_prob=0.8, postnet_layers=oc.postnet_layers, postnet_filts=5,
              postnet_chans=oc.postnet_chans, dropout=dropout)
    toks = ["<blank>", "<unk>", "<space>"] + [f"t{i}" for i in range(oc.vocab - 4)] + ["<sos/eos>"]
    return argparse.Namespace(token_list=toks, odim=80, input_size=80, feats_extract="fbank",
                              feats_extract_conf=dict(n_fft=2048, hop_length=300, win_length=1200, fs=24000, fmin=80,
                                                      fmax=7600, n_mels=80),
                              normalize=None, normalize_conf={}, use_scaled_pos_enc=o["use_scaled_pos_enc"], encoder="transformer",
                              encoder_conf=enc, decoder=o["decoder"], decoder_conf=decc, model_conf=mc, init=None)


def _state(case):
    return {k: v.detach() for k, v in R.procedural(case).items()}


def _model(case, compute="f32", dropout=False):
    from a3t_amd.task import MLMTask
    m = MLMTask.build_model(_task_args(case, dropout), device=DEV, compute=compute)
    m.load_state_dict(_state(case))
    return m


def _engine(case, compute="f32", training=True, dropout=False):
    from a3t_amd.engine import MLMEngine
    m = _model(case)
    return MLMEngine(m.cfg, m.store, compute=compute, training=training, dropout=dropout), m.store


def _check_grads(grads, g):
    n = 0
    for k, ref in g.items():
        if k.startswith("grad."):
            got = grads[k[5:]].cpu().numpy().reshape(ref.shape)
            np.testing.assert_allclose(got, ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=5e-3, err_msg=k[5:])
            n += 1
    assert n == len(grads)


# ---------------------------------------------------------------- softmax without a positional term
# (B, H, T, valid keys per row): T = 40 / 200 / 520 / 1200 walk the register-resident instantiations, 2100 the three-pass one (and, not
# a multiple of 8, the scalar kernel in bf16 too); a fully masked row; one row with a single key
SM_CASES = [(1, 1, 40, [37]), (3, 2, 200, [200, 131, 0]), (2, 1, 520, [520, 1]), (1, 2, 1200, [1111]), (1, 1, 2100, [2099])]


def _scores(B, H, T, lens, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    ac = (3.0 * torch.randn(B, H, T, T, generator=gen)).to(dtype).to(DEV)
    km = torch.zeros(B, T, dtype=torch.uint8)
    for b, n in enumerate(lens):
        km[b, :n] = 1
    return ac, km.to(DEV)


def _softmax64(ac, km, scale):
    s = ac.double() * scale
    dead = (km == 0)[:, None, None, :]
    s = s.masked_fill(dead, -1e300)
    p = torch.softmax(s, dim=-1).masked_fill(dead, 0.0)
    return torch.where(dead.expand_as(p).all(-1, keepdim=True), torch.zeros_like(p), p)


@pytest.mark.parametrize("B,H,T,lens", SM_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_softmax_plain_against_float64_and_the_zero_table_launch(B, H, T, lens, dtype):
    """Forward and backward against the float64 formula, and bit for bit against the existing kernels fed an all-zero bd (every
    positional term is then + 0.0f).  fp32: 2^-20 covers expf and the row sum to a few ulps; bf16 probabilities round at 2^-9."""
    from a3t_amd import ops
    scale = 1.0 / math.sqrt(24.0)
    ac, km = _scores(B, H, T, lens, 100 + T, dtype)
    probs = torch.full_like(ac, float("nan"))
    ops.softmax_plain_fwd(ac, km, probs, B, H, T, scale)
    ref = _softmax64(ac, km, scale)
    tol = 2.0 ** -20 if dtype == torch.float32 else 2.0 ** -8
    assert float((probs.double() - ref).abs().max()) <= tol
    bd = torch.zeros_like(ac)
    old = torch.full_like(ac, float("nan"))
    ops.relpos_softmax_fwd(ac, bd, km, old, B, H, T, scale)
    assert torch.equal(probs, old)
    # backward: ds = p * (dp - sum_j dp p) * scale
    dp = torch.randn(B, H, T, T, generator=torch.Generator().manual_seed(7)).to(dtype).to(DEV)
    ds = torch.full_like(ac, float("nan"))
    ops.softmax_plain_bwd(probs, dp, ds, B, H, T, scale)
    p64, d64 = probs.double(), dp.double()
    want = p64 * (d64 - (p64 * d64).sum(-1, keepdim=True)) * scale
    mag = float((p64 * d64.abs()).sum(-1).max()) * scale + 1e-30
    assert float((ds.double() - want).abs().max()) <= (2.0 ** -20 if dtype == torch.float32 else 2.0 ** -7) * max(mag, 1.0)
    ds_old, dbd = torch.full_like(ac, float("nan")), torch.empty_like(ac)
    ops.relpos_softmax_bwd(probs, dp, ds_old, dbd, B, H, T, scale)
    assert torch.equal(ds, ds_old)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_softmax_plain_dropout_is_the_mask_of_the_existing_kernel(dtype):
    from a3t_amd import ops
    B, H, T, lens = 2, 2, 136, [136, 97]
    scale, drop = 0.25, (0.2, 424242)
    ac, km = _scores(B, H, T, lens, 5, dtype)
    p, pd, q, qd = (torch.full_like(ac, float("nan")) for _ in range(4))
    ops.softmax_plain_fwd(ac, km, p, B, H, T, scale, probs_drop=pd, drop=drop)
    ops.relpos_softmax_fwd(ac, torch.zeros_like(ac), km, q, B, H, T, scale, probs_drop=qd, drop=drop)
    assert torch.equal(p, q) and torch.equal(pd, qd)
    kept = float((pd[0, :, :, :] != 0).float().mean())
    assert 0.7 < kept < 0.9                      # (row 0 has no masked key: 1 - p of its probabilities survive)
    dp = torch.randn(B, H, T, T, generator=torch.Generator().manual_seed(9)).to(dtype).to(DEV)
    ds, ds_old, dbd = torch.full_like(ac, float("nan")), torch.full_like(ac, float("nan")), torch.empty_like(ac)
    ops.softmax_plain_bwd(p, dp, ds, B, H, T, scale, probs_drop=pd, drop_p=drop[0])
    ops.relpos_softmax_bwd(p, dp, ds_old, dbd, B, H, T, scale, probs_drop=pd, drop_p=drop[0])
    assert torch.equal(ds, ds_old) and bool(torch.isfinite(ds.float()).all())


# ---------------------------------------------------------------- absolute positions in the prologue and at the decoder entry
PRO_SHAPES = [(3, 37, 5, 32), (2, 136, 16, 384), (3, 37, 5, 384), (2, 136, 16, 32)]


def _prologue_inputs(B, Tm, Tp, d, seed):
    from a3t_amd.config import A3TConfig
    from a3t_amd.conformer import legacy_pe_table
    V, nseg = 48, 500
    gen = torch.Generator().manual_seed(seed)
    t = dict(e=torch.randn(B * Tm, d, generator=gen), temb=torch.randn(V, d, generator=gen),
             text=torch.randint(0, V, (B, Tp), generator=gen), spos=torch.randint(0, nseg, (B, Tm), generator=gen),
             tpos=torch.randint(0, nseg, (B, Tp), generator=gen), seg=torch.randn(nseg, d, generator=gen),
             spk=torch.randn(B, d, generator=gen), g=torch.randn(B * (Tm + Tp), d, generator=gen),
             pe=legacy_pe_table(A3TConfig(adim=d, heads=2, max_len=200)).flip(0).contiguous(),
             a_s=torch.tensor([1.3]), a_t=torch.tensor([0.7]))
    return {k: v.to(DEV) for k, v in t.items()}, V, nseg


def _keep_mask(n, drop):
    """The counter RNG's keep mask over n elements (the element index is the dropout site's own)."""
    from a3t_amd import ops
    one, out = torch.ones(n, device=DEV), torch.empty(n, device=DEV)
    ops.dropout(one, out, drop[0], drop[1])
    return out != 0


@pytest.mark.parametrize("B,Tm,Tp,d", PRO_SHAPES)
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("drop", [(0.0, 0), (0.25, 1234567)])
def test_embed_finish_abs_forward_and_alpha_gradients_against_float64(B, Tm, Tp, d, scaled, drop):
    """Forward to fp32 rounding of its operations, elementwise.  Alpha gradients against the float64 sum, within the length of
    the longest chain of fp32 additions times 2^-24 of the sum of magnitudes; the same bits on two runs."""
    from a3t_amd import ops
    t, V, nseg = _prologue_inputs(B, Tm, Tp, d, 11 + Tm + d)
    T = Tm + Tp
    xs = torch.full((B * T + 1, d), float("nan"), device=DEV)
    alpha = (t["a_s"], t["a_t"]) if scaled else None
    xscale = math.sqrt(d)
    ops.embed_finish_abs_fwd(t["e"], t["temb"], t["seg"], t["text"], t["spos"], t["tpos"], t["pe"], alpha, xs, B, Tm, Tp, d, xscale,
                             drop=drop, spk=t["spk"])
    assert bool(torch.isnan(xs[-1]).all())          # (one row behind the end stays untouched)
    D = {k: v.double() for k, v in t.items() if v.is_floating_point()}
    a_s, a_t, xsc = (1.3, 0.7, 1.0) if scaled else (1.0, 1.0, float(np.float32(xscale)))
    a_s, a_t = float(np.float32(a_s)), float(np.float32(a_t))
    sp = torch.relu(D["e"]).view(B, Tm, d) * xsc
    tx = D["temb"][t["text"]] * xsc
    pos_s, pos_t = a_s * D["pe"][:Tm], a_t * D["pe"][:Tp]
    v = torch.cat([sp + pos_s, tx + pos_t], dim=1)
    mag = torch.cat([sp.abs() + pos_s.abs(), tx.abs() + pos_t.abs()], dim=1)
    keep = torch.ones(B, T, d, dtype=torch.bool, device=DEV)
    inv = 1.0
    if drop[0] > 0:
        keep = _keep_mask(B * T * d, drop).view(B, T, d)
        inv = float(np.float32(1.0) / np.float32(1.0 - np.float32(drop[0])))
        v, mag = torch.where(keep, v * inv, torch.zeros_like(v)), mag * inv
    add = torch.cat([D["seg"][t["spos"]], D["seg"][t["tpos"]]], dim=1) + D["spk"][:, None, :]
    addmag = torch.cat([D["seg"][t["spos"]], D["seg"][t["tpos"]]], dim=1).abs() + D["spk"][:, None, :].abs()
    want = v + add
    err = (xs[:-1].view(B, T, d).double() - want).abs()
    assert bool((err <= 6 * 2.0 ** -24 * (mag + addmag)).all()), float(err.max())      # (six roundings, each on at most mag + addmag)
    # ---- backward
    g = t["g"]
    runs = []
    for _ in range(2):
        de = torch.full((B * Tm, d), float("nan"), device=DEV)
        dt, dseg = torch.zeros(V, d, device=DEV), torch.zeros(nseg, d, device=DEV)
        da_s, da_t = torch.full((1,), 0.5, device=DEV), torch.full((1,), -0.25, device=DEV)       # accumulated into
        part = torch.empty(ops.embed_finish_abs_partials(B, Tm, Tp, d), device=DEV)
        ops.embed_finish_abs_bwd(g, t["e"], t["text"], t["spos"], t["tpos"], t["pe"], de, dt, dseg,
                                 (da_s, da_t) if scaled else None, part if scaled else None, B, Tm, Tp, d, V, nseg, xscale, drop=drop)
        runs.append((de, dt, da_s.clone(), da_t.clone()))
    gd = torch.where(keep, g.view(B, T, d).double() * inv, torch.zeros(1, dtype=torch.float64, device=DEV))
    de64 = torch.where(D["e"].view(B, Tm, d) > 0, gd[:, :Tm] * xsc, torch.zeros(1, dtype=torch.float64, device=DEV))
    assert float((runs[0][0].view(B, Tm, d).double() - de64).abs().max()) <= 2.0 ** -22 * float(de64.abs().max())
    dt64 = torch.zeros(V, d, dtype=torch.float64, device=DEV).index_add_(0, t["text"].reshape(-1), (gd[:, Tm:] * xsc).reshape(-1, d))
    dt64[V - 1] = 0                                 # padding_idx = -1
    assert float((runs[0][1].double() - dt64).abs().max()) <= 2.0 ** -20 * max(float(dt64.abs().max()), 1.0)
    assert torch.equal(runs[0][0], runs[1][0])
    if not scaled:
        assert float(runs[0][2]) == 0.5 and float(runs[0][3]) == -0.25          # untouched without alphas
        return
    nb = ops.embed_finish_abs_partials(B, Tm, Tp, d) // 2
    chain = -(-(B * T * d) // (nb * 256)) + 6 + 3 + -(-nb // 256) + 8 + 2      # per thread, wave, workgroup, fold thread, fold tree, product and +=
    for got, terms, start in ((runs[0][2], gd[:, :Tm] * D["pe"][:Tm], 0.5), (runs[0][3], gd[:, Tm:] * D["pe"][:Tp], -0.25)):
        want = float(terms.sum()) + start
        bound = chain * 2.0 ** -24 * (float(terms.abs().sum()) + abs(start))
        print(f"dalpha {float(got):.7f} want {want:.7f} distance {abs(float(got) - want):.3e} bound {bound:.3e}")
        assert abs(float(got) - want) <= bound
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])


def test_embed_finish_abs_text_positions_restart_at_zero():
    """With e = 0 and a zero embedding the output IS the table: rows 0..Tm-1, then rows 0..Tp-1 again."""
    from a3t_amd import ops
    B, Tm, Tp, d = 2, 37, 5, 32
    t, V, nseg = _prologue_inputs(B, Tm, Tp, d, 3)
    xs = torch.empty(B * (Tm + Tp), d, device=DEV)
    ops.embed_finish_abs_fwd(torch.zeros_like(t["e"]), torch.zeros_like(t["temb"]), None, t["text"], t["spos"], t["tpos"], t["pe"],
                             None, xs, B, Tm, Tp, d, math.sqrt(d))
    xs = xs.view(B, Tm + Tp, d)
    for b in range(B):
        assert torch.equal(xs[b, :Tm], t["pe"][:Tm]) and torch.equal(xs[b, Tm:], t["pe"][:Tp])


@pytest.mark.parametrize("B,T,d", [(3, 42, 32), (2, 152, 384)])
@pytest.mark.parametrize("drop", [(0.0, 0), (0.25, 99)])
def test_scale_add_pos_against_float64(B, T, d, drop):
    from a3t_amd import ops
    t, _, _ = _prologue_inputs(B, T, 0, d, 5)
    x = t["g"]
    y = torch.full((B * T + 1, d), float("nan"), device=DEV)
    s = math.sqrt(d)
    ops.scale_add_pos(x, t["pe"], y, B, T, d, s, drop=drop)
    assert bool(torch.isnan(y[-1]).all())
    want = x.view(B, T, d).double() * float(np.float32(s)) + t["pe"][:T].double()
    mag = x.view(B, T, d).double().abs() * s + t["pe"][:T].double().abs()
    if drop[0] > 0:
        keep = _keep_mask(B * T * d, drop).view(B, T, d)
        inv = float(np.float32(1.0) / np.float32(1.0 - np.float32(drop[0])))
        want, mag = torch.where(keep, want * inv, torch.zeros_like(want)), mag * inv
        # its backward is a3t_dropout's scaled form with the same key: the same mask
        gb = torch.empty(B * T, d, device=DEV)
        ops.dropout(torch.ones(B * T, d, device=DEV), gb, drop[0], drop[1], scale=s)
        assert torch.equal(gb.view(B, T, d) != 0, keep)
    err = (y[:-1].view(B, T, d).double() - want).abs()
    assert bool((err <= 3 * 2.0 ** -24 * mag).all()), float(err.max())


# ---------------------------------------------------------------- fp32 engine against the reference's records
@pytest.mark.parametrize("case", CASES)
def test_fp32_engine_against_reference_golden(case):
    """Bounds of test_gpu_e2e.py::test_e2e_tiny_against_reference_golden, for the loss, both outputs and every gradient."""
    g = R.load_golden(case)
    c, batch = R.tiny_batch(case)
    eng, store = _engine(case)
    assert set(store.state_dict()) == set(R.golden_keys(case))
    out = eng.forward(_dev(batch))
    ref = _f(g["loss"])
    print(f"{case}: loss {float(out['loss']):.6f} reference {ref:.6f}")
    assert abs(float(out["loss"]) - ref) < 1e-4 * abs(ref)
    np.testing.assert_allclose(out["before"].cpu().numpy(), g["before"], atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["after"].cpu().numpy(), g["after"], atol=2e-4, rtol=1e-4)
    store.zero_grad()
    eng.backward()
    grads = store.state_dict(grads=True)
    _check_grads(grads, g)
    if R.options(case)["use_scaled_pos_enc"]:
        for k in R.ALPHAS:
            print(f"{k}: gradient {float(grads[k]):.7f} reference {_f(g['grad.' + k]):.7f}")
    eng_e, _ = _engine(case, training=False)
    le = float(eng_e.forward(_dev(batch), need_grad=False)["loss"])
    assert abs(le - _f(g["loss_eval"])) < 1e-4 * abs(_f(g["loss_eval"]))
    Tm, Tp = batch["speech"].shape[1], batch["text"].shape[1]
    n_enc = R.options(case)["enc_blocks"]
    assert [eng.block_dims[f"enc.{i}"] for i in range(n_enc)] == [(2, Tm + Tp)] * n_enc
    assert ("dec.0" in eng.block_dims) == (R.options(case)["decoder"] != "no_decoder")
    assert set(eng.attn_path.values()) == {"mat"}


@pytest.mark.parametrize("case", CASES)
def test_inference_splice_against_reference_golden(case):
    g = R.load_golden(case)
    _, batch = R.tiny_batch(case)
    m = _model(case).eval()
    with torch.no_grad():
        out = m.inference(**{k: v[:1] for k, v in batch.items()}, span_boundary=[10, 30], use_teacher_forcing=True)
    fg = out["feat_gen"]
    sp = torch.cat([fg[0][0], fg[1], fg[2][0]], dim=0).cpu().numpy()
    np.testing.assert_allclose(sp, g["infer_splice"], atol=2e-4, rtol=1e-3)
    res, lens = m.inference_batch(**{k: v[:1] for k, v in batch.items()}, span_boundary=[[10, 30]])
    np.testing.assert_allclose(res[0, :int(lens[0])].cpu().numpy(), g["infer_splice"], atol=2e-4, rtol=1e-3)
    with pytest.raises(NotImplementedError, match="rows='alone'"):
        m.inference_batch(**batch, span_boundary=[[10, 30], [5, 9]], rows="alone")


def test_plugin_model_backward_leaves_reference_gradients():
    g = R.load_golden("b")
    _, batch = R.tiny_batch("b")
    m = _model("b").train()
    loss, stats, weight = m(**batch)
    assert abs(float(loss) - _f(g["loss"])) < 1e-4 * abs(_f(g["loss"])) and int(weight) == 2
    loss.backward()
    for n, p in m._params.items():
        assert p.grad is not None, n
    _check_grads(m.store.state_dict(grads=True), g)


# ---------------------------------------------------------------- the other compute modes, dropout
def _step(eng, store, batch):
    store.zero_grad()
    loss = float(eng.forward(batch)["loss"])
    eng.backward()
    torch.cuda.synchronize()
    return loss, store.grad.clone()


@pytest.mark.parametrize("case", CASES)
def test_bf16_tracks_fp32_tiny(case):
    """The project's bf16 bounds (loss 1e-2, gradient cosine >= 0.99) at the tiny size, fixture weights and batch (T_mel = 48,
    T = 56); d_k = 16 is outside the fused kernels' shapes, so this is the materialised path with bf16 scores."""
    from a3t_amd.engine import MLMEngine
    _, batch = R.tiny_batch(case)
    batch = _dev(batch)
    eng, store = _engine(case, compute="bf16")
    l16, g16 = _step(eng, store, batch)
    l32, g32 = _step(MLMEngine(eng.c, store, compute="f32", training=True), store, batch)
    cos = float(torch.nn.functional.cosine_similarity(g16, g32, dim=0))
    print(f"bf16 against fp32 ({case}, tiny): loss {l16:.6f} / {l32:.6f}, gradient cosine {cos:.6f}")
    assert abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert bool(torch.isfinite(g16).all()) and cos >= 0.99, cos
    assert set(eng.attn_path.values()) == {"mat"}


def test_bf16_tracks_fp32_adim64_ragged_lengths():
    """A restated model at adim 64, 2 heads, T_mel = 120, T_phn = 16 (T = 136) with a row of 97 tokens' worth of valid keys, xavier
    weights: the same bounds."""
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.config import A3TConfig
    from a3t_amd.engine import MLMEngine
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    c = A3TConfig(adim=64, heads=2, ff=128, ff_kernel=3, enc_blocks=2, dec_blocks=1, postnet_layers=2, postnet_chans=16, vocab=40,
                  block="transformer", scaled_pos=True)
    store = ParamStore(c, DEV)
    xavier_init_(store, seed=3, bn_gamma=1.0)
    store.p["emb.alpha_s"].fill_(1.3)
    batch = synthetic_batch(c, 3, 120, 16, seed=21, device=DEV)
    batch["speech_mask"][1, ..., 85:] = False           # 85 + 12 = 97 valid keys in row 1
    batch["text_mask"][1, ..., 12:] = False
    batch["masked_position"][1, 85:] = False
    l16, g16 = _step(MLMEngine(c, store, compute="bf16", training=True, dropout=False), store, batch)
    l32, g32 = _step(MLMEngine(c, store, compute="f32", training=True, dropout=False), store, batch)
    cos = float(torch.nn.functional.cosine_similarity(g16, g32, dim=0))
    print(f"bf16 against fp32 (adim 64, T 136): loss {l16:.6f} / {l32:.6f}, gradient cosine {cos:.6f}")
    assert abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert bool(torch.isfinite(g16).all()) and cos >= 0.99, cos


def test_bf16x3_is_closer_to_fp32_than_bf16():
    """tests/test_gpu_bf16x3_model.py::test_one_training_step_runs on case b: |loss - f32| of bf16x3 within 1/64 of bf16's."""
    from a3t_amd.engine import MLMEngine
    _, batch = R.tiny_batch("b")
    batch = _dev(batch)
    eng, store = _engine("b")
    loss = {}
    for compute in ("f32", "bf16", "bf16x3"):
        loss[compute], g = _step(MLMEngine(eng.c, store, compute=compute, training=True), store, batch)
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    d16, d3 = abs(loss["bf16"] - loss["f32"]), abs(loss["bf16x3"] - loss["f32"])
    print(f"loss f32 {loss['f32']:.7f} bf16 {loss['bf16']:.7f} bf16x3 {loss['bf16x3']:.7f}")
    assert d3 <= d16 / 64 + 2.0 ** -22 * abs(loss["f32"]), (d3, d16)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_dropout_step_is_a_function_of_the_step_seed(compute):
    """Dropout on (every rate 0.2): the same step seed gives the same masks, another seed another loss; every parameter receives a
    finite gradient, and with dropout the bias gradients come from the masked gradients (no parameter is left at zero but the
    padding rows)."""
    _, batch = R.tiny_batch("b")
    batch = _dev(batch)
    eng, store = _engine("b", compute=compute, dropout=True)
    assert eng.dropping
    la, ga = _step(eng, store, batch)
    eng.step_seed -= 1
    lb, gb = _step(eng, store, batch)
    # (the forward is deterministic; weight gradients add their split-K partials with fp32 atomics, whose order is free: a few
    #  fp32 roundings of sums of at most some hundred terms, 2^-16 of the largest gradient with room to spare)
    assert la == lb and float((ga - gb).abs().max()) <= 2.0 ** -16 * float(ga.abs().max())
    lc, gc = _step(eng, store, batch)
    assert lc != la and float((gc - ga).abs().max()) > 1e-3 * float(ga.abs().max())
    for k, v in store.state_dict(grads=True).items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    # without dropout the same engine class gives the reference's loss: the sites are the only difference
    e0, s0 = _engine("b", compute=compute, dropout=False)
    l0, _ = _step(e0, s0, batch)
    assert l0 != la and abs(l0 - la) < 0.5 * abs(l0)


# ---------------------------------------------------------------- hooks and buckets, checkpoints, the speech editor
def test_overlapped_allreduce_hooks_single_rank():
    """test_gpu_mlm_variants.py::test_overlapped_allreduce_hooks_single_rank on a 2 + 2 transformer model: the bucket boundaries
    are the blocks' first parameters, the hooks come in backward order, two steps equal the non-overlapped trainer's."""
    import torch.distributed as dist
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.config import A3TConfig
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    from a3t_amd.trainer import A3TTrainer
    c = A3TConfig(adim=128, heads=2, ff=256, ff_kernel=3, enc_blocks=2, dec_blocks=2, postnet_layers=3, postnet_chans=64, vocab=40,
                  block="transformer", scaled_pos=True)
    batch = synthetic_batch(c, 4, 192, 32, seed=7, device=DEV)
    hooks = []

    def run(with_group):
        store = ParamStore(c, DEV)
        xavier_init_(store, seed=3, bn_gamma=1.0)
        tr = A3TTrainer(c, store, compute="bf16", lr=1.0, warmup_steps=10, dropout=True, force_reducer=with_group,
                        bucket_min_elems=100_000)
        if with_group:
            assert tr.reducer is not None and len(tr.reducer.ranges) >= 3
            lows = {lo for lo, _ in tr.reducer.ranges}
            assert 0 in lows and any(store.offsets[f"enc.{i}.mha.ln.g"][0] in lows for i in range(2))
            assert sum(hi - lo for lo, hi in tr.reducer.ranges) == store.total
            orig = tr.engine.backward
            tr.engine.backward = lambda on_group_done=None: orig(
                on_group_done=lambda n: (hooks.append(n), on_group_done(n))[1])
        l1 = float(tr.step(batch))
        torch.cuda.synchronize()
        g1 = store.grad.clone()
        l2 = float(tr.step(batch))
        torch.cuda.synchronize()
        return (l1, l2), g1, store

    ref_l, ref_g, _ = run(False)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29537")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
    try:
        got_l, got_g, store = run(True)
    finally:
        dist.destroy_process_group()
    one = ["sfc.w"] + [f"dec.{i}.mha.ln.g" for i in (1, 0)] + [f"enc.{i}.mha.ln.g" for i in (1, 0)] + ["seg"]
    assert hooks == one + one, hooks
    assert abs(got_l[0] - ref_l[0]) < 1e-5 * abs(ref_l[0])
    assert abs(got_l[1] - ref_l[1]) < 2e-3 * abs(ref_l[1])
    err = float((got_g - ref_g).abs().max() / ref_g.abs().max())
    assert err < 2e-4, err
    assert float(store.g["emb.alpha_s"].abs()) > 0 and float(store.g["emb.alpha_t"].abs()) > 0


def test_checkpoint_save_resume_and_average(tmp_path):
    from a3t_amd import checkpoint as ck
    from a3t_amd.trainer import A3TTrainer
    _, batch = R.tiny_batch("b")
    batch = _dev(batch)
    m = _model("b").train()
    tr = A3TTrainer(m.cfg, m.store, compute="f32", lr=1.0, warmup_steps=10, dropout=False)
    rep = ck.EpochReport()
    for e, vloss in ((1, 3.0), (2, 2.0)):
        tr.step(batch)
        rep.set_epoch(e)
        rep.register("valid", {"loss": vloss})
        ck.save_checkpoint(tmp_path, m, rep, e, trainer=tr)
    ck.average_nbest_models(tmp_path, rep, [("valid", "loss", "min")], 2)
    avg = torch.load(tmp_path / "valid.loss.ave_2best.pth", map_location="cpu")
    e1, e2 = (torch.load(tmp_path / f"{e}epoch.pth", map_location="cpu") for e in (1, 2))
    assert set(avg) == set(R.golden_keys("b"))
    for k in ("encoder.encoders.1.self_attn.linear_q.weight", "encoder.speech_embed.4.alpha", "encoder.text_embed.1.alpha"):
        assert torch.equal(avg[k], (e2[k] + e1[k]) / 2) and not torch.equal(e1[k], e2[k]), k        # (the optimizer moved the alphas)
    m2 = _model("b").train()
    tr2 = A3TTrainer(m2.cfg, m2.store, compute="f32", lr=1.0, warmup_steps=10, dropout=False)
    rep2 = ck.EpochReport()
    ck.resume(tmp_path / "checkpoint.pth", m2, rep2, trainer=tr2)
    assert rep2.get_epoch() == 2 and torch.equal(m2.store.flat, m.store.flat) and torch.equal(tr2.m, tr.m)
    la, lb = float(tr.step(batch)), float(tr2.step(batch))
    assert abs(la - lb) <= 1e-6 * abs(la), (la, lb)


def test_speech_editor_on_a_transformer_model_against_inference_per_request():
    """SpeechEditor.edit unchanged on a transformer model: what it returns is the model's inference() of the batch it collated,
    and that is the restatement's splice of the same batch."""
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import SpeechEditor
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden import fake_phone_duration
    oc = O.tiny_config()
    m = _model("b").eval()
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    seen = []
    orig = m.inference
    m.inference = lambda *a, **k: (seen.append((a, k)), orig(*a, **k))[1]
    ed = SpeechEditor(m, coll, None, ids, fake_phone_duration)
    fx = json.load(open(os.path.join(G, "sedit.json")))
    waves = np.load(os.path.join(G, "sedit_wav.npz"))
    for kind in ("replace", "insert"):
        case = [c for c in fx["cases"] if c["kind"] == kind][0]
        n = waves[case["wav"] + ".in"].shape[0]
        wav = (0.1 * np.random.RandomState(5).standard_normal(n)).astype(np.float32)
        del seen[:]
        res = ed.edit(wav, case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"],
                      case["new_str"], **case["opts"])
        assert tuple(res["new_span_boundary"]) == tuple(case["plan"]["new_span_boundary"])
        assert len(seen) == 1
        a, k = seen[0]
        fg = orig(*a, **k)["feat_gen"]
        alone = torch.cat([fg[0][0], fg[1], fg[2][0]], dim=0)
        feat = torch.as_tensor(res["feat"]).to(alone.device)
        assert feat.shape == alone.shape and torch.equal(feat, alone)
        names = ("speech", "text", "masked_position", "speech_mask", "text_mask", "speech_segment_pos", "text_segment_pos")
        b = {n: (k[n] if n in k else a[names.index(n)]).cpu() for n in names}
        s, e = (int(x) for x in k["span_boundary"])
        with torch.no_grad():
            want = R.model_splice(R.procedural("b"), b, oc, (s, e))
        np.testing.assert_allclose(alone.cpu().numpy(), want.numpy(), atol=2e-4, rtol=1e-3)
