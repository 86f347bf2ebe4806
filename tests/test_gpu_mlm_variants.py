"""The model variants MLMTask builds besides the recipe's on the device -- input_layer 'mlm' (a), pre_speech_layer 2 (b),
no_decoder (c), mlm + pre_speech_layer 1 + no_decoder (d): the fp32 engine against the reference's own records
(tests/golden/mlm_variants*.npz), the bf16 engine against the fp32 engine, the overlapped all-reduce hooks, the model
surface (state dict, checkpoint, speech editor) and the two concatenation kernels / the null-segment prologue bit for bit."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import mlm_variants_ref as R
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
CASES = sorted(R.CASES)


def _f(x):
    return float(np.asarray(x).reshape(-1)[0])


def _cfg(case, oc=None, **kw):
    from a3t_amd.config import A3TConfig
    oc = oc or O.tiny_config()
    seg, pre, dec = R.CASES[case]
    c = A3TConfig(**{k: getattr(oc, k) for k in ("idim", "odim", "vocab", "adim", "heads", "ff", "ff_kernel", "enc_blocks",
                                                  "dec_blocks", "enc_kernel", "dec_kernel", "postnet_layers", "postnet_chans",
                                                  "postnet_filts", "max_len", "seg_table", "lsm_weight")},
                  segment_emb=seg, pre_blocks=pre, has_decoder=dec)
    if not dec:
        c.dec_blocks = 0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _state(case, seed=R.SEED_W):
    return {k: torch.from_numpy(np.array(v)) for k, v in O.procedural_state(R.golden_keys(case), seed).items()}


def _engine(case, compute="f32", training=True):
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    c = _cfg(case)
    store = ParamStore(c, DEV)
    store.load_state_dict(_state(case))
    return MLMEngine(c, store, compute=compute, training=training), store


def _dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _task_args(case, oc=None):
    oc = oc or O.tiny_config()
    seg, pre, dec = R.CASES[case]
    enc = dict(input_layer="sega_mlm" if seg else "mlm", pre_speech_layer=pre, cnn_module_kernel=oc.enc_kernel,
               attention_dim=oc.adim, attention_heads=oc.heads, linear_units=oc.ff, num_blocks=oc.enc_blocks,
               macaron_style=True, use_cnn_module=True, selfattention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos",
               positionwise_layer_type="conv1d", positionwise_conv_kernel_size=3)
    decc = dict(cnn_module_kernel=oc.dec_kernel, attention_dim=oc.adim, attention_heads=oc.heads, linear_units=oc.ff,
                num_blocks=oc.dec_blocks, selfattention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos")
    mc = dict(lsm_weight=0.1, mean_phn_span=8, mlm_prob=0.8, postnet_layers=oc.postnet_layers, postnet_filts=5,
              postnet_chans=oc.postnet_chans, dropout=False)
    toks = ["<blank>", "<unk>", "<space>"] + [f"t{i}" for i in range(oc.vocab - 4)] + ["<sos/eos>"]
    return argparse.Namespace(token_list=toks, odim=80, input_size=80, feats_extract="fbank",
                              feats_extract_conf=dict(n_fft=2048, hop_length=300, win_length=1200, fs=24000, fmin=80,
                                                      fmax=7600, n_mels=80),
                              normalize=None, normalize_conf={}, encoder="conformer", encoder_conf=enc,
                              decoder="conformer" if dec else "no_decoder", decoder_conf=decc, model_conf=mc, init=None)


def _model(case, compute="f32"):
    from a3t_amd.task import MLMTask
    m = MLMTask.build_model(_task_args(case), device=DEV, compute=compute)
    m.load_state_dict(_state(case))
    return m


def _check_grads(grads, g):
    n = 0
    for k, ref in g.items():
        if k.startswith("grad."):
            got = grads[k[5:]].cpu().numpy()
            np.testing.assert_allclose(got, ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=5e-3, err_msg=k[5:])
            n += 1
    assert n == len(grads)


# ---------------------------------------------------------------- fp32 engine against the reference's records
@pytest.mark.parametrize("case", CASES)
def test_fp32_engine_against_reference_golden(case):
    """Bounds of test_gpu_e2e.py::test_e2e_tiny_against_reference_golden."""
    g = R.load_golden(case)
    c, batch = R.tiny_batch(case)
    eng, store = _engine(case)
    assert set(store.state_dict()) == set(R.golden_keys(case))
    out = eng.forward(_dev(batch))
    ref = _f(g["loss"])
    assert abs(float(out["loss"]) - ref) < 1e-4 * abs(ref)
    np.testing.assert_allclose(out["before"].cpu().numpy(), g["before"], atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["after"].cpu().numpy(), g["after"], atol=2e-4, rtol=1e-4)
    store.zero_grad()
    eng.backward()
    _check_grads(store.state_dict(grads=True), g)
    sd = store.state_dict()
    nbuf = 0
    for k in g:
        if k.startswith("buf.") and "running" in k:
            np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), g[k], atol=1e-5, rtol=1e-4, err_msg=k)
            nbuf += 1
    assert nbuf == 2 * (c.postnet_layers + sum(1 for k in store.buf if k.endswith("cnv.bn.rm")))
    eng_e, _ = _engine(case, training=False)
    le = float(eng_e.forward(_dev(batch), need_grad=False)["loss"])
    assert abs(le - _f(g["loss_eval"])) < 1e-4 * abs(_f(g["loss_eval"]))
    # the blocks ran at the shape the reference runs them at
    Tm, Tp = batch["speech"].shape[1], batch["text"].shape[1]
    for i in range(R.CASES[case][1]):
        assert eng.block_dims[f"pre.{i}"] == (2, Tm)
    assert eng.block_dims["enc.0"] == (2, Tm + Tp)
    assert ("dec.0" in eng.block_dims) == R.CASES[case][2]


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
    # the batched infill goes through the same engine
    res, lens = m.inference_batch(**{k: v[:1] for k, v in batch.items()}, span_boundary=[[10, 30]])
    np.testing.assert_allclose(res[0, :int(lens[0])].cpu().numpy(), g["infer_splice"], atol=2e-4, rtol=1e-3)


def test_segment_ids_are_not_read_without_table():
    c, batch = R.tiny_batch("a")
    eng, _ = _engine("a")
    l0 = eng.forward(_dev(batch))["loss"].clone()
    rs = np.random.RandomState(5)
    b2 = dict(batch)
    # any ids, also ones no 500-row table could serve: the kernels must not look at them
    b2["speech_segment_pos"] = torch.from_numpy(rs.randint(0, 1 << 40, size=tuple(batch["speech_segment_pos"].shape)))
    b2["text_segment_pos"] = torch.from_numpy(rs.randint(0, 1 << 40, size=tuple(batch["text_segment_pos"].shape)))
    out = eng.forward(_dev(b2))
    assert torch.equal(out["loss"], l0)
    eng.store.zero_grad()
    eng.backward()
    assert bool(torch.isfinite(eng.store.grad).all())


def test_plugin_model_backward_leaves_reference_gradients():
    g = R.load_golden("d")
    _, batch = R.tiny_batch("d")
    m = _model("d").train()
    assert m.encoder.segment_emb is None and m.encoder.pre_speech_layer == 1 and m.decoder is None
    loss, stats, weight = m(**batch)
    assert abs(float(loss) - _f(g["loss"])) < 1e-4 * abs(_f(g["loss"])) and int(weight) == 2
    loss.backward()
    for n, p in m._params.items():
        assert p.grad is not None, n
        assert p.grad.data_ptr() == m.store.g[n].data_ptr() or torch.equal(p.grad, m.store.g[n]), n
    _check_grads(m.store.state_dict(grads=True), g)


def test_xvector_add_with_pre_speech_blocks_against_the_restatement():
    """spk_embed_dim > 0 with pre-speech blocks: the projected x-vector is added at the prologue (the pre blocks see it) and its
    gradient sums the speech-side and the text-side gradients.  No reference behaviour: the restatement's autograd is the
    yardstick, within the bounds of the fixtures' comparison."""
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    c = _cfg("d", spk_embed_dim=8)
    keys = dict(R.golden_keys("d"), **{"spk_proj.weight": (c.adim, 8), "spk_proj.bias": (c.adim,)})
    state = O.procedural_state(keys, seed=5)
    oc, batch = R.tiny_batch("d")
    batch["spembs"] = torch.from_numpy(np.random.RandomState(2).standard_normal((2, 8)).astype(np.float32))
    p = O.to_torch_state(state, requires_grad=True)
    loss, before, _ = R.variant_loss(p, batch, oc, "d")
    loss.backward()
    store = ParamStore(c, DEV)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    eng = MLMEngine(c, store, compute="f32", training=True)
    out = eng.forward(_dev(batch))
    assert abs(float(out["loss"]) - float(loss.detach())) < 1e-4 * abs(float(loss.detach()))
    np.testing.assert_allclose(out["before"].cpu().numpy(), before.detach().numpy(), atol=2e-4, rtol=1e-4)
    store.zero_grad()
    eng.backward()
    grads = store.state_dict(grads=True)
    assert float(p["spk_proj.weight"].grad.abs().max()) > 0
    for k, t in p.items():
        if t.requires_grad:
            ref = t.grad.numpy()
            np.testing.assert_allclose(grads[k].cpu().numpy(), ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=5e-3,
                                       err_msg=k)


# ---------------------------------------------------------------- bf16 engine against the fp32 engine
def _bf16_against_fp32(c, batch, seed=3):
    from a3t_amd.engine import MLMEngine
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    store = ParamStore(c, DEV)
    xavier_init_(store, seed=seed, bn_gamma=1.0)
    eng = MLMEngine(c, store, compute="bf16", training=True, dropout=False)
    store.zero_grad()
    l16 = float(eng.forward(batch)["loss"])
    eng.backward()
    torch.cuda.synchronize()
    g16 = store.grad.clone()
    e32 = MLMEngine(c, store, compute="f32", training=True, dropout=False)
    store.zero_grad()
    l32 = float(e32.forward(batch)["loss"])
    e32.backward()
    torch.cuda.synchronize()
    g32 = store.grad.clone()
    cos = float(torch.nn.functional.cosine_similarity(g16, g32, dim=0))
    print(f"bf16 against fp32: loss {l16:.6f} / {l32:.6f} (rel {abs(l16 - l32) / abs(l32):.3e}), gradient cosine {cos:.6f}")
    assert abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert bool(torch.isfinite(g16).all())
    assert cos >= 0.99, cos
    return eng, e32


def test_bf16_tracks_fp32_tiny_d():
    """Case (d) at the tiny size with the fixture's weights and batch (T_mel = 48, T = 56: multiples of 8)."""
    from a3t_amd.engine import MLMEngine
    _, batch = R.tiny_batch("d")
    batch = _dev(batch)
    eng, store = _engine("d", compute="bf16")
    store.zero_grad()
    l16 = float(eng.forward(batch)["loss"])
    eng.backward()
    torch.cuda.synchronize()
    g16 = store.grad.clone()
    e32 = MLMEngine(eng.c, store, compute="f32", training=True)
    store.zero_grad()
    l32 = float(e32.forward(batch)["loss"])
    e32.backward()
    torch.cuda.synchronize()
    g32 = store.grad.clone()
    cos = float(torch.nn.functional.cosine_similarity(g16, g32, dim=0))
    print(f"bf16 against fp32 (d, tiny): loss {l16:.6f} / {l32:.6f}, gradient cosine {cos:.6f}")
    assert abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert bool(torch.isfinite(g16).all()) and cos >= 0.99, cos


# d = 384, H = 2 (d_k = 192), 1 pre + 1 encoder block, no decoder, T_mel = 384, T_phn = 40: pre.0 runs at T = 384 (3 query
# tiles of 128 per head), enc.0 at T = 424 (4 tiles).  The fused training forward is taken from 64 workgroups = B * H * tiles:
#   B = 4  (the issue's size): 24 / 32 workgroups, both blocks materialised;
#   B = 9 : pre.0 has 54 (materialised), enc.0 has 72 (fused): the two shapes of ONE step take different paths;
#   B = 11: 66 / 88, the smallest batch at which pre.0 takes the fused training forward.
@pytest.mark.parametrize("B,pre_path,enc_path", [(4, "mat", "mat"), (9, "mat", "train"), (11, "train", "train")])
def test_bf16_tracks_fp32_d384_attention_path_per_block_shape(B, pre_path, enc_path):
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.config import A3TConfig
    c = A3TConfig(adim=384, heads=2, enc_blocks=1, dec_blocks=0, pre_blocks=1, has_decoder=False)
    batch = synthetic_batch(c, B, 384, 40, seed=21, device=DEV)
    eng, e32 = _bf16_against_fp32(c, batch)
    assert eng.attn_path == {"pre.0": pre_path, "enc.0": enc_path}, eng.attn_path
    assert eng.block_dims == {"pre.0": (B, 384), "enc.0": (B, 424)}
    assert e32.attn_path == {"pre.0": "mat", "enc.0": "mat"}
    # the backward followed the forward: the fused training forward leaves 1 / row sum behind, the materialised one nothing
    assert ("pre.0.mha.rs" in eng.sv) == (pre_path == "train") and ("enc.0.mha.rs" in eng.sv) == (enc_path == "train")
    # the decision of the main shape stays where callers read it
    assert eng._fused_train_now == (enc_path == "train") and not eng._fused_now
    # forward only: the same shapes through the forward-only choice
    eng.forward(batch, need_grad=False)
    want = lambda p: "fwd" if p == "train" else "mat"
    assert eng.attn_path == {"pre.0": want(pre_path), "enc.0": want(enc_path)}, eng.attn_path


# ---------------------------------------------------------------- hooks and buckets
@pytest.mark.parametrize("case", ["b", "d"])
def test_overlapped_allreduce_hooks_single_rank(case):
    """test_gpu_e2e.py::test_trainer_overlapped_allreduce_plumbing_single_rank_rccl for the variants: the bucket boundaries
    include the pre.{i} groups and skip the decoder's when there is none; two steps against the non-overlapped trainer."""
    import torch.distributed as dist
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    from a3t_amd.trainer import A3TTrainer
    seg, pre, dec = R.CASES[case]
    oc = O.A3TConfig(adim=128, heads=2, ff=256, enc_blocks=2, dec_blocks=2, postnet_layers=3, postnet_chans=64, vocab=40)
    c = _cfg(case, oc)
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
            assert 0 in lows and any(store.offsets[f"pre.{i}.ffm.ln.g"][0] in lows for i in range(pre))
            assert sorted(tr.reducer.ranges, reverse=True) == tr.reducer.ranges
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
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
    try:
        got_l, got_g, store = run(True)
    finally:
        dist.destroy_process_group()
    first = next(iter(store.offsets))
    assert first == ("seg" if seg else "mask_feature")
    one = ["sfc.w"] + ([f"dec.{i}.ffm.ln.g" for i in (1, 0)] if dec else []) + [f"enc.{i}.ffm.ln.g" for i in (1, 0)] + \
        [f"pre.{i}.ffm.ln.g" for i in reversed(range(pre))] + [first]
    assert hooks == one + one, hooks
    assert abs(got_l[0] - ref_l[0]) < 1e-5 * abs(ref_l[0])
    assert abs(got_l[1] - ref_l[1]) < 2e-3 * abs(ref_l[1])
    err = float((got_g - ref_g).abs().max() / ref_g.abs().max())
    assert err < 2e-4, err
    assert float(torch.nn.functional.cosine_similarity(got_g, ref_g, dim=0)) > 0.999999


# ---------------------------------------------------------------- model surface
@pytest.mark.parametrize("case", CASES)
def test_state_dict_round_trip(case):
    m = _model(case)
    sd = m.state_dict()
    ref = _state(case)
    assert list(sd) and set(sd) == set(ref)
    for k, v in ref.items():
        assert torch.equal(sd[k].cpu(), v), k
    from a3t_amd.task import MLMTask
    m2 = MLMTask.build_model(_task_args(case), device=DEV)
    res = m2.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m2.store.flat, m.store.flat)
    with pytest.raises(RuntimeError):          # another variant's checkpoint does not load silently
        m2.load_state_dict(_state("b" if case != "b" else "c"))


def test_checkpoint_save_resume_and_average(tmp_path):
    from a3t_amd import checkpoint as ck
    from a3t_amd.trainer import A3TTrainer
    _, batch = R.tiny_batch("d")
    batch = _dev(batch)
    m = _model("d").train()
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
    assert set(avg) == set(R.golden_keys("d"))
    k = "encoder.pre_speech_encoders.0.self_attn.linear_q.weight"
    assert torch.equal(avg[k], (e2[k] + e1[k]) / 2) and not torch.equal(e1[k], e2[k])
    m2 = _model("d").train()
    tr2 = A3TTrainer(m2.cfg, m2.store, compute="f32", lr=1.0, warmup_steps=10, dropout=False)
    rep2 = ck.EpochReport()
    ck.resume(tmp_path / "checkpoint.pth", m2, rep2, trainer=tr2)
    assert rep2.get_epoch() == 2 and torch.equal(m2.store.flat, m.store.flat) and torch.equal(tr2.m, tr.m)
    assert tr2.optimizer_steps()[0] == 2
    la, lb = float(tr.step(batch)), float(tr2.step(batch))
    assert abs(la - lb) <= 1e-6 * abs(la), (la, lb)


def test_speech_editor_through_a_no_decoder_model():
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import SpeechEditor
    import json
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden import fake_phone_duration
    oc = O.tiny_config()
    m = _model("c").eval()
    assert m.decoder is None and m.encoder.pre_speech_layer == 0
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    ed = SpeechEditor(m, coll, None, ids, fake_phone_duration)
    fx = json.load(open(os.path.join(G, "sedit.json")))
    waves = np.load(os.path.join(G, "sedit_wav.npz"))
    case = [c for c in fx["cases"] if c["kind"] == "replace"][0]
    n = waves[case["wav"] + ".in"].shape[0]
    wav = (0.1 * np.random.RandomState(5).standard_normal(n)).astype(np.float32)
    res = ed.edit(wav, case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"],
                  case["new_str"], **case["opts"])
    assert tuple(res["old_span_boundary"]) == tuple(case["plan"]["old_span_boundary"])
    assert tuple(res["new_span_boundary"]) == tuple(case["plan"]["new_span_boundary"])
    feat = torch.as_tensor(res["feat"])
    s, e = res["new_span_boundary"]
    assert feat.dim() == 2 and feat.shape[1] == 80 and feat.shape[0] >= e > s and bool(torch.isfinite(feat).all())


# ---------------------------------------------------------------- the new kernels, bit for bit
SHAPES = [(3, 37, 5, 32), (2, 1, 0, 384), (2, 1, 1, 384)]


@pytest.mark.parametrize("B,Tm,Tp,d", SHAPES)
def test_concat_rows_and_its_backward(B, Tm, Tp, d):
    from a3t_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + Tm * 10 + Tp)
    sp = torch.randn(B * Tm, d, generator=gen).to(DEV)
    tx = torch.randn(B * Tp, d, generator=gen).to(DEV)
    xs = torch.full((B * (Tm + Tp) + 1, d), float("nan"), device=DEV)       # (one row behind the end: must stay untouched)
    ops.concat_rows(sp, tx, xs, B, Tm, Tp, d)
    want = torch.cat([sp.view(B, Tm, d), tx.view(B, Tp, d)], dim=1)
    assert torch.equal(xs[:-1].view(B, Tm + Tp, d), want) and bool(torch.isnan(xs[-1]).all())
    g = torch.randn(B, Tm + Tp, d, generator=gen).to(DEV)
    ds = torch.full((B * Tm + 1, d), float("nan"), device=DEV)
    dt = torch.full((B * Tp + 1, d), float("nan"), device=DEV)
    ops.split_rows(g, ds, dt, B, Tm, Tp, d)
    assert torch.equal(ds[:-1].view(B, Tm, d), g[:, :Tm]) and torch.equal(dt[:-1].view(B, Tp, d), g[:, Tm:])
    assert bool(torch.isnan(ds[-1]).all()) and bool(torch.isnan(dt[-1]).all())


def test_concat_rows_refuses_what_it_cannot_vectorise():
    from a3t_amd import _lib, ops
    a, b, o = (torch.zeros(64, device=DEV) for _ in range(3))
    with pytest.raises(_lib.A3TLibraryError):
        ops.concat_rows(a, b, o, 1, 2, 2, 6)              # D % 4
    with pytest.raises(_lib.A3TLibraryError):
        ops.split_rows(o[1:], a, b, 1, 2, 2, 4)           # 16-byte alignment
    lib = _lib.load()
    assert "a3t_concat_rows" in _lib.EXPORTS and "a3t_split_rows" in _lib.EXPORTS
    assert hasattr(lib, "a3t_concat_rows") and hasattr(lib, "a3t_split_rows")


@pytest.mark.parametrize("B,Tm,Tp,d", SHAPES)
@pytest.mark.parametrize("drop", [(0.0, 0), (0.25, 1234567)])
def test_embed_finish_null_segment_pointers(B, Tm, Tp, d, drop):
    """seg == NULL / dseg == NULL against the same call with an all-zero table, bit for bit; the ids are then not read."""
    import math
    from a3t_amd import ops
    V, nseg = 16, 500
    gen = torch.Generator().manual_seed(7 + B + Tm + Tp)
    e = torch.randn(B * Tm, d, generator=gen).to(DEV)
    temb = torch.randn(V, d, generator=gen).to(DEV)
    text = torch.randint(0, V, (B, Tp), generator=gen).to(DEV)
    spos = torch.randint(0, nseg, (B, Tm), generator=gen).to(DEV)
    tpos = torch.randint(0, nseg, (B, Tp), generator=gen).to(DEV)
    bad_s, bad_t = torch.full_like(spos, 1 << 40), torch.full_like(tpos, 1 << 40)       # (ids no table has)
    spk = torch.randn(B, d, generator=gen).to(DEV)
    zero = torch.zeros(nseg, d, device=DEV)
    T = Tm + Tp
    a, b = torch.empty(B * T, d, device=DEV), torch.empty(B * T, d, device=DEV)
    ops.embed_finish_fwd(e, temb, zero, text, spos, tpos, a, B, Tm, Tp, d, math.sqrt(d), drop=drop, spk=spk)
    ops.embed_finish_fwd(e, temb, None, text, bad_s, bad_t, b, B, Tm, Tp, d, math.sqrt(d), drop=drop, spk=spk)
    assert torch.equal(a, b)
    # backward: temb's gradient has one writer per (token, column) when every phone of the batch is different
    text = (torch.arange(B * Tp) % V).view(B, Tp).to(DEV)
    assert B * Tp <= V
    g = torch.randn(B * T, d, generator=gen).to(DEV)
    de_a, de_b = torch.zeros(B * Tm, d, device=DEV), torch.zeros(B * Tm, d, device=DEV)
    dt_a, dt_b = torch.zeros(V, d, device=DEV), torch.zeros(V, d, device=DEV)
    dseg = torch.zeros(nseg, d, device=DEV)
    ops.embed_finish_bwd(g, e, text, spos, tpos, de_a, dt_a, dseg, B, Tm, Tp, d, V, nseg, math.sqrt(d), drop=drop)
    ops.embed_finish_bwd(g, e, text, bad_s, bad_t, de_b, dt_b, None, B, Tm, Tp, d, V, nseg, math.sqrt(d), drop=drop)
    assert torch.equal(de_a, de_b) and torch.equal(dt_a, dt_b)
    assert float(dseg.abs().sum()) > 0
