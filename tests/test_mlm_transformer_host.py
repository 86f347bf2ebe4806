"""Host side of the transformer MLM model (`encoder: transformer`, plain attention, absolute positions): the CPU restatement
tests/mlm_transformer_ref.py against the reference's own records (tests/golden/mlm_transformer*.npz / .json, written by
tests/golden/make_golden_mlm_transformer.py), and config, task, parameter layout, key maps, initialisation, checkpoints and the
refusals of the three recorded cases."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import mlm_transformer_ref as R
from oracle import a3t_oracle as O

CASES = R.CASES
N_KEYS = {"a": 57, "b": 75, "c": 38}


def _f(x):
    return float(np.asarray(x.detach() if torch.is_tensor(x) else x).reshape(-1)[0])


def _conf(case, enc_extra=None, dec_extra=None):
    """encoder_conf / decoder / decoder_conf as a recipe yaml would spell the case, at the tiny size (what the generator passed)."""
    o = R.options(case)
    c = O.tiny_config()
    enc = dict(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=o["enc_blocks"], dropout_rate=0.2,
               positional_dropout_rate=0.2, attention_dropout_rate=0.2, input_layer=o["input_layer"], normalize_before=True,
               concat_after=False, positionwise_layer_type=o["positionwise_layer_type"],
               positionwise_conv_kernel_size=o["positionwise_conv_kernel_size"], selfattention_layer_type="selfattn",
               pre_speech_layer=0)
    dec = dict(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=c.dec_blocks, dropout_rate=0.2,
               positional_dropout_rate=0.2, attention_dropout_rate=0.2, normalize_before=True, concat_after=False,
               positionwise_layer_type=o["positionwise_layer_type"],
               positionwise_conv_kernel_size=o["positionwise_conv_kernel_size"], selfattention_layer_type="selfattn")
    enc.update(enc_extra or {})
    dec.update(dec_extra or {})
    mc = dict(postnet_layers=c.postnet_layers, postnet_chans=c.postnet_chans, postnet_filts=c.postnet_filts, lsm_weight=0.1,
              mlm_prob=c.mlm_prob, mean_phn_span=c.mean_phn_span)
    return c, enc, o["decoder"], dec, mc, o["use_scaled_pos_enc"]


def cfg_of(case):
    from a3t_amd.config import A3TConfig
    c, enc, decoder, dec, mc, scaled = _conf(case)
    return A3TConfig.from_espnet(enc, dec, mc, c.idim, c.odim, c.vocab, has_decoder=(decoder != "no_decoder"),
                                 block="transformer", scaled_pos=scaled)


def args_of(case, enc_extra=None, dec_extra=None, **top):
    c, enc, decoder, dec, mc, scaled = _conf(case, enc_extra, dec_extra)
    toks = ["<blank>", "<unk>", "<space>"] + [f"t{i}" for i in range(c.vocab - 4)] + ["<sos/eos>"]
    ns = argparse.Namespace(token_list=toks, odim=c.odim, input_size=c.idim, feats_extract="fbank", feats_extract_conf={},
                            normalize=None, normalize_conf={}, use_scaled_pos_enc=scaled, encoder="transformer", encoder_conf=enc,
                            decoder=decoder, decoder_conf=dec, model_conf=mc, init="xavier_uniform")
    for k, v in top.items():
        setattr(ns, k, v)
    return ns


# ---------------------------------------------------------------- the restatement against the reference's records
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_within_its_own_rounding(case):
    """Every recorded output within R.tolerance: four times the reference's own fp32-against-fp64 distance of that output."""
    g = R.load_golden(case)
    c, batch = R.tiny_batch(case)
    p = R.procedural(case, requires_grad=True)
    assert len(p) == N_KEYS[case]
    loss, before, after = R.model_loss(p, batch, c, True)
    loss.backward()
    got = dict(loss=loss.detach().numpy(), before=before.detach().numpy(), after=after.detach().numpy())
    ngrad = 0
    for k in g:
        if k.startswith("grad."):
            assert p[k[5:]].grad is not None, k
            got[k] = p[k[5:]].grad.numpy()
            ngrad += 1
    assert ngrad == sum(1 for k in p if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    with torch.no_grad():
        got["loss_eval"] = R.model_loss(p, batch, c, False)[0].numpy()
        got["infer_splice"] = R.model_splice(p, {k: v[:1] for k, v in batch.items()}, c, (10, 30)).numpy()
    worst = []
    for k, v in got.items():
        err = float(np.abs(np.asarray(v, np.float64).reshape(g[k].shape) - g[k]).max())
        print(f"{case}.{k}: distance {err:.3e}, bound {R.tolerance(g, k):.3e}")
        if err > R.tolerance(g, k):
            worst.append((k, err, R.tolerance(g, k)))
    assert not worst, worst


def test_alpha_gradients_are_recorded_and_differ():
    g = R.load_golden("b")
    a_s, a_t = _f(g["grad.encoder.speech_embed.4.alpha"]), _f(g["grad.encoder.text_embed.1.alpha"])
    assert a_s != 0.0 and a_t != 0.0 and a_s != a_t
    assert sorted(R.ALPHAS.values()) == [0.7, 1.3]
    p = R.procedural("b")
    assert _f(p["encoder.speech_embed.4.alpha"]) == np.float32(1.3) and _f(p["encoder.text_embed.1.alpha"]) == np.float32(0.7)


def test_restatement_runs_in_fp64():
    c, batch = R.tiny_batch("b")
    with torch.no_grad():
        l64, b64, _ = R.model_loss(R.procedural("b", torch.float64), batch, c)
        l32, _, _ = R.model_loss(R.procedural("b"), batch, c)
    assert b64.dtype == torch.float64
    assert abs(float(l64) - float(l32)) < 1e-5 * abs(float(l64))


def test_absolute_table_is_the_legacy_table_in_forward_order():
    """What the engine adds is conformer.legacy_pe_table flipped: row t = PE(t), bit for bit the reference's PositionalEncoding.pe."""
    from a3t_amd.config import A3TConfig
    from a3t_amd.conformer import legacy_pe_table
    c = A3TConfig(adim=32, heads=2, max_len=300)
    assert torch.equal(legacy_pe_table(c).flip(0)[:200], R.abs_pe(c, 200))


# ---------------------------------------------------------------- config and task
@pytest.mark.parametrize("case", CASES)
def test_from_espnet_maps_the_options(case):
    o, cfg = R.options(case), cfg_of(case)
    assert cfg.block == "transformer" and cfg.scaled_pos == o["use_scaled_pos_enc"]
    assert cfg.ff_kernel == o["positionwise_conv_kernel_size"] and cfg.enc_blocks == o["enc_blocks"]
    assert cfg.has_decoder == (o["decoder"] != "no_decoder") and cfg.dec_blocks == (1 if cfg.has_decoder else 0)
    assert cfg.segment_emb == (o["input_layer"] == "sega_mlm") and cfg.pre_blocks == 0


def test_from_espnet_takes_the_transformer_constructor_defaults():
    from a3t_amd.config import A3TConfig
    cfg = A3TConfig.from_espnet(dict(input_layer="sega_mlm"), {}, {}, 80, 80, 11, block="transformer")
    assert (cfg.adim, cfg.heads, cfg.ff, cfg.ff_kernel, cfg.enc_blocks, cfg.dec_blocks) == (256, 4, 2048, 1, 6, 6)
    assert (cfg.dropout_rate, cfg.positional_dropout_rate, cfg.attention_dropout_rate) == (0.1, 0.1, 0.0)


@pytest.mark.parametrize("case", CASES)
def test_build_model_accepts_the_case(case):
    from a3t_amd.task import MLMTask
    args = args_of(case)
    econf, dconf = dict(args.encoder_conf), dict(args.decoder_conf)
    model = MLMTask.build_model(args, device="cpu")
    assert args.encoder_conf == econf and args.decoder_conf == dconf        # no legacy rel-pos strings written into them
    assert (model.decoder is None) == (R.options(case)["decoder"] == "no_decoder")
    sd = model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.golden_keys(case)
    assert len(list(model.parameters())) == len(model.store.layout)
    for k, v in sd.items():      # initialize(): a 0-d parameter is touched by neither loop, alpha stays at its constructor value
        if k.endswith(".alpha"):
            assert float(v) == 1.0
    # init=None: norm scales and alphas start at 1, everything else at zero
    args = args_of(case, init=None)
    sd = MLMTask.build_model(args, device="cpu").state_dict()
    assert all(float(v) == 1.0 for k, v in sd.items() if k.endswith(".alpha"))
    assert torch.all(sd["encoder.encoders.0.norm1.weight"] == 1.0) and torch.all(sd["sfc.weight"] == 0.0)


def test_task_arguments_carry_use_scaled_pos_enc():
    from a3t_amd.task import MLMTask
    ns = MLMTask.add_task_arguments(argparse.ArgumentParser()).parse_args(
        ["--encoder", "transformer", "--decoder", "transformer", "--use_scaled_pos_enc", "true"])
    assert ns.encoder == "transformer" and ns.use_scaled_pos_enc is True


# ---------------------------------------------------------------- parameter layout and key maps
@pytest.mark.parametrize("case", CASES)
def test_key_map_equals_recorded_key_set_and_maps_both_ways(case):
    from a3t_amd.params import ParamStore, reference_shape
    ref = R.golden_keys(case)
    assert len(ref) == N_KEYS[case]
    store = ParamStore(cfg_of(case), "cpu")
    sd = store.state_dict()
    assert list(sd) == [k for k, _, _, kind in store.keymap] and len(set(sd)) == len(sd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    state = O.procedural_state(ref, seed=3)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    for k, v in store.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), state[k], err_msg=k)
    # gradients leave under the same keys and shapes; a `linear` FFN weight [ff][d] is the k = 1 case of the conv layout
    store.grad.copy_(torch.arange(store.total, dtype=torch.float32))
    gd = store.state_dict(grads=True)
    assert {k: tuple(v.shape) for k, v in gd.items()} == {k: s for k, s in ref.items() if "running" not in k and "num_batches" not in k}
    w1 = gd["encoder.encoders.0.feed_forward.w_1.weight"]
    g1 = store.g["enc.0.ff.w1"]
    if store.cfg.ff_kernel == 1:
        assert g1.shape == (store.cfg.ff, 1, store.cfg.adim) and torch.equal(w1, g1[:, 0, :])
    else:
        assert torch.equal(w1, g1.permute(0, 2, 1))
    for key, name, rows, kind in store.keymap:
        if kind in ("lin1", "conv", "scalar"):
            assert reference_shape(kind, store.offsets[name][1], key) == ref[key], key


def test_layout_of_a_transformer_block():
    from a3t_amd.params import buffer_layout, param_layout
    cfg = cfg_of("b")
    lay = list(param_layout(cfg))
    blk = [k[6:] for k in lay if k.startswith("enc.0.")]
    assert blk == ["mha.ln.g", "mha.ln.b", "mha.wqkv", "mha.bqkv", "mha.wo", "mha.bo", "ff.ln.g", "ff.ln.b", "ff.w1", "ff.b1",
                   "ff.w2", "ff.b2"]
    assert blk == [k[6:] for k in lay if k.startswith("enc.1.")] == [k[6:] for k in lay if k.startswith("dec.0.")]
    assert not [k for k in lay if "wpos" in k or k.endswith((".u", ".v")) or ".ffm." in k or ".cnv." in k or ".fin." in k]
    assert lay[lay.index("temb") + 1:lay.index("temb") + 3] == ["emb.alpha_s", "emb.alpha_t"]
    assert "enc.after.g" in lay and "dec.after.g" in lay
    assert list(buffer_layout(cfg)) == ["post.0.bn.rm", "post.0.bn.rv", "post.1.bn.rm", "post.1.bn.rv"]
    assert not [k for k in param_layout(cfg_of("a")) if "alpha" in k]
    lay_c = list(param_layout(cfg_of("c")))
    assert lay_c[0] == "mask_feature" and not [k for k in lay_c if k.startswith("dec.")]
    assert param_layout(cfg_of("a"))["enc.0.ff.w1"] == (64, 1, 32) and param_layout(cfg)["enc.0.ff.w1"] == (64, 3, 32)


def test_trainer_bucket_bounds_exist_for_the_layout():
    """Trainer's all-reduce buckets start at a block's first parameter: the name engine.backward hands its hook."""
    import inspect
    from a3t_amd import trainer
    from a3t_amd.params import ParamStore
    store = ParamStore(cfg_of("b"), "cpu")
    src = inspect.getsource(trainer)
    assert '"mha.ln.g" if cfg.block == "transformer" else "ffm.ln.g"' in src
    offs = [store.offsets[f"{s}.{i}.mha.ln.g"][0] for s, n in (("enc", 2), ("dec", 1)) for i in range(n)]
    assert offs == sorted(offs) and offs[0] > store.offsets["emb.alpha_t"][0] and offs[-1] < store.offsets["sfc.w"][0]
    for s, n in (("enc", 2), ("dec", 1)):      # nothing of a block lies in front of its first parameter
        for i in range(n):
            assert min(o for k, (o, _) in store.offsets.items() if k.startswith(f"{s}.{i}.")) == store.offsets[f"{s}.{i}.mha.ln.g"][0]


@pytest.mark.parametrize("case", CASES)
def test_checkpoint_save_resume_and_average_on_the_layout(case, tmp_path):
    from a3t_amd.checkpoint import EpochReport, average_nbest_models, resume, save_checkpoint
    from a3t_amd.task import MLMTask
    models, rep = [], EpochReport()
    for ep, seed in ((1, 5), (2, 6)):
        m = MLMTask.build_model(args_of(case, seed=seed), device="cpu")
        if R.options(case)["use_scaled_pos_enc"]:
            m.store.p["emb.alpha_s"].fill_(1.0 + 0.25 * ep)
        rep.set_epoch(ep)
        rep.register("valid", dict(loss=1.0 / ep), ep)
        save_checkpoint(tmp_path, m, rep, ep, best_model_criterion=[("valid", "loss", "min")])
        models.append(m)
    again = MLMTask.build_model(args_of(case, seed=9), device="cpu")
    rep2 = EpochReport()
    resume(tmp_path / "checkpoint.pth", again, rep2)
    for k, v in models[-1].state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
    average_nbest_models(tmp_path, rep, [("valid", "loss", "min")], nbest=2)
    avg = torch.load(tmp_path / "valid.loss.ave_2best.pth", map_location="cpu")
    assert set(avg) == set(R.golden_keys(case))
    for k, v in avg.items():
        if v.is_floating_point():
            want = (models[0].state_dict()[k] + models[1].state_dict()[k]) / 2
            assert torch.allclose(v, want, atol=1e-7), k
    if R.options(case)["use_scaled_pos_enc"]:
        assert avg["encoder.speech_embed.4.alpha"].shape == () and abs(float(avg["encoder.speech_embed.4.alpha"]) - 1.375) < 1e-6


# ---------------------------------------------------------------- what stays refused, by its field
@pytest.mark.parametrize("who", ["encoder_conf", "decoder_conf"])
@pytest.mark.parametrize("field,value", [
    ("normalize_before", False), ("concat_after", True), ("stochastic_depth_rate", 0.1), ("intermediate_layers", [1]),
    ("positionwise_layer_type", "conv1d-linear"), ("selfattention_layer_type", "lightconv"),
    ("selfattention_layer_type", "lightconv2d"), ("selfattention_layer_type", "dynamicconv"),
    ("selfattention_layer_type", "dynamicconv2d"), ("selfattention_layer_type", "longformer")])
def test_from_espnet_refusals_name_their_field(who, field, value):
    from a3t_amd.task import MLMTask
    extra = {field: value}
    args = args_of("b", enc_extra=extra if who == "encoder_conf" else None, dec_extra=extra if who == "decoder_conf" else None)
    with pytest.raises(NotImplementedError, match=rf"{who}\.{field}"):
        MLMTask.build_model(args, device="cpu")


def test_other_refusals_name_their_field():
    from a3t_amd.config import A3TConfig
    from a3t_amd.task import MLMTask
    with pytest.raises(NotImplementedError, match="pre_speech_layer"):
        MLMTask.build_model(args_of("a", enc_extra=dict(pre_speech_layer=1)), device="cpu")
    with pytest.raises(NotImplementedError, match="positionwise_conv_kernel_size"):
        MLMTask.build_model(args_of("b", enc_extra=dict(positionwise_conv_kernel_size=4)), device="cpu")
    with pytest.raises(NotImplementedError, match="input_layer"):
        MLMTask.build_model(args_of("a", enc_extra=dict(input_layer="linear")), device="cpu")
    # the two block types do not mix
    with pytest.raises(NotImplementedError, match="decoder='conformer' with encoder='transformer'"):
        MLMTask.build_model(args_of("a", decoder="conformer"), device="cpu")
    with pytest.raises(NotImplementedError, match="decoder='transformer' with encoder='conformer'"):
        MLMTask.build_model(args_of("a", encoder="conformer"), device="cpu")
    # one block size per model
    with pytest.raises(NotImplementedError, match="decoder_conf.linear_units"):
        MLMTask.build_model(args_of("a", dec_extra=dict(linear_units=128)), device="cpu")
    # the conformer encoder never builds pos_enc_class
    c = O.tiny_config()
    with pytest.raises(NotImplementedError, match="use_scaled_pos_enc"):
        A3TConfig.from_espnet(dict(attention_dim=32, attention_heads=2, linear_units=64, num_blocks=1), dict(num_blocks=1), {},
                              c.idim, c.odim, c.vocab, scaled_pos=True)


def test_rows_alone_is_refused_on_a_transformer_model():
    """lens= / rows="alone": the packed ragged rows exist for the conformer blocks only."""
    from a3t_amd.engine import MLMEngine
    from a3t_amd.params import ParamStore
    cfg = cfg_of("a")
    eng = MLMEngine(cfg, ParamStore(cfg, "cpu"), compute="f32", training=False)
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="lens="):
        eng.forward(dict(speech=torch.zeros(2, 8, 80), text=torch.zeros(2, 4, dtype=torch.long)), need_grad=False, lens=(z, z))


# ---------------------------------------------------------------- C ABI of the new entry points
NEW_EXPORTS = {"a3t_attn_fwd_plain": 17, "a3t_attn_fwd_train_plain": 20, "a3t_softmax_plain_fwd": 15, "a3t_softmax_plain_bwd": 18, "a3t_embed_finish_abs_fwd": 19,
               "a3t_embed_finish_abs_bwd": 22, "a3t_embed_finish_abs_partials": 4, "a3t_scale_add_pos": 10}


def test_new_exports_are_declared_with_matching_signatures():
    from a3t_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "a3t_hip.h")).read(), flags=re.S)
    build.build(verbose=False)
    lib = _lib.load()
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert name in _lib.EXPORTS and len(args) == len(_lib._SIGS[name]) == nargs, (name, len(args))
        assert [("*" in a) for a in args] == [t is _lib._P for t in _lib._SIGS[name]], name
        assert hasattr(lib, name)
    # the old softmax exports keep their signatures: the positional operands did not become optional
    assert len(_lib._SIGS["a3t_relpos_softmax_fwd"]) == 17 and len(_lib._SIGS["a3t_relpos_softmax_bwd"]) == 21
    assert len(_lib._SIGS["a3t_attn_fwd"]) == 22 and len(_lib._SIGS["a3t_attn_fwd_train"]) == 25


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Argument checks run on the host in front of any launch (A3T_EINVAL = a non-zero return code)."""
    from a3t_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.a3t_softmax_plain_fwd(None, 0, None, None, 0, 1, 1, 8, 64, 64, 1.0, None, 0.0, 0, None) != 0
    assert lib.a3t_softmax_plain_bwd(None, 0, None, 0, None, 0, 1, 1, 8, 64, 64, 64, 1.0, None, 0.0, 0, None, None) != 0
    assert lib.a3t_scale_add_pos(None, None, None, 1, 8, 32, 1.0, 0.0, 0, None) != 0
    assert lib.a3t_attn_fwd_plain(None, None, None, None, None, None, 1, 2, 136, 32, 192, 192, 64, 0.25, 0.0, 0, None) != 0
    assert lib.a3t_attn_fwd_train_plain(*([None] * 9), 1, 2, 136, 32, 192, 192, 64, 0.25, 0.0, 0, None) != 0
    assert lib.a3t_embed_finish_abs_fwd(*([None] * 10), 1, 8, 4, 32, 1.0, 0.0, 0, None, None) != 0
    assert lib.a3t_embed_finish_abs_bwd(*([None] * 12), 1, 8, 4, 32, 11, 500, 1.0, 0.0, 0, None) != 0
    assert lib.a3t_embed_finish_abs_partials(2, 48, 8, 32) == 2 * ((2 * 56 * 32 + 255) // 256)
    assert lib.a3t_embed_finish_abs_partials(64, 1120, 200, 384) == 2 * 4096        # the grid's cap
