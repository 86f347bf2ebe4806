"""Host-side checks of the FastSpeech2 duration model (a3t_amd/duration.py): config translation, rejections, the
checkpoint key map and the token mapping of duration_predict.  No GPU: the store lives on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import a3t_oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")

# the tts_conf of egs2/ljspeech/tts1/conf/tuning/train_conformer_fastspeech2.yaml (the keys the duration path reads and
# a few it ignores)
LJ_CONF = dict(adim=384, aheads=2, elayers=4, eunits=1536, dlayers=4, dunits=1536, positionwise_layer_type="conv1d",
               positionwise_conv_kernel_size=3, duration_predictor_layers=2, duration_predictor_chans=256,
               duration_predictor_kernel_size=3, postnet_layers=5, postnet_filts=5, postnet_chans=256,
               use_masking=True, encoder_normalize_before=True, decoder_normalize_before=True, reduction_factor=1,
               encoder_type="conformer", decoder_type="conformer", conformer_pos_enc_layer_type="rel_pos",
               conformer_self_attn_layer_type="rel_selfattn", conformer_activation_type="swish",
               use_macaron_style_in_conformer=True, use_cnn_in_conformer=True, conformer_enc_kernel_size=7,
               conformer_dec_kernel_size=31, init_type="xavier_uniform", transformer_enc_dropout_rate=0.2)
TOKENS = ["<blank>", "<unk>", "AH0", "B", "K", "T", "<sos/eos>"]


def _conf(**kw):
    t = dict(LJ_CONF)
    t.update(kw)
    return {"tts": "fastspeech2", "tts_conf": t, "token_list": list(TOKENS), "normalize": "global_mvn",
            "pitch_normalize": "global_mvn", "energy_normalize": "global_mvn"}


def test_config_translation_ljspeech():
    from a3t_amd.config import A3TConfig
    from a3t_amd.duration import FS2DurationConfig
    c = FS2DurationConfig.from_espnet(_conf())
    assert isinstance(c, A3TConfig)
    assert (c.adim, c.heads, c.ff, c.ff_kernel, c.enc_blocks, c.enc_kernel) == (384, 2, 1536, 3, 4, 7)
    assert (c.dp_layers, c.dp_chans, c.dp_kernel, c.dp_offset) == (2, 256, 3, 1.0)
    assert c.vocab == len(TOKENS) and c.token_list == TOKENS
    assert c.spk_embed_dim == 0 and c.dec_blocks == 0 and c.postnet_layers == 0
    assert c.dropout_rate == c.attention_dropout_rate == c.positional_dropout_rate == 0.0
    x = FS2DurationConfig.from_espnet(_conf(spk_embed_dim=512, spk_embed_integration_type="concat"))
    assert (x.spk_embed_dim, x.spk_integration) == (512, "concat")
    # FastSpeech2's own defaults fill what tts_conf leaves out (aheads=4, duration_predictor_chans=384)
    t = {k: v for k, v in LJ_CONF.items() if k not in ("aheads", "duration_predictor_chans")}
    d = FS2DurationConfig.from_espnet({"tts": "fastspeech2", "tts_conf": t, "token_list": TOKENS})
    assert (d.heads, d.dp_chans) == (4, 384)


@pytest.mark.parametrize("kw,field", [
    (dict(use_gst=True), "use_gst"),
    (dict(encoder_type="transformer"), "encoder_type"),
    (dict(conformer_rel_pos_type="latest", conformer_pos_enc_layer_type="rel_pos"), "conformer_rel_pos_type"),
    (dict(spk_embed_dim=256, spk_embed_integration_type="film"), "spk_embed_integration_type"),
    (dict(positionwise_layer_type="linear"), "positionwise_layer_type"),
    (dict(use_macaron_style_in_conformer=False), "use_macaron_style_in_conformer"),
    (dict(use_cnn_in_conformer=False), "use_cnn_in_conformer"),
    (dict(encoder_normalize_before=False), "encoder_normalize_before"),
    (dict(encoder_concat_after=True), "encoder_concat_after"),
    (dict(conformer_activation_type="relu"), "conformer_activation_type"),
])
def test_config_rejections_name_the_field(kw, field):
    from a3t_amd.duration import FS2DurationConfig
    with pytest.raises(NotImplementedError, match=field):
        FS2DurationConfig.from_espnet(_conf(**kw))


def test_transformer_encoder_is_the_fs2_default_and_is_rejected():
    from a3t_amd.duration import FS2DurationConfig
    t = {k: v for k, v in LJ_CONF.items() if k != "encoder_type"}
    with pytest.raises(NotImplementedError, match="encoder_type"):
        FS2DurationConfig.from_espnet({"tts": "fastspeech2", "tts_conf": t, "token_list": TOKENS})


def _fixture_checkpoint(case):
    meta = json.load(open(os.path.join(G, "fs2_duration.json")))
    m = meta["cases"][case]
    cfg = {"tts": "fastspeech2", "tts_conf": m["tts_conf"], "token_list": meta["token_list"]}
    shapes = {k: tuple(v) for k, v in m["shapes"].items()}
    state = O.procedural_state(shapes, m["seed"])
    return cfg, {"tts." + k: torch.from_numpy(np.array(v)) for k, v in state.items()}


@pytest.mark.parametrize("case", ["lj", "lj_xcat", "lj_xadd"])
def test_key_map_loads_the_duration_path_and_ignores_the_rest(case):
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    cfg, sd = _fixture_checkpoint(case)
    c = FS2DurationConfig.from_espnet(cfg)
    sd["normalize.mean"] = torch.zeros(80)
    sd["pitch_normalize.std"] = torch.ones(1)
    if case == "lj":
        sd["tts.sid_emb.weight"] = torch.zeros(3, c.adim)       # loaded and ignored, as duration_predict never adds it
    assert any(k.startswith("tts.decoder.") for k in sd) and any(k.startswith("tts.pitch_predictor.") for k in sd)
    m = FS2DurationModel(c, "cpu").load_state_dict(sd)
    p, d = m.store.p, c.adim
    assert torch.equal(p["temb"], sd["tts.encoder.embed.0.weight"])
    a = "tts.encoder.encoders.1.self_attn."
    assert torch.equal(p["enc.1.mha.wqkv"][d:2 * d], sd[a + "linear_k.weight"])
    assert torch.equal(p["enc.1.mha.u"], sd[a + "pos_bias_u"].reshape(-1))
    assert torch.equal(m.store.buf["enc.3.cnv.bn.rv"], sd["tts.encoder.encoders.3.conv_module.norm.running_var"])
    assert torch.equal(p["enc.after.g"], sd["tts.encoder.after_norm.weight"])
    # Conv1d [out][in][tap] -> [out][tap][in]
    w = sd["tts.duration_predictor.conv.1.0.weight"]
    assert torch.equal(p["dp.1.w"], w.permute(0, 2, 1))
    assert torch.equal(p["dp.0.ln.g"], sd["tts.duration_predictor.conv.0.2.weight"])
    assert torch.equal(p["dp.lin.w"], sd["tts.duration_predictor.linear.weight"].reshape(-1))
    assert torch.equal(p["dp.lin.b"], sd["tts.duration_predictor.linear.bias"])
    if case == "lj_xcat":
        W = sd["tts.projection.weight"]
        assert W.shape == (d, d + 512)
        assert torch.equal(p["spk.wh"], W[:, :d]) and torch.equal(p["spk.ws"], W[:, d:])
    elif case == "lj_xadd":
        assert torch.equal(p["spk.ws"], sd["tts.projection.weight"])
        assert "spk.wh" not in p
    else:
        assert "spk.ws" not in p


def test_key_map_missing_and_unexpected_keys():
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    cfg, sd = _fixture_checkpoint("lj")
    c = FS2DurationConfig.from_espnet(cfg)
    bad = dict(sd)
    del bad["tts.duration_predictor.linear.bias"]
    del bad["tts.encoder.encoders.2.conv_module.norm.running_mean"]
    with pytest.raises(KeyError) as e:
        FS2DurationModel(c, "cpu").load_state_dict(bad)
    assert "tts.duration_predictor.linear.bias" in str(e.value)
    assert "tts.encoder.encoders.2.conv_module.norm.running_mean" in str(e.value)
    extra = dict(sd)
    extra["tts.encoder.encoders.4.norm_ff.weight"] = torch.ones(c.adim)     # a fifth block the config does not have
    with pytest.raises(KeyError, match="encoders.4"):
        FS2DurationModel(c, "cpu").load_state_dict(extra)


def test_token_mapping_sp_unknown_eos():
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    c = FS2DurationConfig.from_espnet(_conf())
    m = FS2DurationModel(c, "cpu")
    assert m.eos == len(TOKENS) - 1
    assert m.tokens_to_ids(["sp", "K", "AH0", "ZZ", "T", "sp"]) == [0, 4, 2, 1, 5, 0, 6]
    assert m.tokens_to_ids([]) == [6]
    assert m.tokens_to_ids(["<blank>", "[MASK]"]) == [0, 1, 6]


def test_fixture_is_data_only_and_small():
    meta = json.load(open(os.path.join(G, "fs2_duration.json")))
    assert set(meta["cases"]) == {"lj", "lj_xadd", "lj_xcat", "small_c384"}
    for n in ("fs2_duration.json", "fs2_duration.npz"):
        assert os.path.getsize(os.path.join(G, n)) < 1 << 20
    z = np.load(os.path.join(G, "fs2_duration.npz"))
    for case in meta["cases"]:
        for T in meta["lengths"]:
            assert z[f"{case}.T{T}.frames"].dtype == np.int64 and z[f"{case}.T{T}.ids"].shape == (T,)
