"""Host side of the model variants MLMTask builds besides the recipe's -- input_layer 'mlm' (no segment embedding),
pre_speech_layer N and decoder 'no_decoder': the CPU restatement tests/mlm_variants_ref.py against the reference's own
records (tests/golden/mlm_variants*.npz / .json, written by tests/golden/make_golden_mlm_variants.py), and config, task,
parameter layout and initialisation of the four recorded cases.  The default layout is pinned to what it was before."""
import argparse
import hashlib
import json

import numpy as np
import pytest
import torch

import mlm_variants_ref as R
from oracle import a3t_oracle as O

CASES = sorted(R.CASES)


def _f(x):
    return float(np.asarray(x.detach() if torch.is_tensor(x) else x).reshape(-1)[0])


N_KEYS = {"a": 104, "b": 185, "c": 63, "d": 102}


def _conf(case, **enc_extra):
    """encoder_conf / decoder / decoder_conf as the recipe's yaml would spell the case, at the tiny size."""
    seg, pre, dec = R.CASES[case]
    c = O.tiny_config()
    enc = dict(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=c.enc_blocks,
               cnn_module_kernel=c.enc_kernel, input_layer="sega_mlm" if seg else "mlm", pre_speech_layer=pre,
               positionwise_layer_type="conv1d", positionwise_conv_kernel_size=3, macaron_style=True, use_cnn_module=True,
               pos_enc_layer_type="legacy_rel_pos", selfattention_layer_type="legacy_rel_selfattn", dropout_rate=0.0,
               positional_dropout_rate=0.0, attention_dropout_rate=0.0)
    enc.update(enc_extra)
    decc = dict(attention_dim=c.adim, attention_heads=c.heads, linear_units=c.ff, num_blocks=c.dec_blocks,
                cnn_module_kernel=c.dec_kernel, pos_enc_layer_type="legacy_rel_pos",
                selfattention_layer_type="legacy_rel_selfattn")
    mc = dict(postnet_layers=c.postnet_layers, postnet_chans=c.postnet_chans, postnet_filts=c.postnet_filts, lsm_weight=0.1,
              mlm_prob=c.mlm_prob, mean_phn_span=c.mean_phn_span)
    return c, enc, ("conformer" if dec else "no_decoder"), decc, mc


def _cfg(case):
    from a3t_amd.config import A3TConfig
    c, enc, decoder, decc, mc = _conf(case)
    return A3TConfig.from_espnet(enc, decc, mc, c.idim, c.odim, c.vocab, has_decoder=(decoder != "no_decoder"))


def _args(case, **enc_extra):
    c, enc, decoder, decc, mc = _conf(case, **enc_extra)
    toks = ["<blank>", "<unk>", "<space>"] + [f"t{i}" for i in range(c.vocab - 4)] + ["<sos/eos>"]
    return argparse.Namespace(token_list=toks, odim=c.odim, input_size=c.idim, feats_extract="fbank", feats_extract_conf={},
                              normalize=None, normalize_conf={}, encoder="conformer", encoder_conf=enc, decoder=decoder,
                              decoder_conf=decc, model_conf=mc, init="xavier_uniform")


# ---------------------------------------------------------------- the restatement against the reference's records
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference(case):
    """Bounds of tests/test_oracle_golden.py::test_e2e_tiny_train_and_eval."""
    g = R.load_golden(case)
    c, batch = R.tiny_batch(case)
    p = R.procedural(case, requires_grad=True)
    assert len(p) == N_KEYS[case]
    stats = {}
    loss, before, after = R.variant_loss(p, batch, c, case, True, stats)
    assert abs(_f(loss) - _f(g["loss"])) < 1e-3
    np.testing.assert_allclose(before.detach().numpy(), g["before"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(after.detach().numpy(), g["after"], atol=1e-4, rtol=1e-4)
    loss.backward()
    ngrad = 0
    for k in g:
        if k.startswith("grad."):
            n = k[5:]
            assert p[n].grad is not None, n
            ref = g[k]
            np.testing.assert_allclose(p[n].grad.numpy(), ref, atol=3e-4 * max(1.0, float(np.abs(ref).max())), rtol=2e-3,
                                       err_msg=n)
            ngrad += 1
    assert ngrad == sum(1 for k in p if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    assert stats
    for pre, (mean, var_u) in stats.items():
        rm = 0.9 * p[pre + ".running_mean"] + 0.1 * mean
        rv = 0.9 * p[pre + ".running_var"] + 0.1 * var_u
        np.testing.assert_allclose(rm.numpy(), g["buf." + pre + ".running_mean"], atol=1e-5, rtol=1e-5)
        np.testing.assert_allclose(rv.numpy(), g["buf." + pre + ".running_var"], atol=1e-5, rtol=1e-4)
    with torch.no_grad():
        le, _, _ = R.variant_loss(p, batch, c, case, False)
        assert abs(_f(le) - _f(g["loss_eval"])) < 1e-3
        sp = R.variant_splice(p, {k: v[:1] for k, v in batch.items()}, c, case, (10, 30))
    np.testing.assert_allclose(sp.numpy(), g["infer_splice"], atol=1e-4, rtol=1e-4)


def test_reference_ignores_segment_ids_without_table():
    g = R.load_golden("a")
    assert _f(g["loss_nonzero_seg"]) == _f(g["loss"])
    c, batch = R.tiny_batch("a")
    nz = O.synthetic_batch(c, B=2, T_mel=48, T_phn=8, seed=R.SEED_B, lengths=[48, 37], text_lengths=[8, 6])
    assert int(nz["speech_segment_pos"].max()) > 0
    p = R.procedural("a")
    with torch.no_grad():
        l0, _, _ = R.variant_loss(p, batch, c, "a")
        l1, _, _ = R.variant_loss(p, nz, c, "a")
    assert float(l0) == float(l1)


def test_restatement_runs_in_fp64():
    c, batch = R.tiny_batch("d")
    with torch.no_grad():
        l64, b64, _ = R.variant_loss(R.procedural("d", torch.float64), batch, c, "d")
        l32, _, _ = R.variant_loss(R.procedural("d"), batch, c, "d")
    assert b64.dtype == torch.float64
    assert abs(float(l64) - float(l32)) < 1e-4 * abs(float(l64))


# ---------------------------------------------------------------- config and task
@pytest.mark.parametrize("case", CASES)
def test_from_espnet_maps_the_options(case):
    seg, pre, dec = R.CASES[case]
    cfg = _cfg(case)
    assert (cfg.segment_emb, cfg.pre_blocks, cfg.has_decoder) == (seg, pre, dec)
    assert cfg.enc_blocks == 1 and cfg.dec_blocks == (1 if dec else 0)


def test_from_espnet_does_not_read_decoder_conf_without_decoder():
    from a3t_amd.config import A3TConfig
    c, enc, _, _, mc = _conf("c")

    class Untouchable(dict):
        def __getitem__(self, k):
            raise AssertionError(f"decoder_conf[{k!r}] was read")

        def get(self, k, default=None):
            raise AssertionError(f"decoder_conf.get({k!r}) was read")

    cfg = A3TConfig.from_espnet(enc, Untouchable(), mc, c.idim, c.odim, c.vocab, has_decoder=False)
    assert not cfg.has_decoder and cfg.dec_blocks == 0
    # a conformer decoder with zero blocks is another model: it still scales by sqrt(d) and applies decoder.after_norm
    z = A3TConfig.from_espnet(enc, dict(num_blocks=0), mc, c.idim, c.odim, c.vocab)
    assert z.has_decoder and z.dec_blocks == 0
    from a3t_amd.params import param_layout
    assert "dec.after.g" in param_layout(z) and "dec.after.g" not in param_layout(cfg)


@pytest.mark.parametrize("case", CASES)
def test_build_model_accepts_the_case(case):
    from a3t_amd.task import MLMTask
    seg, pre, dec = R.CASES[case]
    args = _args(case)
    dconf = dict(args.decoder_conf)
    if not dec:        # no_decoder: decoder_conf is left alone (not even the legacy rel-pos strings are written into it)
        args.decoder_conf = dconf = dict(dconf, pos_enc_layer_type="rel_pos", selfattention_layer_type="rel_selfattn")
    model = MLMTask.build_model(args, device="cpu")
    assert (model.encoder.segment_emb is None) == (not seg)
    assert model.encoder.pre_speech_layer == pre
    assert (model.decoder is None) == (not dec)
    assert args.decoder_conf == dconf
    sd = model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.golden_keys(case)
    assert len(list(model.parameters())) == len(model.store.layout)
    # collate: all-zero segment ids for a model without segment embedding (tasks/mlm.py:274)
    assert (args.encoder_conf["input_layer"] == "sega_mlm") == seg


# ---------------------------------------------------------------- parameter layout
@pytest.mark.parametrize("case", CASES)
def test_key_map_equals_recorded_key_set(case):
    from a3t_amd.params import ParamStore
    ref = R.golden_keys(case)
    assert len(ref) == N_KEYS[case]
    store = ParamStore(_cfg(case), "cpu")
    sd = store.state_dict()
    assert list(sd) == [k for k, _, _, kind in store.keymap if kind != "optional"] and len(set(sd)) == len(sd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    # the reference's own values round-trip through the flat store
    state = O.procedural_state(ref, seed=3)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    for k, v in store.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), state[k], err_msg=k)


def test_layout_order_of_the_variants():
    from a3t_amd.params import buffer_layout, param_layout
    lay = list(param_layout(_cfg("b")))
    assert lay[0] == "seg"
    i_emb, i_pre0, i_pre1, i_enc = (lay.index(k) for k in ("temb", "pre.0.ffm.ln.g", "pre.1.ffm.ln.g", "enc.0.ffm.ln.g"))
    assert i_emb < i_pre0 < i_pre1 < i_enc
    assert [k[6:] for k in lay if k.startswith("pre.0.")] == [k[6:] for k in lay if k.startswith("enc.0.")]
    assert list(buffer_layout(_cfg("b")))[:4] == ["pre.0.cnv.bn.rm", "pre.0.cnv.bn.rv", "pre.1.cnv.bn.rm", "pre.1.cnv.bn.rv"]
    lay = list(param_layout(_cfg("d")))
    assert lay[0] == "mask_feature" and "seg" not in lay
    assert not [k for k in lay if k.startswith("dec.")] and lay[lay.index("enc.after.b") + 1] == "sfc.w"
    assert not [k for k in buffer_layout(_cfg("d")) if k.startswith("dec.")]


def _digest(rows):
    return hashlib.sha256(json.dumps(rows).encode()).hexdigest()[:16]


def test_default_layout_is_what_it_was():
    """Total size, first / last offsets, entry counts and digests of the default layouts, taken from the commit before the
    variants existed (ParamStore(A3TConfig()) and ParamStore(config_c2()))."""
    from a3t_amd.config import A3TConfig, config_c2
    from a3t_amd.params import ParamStore, param_layout
    pins = [(A3TConfig(), 67691520, 67691328, 67691392, 292, 363, "9a0fef96b522f1f2", "9a2a314524babd24"),
            (config_c2(), 100800000, 100799808, 100799872, 424, 523, "5e30f139524d3a21", "8f90cee2981ae256")]
    for c, total, n_params, last_off, n_lay, n_map, h_off, h_map in pins:
        assert (c.segment_emb, c.pre_blocks, c.has_decoder) == (True, 0, True)
        s = ParamStore(c, "cpu")
        ks = list(s.offsets)
        assert list(param_layout(c)) == ks
        assert (s.total, s.n_params) == (total, n_params)
        assert ks[0] == "seg" and s.offsets["seg"] == (0, (500, 384))
        assert ks[-1] == "post.4.bn.b" and s.offsets[ks[-1]] == (last_off, (80,))
        assert (len(ks), len(s.keymap)) == (n_lay, n_map)
        assert _digest([[k, o, list(sh)] for k, (o, sh) in s.offsets.items()]) == h_off
        assert _digest([[a, b, list(r) if r else None, k] for a, b, r, k in s.keymap]) == h_map


# ---------------------------------------------------------------- initialisation
@pytest.mark.parametrize("case", CASES)
def test_xavier_init_runs_on_the_case(case):
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    store = xavier_init_(ParamStore(_cfg(case), "cpu"), seed=3, bn_gamma=0.5)
    sd = store.state_dict()
    assert set(sd) == set(R.golden_keys(case))
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("conv_module.norm.weight") or (k.startswith("postnet.") and k.endswith(".1.weight")):
            assert torch.all(v == 0.5), k                 # BatchNorm scale: the 1-d zeroing (bn_gamma)
        elif ("norm" in k and "conv_module.norm" not in k and "running" not in k) or k.startswith("encoder.speech_embed.2"):
            assert torch.all(v == (1.0 if k.endswith("weight") else 0.0)), k          # LayerNorm reset
        elif k.endswith("running_var"):
            assert torch.all(v == 1.0), k
        elif v.dim() == 1 or k.endswith("running_mean"):
            assert torch.all(v == 0.0), k
        else:
            assert float(v.abs().max()) > 0, k
    # the reference's padding-row rule (padding_idx = -1: the last row of an embedding table is zero)
    temb = sd["encoder.text_embed.0.weight"]
    assert torch.all(temb[-1] == 0) and float(temb[:-1].abs().min()) > 0
    if R.CASES[case][0]:
        assert torch.all(sd["encoder.segment_emb.weight"][-1] == 0)
    pre = [k for k in sd if k.startswith("encoder.pre_speech_encoders.")]
    assert len(pre) == R.CASES[case][1] * len([k for k in sd if k.startswith("encoder.encoders.0.")])


# ---------------------------------------------------------------- what stays refused
@pytest.mark.parametrize("field,value", [("input_layer", "linear"), ("input_layer", "conv2d"),
                                         ("positionwise_layer_type", "linear"), ("macaron_style", False),
                                         ("use_cnn_module", False)])
def test_from_espnet_refusals_name_their_field(field, value):
    from a3t_amd.config import A3TConfig
    c, enc, _, decc, mc = _conf("b", **{field: value})
    with pytest.raises(NotImplementedError, match=field):
        A3TConfig.from_espnet(enc, decc, mc, c.idim, c.odim, c.vocab)


@pytest.mark.parametrize("field,value", [("encoder", "transformer"), ("decoder", "transformer"), ("decoder", "rnn")])
def test_build_model_refusals_name_their_field(field, value):
    from a3t_amd.task import MLMTask
    args = _args("b")
    setattr(args, field, value)
    with pytest.raises(NotImplementedError, match=f"{field}='{value}'"):
        MLMTask.build_model(args, device="cpu")


def test_build_model_refuses_other_attention_and_the_tts_model():
    from a3t_amd.task import MLMTask
    args = _args("c", selfattention_layer_type="longformer")
    with pytest.raises(NotImplementedError, match="legacy_rel_selfattn"):
        MLMTask.build_model(args, device="cpu")
    args = _args("c")
    args.model_conf["duration_predictor_layers"] = 2
    with pytest.raises(NotImplementedError, match="ESPnetMLMTTSModel"):
        MLMTask.build_model(args, device="cpu")


# ---------------------------------------------------------------- C ABI of the two new entry points
def test_new_exports_are_declared_with_matching_signatures():
    import os
    import re
    from a3t_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "a3t_hip.h")).read(), flags=re.S)
    for name in ("a3t_concat_rows", "a3t_split_rows"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert name in _lib.EXPORTS and len(args) == len(_lib._SIGS[name]) == 8, (name, args)
        assert [("*" in a) for a in args] == [True, True, True, False, False, False, False, True]
    lib = _lib.load()
    assert hasattr(lib, "a3t_concat_rows") and hasattr(lib, "a3t_split_rows")
