"""The engine's host code on the CPU: a stub in the place of liba3t_hip.so records every call and returns success, so every
route of MLMEngine.forward / backward, a bare ConformerStack and EngineOptions run to their end without a device (the
one-stream schedule: the side streams need dev.type == "cuda").  Nothing is computed: these tests find host errors (a name,
a shape, a branch nobody took), not numeric ones.  No GPU."""
import dataclasses

import pytest
import torch


class StubLib:
    """Every attribute is a recorder that returns 0 (so the *_supported probes say no); the few calls whose result is used
    as a string or a size return one."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == "a3t_gemm_last_kernel":
                return b"stub"
            return 64 if name in ("a3t_mlm_loss_scratch_floats", "a3t_gemm_keep_bytes") else 0
        return fn


@pytest.fixture
def lib(monkeypatch):
    import a3t_amd._lib
    import a3t_amd.ops
    stub = StubLib()
    monkeypatch.setattr(a3t_amd._lib, "_lib", stub)
    monkeypatch.setattr(a3t_amd.ops, "_stream", lambda: None)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return stub


def _model(**kw):
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.config import A3TConfig
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    c = A3TConfig(adim=128, heads=2, ff=256, enc_blocks=2, dec_blocks=1, postnet_layers=2, postnet_chans=32, vocab=40,
                  dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.2, postnet_dropout_rate=0.5, **kw)
    store = ParamStore(c, "cpu")
    xavier_init_(store, seed=3, bn_gamma=1.0)
    return c, store, synthetic_batch(c, 2, 64, 16, seed=7, device="cpu")


def _lens(B=2, Tm=64, Tp=16):
    return (torch.tensor([Tm, Tm - 9], dtype=torch.int32), torch.tensor([Tp, Tp - 3], dtype=torch.int32))


# (compute, training, dropout, need_grad, environment, config, lens, the attention path of every block)
MODES = {
    "f32-train": ("f32", True, False, True, {}, {}, False, "mat"),
    "f32-train-dropout": ("f32", True, True, True, {}, {}, False, "mat"),
    "bf16-train-dropout": ("bf16", True, True, True, {}, {}, False, "mat"),
    "bf16-train-dropout-fused": ("bf16", True, True, True, {"A3T_FUSED_ATTN_TRAIN": "2"}, {}, False, "train"),
    "bf16-train-fused": ("bf16", True, False, True, {"A3T_FUSED_ATTN_TRAIN": "2"}, {}, False, "train"),
    "bf16-eval-fwd": ("bf16", False, False, False, {"A3T_FUSED_ATTN": "fwd"}, {}, False, "fwd"),
    "f32-eval-lens": ("f32", False, False, False, {}, {}, True, None),
    "f32-eval-lens-pre": ("f32", False, False, False, {}, dict(pre_blocks=1), True, None),
    "bf16-train-pre": ("bf16", True, False, True, {}, dict(pre_blocks=1), False, None),
}


def run_mode(mode, monkeypatch):
    """One forward (and backward where gradients are wanted) of `mode`; the engine it ran on."""
    from a3t_amd.engine import MLMEngine
    compute, training, dropout, need_grad, env, ckw, lens, _ = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c, store, batch = _model(**ckw)
    eng = MLMEngine(c, store, compute=compute, training=training, dropout=dropout)
    out = eng.forward(batch, need_grad=need_grad, lens=_lens() if lens else None)
    assert out["before"].shape == out["after"].shape == (2, 64, c.odim) and (out["loss"] is None) == lens
    if need_grad:
        eng.backward()
    return eng


@pytest.mark.parametrize("mode", list(MODES))
def test_every_route_runs_to_its_end(mode, lib, monkeypatch):
    eng = run_mode(mode, monkeypatch)
    assert lib.calls
    want = MODES[mode][7]
    nblk = eng.c.pre_blocks + eng.c.enc_blocks + eng.c.dec_blocks
    assert len(eng.attn_path) == len(eng.block_dims) == nblk
    if want is not None:
        assert set(eng.attn_path.values()) == {want}
    assert eng.side is None and eng.dims == (2, 64, 16, 80)
    assert MODES[mode][6] or len(eng.sv["head"]) == 5


# ------------------------------------------------------------------------------------------------- the stack alone
def _fs2(which):
    if which == "duration":
        import fs2_ragged_ref as R
        from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
        cfg, p = R.checkpoint(R.meta(), "small_c384")
        return FS2DurationModel(FS2DurationConfig.from_espnet(cfg), "cpu").load_state_dict({"tts." + k: v for k, v in p.items()})
    import fs2_tts_ref as R
    from a3t_amd.fs2_tts import FS2TTSConfig, FS2TTSModel
    cfg, p = R.checkpoint(R.meta(), "plain")
    return FS2TTSModel(FS2TTSConfig.from_espnet(cfg), "cpu").load_state_dict({"tts." + k: v for k, v in p.items()})


def test_conformer_stack_runs_a_block_without_a_model_around_it(lib):
    from a3t_amd.conformer import ConformerStack
    from a3t_amd.schedule import StepSchedule, _RowWorkspace
    m = _fs2("duration")
    st = ConformerStack(m.c, m.store, "f32", False, False)
    assert isinstance(st, StepSchedule) and not hasattr(st, "forward") and not hasattr(st, "backward")
    st.ws = _RowWorkspace("cpu")
    B, T, d = 2, 24, m.c.adim
    x = torch.zeros(B * T, d)
    for lens in (None, torch.tensor([T, T - 5], dtype=torch.int32)):
        lib.calls.clear()
        y = st.block_fwd("enc.0", x, st.pe[:T], torch.ones(B, T, dtype=torch.uint8), B, T, lens=lens)
        z = st._ln_fwd("enc.after", y, "enc.after", out_dtype=torch.float32)
        assert y.shape == z.shape == (B * T, d) and z.dtype == torch.float32
        assert st.attn_path == {"enc.0": "mat"} and st.block_dims == {"enc.0": (B, T)}
        names = [n for n, _ in lib.calls]
        assert ("a3t_relpos_softmax_fwd_ragged" in names) == (lens is not None)
        assert ("a3t_relpos_softmax_fwd" in names) == (lens is None)


@pytest.mark.parametrize("which", ["duration", "tts"])
def test_fs2_models_build_a_stack_and_no_mlm_engine(which, lib):
    from a3t_amd.conformer import ConformerStack
    from a3t_amd.engine import MLMEngine
    from a3t_amd.schedule import _RowWorkspace
    m = _fs2(which)
    engines = [m.eng] + ([m.eng_dec] if which == "tts" else [])
    for e in engines:
        assert isinstance(e, ConformerStack) and not isinstance(e, MLMEngine)
        assert isinstance(e.ws, _RowWorkspace) and e.ws is m.ws


# ------------------------------------------------------------------------------------------------------- the options
ENV = {   # variable -> (field, default, {value: parsed})
    "A3T_SIDE_STREAM": ("side_stream", True, {"0": False, "1": True, "": True}),
    "A3T_SIDE2": ("side2", True, {"0": False, "1": True}),
    "A3T_SIDE_DEPTH": ("side_depth", 48, {"1": 2, "2": 2, "8": 8, "64": 64}),
    "A3T_WGRAD_GROUP": ("wgrad_group", True, {"0": False, "1": True}),
    "A3T_POST_F32_FIRST": ("post_f32_first", True, {"0": False, "1": True}),
    "A3T_ATTN_BWD_DS": ("attn_bwd_ds", True, {"0": False, "1": True}),
    "A3T_ATTN_SIGNED": ("attn_signed", True, {"0": False, "1": True}),
    "A3T_ATTN_DQ_DUAL": ("attn_dq_dual", True, {"0": False, "1": True}),
    "A3T_ATTN_DBD_VIEW": ("attn_dbd_view", True, {"0": False, "1": True}),
    "A3T_ATTN_DK_MAIN": ("attn_dk_main", True, {"0": False, "1": True}),
    "A3T_FUSED_ATTN": ("fused_attn", "auto", {"auto": "auto", "fwd": "fwd", "0": "0"}),
    "A3T_FUSED_ATTN_TRAIN": ("fused_attn_train", 1, {"0": 0, "1": 1, "2": 2, "yes": 1}),
    "A3T_FFN_8P": ("ffn_8p", True, {"0": False, "1": True}),
    "A3T_FFN_KEEP4": ("ffn_keep4", True, {"0": False, "1": True}),
    "A3T_LIN_DGRAD_T": ("lin_dgrad_t", True, {"0": False, "1": True}),
}


def test_options_defaults_and_every_variable():
    from a3t_amd.conformer import EngineOptions
    base = EngineOptions.from_env({})
    assert base == EngineOptions() and base.fuse_ln_dropout is True
    assert {f.name for f in dataclasses.fields(base)} == {f for f, _, _ in ENV.values()} | {"fuse_ln_dropout"}
    for var, (field, default, values) in ENV.items():
        assert getattr(base, field) == default and type(getattr(base, field)) is type(default), var
        for raw, want in values.items():
            got = EngineOptions.from_env({var: raw})
            assert getattr(got, field) == want and type(getattr(got, field)) is type(want), (var, raw)
            assert dataclasses.replace(got, **{field: default}) == base      # ... and touches no other field
    for bad in ("1", "on", ""):
        with pytest.raises(ValueError, match="A3T_FUSED_ATTN="):
            EngineOptions.from_env({"A3T_FUSED_ATTN": bad})
    with pytest.raises(ValueError):
        EngineOptions.from_env({"A3T_SIDE_DEPTH": "deep"})


def test_the_documented_table_is_the_record():
    import os
    import re
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    rows = re.findall(r"^\| (?:`(A3T_\w+)`|\(none\)) \| `(\w+)` \|", doc, flags=re.M)
    assert rows == [(var, field) for var, (field, _, _) in ENV.items()] + [("", "fuse_ln_dropout")]


def test_options_reach_the_engine_and_its_derived_values(lib, monkeypatch):
    from a3t_amd.conformer import EngineOptions
    from a3t_amd.engine import MLMEngine
    c, store, _ = _model()
    monkeypatch.setenv("A3T_FUSED_ATTN_TRAIN", "2")
    monkeypatch.setenv("A3T_SIDE_DEPTH", "1")
    e = MLMEngine(c, store, compute="bf16")
    assert e.opt == EngineOptions(fused_attn_train=2, side_depth=2)
    assert (e.fused_attn_auto, e.fused_attn_fwd_only, e.fused_attn_train, e.fused_attn_train_min) == (True, False, True, 1)
    assert e._depth == 2 and len(e._side_ev) == 2 and e._wg_group == 1      # (no side stream on the CPU: nothing to group)
    e = MLMEngine(c, store, compute="f32")                                    # the fused kernels are bf16 only
    assert not (e.fused_attn_auto or e.fused_attn_fwd_only or e.fused_attn_train)
    e = MLMEngine(c, store, compute="bf16", options=EngineOptions(fused_attn="fwd"))      # given: the environment is not read
    assert e.opt.fused_attn_train == 1 and e._depth == 48
    assert (e.fused_attn_auto, e.fused_attn_fwd_only, e.fused_attn_train, e.fused_attn_train_min) == (False, True, False, 64)
    monkeypatch.setenv("A3T_FUSED_ATTN", "1")
    with pytest.raises(ValueError, match="expected auto, fwd or 0"):
        MLMEngine(c, store, compute="bf16")


def test_a_variable_changed_after_construction_changes_nothing(lib, monkeypatch):
    """The plan functions used to read A3T_FFN_8P / A3T_FFN_KEEP4 / A3T_LIN_DGRAD_T at first use.  With probes that say yes
    (and a device that claims to be one), the decisions follow the options the engine was built with."""
    from a3t_amd import ops
    from a3t_amd.engine import MLMEngine
    c, store, _ = _model()
    monkeypatch.setattr(ops, "gemm_8p_supported", lambda *a: False)
    monkeypatch.setattr(ops, "gemm_pn_supported", lambda *a: True)
    plans = {}
    for built_with in ("1", "0"):
        for k in ("A3T_FFN_8P", "A3T_LIN_DGRAD_T"):
            monkeypatch.setenv(k, built_with)
        eng = MLMEngine(c, store, compute="bf16")
        before = dataclasses.replace(eng.opt)
        for k in ENV:
            monkeypatch.setenv(k, "0")
        assert eng.opt == before

        def shadows(suf, shape, eng=eng):      # _setup_wt without its device tensors: zeros of the transposed shape
            eng._wt[suf] = (None, None, {n: torch.zeros(shape[2], shape[1], shape[0], dtype=torch.bfloat16)
                                         for n in store.offsets if n.endswith("." + suf)}, None, tuple(shape))
        eng.dev, eng._setup_wt = torch.device("cuda"), shadows      # (the plans ask for a GPU before they ask the library)
        plans[built_with] = eng._ffn_plan(160)
        dy, dx = torch.zeros(160, c.adim, dtype=torch.bfloat16), torch.zeros(160, c.adim, dtype=torch.bfloat16)
        lib.calls.clear()
        eng._lin_dgrad(dy, "enc.0.mha.wo", dx)
        assert list(eng._lin_plans.values()) == [built_with == "1"] and [n for n, _ in lib.calls] == ["a3t_gemm"]
        for k in ENV:
            monkeypatch.delenv(k)
    assert plans["1"] == (False, True, True, True) and plans["0"] == (False, False, False, False)
