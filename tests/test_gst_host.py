"""Host-side checks of the GST style encoder of the duration model (a3t_amd/duration.py, a3t_amd/sedit.py): the opt-in
config translation and its refusals, the checkpoint key map, the torch restatement tests/gst_ref.py against the reference's own
outputs (tests/golden/gst_duration.{npz,json}, tests/golden/make_golden_gst.py) and its ragged rule, and the planning of a
batch of edits with a duration function that needs the prompt.  No GPU."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import gst_ref as R
from test_duration_host import LJ_CONF, TOKENS

G = os.path.join(os.path.dirname(__file__), "golden")
CASES = ("gst_xadd", "gst_xcat", "gst_plain", "gst_small")
FBANK = dict(fs=24000, n_fft=2048, win_length=1200, hop_length=300, n_mels=80, fmin=80, fmax=7600)


def _conf(feats=None, fe="fbank", **kw):
    t = dict(LJ_CONF, use_gst=True)
    t.update(kw)
    return {"tts": "fastspeech2", "tts_conf": t, "token_list": list(TOKENS), "feats_extract": fe,
            "feats_extract_conf": dict(FBANK if feats is None else feats), "normalize": "global_mvn"}


# ------------------------------------------------------------------------------------------------------------ config
def test_config_translation_with_gst_defaults_and_a_non_default_plan():
    from a3t_amd.duration import FS2DurationConfig
    c = FS2DurationConfig.from_espnet(_conf(), gst=True)
    assert c.use_gst and (c.gst_tokens, c.gst_heads, c.gst_conv_kernel, c.gst_conv_stride, c.gst_gru_units) == (10, 4, 3, 2, 128)
    assert c.gst_conv_chans == [32, 32, 64, 64, 128, 128] and c.n_mels == 80
    # frequency 80 -> 40 -> 20 -> 10 -> 5 -> 3 -> 2, channels 1 -> 32, 32, 64, 64, 128, 128: the GRU reads 2 * 128
    assert c.gst_plan() == [(1, 32, 80, 40), (32, 32, 40, 20), (32, 64, 20, 10), (64, 64, 10, 5), (64, 128, 5, 3), (128, 128, 3, 2)]
    assert c.gst_feats_conf["fs"] == 24000 and c.gst_feats_conf["win_length"] == 1200 and "log_base" not in c.gst_feats_conf
    s = FS2DurationConfig.from_espnet(_conf(gst_conv_layers=4, gst_conv_chans_list=[16, 32, 32, 64], gst_conv_kernel_size=5,
                                            gst_gru_units=96, gst_heads=2, gst_tokens=7, spk_embed_dim=512), gst=True)
    assert (s.gst_tokens, s.gst_heads, s.gst_conv_kernel, s.gst_gru_units, s.spk_embed_dim) == (7, 2, 5, 96, 512)
    assert s.gst_plan() == [(1, 16, 80, 40), (16, 32, 40, 20), (32, 32, 20, 10), (32, 64, 10, 5)]
    # the extractor's own defaults fill what feats_extract_conf leaves out
    d = FS2DurationConfig.from_espnet(_conf(feats=dict(fs="22050", n_mels=64)), gst=True)
    assert (d.gst_feats_conf["fs"], d.gst_feats_conf["n_fft"], d.gst_feats_conf["hop_length"], d.n_mels) == (22050, 1024, 256, 64)
    assert d.gst_plan()[0] == (1, 32, 64, 32)
    # a model without GST is what it was, and gst=True does not fit it
    plain = FS2DurationConfig.from_espnet({"tts": "fastspeech2", "tts_conf": dict(LJ_CONF), "token_list": TOKENS})
    assert not plain.use_gst
    with pytest.raises(ValueError, match="use_gst"):
        FS2DurationConfig.from_espnet({"tts": "fastspeech2", "tts_conf": dict(LJ_CONF), "token_list": TOKENS}, gst=True)


def test_default_refusal_points_to_the_argument():
    from a3t_amd.duration import FS2DurationConfig
    with pytest.raises(NotImplementedError, match="use_gst") as e:
        FS2DurationConfig.from_espnet(_conf())
    assert "gst=True" in str(e.value)


@pytest.mark.parametrize("kw,field", [
    (dict(gst_gru_layers=2), "gst_gru_layers"),
    (dict(gst_conv_kernel_size=4), "gst_conv_kernel_size"),
    (dict(gst_conv_stride=0), "gst_conv_stride"),
    (dict(gst_gru_units=256), "gst_gru_units"),
    (dict(gst_tokens=200), "gst_tokens"),
    (dict(fe="linear_spectrogram"), "feats_extract"),
    (dict(feats=dict(FBANK, log_base=None)), "log_base"),
    (dict(feats=dict(FBANK, htk=True)), "Slaney"),
])
def test_gst_refusals_name_the_field(kw, field):
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    with pytest.raises(NotImplementedError, match=field):
        FS2DurationModel(FS2DurationConfig.from_espnet(_conf(**kw), gst=True), "cpu")


def test_gst_conv_layers_must_fit_the_channel_list():
    from a3t_amd.duration import FS2DurationConfig
    with pytest.raises(ValueError, match="gst_conv_layers"):
        FS2DurationConfig.from_espnet(_conf(gst_conv_layers=5), gst=True)
    with pytest.raises(ValueError, match="gst_heads"):
        FS2DurationConfig.from_espnet(_conf(gst_heads=5), gst=True)


# ----------------------------------------------------------------------------------------------------------- key map
@pytest.mark.parametrize("case", CASES)
def test_key_map_covers_every_gst_tensor(case):
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel, key_map
    meta = R.meta()
    cfg, sd = R.checkpoint(meta, case)
    c = FS2DurationConfig.from_espnet(cfg, gst=True)
    mapped = {k for k, _, _, _ in key_map(c)}
    gst = {"tts." + k for k in meta["cases"][case]["shapes"] if k.startswith("gst.")}
    assert len(gst) >= 30 - 12 * (case == "gst_small")
    assert {k for k in gst if not k.endswith("num_batches_tracked")} == {k for k in mapped if k.startswith("tts.gst.")}
    sd = {"tts." + k: v for k, v in sd.items()}
    m = FS2DurationModel(c, "cpu").load_state_dict(sd)      # num_batches_tracked is there and is ignored
    p, buf = m.store.p, m.store.buf
    # Conv2d [Cout][Cin][kt][kf] -> [kt][kf][Cin][Cout]
    w = sd["tts.gst.ref_enc.convs.3.weight"]
    assert torch.equal(p["gst.conv.1.w"], w.permute(2, 3, 1, 0)) and p["gst.conv.1.w"].shape[2] == c.gst_conv_chans[0]
    assert torch.equal(buf["gst.conv.2.bn.rv"], sd["tts.gst.ref_enc.convs.7.running_var"])
    assert torch.equal(p["gst.conv.0.bn.g"], sd["tts.gst.ref_enc.convs.1.weight"])
    # weight_ih columns c * F' + f -> f * C + c (the conv output is channels-last)
    C, Fq = c.gst_plan()[-1][1], c.gst_plan()[-1][3]
    wih = sd["tts.gst.ref_enc.gru.weight_ih_l0"]
    assert wih.shape == (3 * c.gst_gru_units, C * Fq)
    assert p["gst.gru.wih"][5, 1 * C + 3] == wih[5, 3 * Fq + 1]
    x = torch.randn(Fq, C)
    assert torch.allclose(p["gst.gru.wih"] @ x.reshape(-1), wih @ x.t().reshape(-1), atol=1e-5)
    assert torch.equal(p["gst.stl.embs"], sd["tts.gst.stl.gst_embs"])
    assert torch.equal(p["gst.stl.q.w"], sd["tts.gst.stl.mha.linear_q.weight"])
    # what the weights alone decide: folded BatchNorm and the tokens' keys and values
    g = m._gst_derived()
    bn = "tts.gst.ref_enc.convs.4."
    sc = sd[bn + "weight"].double() / torch.sqrt(sd[bn + "running_var"].double() + 1e-5)
    assert torch.allclose(g["scale.1"].double(), sc, rtol=1e-6, atol=0)
    assert torch.allclose(g["shift.1"].double(), sd[bn + "bias"].double() - sd[bn + "running_mean"].double() * sc, rtol=1e-6, atol=1e-7)
    e = torch.tanh(sd["tts.gst.stl.gst_embs"])
    assert torch.allclose(g["k"], e @ sd["tts.gst.stl.mha.linear_k.weight"].t() + sd["tts.gst.stl.mha.linear_k.bias"], atol=1e-5)
    assert g["v"].shape == (c.gst_tokens, c.adim)
    # a missing GST tensor and a GST tensor the config does not have are both named
    bad = dict(sd)
    del bad["tts.gst.ref_enc.gru.bias_hh_l0"]
    with pytest.raises(KeyError, match="bias_hh_l0"):
        FS2DurationModel(c, "cpu").load_state_dict(bad)
    extra = dict(sd, **{"tts.gst.ref_enc.gru.weight_ih_l1": torch.zeros(3, 3)})
    with pytest.raises(KeyError, match="weight_ih_l1"):
        FS2DurationModel(c, "cpu").load_state_dict(extra)


def test_a_plain_model_still_refuses_gst_tensors_and_style():
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    c = FS2DurationConfig.from_espnet({"tts": "fastspeech2", "tts_conf": dict(LJ_CONF), "token_list": TOKENS})
    m = FS2DurationModel(c, "cpu")
    assert m.feats is None and not any(k.startswith("gst.") for k in m.store.p)
    with pytest.raises(ValueError, match="GST"):
        m.style_embedding(np.zeros(4000, np.float32))
    with pytest.raises(ValueError, match="style"):
        m._check_style(torch.zeros(1, c.adim), 1, None)
    fn = m.duration_fn(24000, 300)
    assert not getattr(fn, "needs_prompt", False) and not hasattr(fn, "with_prompt")


def test_gst_duration_fn_needs_the_prompt_and_the_extractors_rate():
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    m = FS2DurationModel(FS2DurationConfig.from_espnet(_conf(), gst=True), "cpu")
    with pytest.raises(ValueError, match="sampling rate"):
        m.duration_fn(16000, 300)
    fn = m.duration_fn(24000, 300)
    assert fn.needs_prompt is True and callable(fn.with_prompt) and callable(fn.batch)
    with pytest.raises(ValueError, match="prompt"):
        fn(["K", "AH0"])
    with pytest.raises(ValueError, match="prompts"):
        fn.batch([["K"], ["T"]])
    with pytest.raises(ValueError, match="prompts"):
        fn.batch([["K"], ["T"]], prompts=[np.zeros(3000, np.float32)])
    with pytest.raises(ValueError, match="style"):
        m._check_style(None, 1, None)


# ------------------------------------------------------------------------------------- the restatement and the fixture
def test_fixture_is_data_only_small_and_not_vacuous():
    meta = R.meta()
    assert set(meta["cases"]) == set(CASES)
    for n in ("gst_duration.json", "gst_duration.npz"):
        assert os.path.getsize(os.path.join(G, n)) < 1 << 20
    assert meta["mel_lengths"] == list(R.MEL_LENGTHS) and 64 in R.MEL_LENGTHS and 65 in R.MEL_LENGTHS and max(R.MEL_LENGTHS) > 2000
    assert meta["overrides"] == R.OVERRIDES
    for case, info in meta["cases"].items():
        for fr in info["nonzero"].values():
            assert all(0.1 <= v <= 0.9 for v in fr)
        assert info["prompts_apart"] >= 0.1 and info["frames_changed_by_style"] >= 1 and info["frames_changed_by_prompt"] >= 1
        assert all(v["style"] < 1e-5 for k, v in info["fp64"].items() if k != "logd_abs")
        assert all(0 < v["style_moved"] < 1e-3 for v in info["sensitivity"].values())
    recs = meta["duration_predict"]
    assert len(recs) >= 20 and {r["wav"] for r in recs} == {"a", "b"} and any(r["spembs"] for r in recs)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(case):
    """Every stage within 1e-4 of its scale (the project's fp32 bound for this model); on the CPU both sides run torch's own
    kernels, so the distance is in fact a few ulp."""
    meta, z = R.meta(), R.arrays()
    cfg, sd = R.checkpoint(meta, case)
    seed = meta["cases"][case]["seed"]
    for L in R.MEL_LENGTHS:
        conv, ref, style = R.style_encoder(sd, cfg["tts_conf"], torch.from_numpy(R.mel_input(L, seed))[None])
        p = f"{case}.M{L}."
        if L in R.CONV_LENGTHS:
            assert conv[0].shape == z[p + "conv"].shape
            assert np.abs(conv[0].numpy() - z[p + "conv"]).max() <= 1e-4 * max(1.0, np.abs(z[p + "conv"]).max())
        assert np.abs(ref[0].numpy() - z[p + "ref_embs"]).max() <= 1e-4
        assert np.abs(style[0].numpy() - z[p + "style"]).max() <= 1e-4 * max(1.0, np.abs(z[p + "style"]).max())
    if case != "gst_small":     # the GRU of the default plan: one step up to 64 frames, the second at 65
        chans, k, s, _, _ = R.plan_of(cfg["tts_conf"])
        steps = {}
        for L in (64, 65):
            steps[L] = L
            for _ in chans:
                steps[L] = R.out_len(steps[L], k, s)
        assert steps == {64: 1, 65: 2}


@pytest.mark.parametrize("case", ["gst_xadd", "gst_small"])
@pytest.mark.parametrize("fill", [0.0, 1e3])
def test_ragged_rows_of_the_restatement_equal_the_rows_alone(case, fill):
    """Whatever is behind a row's length.  Bound: 1e-5 of scale -- the batch and the single run may take different blocking
    inside torch's conv and matmul, which reorders fp32 sums; nothing else may differ."""
    meta = R.meta()
    cfg, sd = R.checkpoint(meta, case)
    seed = meta["cases"][case]["seed"]
    order = (65, 1, 401, 64, 63, 130)
    mels = [R.mel_input(L, seed) for L in order]
    x, lens = R.pad_batch(mels, fill)
    conv, ref, style = R.style_encoder(sd, cfg["tts_conf"], x, lens)
    for b, m in enumerate(mels):
        c1, r1, s1 = R.style_encoder(sd, cfg["tts_conf"], torch.from_numpy(m)[None])
        n = c1.shape[2]
        assert np.abs((conv[b, :, :n] - c1[0]).numpy()).max() <= 1e-5 * max(1.0, float(c1.abs().max()))
        assert float(conv[b, :, n:].abs().max()) == 0.0 if conv.shape[2] > n else True
        assert float((ref[b] - r1[0]).abs().max()) <= 1e-5 and float((style[b] - s1[0]).abs().max()) <= 1e-5 * max(1.0, float(s1.abs().max()))
    if fill == 0.0:     # and the rule is needed: plain zero padding without it moves the style embedding
        _, _, loose = R.style_encoder(sd, cfg["tts_conf"], x, None)
        assert float((loose[4] - style[4]).abs().max()) > 1e-5


# ------------------------------------------------------------------------------------------------------------ planning
class _PromptedDur:
    """A stand-in for FS2DurationModel.duration_fn of a GST checkpoint: the durations depend on the prompt's mean level."""

    def __init__(self, base, with_batch=True):
        self.base, self.needs_prompt = base, True
        self.batch_calls, self.bound, self.styles = [], [], []
        if with_batch:
            self.batch = self._batch

    def _scale(self, wav):
        self.styles.append(id(wav))
        return 1.0 + float(np.abs(np.asarray(wav)).mean())

    def __call__(self, phns):
        raise ValueError("needs a prompt")

    def with_prompt(self, wav):
        self.bound.append(id(wav))
        k = self._scale(wav)
        return lambda phns: [k * v for v in self.base(phns)]

    def _batch(self, phn_lists, prompts=None):
        assert prompts is not None and len(prompts) == len(phn_lists)
        self.batch_calls.append(([tuple(p) for p in phn_lists], [id(w) for w in prompts]))
        scale = {}
        for w in prompts:       # one style per distinct prompt object
            if id(w) not in scale:
                scale[id(w)] = self._scale(w)
        return [[scale[id(w)] * v for v in self.base(p)] for p, w in zip(phn_lists, prompts)]


def _requests():
    from test_sedit_batch_host import _fixture, _requests as make
    fx, waves, dur = _fixture()
    reqs, cases = make(fx, waves)
    return fx, reqs, cases, dur


def test_plan_batch_with_a_prompted_duration_function():
    from a3t_amd import sedit
    from test_sedit_batch_host import _ids
    fx, reqs, cases, base = _requests()
    reqs = list(reqs) + [replace(reqs[0])]          # the same prompt OBJECT and the same edit once more
    cases = list(cases) + [cases[0]]
    fs, hop = fx["fs"], fx["hop"]
    fn = _PromptedDur(base)
    plans, data = sedit.plan_batch(reqs, fs, hop, fn, _ids)
    assert len(fn.batch_calls) == 1 and not fn.bound                   # ONE .batch call, nothing asked one by one
    lists, prompts = fn.batch_calls[0]
    want = []
    for i, r in enumerate(reqs):
        _, _, old_phns, phns, _, _ = sedit.get_phns_and_spans(r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)
        for q in sedit.duration_queries(old_phns, phns, r.new_str, r.mask_reconstruct, r.start_end_sp):
            if (i, tuple(q)) not in [(j, l) for j, l, _ in want]:
                want.append((i, tuple(q), id(r.wav_org)))
    assert lists == [l for _, l, _ in want] and prompts == [w for _, _, w in want]      # the right prompt per query
    assert len(lists) > len(set(lists))                 # the same phone list under two requests is asked for each of them
    # shared prompt objects: one style each
    assert len(fn.styles) == len({id(r.wav_org) for r in reqs}) < len(reqs)
    # plans equal to the per-request plans
    for r, c, p in zip(reqs, cases, plans):
        args = (r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)
        ms, me, op, nph, rep, add = sedit.get_phns_and_spans(*args)
        one = sedit.prepare_features_with_duration(np.asarray(r.wav_org, np.float32), fs, hop, ms, me, op, nph, rep, add,
                                                   sedit.bind_prompt(_PromptedDur(base), r.wav_org), r.new_str, **c["opts"])
        assert np.array_equal(p.wav, np.asarray(one[0])) and list(p.phns) == list(one[1])
        assert list(p.align_start) == list(one[2]) and list(p.align_end) == list(one[3])
        assert list(p.old_span_boundary) == [int(x) for x in one[4]] and list(p.new_span_boundary) == [int(x) for x in one[5]]
    # the prompt matters: a plain function of the same base plans differently
    plain, _ = sedit.plan_batch(reqs, fs, hop, base, _ids)
    assert any(list(a.new_span_boundary) != list(b.new_span_boundary) for a, b in zip(plans, plain))


def test_plan_batch_without_a_batch_attribute_binds_each_request_once():
    from a3t_amd import sedit
    from test_sedit_batch_host import _ids
    fx, reqs, cases, base = _requests()
    fn = _PromptedDur(base, with_batch=False)
    plans, _ = sedit.plan_batch(reqs, fx["fs"], fx["hop"], fn, _ids)
    with_batch, _ = sedit.plan_batch(reqs, fx["fs"], fx["hop"], _PromptedDur(base), _ids)
    assert len(fn.bound) == len(set(fn.bound)) <= len(reqs)          # at most one binding (one style) per request
    for a, b in zip(plans, with_batch):
        assert np.array_equal(a.wav, b.wav) and a.new_span_boundary == b.new_span_boundary


def test_bind_prompt_leaves_plain_callables_alone():
    from a3t_amd import sedit
    f = lambda phns: [0.1] * len(phns)
    assert sedit.bind_prompt(f, np.zeros(10)) is f
    fn = _PromptedDur(lambda phns: [0.1] * len(phns))
    wav = np.ones(10, np.float32)
    assert sedit.bind_prompt(fn, wav)(["K"]) == [0.2] and fn.bound == [id(wav)]
