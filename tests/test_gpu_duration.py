"""The FastSpeech2 duration model on the MI355X (a3t_amd/duration.py, csrc/duration.hip) against the reference's own
outputs in tests/golden/fs2_duration.{npz,json} (tests/golden/make_golden_fs2.py)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"


def _meta():
    return json.load(open(os.path.join(G, "fs2_duration.json")))


def _checkpoint(meta, case):
    m = meta["cases"][case]
    shapes = {k: tuple(v) for k, v in m["shapes"].items()}
    state = O.procedural_state(shapes, m["seed"])
    import sys
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden_fs2 import apply_overrides      # the fixture's documented overrides (imports nothing of the reference)
    apply_overrides(state, m["tts_conf"].get("duration_predictor_layers", 2))
    cfg = {"tts": "fastspeech2", "tts_conf": m["tts_conf"], "token_list": meta["token_list"]}
    # (procedural_state seeds by name: the weights are drawn under the FastSpeech2 names, the checkpoint carries 'tts.')
    return cfg, {"tts." + k: torch.from_numpy(np.array(v)) for k, v in state.items()}


_MODELS = {}


def _model(case):
    if case not in _MODELS:
        from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
        cfg, sd = _checkpoint(_meta(), case)
        _MODELS[case] = FS2DurationModel(FS2DurationConfig.from_espnet(cfg), DEV).load_state_dict(sd)
    return _MODELS[case]


def _tie_distance(e):
    """Distance of e to the nearest k + 0.5."""
    e = np.asarray(e, np.float64)
    return np.abs(e - np.floor(e) - 0.5)


# ---------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("C", [256, 384])
@pytest.mark.parametrize("M", [1, 37, 301])
def test_duration_head_against_fp64(C, M):
    from a3t_amd import ops
    g = torch.Generator().manual_seed(C * 1000 + M)
    z = torch.relu(torch.randn(M, C, generator=g) * 2.0)
    gam = 1.0 + 0.2 * torch.rand(C, generator=g)
    bet = 0.1 * torch.randn(C, generator=g)
    w = torch.randn(C, generator=g) / C ** 0.5
    b = torch.tensor([1.7])
    d = lambda t: t.to(DEV).contiguous()
    logd = torch.empty(M, device=DEV)
    frames = torch.empty(M, dtype=torch.int64, device=DEV)
    ops.duration_head(d(z), d(gam), d(bet), d(w), d(b), logd, frames, eps=1e-12, offset=1.0)
    torch.cuda.synchronize()
    z64 = z.double()
    mu = z64.mean(1, keepdim=True)
    var = ((z64 - mu) ** 2).mean(1, keepdim=True)
    y = (z64 - mu) / torch.sqrt(var + 1e-12) * gam.double() + bet.double()
    x = (y * w.double()).sum(1) + 1.7
    got = logd.cpu().double()
    assert (got - x).abs().max().item() < 1e-5
    e = np.exp(got.numpy()) - 1.0
    want = np.maximum(np.rint(e), 0).astype(np.int64)
    ok = _tie_distance(e) > 1e-6
    assert ok.sum() >= M - 1
    assert np.array_equal(frames.cpu().numpy()[ok], want[ok])


@pytest.mark.parametrize("offset,want", [(0.5, 0), (-0.5, 2), (-1.5, 2), (1.0, 0), (0.0, 1)])
def test_duration_head_exact_ties_round_half_to_even(offset, want):
    """Zero gamma, beta and bias make x = 0 exactly: exp(0) - offset = 0.5, 1.5, 2.5 are ties (torch.round: to even)."""
    from a3t_amd import ops
    M, C = 9, 384
    z = torch.rand(M, C, device=DEV)
    zero = torch.zeros(C, device=DEV)
    logd = torch.empty(M, device=DEV)
    frames = torch.empty(M, dtype=torch.int64, device=DEV)
    ops.duration_head(z, zero, zero, torch.ones(C, device=DEV), torch.zeros(1, device=DEV), logd, frames, offset=offset)
    torch.cuda.synchronize()
    assert torch.all(logd == 0)
    assert frames.cpu().tolist() == [want] * M
    assert int(torch.round(torch.exp(torch.zeros(1)) - offset).clamp(min=0)) == want


def test_duration_head_rejects_unsupported_width():
    from a3t_amd import _lib, ops
    z = torch.zeros(4, 576, device=DEV)
    with pytest.raises(_lib.A3TLibraryError):
        ops.duration_head(z, z[0], z[0], z[0], z[0, :1], torch.empty(4, device=DEV),
                          torch.empty(4, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------------ the whole model
@pytest.mark.parametrize("case", ["lj", "lj_xadd", "lj_xcat", "small_c384"])
def test_model_against_reference(case):
    meta = _meta()
    z = np.load(os.path.join(G, "fs2_duration.npz"))
    m = _model(case)
    bias = m.speaker_bias(z[f"{case}.spembs"]) if f"{case}.spembs" in z else None
    for T in meta["lengths"]:
        p = f"{case}.T{T}."
        ids = torch.from_numpy(z[p + "ids"]).to(DEV)
        hs, logd, frames = m.forward_ids(ids, bias)
        torch.cuda.synchronize()
        logd, frames = logd.cpu().numpy(), frames.cpu().numpy()
        assert np.abs(logd - z[p + "logd"]).max() <= 1e-4, (T, np.abs(logd - z[p + "logd"]).max())
        far = _tie_distance(z[p + "expm1"]) > 1e-3
        assert np.array_equal(frames[far], z[p + "frames"][far]), T
        assert np.abs(frames - z[p + "frames"]).max() <= 1
        if T == meta["hs_length"]:
            ref = z[p + "hs"]
            err = np.abs(hs.cpu().numpy() - ref).max()
            assert err <= 1e-4 * max(1.0, np.abs(ref).max()), err


def test_duration_fn_matches_duration_predict_bit_for_bit():
    meta = _meta()
    z = np.load(os.path.join(G, "fs2_duration.npz"))
    assert len(meta["duration_predict"]) >= 8
    for r in meta["duration_predict"]:
        m = _model(r["model"])
        fn = m.duration_fn(meta["fs"], meta["hop"], spembs=z[f"{r['model']}.spembs"] if r["spembs"] else None)
        got = fn(r["phns"])
        assert all(type(v) is float for v in got)
        assert got == r["seconds"], (r["phns"], got, r["seconds"])


def test_duration_fn_copies_to_the_host_once_per_call():
    """The ids go up through a pinned buffer without a host wait; the one synchronisation is the frames coming down."""
    m = _model("lj")
    fn = m.duration_fn(24000, 300)
    fn(["sp", "K", "AE1", "T"])
    n = {"sync": 0}
    orig = torch.Tensor.cpu

    def counting(self, *a, **k):
        n["sync"] += 1
        return orig(self, *a, **k)
    torch.Tensor.cpu = counting
    try:
        out = fn(["sp", "K", "AE1", "T", "sp"])
    finally:
        torch.Tensor.cpu = orig
    assert n["sync"] == 1 and len(out) == 5


def test_from_file_matches_in_memory(tmp_path):
    import yaml
    from a3t_amd.duration import FS2DurationModel
    meta = _meta()
    cfg, sd = _checkpoint(meta, "lj_xcat")
    sd["normalize.mean"] = torch.zeros(80)
    sd["energy_normalize.std"] = torch.ones(1)
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(dict(cfg, normalize="global_mvn", optim="adam"), f)
    torch.save(sd, tmp_path / "train.loss.ave.pth")
    a = FS2DurationModel.from_file(None, str(tmp_path / "train.loss.ave.pth"), DEV)
    b = FS2DurationModel.from_file(str(tmp_path / "config.yaml"), str(tmp_path / "train.loss.ave.pth"), DEV)
    m = _model("lj_xcat")
    z = np.load(os.path.join(G, "fs2_duration.npz"))
    phns = ["sp", "HH", "AH0", "L", "OW1", "sp", "W", "ER1", "L", "D"]
    want = m.predict_frames(phns, m.speaker_bias(z["lj_xcat.spembs"]))
    for x in (a, b):
        assert np.array_equal(x.predict_frames(phns, x.speaker_bias(z["lj_xcat.spembs"])), want)


@pytest.mark.parametrize("kind", ["replace", "mask", "append", "delete"])
def test_speech_editor_with_native_durations(kind):
    """SpeechEditor(duration_fn=<the native model>) plans every sedit.json edit kind exactly as the oracle's restatement of
    prepare_features_with_duration does when it is driven by the reference's recorded duration_predict outputs."""
    from a3t_amd import sedit
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import SpeechEditor
    from a3t_amd.task import MLMTask
    from test_gpu_e2e import _task_args
    meta = _meta()
    rec = {tuple(r["phns"]): r["seconds"] for r in meta["duration_predict"] if r["model"] == "lj" and not r["spembs"]}
    asked = []

    def recorded(phns):
        asked.append(tuple(phns))
        return list(rec[tuple(phns)])
    fx = json.load(open(os.path.join(G, "sedit.json")))
    case = [c for c in fx["cases"] if c["kind"] == kind][0]
    oc = O.tiny_config()
    wav = (0.1 * np.random.RandomState(5).standard_normal(
        np.load(os.path.join(G, "sedit_wav.npz"))[case["wav"] + ".in"].shape[0])).astype(np.float32)
    args = (case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"], case["new_str"])
    native = _model("lj").duration_fn(oc.fs, oc.hop_length)
    ms, me, op, nph, rep, add = O.sedit_phone_spans(*args)
    want = O.sedit_plan_edit(wav, oc.fs, oc.hop_length, ms, me, op, nph, rep, add, recorded, case["new_str"], **case["opts"])
    assert asked, "the plan asked for no durations"
    got = sedit.prepare_features_with_duration(wav, oc.fs, oc.hop_length, list(ms), list(me), list(op), list(nph), rep, add,
                                               native, case["new_str"], **case["opts"])
    assert np.array_equal(got[0], want[0])
    assert list(got[1]) == list(want[1]) and list(got[2]) == list(want[2]) and list(got[3]) == list(want[3])
    assert tuple(got[4]) == tuple(want[4]) and tuple(got[5]) == tuple(want[5])
    # and the whole editor with it
    model = MLMTask.build_model(_task_args(oc), device=DEV)
    state = O.procedural_state(O.param_shapes(oc), 1)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    ed = SpeechEditor(model, coll, None, ids, native)
    res = ed.edit(wav, *args, **case["opts"])
    assert tuple(res["old_span_boundary"]) == tuple(want[4]) and tuple(res["new_span_boundary"]) == tuple(want[5])
    assert res["feat"].shape[1] == 80 and torch.isfinite(torch.as_tensor(res["feat"])).all()
