"""The GST style encoder of the duration model on the MI355X (a3t_amd/csrc/gst.hip, FS2DurationModel.style_embedding(_batch),
the style= argument of the forwards, duration_fn(...).with_prompt and the speech editor with a GST duration model) against the
reference's own outputs in tests/golden/gst_duration.{npz,json} and the CPU restatement tests/gst_ref.py.

Bounds.  From given log-mel frames every stage is held to 1e-4 of the tensor's scale, max(1, max |reference|): the project's
fp32 bound for this model (test_model_against_reference puts it on hs).  From a waveform the device's own log-mel comes first,
which tests/golden/logmel.npz holds to 2e-4 per element; the fixture records how far the reference's style embedding (and the
log-domain durations behind it) move when its mel moves by +-2e-4, and the bound is the one above plus twice that.  The
log-domain durations are held to 1e-4 and the frames are exact away from rounding ties, as in test_gpu_duration.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import gst_ref as R
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
CASES = ("gst_xadd", "gst_xcat", "gst_plain", "gst_small")
TOL = 1e-4

_MODELS, _SD = {}, {}


def _checkpoint(case):
    if case not in _SD:
        _SD[case] = R.checkpoint(R.meta(), case)
    return _SD[case]


def _model(case):
    if case not in _MODELS:
        from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
        cfg, sd = _checkpoint(case)
        _MODELS[case] = FS2DurationModel(FS2DurationConfig.from_espnet(cfg, gst=True), DEV).load_state_dict(
            {"tts." + k: v for k, v in sd.items()})
    return _MODELS[case]


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _scale(a):
    return max(1.0, float(np.abs(np.asarray(a)).max()))


def _token_ids(T, seed):
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden_fs2 import token_ids
    return token_ids(T, seed)


def _tie_distance(e):
    e = np.asarray(e, np.float64)
    return np.abs(e - np.floor(e) - 0.5)


def _sd64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


# --------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("lens", [[1], [63, 64, 65, 1], [401, 65, 130, 2], [1003, 7], [2050, 1, 64]])
@pytest.mark.parametrize("case", ["gst_xadd", "gst_small"])
def test_conv_bn_relu_layers_against_the_restatement(case, lens):
    """Every layer on its own: the restatement's (fp64) input of layer i, NaN behind every row's length, through the kernel,
    against the restatement's output of layer i.  Valid positions within 1e-4 of scale, exact zeros behind n'."""
    from a3t_amd import ops
    m = _model(case)
    cfg, sd = _checkpoint(case)
    seed = R.meta()["cases"][case]["seed"]
    mels = [R.mel_input(n, seed + b) for b, n in enumerate(lens)]
    x, _ = R.pad_batch(mels, 0.0)
    sd64 = _sd64(sd)
    k, s = m.c.gst_conv_kernel, m.c.gst_conv_stride
    g = m._gst_derived()
    cur, cur_lens = x.double().unsqueeze(1), list(lens)          # [B][C][T][F]
    for i in range(len(m.c.gst_conv_chans)):
        nxt, nxt_lens = R.conv_stack(sd64, cfg["tts_conf"], x.double(), lens, upto=i + 1)
        xin = cur.permute(0, 2, 3, 1).float().contiguous()       # channels-last
        for b, n in enumerate(cur_lens):
            xin[b, n:] = float("nan")
        B, T, F_, C = xin.shape
        y = torch.full((B, R.out_len(T, k, s), R.out_len(F_, k, s), m.c.gst_conv_chans[i]), float("nan"), device=DEV)
        ops.gst_conv_bn_relu(xin.to(DEV), m.store.p[f"gst.conv.{i}.w"], g[f"scale.{i}"], g[f"shift.{i}"], y, _lens(cur_lens), k, s)
        torch.cuda.synchronize()
        got = y.cpu().permute(0, 3, 1, 2).double()
        assert got.shape == nxt.shape
        for b, n in enumerate(nxt_lens):
            assert torch.all(got[b, :, n:] == 0), (i, b, n)
            err = (got[b, :, :n] - nxt[b, :, :n]).abs().max().item()
            assert err <= TOL * max(1.0, nxt[b, :, :n].abs().max().item()), (i, b, n, err)
        cur, cur_lens = nxt, nxt_lens


def test_conv_without_lengths_is_the_full_rows_and_bad_shapes_are_refused():
    from a3t_amd import _lib, ops
    m = _model("gst_xadd")
    g = m._gst_derived()
    x = torch.from_numpy(np.stack([R.mel_input(65, 1), R.mel_input(65, 2)]))[..., None].to(DEV)
    a = torch.empty(2, 33, 40, 32, device=DEV)
    b = torch.empty_like(a)
    w = m.store.p["gst.conv.0.w"]
    ops.gst_conv_bn_relu(x, w, g["scale.0"], g["shift.0"], a, None, 3, 2)
    ops.gst_conv_bn_relu(x, w, g["scale.0"], g["shift.0"], b, _lens([65, 65]), 3, 2)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and float(a.max()) > 0
    with pytest.raises(ValueError):
        ops.gst_conv_bn_relu(x, w, g["scale.0"], g["shift.0"], torch.empty(2, 32, 40, 32, device=DEV), None, 3, 2)
    rc = _lib.load().a3t_gst_conv_bn_relu(None, None, None, None, None, None, 2, 65, 80, 1, 32, 4, 2, None)      # even kernel
    assert rc == -22
    assert _lib.load().a3t_gst_gru_stl(*([None] * 12), 1, 4, 129, 384, 4, 10, None) == -22                          # H > 128
    assert _lib.load().a3t_gst_gru_stl(*([None] * 12), 1, 4, 128, 384, 5, 10, None) == -22                          # d % heads
    assert _lib.load().a3t_gst_add_style(None, None, None, 3, 4, 8, 2, None) == -22                                 # 2 styles, 3 rows


@pytest.mark.parametrize("T,lens", [(1, [1]), (2, [2, 1]), (16, [16, 1, 7, 15]), (33, [33, 32, 2])])
@pytest.mark.parametrize("case", ["gst_xcat", "gst_small"])
def test_gru_and_token_attention_against_the_restatement(case, T, lens):
    """Random GRU inputs of the scale the conv stack gives; the input projections computed on the host in fp64, NaN behind
    every row's steps; ref_embs and style against the restatement in fp64."""
    from a3t_amd import ops
    m = _model(case)
    cfg, sd = _checkpoint(case)
    sd64, p = _sd64(sd), m.store.p
    H, d, B = m.c.gst_gru_units, m.c.adim, len(lens)
    n_in = sd["gst.ref_enc.gru.weight_ih_l0"].shape[1]
    gen = torch.Generator().manual_seed(T * 100 + B)
    xs = torch.relu(torch.randn(B, T, n_in, generator=gen) * 3.0).double()
    ref = R.gru(sd64, xs, lens)
    style = R.style_tokens(sd64, cfg["tts_conf"], ref)
    gi = (xs @ sd64["gst.ref_enc.gru.weight_ih_l0"].t() + sd64["gst.ref_enc.gru.bias_ih_l0"]).float()
    for b, n in enumerate(lens):
        gi[b, n:] = float("nan")
    g = m._gst_derived()
    got_ref = torch.full((B, H), float("nan"), device=DEV)
    got = torch.full((B, d), float("nan"), device=DEV)
    ops.gst_gru_stl(gi.to(DEV), p["gst.gru.whh"], p["gst.gru.bhh"], _lens(lens), p["gst.stl.q.w"], p["gst.stl.q.b"], g["k"], g["v"],
                    p["gst.stl.out.w"], p["gst.stl.out.b"], got_ref, got, m.c.gst_heads)
    torch.cuda.synchronize()
    e_ref = (got_ref.cpu().double() - ref).abs().max().item()
    e_sty = (got.cpu().double() - style).abs().max().item()
    print(f"{case} T={T} lens={lens}: ref_embs err {e_ref:.3g}, style err {e_sty:.3g} (scale {style.abs().max().item():.3g})")
    assert float(ref.abs().max()) > 0.05
    assert e_ref <= TOL and e_sty <= TOL * max(1.0, style.abs().max().item())
    # ref_embs is optional
    again = torch.empty_like(got)
    ops.gst_gru_stl(gi.to(DEV), p["gst.gru.whh"], p["gst.gru.bhh"], _lens(lens), p["gst.stl.q.w"], p["gst.stl.q.b"], g["k"], g["v"],
                    p["gst.stl.out.w"], p["gst.stl.out.b"], None, again, m.c.gst_heads)
    torch.cuda.synchronize()
    assert torch.equal(again, got)


def test_add_style_rows():
    from a3t_amd import ops
    B, T, d = 5, 37, 384
    gen = torch.Generator().manual_seed(1)
    hs = torch.randn(B, T, d, generator=gen)
    st = torch.randn(3, d, generator=gen)
    rows = [2, 0, 0, 1, 2]
    a = hs.clone().to(DEV)
    ops.gst_add_style(a, st.to(DEV), B, T, rows=_lens(rows))
    b = hs.clone().to(DEV)
    ops.gst_add_style(b, st[:1].contiguous().to(DEV), B, T)
    c = hs[:3].clone().to(DEV)
    ops.gst_add_style(c.view(3 * T, d), st.to(DEV), 3, T)
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), hs + st[rows][:, None, :])
    assert torch.equal(b.cpu(), hs + st[0][None, None, :])
    assert torch.equal(c.cpu(), hs[:3] + st[:, None, :])


# ---------------------------------------------------------------------------------------------------- the style encoder
@pytest.mark.parametrize("case", CASES)
def test_style_from_the_fixtures_mels(case):
    """Per model and per length, one prompt per call: last conv output, ref_embs and style against the reference."""
    meta, z = R.meta(), R.arrays()
    m = _model(case)
    info = meta["cases"][case]
    worst = {"conv": 0.0, "ref_embs": 0.0, "style": 0.0}
    for L in R.MEL_LENGTHS:
        keep = {}
        style = m.style_from_mel(torch.from_numpy(R.mel_input(L, info["seed"]))[None].to(DEV), keep=keep)
        torch.cuda.synchronize()
        p = f"{case}.M{L}."
        assert style.shape == (1, m.c.adim)
        got = {"ref_embs": keep["ref_embs"][0].cpu().numpy(), "style": style[0].cpu().numpy()}
        if L in R.CONV_LENGTHS:
            got["conv"] = keep["conv"][0].permute(2, 0, 1).cpu().numpy()        # [T'][F'][C] -> the reference's [C][T'][F']
        for k, v in got.items():
            ref = z[p + k]
            assert v.shape == ref.shape
            err = np.abs(v - ref).max() / _scale(ref)
            worst[k] = max(worst[k], err)
            print(f"{case} mel {L} {k}: err {err:.3g} of scale (reference's own fp32-vs-fp64: {info['fp64'][str(L)][k]:.3g})")
            assert err <= TOL, (L, k, err)
    print(case, "worst", worst)


@pytest.mark.parametrize("case", CASES)
def test_a_batch_of_all_lengths_equals_the_single_calls(case):
    """The seven lengths as ONE ragged pass, through the length table: every row within the fixture's bound and the single
    call's; the conv output is the single call's bit for bit (the same kernel does the same sums), exact zeros behind it."""
    meta, z = R.meta(), R.arrays()
    m = _model(case)
    seed = meta["cases"][case]["seed"]
    order = [65, 1, 2050, 64, 401, 63, 1003]
    mels = [R.mel_input(L, seed) for L in order]
    x, lens = R.pad_batch(mels, float("nan"))
    keep = {}
    style = m.style_from_mel(x.to(DEV), m._gst_len_table(lens), keep=keep)
    torch.cuda.synchronize()
    style, ref, conv = style.cpu().numpy(), keep["ref_embs"].cpu().numpy(), keep["conv"].cpu().numpy()
    assert np.isfinite(style).all() and np.isfinite(conv).all()
    for b, L in enumerate(order):
        p = f"{case}.M{L}."
        assert np.abs(style[b] - z[p + "style"]).max() <= TOL * _scale(z[p + "style"]), L
        assert np.abs(ref[b] - z[p + "ref_embs"]).max() <= TOL, L
        k1 = {}
        s1 = m.style_from_mel(torch.from_numpy(mels[b])[None].to(DEV), keep=k1)
        torch.cuda.synchronize()
        c1 = k1["conv"][0].cpu().numpy()
        assert np.array_equal(conv[b, :c1.shape[0]].view(np.int32), c1.view(np.int32)) and not conv[b, c1.shape[0]:].any(), L
        assert np.abs(style[b] - s1[0].cpu().numpy()).max() <= TOL * _scale(z[p + "style"]), L


def test_nan_padding_changes_no_bit():
    """The same ragged batch twice: zeros behind every row over a zeroed workspace, then NaN behind every row over a workspace
    filled with NaN.  Same shapes, same kernels: ref_embs and style are equal bit for bit, and finite."""
    m = _model("gst_xadd")
    order = [130, 65, 1, 401, 64]
    mels = [R.mel_input(L, 5) for L in order]
    runs = []
    for fill in (0.0, float("nan")):
        x, lens = R.pad_batch(mels, fill)
        xd, tab = x.to(DEV), m._gst_len_table(lens)
        if not runs:
            m.style_from_mel(xd, tab)          # (allocates every buffer of this shape)
            torch.cuda.synchronize()
        for t in m.ws.bufs.values():
            if t.is_floating_point():
                t.fill_(fill)
        keep = {}
        style = m.style_from_mel(xd, tab, keep=keep)
        torch.cuda.synchronize()
        runs.append((style.cpu().numpy().copy(), keep["ref_embs"].cpu().numpy().copy()))
    for a, b in zip(*runs):
        assert np.isfinite(b).all() and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_the_style_path_is_conv_layers_plus_two_launches_whatever_b():
    """Every device operation of style_from_mel goes through a3t_amd.ops; counted there for B = 1 and B = 6."""
    from a3t_amd import ops
    m = _model("gst_xadd")
    names = ("gst_conv_bn_relu", "linear_fwd", "gst_gru_stl")
    calls = []
    orig = {n: getattr(ops, n) for n in names}

    def counted(n):
        def f(*a, **k):
            calls.append(n)
            return orig[n](*a, **k)
        return f
    mels = [R.mel_input(L, 3) for L in (401, 65, 64, 1, 130, 401)]
    x1 = torch.from_numpy(mels[0])[None].to(DEV)
    x, lens = R.pad_batch(mels, 0.0)
    xd, tab = x.to(DEV), m._gst_len_table(lens)
    m.style_from_mel(xd, tab)
    m._gst_derived()
    for n in names:
        setattr(ops, n, counted(n))
    try:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            m.style_from_mel(x1)
            one = list(calls)
            m.style_from_mel(xd, tab)
    finally:
        for n in names:
            setattr(ops, n, orig[n])
    torch.cuda.synchronize()
    L = len(m.c.gst_conv_chans)
    assert one == ["gst_conv_bn_relu"] * L + ["linear_fwd", "gst_gru_stl"] and calls == one * 2
    # and nothing else ran on the device: what torch itself did only allocates or makes views
    ran = {e.key for e in prof.key_averages() if e.key.startswith("aten::")}
    views = {"aten::empty", "aten::empty_strided", "aten::view", "aten::_unsafe_view", "aten::reshape", "aten::select",
             "aten::slice", "aten::as_strided", "aten::unsqueeze", "aten::squeeze", "aten::expand", "aten::alias", "aten::detach",
             "aten::detach_", "aten::lift_fresh", "aten::transpose", "aten::permute", "aten::t"}
    assert ran <= views, sorted(ran - views)


# ------------------------------------------------------------------------------------------------- durations with a style
@pytest.mark.parametrize("case", CASES)
def test_forward_ids_with_style_against_the_reference(case):
    """The FS2 fixture's five text lengths behind the 401-frame prompt: the conventions of test_model_against_reference.  The
    style is the device's own, from the fixture's mel."""
    meta, z = R.meta(), R.arrays()
    m = _model(case)
    info = meta["cases"][case]
    bias = m.speaker_bias(z[f"{case}.spembs"]) if f"{case}.spembs" in z else None
    style = m.style_from_mel(torch.from_numpy(R.mel_input(meta["text_prompt"], info["seed"]))[None].to(DEV))
    other = m.style_from_mel(torch.from_numpy(R.mel_input(1003, info["seed"]))[None].to(DEV))
    changed = 0
    for T in meta["lengths"]:
        p = f"{case}.T{T}."
        ids = torch.from_numpy(_token_ids(T, info["seed"])).to(DEV)
        _, logd, frames = m.forward_ids(ids, bias, style)
        torch.cuda.synchronize()
        logd, frames = logd.cpu().numpy(), frames.cpu().numpy()
        err = np.abs(logd - z[p + "logd"]).max()
        print(f"{case} T={T}: max |dlogd| {err:.3g} (reference's own fp32-vs-fp64: {info['fp64']['logd_abs']:.3g})")
        assert err <= 1e-4, (T, err)
        far = _tie_distance(z[p + "expm1"]) > 1e-3
        assert far.sum() >= T - 1
        assert np.array_equal(frames[far], z[p + "frames"][far]), T
        assert np.abs(frames - z[p + "frames"]).max() <= 1
        _, _, f2 = m.forward_ids(ids, bias, other)
        changed += int((f2.cpu().numpy() != frames).sum())
    assert changed >= 1         # another prompt, other durations
    with pytest.raises(ValueError, match="style"):
        m.forward_ids(ids, bias)


@pytest.mark.parametrize("case", CASES)
def test_forward_ids_batch_with_styles_against_the_reference(case):
    """The five lengths as ONE batch: one shared style [1][d], the same style five times [B][d], and a table of two styles
    with a row index per sequence; every row within the bounds above, rows that take the other style differ."""
    meta, z = R.meta(), R.arrays()
    m = _model(case)
    info = meta["cases"][case]
    bias = m.speaker_bias(z[f"{case}.spembs"]) if f"{case}.spembs" in z else None
    prompt = torch.from_numpy(R.mel_input(meta["text_prompt"], info["seed"]))[None].to(DEV)
    style = m.style_from_mel(prompt)
    other = m.style_from_mel(torch.from_numpy(R.mel_input(1003, info["seed"]))[None].to(DEV))
    lens = list(meta["lengths"])
    ids = np.zeros((len(lens), max(lens)), np.int64)
    for b, T in enumerate(lens):
        ids[b, :T] = _token_ids(T, info["seed"])
    ids, dl = torch.from_numpy(ids).to(DEV), _lens(lens)
    table = torch.cat([other, style]).contiguous()
    variants = [(style, None, lens), (style.expand(len(lens), -1).contiguous(), None, lens),
                (table, _lens([1, 1, 0, 1, 0]), [lens[0], lens[1], lens[3]])]
    for st, rows, held in variants:
        _, logd, frames = m.forward_ids_batch(ids, dl, bias, st, rows)
        torch.cuda.synchronize()
        logd, frames = logd.cpu().numpy(), frames.cpu().numpy()
        for b, T in enumerate(lens):
            p = f"{case}.T{T}."
            if T in held:
                assert np.abs(logd[b, :T] - z[p + "logd"]).max() <= 1e-4, (T, np.abs(logd[b, :T] - z[p + "logd"]).max())
                far = _tie_distance(z[p + "expm1"]) > 1e-3
                assert np.array_equal(frames[b, :T][far], z[p + "frames"][far]), T
            else:
                assert np.abs(logd[b, :T] - z[p + "logd"]).max() > 1e-3, T
    with pytest.raises(ValueError, match="style"):
        m.forward_ids_batch(ids, dl, bias, torch.cat([style, style]).contiguous())       # 2 rows for 5 sequences, no index


# ------------------------------------------------------------------------------------------------------- from a waveform
def _wavs(meta):
    return {k: R.waveform(n, seed=i) for i, (k, n) in enumerate(sorted(meta["wav_samples"].items()))}


@pytest.mark.parametrize("case", CASES)
def test_style_embedding_from_the_waveform(case):
    """style_embedding(wav) and style_embedding_batch against the reference's gst(feats_extract(wav)): 1e-4 of scale plus twice
    what +-2e-4 on the mel moved the reference's own style."""
    meta, z = R.meta(), R.arrays()
    m = _model(case)
    wavs = _wavs(meta)
    sens = meta["cases"][case]["sensitivity"]
    single = {}
    for w, wav in wavs.items():
        ref = z[f"{case}.wav_{w}.style"]
        got = m.style_embedding(wav)
        assert got.shape == (1, m.c.adim)
        single[w] = got[0].cpu().numpy()
        err = np.abs(single[w] - ref).max() / _scale(ref)
        bound = TOL + 2 * sens[w]["style_moved"]
        print(f"{case} wav {w} ({sens[w]['frames']} frames): style err {err:.3g} of scale, bound {bound:.3g}")
        assert err <= bound, (w, err, bound)
    keys = sorted(wavs)
    both = m.style_embedding_batch([wavs[k] for k in keys] + [wavs[keys[0]]]).cpu().numpy()
    assert both.shape == (3, m.c.adim)
    for b, k in enumerate(keys + [keys[0]]):
        ref = z[f"{case}.wav_{k}.style"]
        assert np.abs(both[b] - ref).max() / _scale(ref) <= TOL + 2 * sens[k]["style_moved"]
        assert np.abs(both[b] - single[k]).max() / _scale(ref) <= TOL
    assert np.array_equal(both[0], both[2])


def test_duration_fn_with_prompt_against_duration_predict():
    """The recorded duration_predict calls (wav_org and sid given): seconds equal wherever the reference's log-domain output
    is further from a rounding tie than 1e-4 + twice what +-2e-4 on the mel moved it; one frame off at most elsewhere."""
    meta, z = R.meta(), R.arrays()
    wavs = _wavs(meta)
    recs = meta["duration_predict"]
    assert len(recs) >= 20
    step = np.float32(meta["hop"]) / np.float32(meta["fs"])
    compared = total = 0
    fns = {}
    for r in recs:
        key = (r["model"], r["wav"])
        if key not in fns:
            m = _model(r["model"])
            assert r["spembs"] == (m.c.spk_embed_dim > 0)
            fn = m.duration_fn(meta["fs"], meta["hop"], spembs=z[f"{r['model']}.spembs"] if r["spembs"] else None)
            assert fn.needs_prompt
            fns[key] = fn.with_prompt(wavs[r["wav"]])
        got = fns[key](r["phns"])
        assert all(type(v) is float for v in got) and len(got) == len(r["seconds"])
        far = np.asarray(r["tie_log"]) > 1e-4 + 2 * meta["cases"][r["model"]]["sensitivity"][r["wav"]]["logd_moved"]
        g, w = np.asarray(got, np.float32), np.asarray(r["seconds"], np.float32)
        assert np.array_equal(g[far], w[far]), (r["model"], r["wav"], r["phns"], got, r["seconds"])
        assert np.abs(g - w).max() <= step * 1.001
        compared += int(far.sum())
        total += len(got)
    assert compared >= 0.95 * total
    # .batch of a bound callable, and fn.batch with one prompt per list, answer as the single calls do
    m = _model("gst_xadd")
    fn = m.duration_fn(meta["fs"], meta["hop"], spembs=z["gst_xadd.spembs"])
    lists = [r["phns"] for r in recs if r["model"] == "gst_xadd" and r["wav"] == "a"]
    a, b = fn.with_prompt(wavs["a"]), fn.with_prompt(wavs["b"])
    assert a.batch(lists) == [a(x) for x in lists]
    prompts = [wavs["a"], wavs["b"], wavs["a"], wavs["b"]][:len(lists)]
    want = [(a if w is wavs["a"] else b)(x) for x, w in zip(lists, prompts)]
    assert fn.batch(lists, prompts=prompts) == want
    assert fn.batch(lists, prompts=prompts, max_score_elems=1) == want          # every list alone: its style stays with it
    assert fn.batch(lists[:1], prompts=prompts[1:2]) == [b(lists[0])]
    assert a(lists[0]) != b(lists[0])
    with pytest.raises(ValueError, match="prompt"):
        fn(lists[0])


def test_prompts_are_deduplicated_and_the_batch_copies_to_the_host_once():
    meta, z = R.meta(), R.arrays()
    wavs = _wavs(meta)
    m = _model("gst_plain")
    fn = m.duration_fn(meta["fs"], meta["hop"])
    lists = [r["phns"] for r in meta["duration_predict"] if r["model"] == "gst_plain" and r["wav"] == "a"]
    prompts = [wavs["a"], wavs["b"], wavs["a"], wavs["a"]][:len(lists)]
    fn.batch(lists, prompts=prompts)
    n = {"sync": 0, "mel": 0, "style": 0}
    orig_cpu, orig_mel, orig_style = torch.Tensor.cpu, m._prompt_mel, m.style_from_mel

    def counting(self, *a, **k):
        n["sync"] += 1
        return orig_cpu(self, *a, **k)

    def mel(w):
        n["mel"] += 1
        return orig_mel(w)

    def style(*a, **k):
        n["style"] += 1
        return orig_style(*a, **k)
    torch.Tensor.cpu, m._prompt_mel, m.style_from_mel = counting, mel, style
    try:
        out = fn.batch(lists, prompts=prompts)
        bound = fn.with_prompt(wavs["a"])
        after_bind = dict(n)
        for x in lists:
            bound(x)
    finally:
        torch.Tensor.cpu = orig_cpu
        del m._prompt_mel, m.style_from_mel
    assert len(out) == len(lists)
    assert after_bind == {"sync": 1, "mel": 2, "style": 1}          # two distinct prompt objects, ONE ragged pass, one copy down
    assert n == {"sync": 1 + len(lists), "mel": 3, "style": 2}      # a bound callable: one style for all its queries


def test_from_file_with_gst(tmp_path):
    import yaml
    from a3t_amd.duration import FS2DurationModel
    meta = R.meta()
    cfg, sd = _checkpoint("gst_xcat")
    sd = {"tts." + k: v for k, v in sd.items()}
    sd["normalize.mean"] = torch.zeros(80)
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(dict(cfg, normalize="global_mvn", optim="adam"), f)
    torch.save(sd, tmp_path / "train.loss.ave.pth")
    with pytest.raises(NotImplementedError, match="use_gst"):
        FS2DurationModel.from_file(None, str(tmp_path / "train.loss.ave.pth"), DEV)
    a = FS2DurationModel.from_file(None, str(tmp_path / "train.loss.ave.pth"), DEV, gst=True)
    m = _model("gst_xcat")
    wav = _wavs(meta)["b"]
    z = R.arrays()
    phns = ["sp", "HH", "AH0", "L", "OW1", "sp", "W", "ER1", "L", "D"]
    want = m.predict_frames(phns, m.speaker_bias(z["gst_xcat.spembs"]), m.style_embedding(wav))
    assert np.array_equal(a.predict_frames(phns, a.speaker_bias(z["gst_xcat.spembs"]), a.style_embedding(wav)), want)


# ------------------------------------------------------------------------------------------------------------ the editor
def test_speech_editor_with_a_gst_duration_model():
    """SpeechEditor.edit and edit_batch with a gst+xvector duration model: every request's durations come from ITS waveform,
    the batch asks the duration model once (one .batch call, one host copy) and plans as the single requests do."""
    from a3t_amd import sedit
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import EditRequest, SpeechEditor
    from a3t_amd.task import MLMTask
    from test_gpu_e2e import _task_args
    z = R.arrays()
    fx = json.load(open(os.path.join(G, "sedit.json")))
    oc = O.tiny_config()
    wavs = np.load(os.path.join(G, "sedit_wav.npz"))
    reqs, opts = [], []
    for i, kind in enumerate(("replace", "mask", "append", "delete")):
        case = [c for c in fx["cases"] if c["kind"] == kind][0]
        n = wavs[case["wav"] + ".in"].shape[0]
        wav = (0.1 * R.waveform(n, seed=20 + i) / 0.3 + 0.01 * np.random.RandomState(5 + i).standard_normal(n)).astype(np.float32)
        args = (case["times2"], case["word2phns"], case["new_phns"], case["new_word2phns"], case["old_str"], case["new_str"])
        reqs.append(EditRequest(wav, *args, **case["opts"]))
        opts.append(case["opts"])
    # a fifth request: the append edit behind request 0's waveform OBJECT (long enough for it): one style for the two
    reqs.append(EditRequest(reqs[0].wav_org, *[getattr(reqs[2], k) for k in ("times2", "word2phns", "new_phns", "new_word2phns",
                                                                              "old_str", "new_str")], **opts[2]))
    opts.append(opts[2])
    dm = _model("gst_xadd")
    native = dm.duration_fn(oc.fs, oc.hop_length, spembs=z["gst_xadd.spembs"])
    calls = {"batch": 0, "prompts": None, "sync": 0}

    def refuse(phns):
        raise AssertionError("a GST duration function was called without its prompt")

    def counted_batch(lists, prompts=None):
        calls["batch"] += 1
        calls["prompts"] = list(prompts)
        return native.batch(lists, prompts=prompts)
    refuse.needs_prompt, refuse.with_prompt, refuse.batch = True, native.with_prompt, counted_batch
    model = MLMTask.build_model(_task_args(oc), device=DEV)
    state = O.procedural_state(O.param_shapes(oc), 1)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device=DEV)
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    ed = SpeechEditor(model, coll, None, ids, refuse)
    # the planning alone: one .batch call, one copy to the host, the request's own waveform object with every query
    orig = torch.Tensor.cpu

    def counting(self, *a, **k):
        calls["sync"] += 1
        return orig(self, *a, **k)
    sedit.plan_batch(reqs, oc.fs, oc.hop_length, refuse, ids)          # (warm: buffers of these shapes)
    calls.update(batch=0, sync=0)
    torch.Tensor.cpu = counting
    try:
        plans, _ = sedit.plan_batch(reqs, oc.fs, oc.hop_length, refuse, ids)
    finally:
        torch.Tensor.cpu = orig
    assert calls["batch"] == 1 and calls["sync"] == 1
    assert {id(w) for w in calls["prompts"]} == {id(r.wav_org) for r in reqs if sedit.duration_queries(
        *sedit.get_phns_and_spans(r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str)[2:4], r.new_str,
        r.mask_reconstruct, r.start_end_sp)}
    calls.update(batch=0)
    res = ed.edit_batch(reqs)
    assert calls["batch"] == 1 and len(res) == len(reqs)
    for r, o, p, rb in zip(reqs, opts, plans, res):
        one = ed.edit(r.wav_org, r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str, **o)
        assert tuple(one["old_span_boundary"]) == tuple(p.old_span_boundary) == tuple(rb["old_span_boundary"])
        assert tuple(one["new_span_boundary"]) == tuple(p.new_span_boundary) == tuple(rb["new_span_boundary"])
        assert rb["feat"].shape[1] == 80 and torch.isfinite(torch.as_tensor(rb["feat"])).all()
        assert one["feat"].shape[1] == 80 and torch.isfinite(torch.as_tensor(one["feat"])).all()
