"""FastSpeech2 text-to-mel synthesis on the MI355X: the kernels of csrc/fs2_tts.hip against the CPU restatement
tests/fs2_tts_ref.py at the smallest shapes that can break them, and FS2TTSModel.synthesize / synthesize_batch against the
reference's own outputs in tests/golden/fs2_tts*.npz (bounds: durations and frame counts exact; pitch, energy, before,
feat_gen, feat_gen_denorm within max(4 F, 1e-4) of scale, F the reference's own fp32-vs-fp64 distance of the stage, 1e-4
the project's fp32 standard for mel outputs)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import fs2_tts_ref as R
from test_fs2_tts_host import MODELS, _inputs

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
NAN = float("nan")
OUT = ("pitch", "energy", "before", "feat_gen", "feat_gen_denorm")


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


# --------------------------------------------------------------------------------------------------------- the kernels
def _durations(T, lens, seed):
    """int64 [B][T]: small durations with leading, trailing and consecutive zeros in every row that has the room, one
    duration of 70 frames (longer than the kernel's 64-frame output tile) in row 0, and garbage behind every row's length."""
    rs = np.random.RandomState(seed)
    d = rs.randint(0, 5, size=(len(lens), T)).astype(np.int64)
    for b, n in enumerate(lens):
        if n >= 5:
            d[b, 0] = d[b, n - 1] = d[b, n - 2] = 0
            d[b, 1] = 3
        d[b, n:] = 1 << 40
    d[0, min(1, lens[0] - 1)] = 70
    return d


@pytest.mark.parametrize("alpha", [1.0, 1.3])
@pytest.mark.parametrize("d", [8, 384])
@pytest.mark.parametrize("T", [1, 5, 64, 65, 130])
def test_length_offsets_and_expand(T, d, alpha):
    from a3t_amd import ops
    lens = [T, max(1, T - 1), max(1, T // 2)]
    B = len(lens)
    dur = _durations(T, lens, 7 * T + d)
    hs = torch.randn(B, T, d, generator=torch.Generator().manual_seed(T))
    for b, n in enumerate(lens):
        hs[b, n:] = NAN
    want_ds, want_off = R.length_offsets(torch.from_numpy(dur), lens, alpha)
    Fp = int(want_off[:, -1].max()) + 3
    want, want_fl = R.length_expand(hs, want_ds, Fp, scale=1.0)
    off = torch.full((B, T + 1), -7, dtype=torch.int32, device=DEV)
    fl = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((B, T), -7, dtype=torch.int64, device=DEV)
    out = torch.full((B, Fp, d), NAN, device=DEV)
    ops.length_offsets(torch.from_numpy(dur).to(DEV), _lens(lens), alpha, off, fl, sc)
    ops.length_expand(hs.to(DEV), off, _lens(lens), fl, out, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(off.cpu(), want_off) and fl.cpu().tolist() == want_fl
    assert torch.equal(sc.cpu(), want_ds)
    assert torch.equal(out.cpu(), want)          # copied values bit for bit, zeros behind, no NaN from the tails
    # the decoder entry's scale, and full rows without a length table
    out2 = torch.full((B, Fp, d), NAN, device=DEV)
    ops.length_expand(hs.to(DEV), off, _lens(lens), fl, out2, 1.5)
    full = torch.from_numpy(np.where(dur > 100, 2, dur))
    ds3, off3 = R.length_offsets(full, [T] * B, alpha)
    off_d, fl_d = torch.empty_like(off), torch.empty_like(fl)
    ops.length_offsets(full.to(DEV), None, alpha, off_d, fl_d)
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu(), want * 1.5)
    assert torch.equal(off_d.cpu(), off3) and fl_d.cpu().tolist() == off3[:, -1].tolist()


@pytest.mark.parametrize("kp,ke", [(1, 9), (9, 1)])
@pytest.mark.parametrize("d", [8, 384])
@pytest.mark.parametrize("T", [1, 3, 65])
def test_variance_embed(T, d, kp, ke):
    from a3t_amd import ops
    lens = [T, max(1, T - 2), 1]
    B = len(lens)
    g = torch.Generator().manual_seed(100 * T + d + kp)
    hs, pitch, energy = torch.randn(B, T, d, generator=g), torch.randn(B, T, generator=g), torch.randn(B, T, generator=g)
    wp, we = torch.randn(d, 1, kp, generator=g), torch.randn(d, 1, ke, generator=g)
    bp, be = torch.randn(d, generator=g), torch.randn(d, generator=g)
    for b, n in enumerate(lens):
        hs[b, n:], pitch[b, n:], energy[b, n:] = NAN, NAN, NAN
    want = R.variance_embed(hs.double(), pitch.double(), energy.double(), wp.double(), bp.double(), we.double(), be.double(), lens)
    x = hs.to(DEV).clone()
    ops.fs2_variance_embed(x, pitch.to(DEV), energy.to(DEV), wp[:, 0, :].t().contiguous().to(DEV), bp.to(DEV),
                           we[:, 0, :].t().contiguous().to(DEV), be.to(DEV), _lens(lens), B, T)
    torch.cuda.synchronize()
    got = x.cpu()
    for b, n in enumerate(lens):
        err = float((got[b, :n].double() - want[b, :n]).abs().max()) / R.scale_of(want[b, :n].numpy())
        assert err <= 1e-6, (b, n, err)
        assert torch.isnan(got[b, n:]).all()          # rows behind the length are left alone
    if T == 65:     # full rows without a length table
        h2 = torch.randn(B, T, d, generator=g)
        p2, e2 = torch.randn(B, T, generator=g), torch.randn(B, T, generator=g)
        w2 = R.variance_embed(h2.double(), p2.double(), e2.double(), wp.double(), bp.double(), we.double(), be.double(), [T] * B)
        x2 = h2.to(DEV).clone()
        ops.fs2_variance_embed(x2, p2.to(DEV), e2.to(DEV), wp[:, 0, :].t().contiguous().to(DEV), bp.to(DEV),
                               we[:, 0, :].t().contiguous().to(DEV), be.to(DEV), None, B, T)
        assert float((x2.cpu().double() - w2).abs().max()) <= 1e-6 * R.scale_of(w2.numpy())


@pytest.mark.parametrize("C", [80, 6])
@pytest.mark.parametrize("stats", [False, True])
def test_finish(stats, C):
    from a3t_amd import ops
    B, Fm, lens = 3, 37, [37, 20, 1]
    g = torch.Generator().manual_seed(C)
    before, post = torch.randn(B, Fm, C, generator=g), torch.randn(B, Fm, C, generator=g)
    mean, std = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    for b, n in enumerate(lens):
        before[b, n:], post[b, n:] = NAN, NAN
    want, want_dn = R.finish(before, post, lens, mean if stats else None, std if stats else None)
    want, want_dn = torch.nan_to_num(want, nan=0.0), None if want_dn is None else torch.nan_to_num(want_dn, nan=0.0)
    for b, n in enumerate(lens):      # (0 * NaN in the restatement's mask)
        want[b, n:] = 0
        if want_dn is not None:
            want_dn[b, n:] = 0
    after = torch.full((B, Fm, C), NAN, device=DEV)
    dn = torch.full((B, Fm, C), NAN, device=DEV) if stats else None
    ops.fs2_finish(before.to(DEV), post.to(DEV), after, _lens(lens), mean.to(DEV) if stats else None,
                   std.to(DEV) if stats else None, dn)
    torch.cuda.synchronize()
    assert torch.equal(after.cpu(), want)
    if stats:
        assert torch.equal(dn.cpu(), want_dn)
    # no postnet, full rows
    a2 = torch.empty(B, Fm, C, device=DEV)
    b2 = torch.nan_to_num(before, nan=1.0)
    ops.fs2_finish(b2.to(DEV), None, a2)
    assert torch.equal(a2.cpu(), b2)
    y = torch.empty(B * Fm, C, device=DEV)
    ops.fs2_mvn(b2.view(-1, C).to(DEV), mean.to(DEV), std.to(DEV), y)
    ref = (b2.view(-1, C) - mean) / std
    assert float((y.cpu() - ref).abs().max()) <= 1e-6 * R.scale_of(ref.numpy())


# ------------------------------------------------------------------------------------------------------ the whole model
@functools.lru_cache(maxsize=None)
def _model(case):
    from a3t_amd.fs2_tts import FS2TTSConfig, FS2TTSModel
    cfg, p = R.checkpoint(R.meta(), case)
    c = FS2TTSConfig.from_espnet(cfg, gst=bool(cfg["tts_conf"].get("use_gst")))
    return FS2TTSModel(c, DEV).load_state_dict({"tts." + k: v for k, v in p.items()})


@functools.lru_cache(maxsize=None)
def _fixture():
    return R.meta(), R.arrays(), np.load(os.path.join(G, "fs2_tts_stages.npz"))


def _check_run(case, tag, out, record=None):
    meta, z, zs = _fixture()
    run = meta["cases"][case]["runs"][tag]
    assert np.array_equal(out["duration"].cpu().numpy(), z[tag + ".duration"]), tag
    assert out["feat_gen"].shape[0] == run["frames"], tag
    assert ("feat_gen_denorm" in out) == meta["cases"][case]["normalize"]
    for k in OUT:
        src = zs if k == "before" else z
        if f"{tag}.{k}" not in src:
            continue
        want, F = src[f"{tag}.{k}"], run["fp64"][k]
        got = out[k].cpu().numpy()
        assert got.shape == want.shape and np.isfinite(got).all(), (tag, k)
        err = float(np.abs(got - want).max()) / R.scale_of(want)
        print(f"{tag} {k}: device error {err:.2e} of scale, F {F:.2e}, bound {max(4 * F, 1e-4):.2e}")
        if record is not None:
            record.setdefault(k, []).append((err, F))
        assert err <= max(4 * F, 1e-4), (tag, k, err, F)


@pytest.mark.parametrize("case", MODELS)
def test_synthesize_against_the_reference(case):
    meta, z, _ = _fixture()
    m = _model(case)
    runs, spk, prompt, _, _ = _inputs(meta, z, case)
    for tag, (ids, alpha) in runs.items():
        style = None if prompt is None else m.style_from_prompts(prompt_mels=[prompt])
        out = m.synthesize_ids_batch([ids.tolist()], spk, style, None, alpha)[0]
        torch.cuda.synchronize()
        _check_run(case, tag, out)


@pytest.mark.parametrize("case", MODELS)
def test_synthesize_batch_equals_the_single_calls_with_one_copy_down(case):
    meta, z, _ = _fixture()
    m = _model(case)
    runs, spk, prompt, _, _ = _inputs(meta, z, case)
    tags = [t for t, (_, a) in runs.items() if a == 1.0]
    lists = [runs[t][0].tolist() for t in tags]
    style = None if prompt is None else m.style_from_prompts(prompt_mels=[prompt])
    single = [m.synthesize_ids_batch([ids], spk, style)[0] for ids in lists]
    single = [{k: v.clone() for k, v in o.items()} for o in single]
    n = {"down": 0}
    orig = torch.Tensor.cpu

    def counting(self, *a, **k):
        n["down"] += 1
        return orig(self, *a, **k)
    torch.Tensor.cpu = counting
    try:
        batch = m.synthesize_ids_batch(lists, spk, style)
        one = n["down"]
        cap = 2 * m.c.heads * max(o["feat_gen"].shape[0] for o in single) ** 2       # several chunks, the decoder in parts
        parts = m.synthesize_ids_batch(lists, spk, style, max_score_elems=cap)
    finally:
        torch.Tensor.cpu = orig
    torch.cuda.synchronize()
    assert one == 1 and n["down"] == 2
    for tag, a, b, c in zip(tags, single, batch, parts):
        _check_run(case, tag, b)
        _check_run(case, tag, c)
        assert torch.equal(a["duration"], b["duration"]) and torch.equal(a["duration"], c["duration"])
        assert a["feat_gen"].shape == b["feat_gen"].shape == c["feat_gen"].shape


def test_a_nan_filled_workspace_changes_no_valid_output():
    meta, z, _ = _fixture()
    m = _model("plain")
    runs, spk, prompt, _, _ = _inputs(meta, z, "plain")
    lists = [ids.tolist() for ids, a in runs.values() if a == 1.0]
    m.synthesize_ids_batch(lists)                     # (allocates every buffer of these shapes)
    torch.cuda.synchronize()
    got = []
    for fill in (0.0, NAN):
        for t in m.ws.bufs.values():
            t.fill_(fill) if t.is_floating_point() else t.fill_(0 if fill == 0.0 else 1 << 40)
        out = m.synthesize_ids_batch(lists)
        torch.cuda.synchronize()
        got.append([{k: v.cpu().numpy().copy() for k, v in o.items()} for o in out])
    for a, b in zip(*got):
        for k in a:
            assert np.isfinite(b[k]).all() and np.array_equal(a[k], b[k]), k


def test_phone_lists_a_prompt_waveform_and_the_refusals():
    """synthesize on phone strings is synthesize_ids_batch on tokens_to_ids; a GST model takes the prompt as a waveform
    through its own extractor and the checkpoint's normaliser; what cannot be decoded is refused."""
    import gst_ref as GR
    meta, z, _ = _fixture()
    m = _model("plain")
    phns = ["HH", "AH0", "sp", "L", "OW1"]
    a = m.synthesize(phns)
    b = m.synthesize_ids_batch([m.tokens_to_ids(phns)])[0]
    assert torch.equal(a["feat_gen"], b["feat_gen"]) and torch.equal(a["duration"], b["duration"])
    assert a["duration"].dtype == torch.int64 and a["duration"].shape[0] == len(phns) + 1
    assert a["feat_gen"].shape == (int(a["duration"].sum()), 80)
    assert m.synthesize_batch([]) == []
    with pytest.raises(ValueError, match="alpha"):
        m.synthesize(phns, alpha=0.0)
    with pytest.raises(ValueError, match="GST"):
        m.synthesize(phns, prompt=np.zeros(24000, np.float32))
    with pytest.raises(ValueError, match="spembs"):
        _model("xadd").synthesize(phns)
    # durations that sum to 0 frames: a tiny alpha rounds every token to 0
    with pytest.raises(ValueError, match="0 frames"):
        m.synthesize(phns, alpha=1e-3)
    g = _model("gst_norm")
    spk = _inputs(meta, z, "gst_norm")[1]
    wav = GR.waveform(39217, seed=1)
    with pytest.raises(ValueError, match="prompt"):
        g.synthesize(phns, spk)
    out = g.synthesize(phns, spk, prompt=wav)
    mel = g._prompt_mel(wav)[0][0]
    same = g.synthesize(phns, spk, prompt_mel=mel)
    two = g.synthesize_batch([phns, phns[:3]], spk, prompts=[wav, wav])
    torch.cuda.synchronize()
    assert torch.equal(out["feat_gen_denorm"], same["feat_gen_denorm"])
    assert torch.equal(out["duration"], two[0]["duration"]) and "feat_gen_denorm" in two[1]
    want = R.normalize_mel(mel.cpu(), *[None if s is None else s.cpu() for s in (g.mean, g.std)])
    y = torch.empty_like(mel)
    g._norm_mel(mel.contiguous(), out=y)
    assert float((y.cpu() - want).abs().max()) <= 1e-6 * R.scale_of(want.numpy())


def test_a_baseline_mel_through_a_vocoder():
    import melgan_ref as MR
    from a3t_amd import tts_baselines as TB
    from a3t_amd.vocoder import MelGANGeneratorHIP
    import gst_ref as GR
    meta, z, _ = _fixture()
    case = MR.CASES["plain_small"]
    voc = MelGANGeneratorHIP(MR.procedural_melgan_state(case["cfg"], case["seed"], case["weight_norm"]), device=DEV, fused=True,
                             pqmf=case["pqmf"], **case["cfg"])
    m = _model("plain")
    tag = "plain.T7"
    run = meta["cases"]["plain"]["runs"][tag]["baseline"]
    ids = _inputs(meta, z, "plain")[0][tag][0]
    out = m.synthesize_ids_batch([ids.tolist()])[0]
    orig = torch.from_numpy(GR.mel_input(meta["orig_frames"], run["orig_seed"])).to(DEV)
    mel = TB.baseline3_mel(out, orig, run["mfa_start"], run["span_tobe_replaced"], run["span_tobe_added"], meta["fs"], meta["hop"])
    assert mel.shape == z[tag + ".baseline3"].shape
    assert float(np.abs(mel.cpu().numpy() - z[tag + ".baseline3"]).max()) <= 1e-4 * R.scale_of(z[tag + ".baseline3"])
    wav = voc.inference(mel.contiguous())
    torch.cuda.synchronize()
    assert wav.numel() == MR.hop_of(case["cfg"]) * mel.shape[0] and torch.isfinite(wav).all()
