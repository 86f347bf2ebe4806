"""Host-side checks of FastSpeech2 text-to-mel synthesis (a3t_amd/fs2_tts.py, a3t_amd/tts_baselines.py): the torch
restatement tests/fs2_tts_ref.py against the reference's own outputs (tests/golden/fs2_tts*.npz, fs2_tts.json, written by
tests/golden/make_golden_fs2_tts.py) and its ragged rule, the length regulator's integer arithmetic, the config translation
and its refusals, the checkpoint key map, the GlobalMVN arithmetic, the driver's baseline mels and the C ABI.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import fs2_tts_ref as R
import gst_ref as GR
from test_duration_host import LJ_CONF, TOKENS

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("plain", "xadd", "xcat", "gst_norm")
STAGES = ("pitch", "energy", "hs_embed", "regulated", "before", "feat_gen", "feat_gen_denorm")
FBANK = dict(fs=24000, n_fft=2048, win_length=1200, hop_length=300, n_mels=80, fmin=80, fmax=7600)
NEW_EXPORTS = ("a3t_fs2_variance_embed", "a3t_length_offsets", "a3t_length_expand", "a3t_fs2_finish", "a3t_fs2_mvn")


def _conf(norm=None, **kw):
    t = dict(LJ_CONF)
    t.update(kw)
    c = {"tts": "fastspeech2", "tts_conf": t, "token_list": list(TOKENS), "feats_extract": "fbank",
         "feats_extract_conf": dict(FBANK)}
    if norm is not None:
        c.update(normalize=norm, normalize_conf={"stats_file": R.stats_file()})
    return c


def _inputs(meta, z, case):
    """Per run tag of one fixture model: (ids, alpha); and the model's (spembs, raw prompt mel, mean, std)."""
    import sys
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden_fs2 import speaker_vector
    mc = meta["cases"][case]
    conf = mc["tts_conf"]
    spk = speaker_vector(conf["spk_embed_dim"]) if conf.get("spk_embed_dim") else None
    prompt = GR.mel_input(meta["prompt_frames"], mc["seed"]) if conf.get("use_gst") else None
    mean, std = R.mvn_mean_std(np.load(R.stats_file())) if mc["normalize"] else (None, None)
    runs = {}
    for tag, run in mc["runs"].items():
        T = int(re.search(r"\.T(\d+)", tag).group(1))
        runs[tag] = (R.token_ids(T, mc["input_seeds"][str(T)], len(meta["token_list"])), run["alpha"])
    return runs, spk, prompt, mean, std


def _stage_arrays(z, zs, tag):
    out = {}
    for k in STAGES + ("duration",):
        for src in (z, zs):
            if f"{tag}.{k}" in src:
                out[k] = src[f"{tag}.{k}"]
    return out


# ------------------------------------------------------------------------------------------------- the fixture itself
def test_fixture_is_not_vacuous():
    meta = R.meta()
    assert meta["largest_duration"] <= 19 and meta["tie_margin"] >= 10 * 1e-4 * (meta["largest_duration"] + 1)
    z = R.arrays()
    n = 0
    for case in MODELS:
        for tag, run in meta["cases"][case]["runs"].items():
            d = z[tag + ".duration"]
            assert (d == 0).sum() >= 1 and (d >= 3).sum() >= 1, tag
            assert run["tie"] >= meta["tie_margin"] and run["moved_embed"] >= 0.1 and run["moved_post"] >= 0.01, tag
            n += 1
    assert n == 4 * len(meta["lengths"]) + 1 and sorted(meta["lengths"]) == [2, 7, 33, 130]
    assert meta["cases"]["plain"]["tts_conf"]["postnet_layers"] == 5
    for f in ("fs2_tts.npz", "fs2_tts_stages.npz", "fs2_tts_stats.npz", "fs2_tts.json"):
        assert os.path.getsize(os.path.join(G, f)) < (1 << 20), f


# ------------------------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("case", MODELS)
def test_restatement_against_the_reference(case):
    """Every stage within max(4 F, 1e-5) of scale, F the reference's own fp32-vs-fp64 distance of that stage; durations and
    frame counts exact.  The restatement runs in fp64, so that the distance to the reference's fp32 output is the reference's
    own rounding (= F when the formulas agree) on any host: in fp32 the restatement's own rounding comes on top and depends on
    the host's BLAS (4e-7 ... 1.8e-6 of scale on one machine, up to 1.04e-5 on another)."""
    meta, z, zs = R.meta(), R.arrays(), np.load(os.path.join(G, "fs2_tts_stages.npz"))
    cfg, p = R.checkpoint(meta, case)
    runs, spk, prompt, mean, std = _inputs(meta, z, case)
    for tag, (ids, alpha) in runs.items():
        want = _stage_arrays(z, zs, tag)
        got = R.synthesize(p, cfg["tts_conf"], ids[None], [len(ids)], spk, prompt, alpha, mean, std, dtype=torch.float64)
        assert np.array_equal(got["duration"][0].numpy(), want["duration"]), tag
        assert got["frame_lens"] == [meta["cases"][case]["runs"][tag]["frames"]] == [want["feat_gen"].shape[0]]
        for k in STAGES:
            if k not in want:
                continue
            F = meta["cases"][case]["runs"][tag]["fp64"][k]
            err = float(np.abs(got[k][0].numpy() - want[k]).max()) / R.scale_of(want[k])
            print(f"{tag} {k}: err {err:.2e} of scale, F {F:.2e}")
            assert err <= max(4 * F, 1e-5), (tag, k, err, F)
        assert ("feat_gen_denorm" in want) == meta["cases"][case]["normalize"]


def test_ragged_rows_equal_the_rows_alone():
    """All lengths of one model in one padded batch, the padding drawn from valid ids: every row within 1e-5 of scale of the
    row alone, durations equal (fp64, as above: the rule is what is checked, not a host's fp32 GEMM)."""
    meta, z = R.meta(), R.arrays()
    for case in ("plain", "gst_norm"):
        cfg, p = R.checkpoint(meta, case)
        runs, spk, prompt, mean, std = _inputs(meta, z, case)
        rows = [ids for tag, (ids, alpha) in runs.items() if alpha == 1.0]
        lens = [len(r) for r in rows]
        ids = np.random.RandomState(5).randint(0, len(meta["token_list"]), size=(len(rows), max(lens)))
        for b, r in enumerate(rows):
            ids[b, :lens[b]] = r
        batch = R.synthesize(p, cfg["tts_conf"], ids, lens, spk, prompt, 1.0, mean, std, dtype=torch.float64)
        for b, r in enumerate(rows):
            alone = R.synthesize(p, cfg["tts_conf"], r[None], [lens[b]], spk, prompt, 1.0, mean, std, dtype=torch.float64)
            Fb = alone["frame_lens"][0]
            assert batch["frame_lens"][b] == Fb
            assert torch.equal(batch["duration"][b, :lens[b]], alone["duration"][0])
            for k in STAGES:
                if alone[k] is None:
                    continue
                n = lens[b] if k in ("pitch", "energy", "hs_embed") else Fb
                a, w = batch[k][b, :n], alone[k][0, :n]
                err = float((a - w).abs().max()) / R.scale_of(w.numpy())
                assert err <= 1e-5, (case, b, k, err)
                if k in ("regulated", "before", "feat_gen", "feat_gen_denorm"):
                    assert torch.all(batch[k][b, Fb:] == 0), (case, b, k)


# ------------------------------------------------------------------------------------------ the length regulator's integers
@pytest.mark.parametrize("alpha", [0.5, 0.77, 1.3, 2.0, 1.0])
def test_offsets_and_alpha_rounding_match_torch_bit_for_bit(alpha):
    """The kernel's arithmetic (one fp32 product, rintf) against LengthRegulator's torch.round(ds.float() * alpha).long() and
    torch.cumsum, for every duration 0 .. 300."""
    d = np.arange(0, 301, dtype=np.int64)
    ds, off = R.kernel_offsets(d, alpha)
    want = R.scale_durations(torch.from_numpy(d), alpha)
    assert np.array_equal(ds, want.numpy())
    assert off[0] == 0 and np.array_equal(off[1:], torch.cumsum(want, 0).numpy().astype(np.int32))
    s2, o2 = R.length_offsets(torch.from_numpy(d)[None], [200], alpha)
    assert torch.equal(s2[0, :200], want[:200]) and torch.all(s2[0, 200:] == 0) and int(o2[0, -1]) == int(want[:200].sum())
    x = torch.arange(301 * 4, dtype=torch.float32).view(1, 301, 4)
    y, fl = R.length_expand(x, want[None])
    assert fl == [int(want.sum())] and torch.equal(y[0], torch.repeat_interleave(x[0], want, dim=0))


# ------------------------------------------------------------------------------------------------------------ config
def test_config_translation():
    from a3t_amd.duration import FS2DurationConfig
    from a3t_amd.fs2_tts import FS2TTSConfig
    c = FS2TTSConfig.from_espnet(_conf())
    assert isinstance(c, FS2DurationConfig)
    assert (c.dec_blocks, c.dec_ff, c.dec_kernel, c.postnet_layers, c.postnet_chans, c.postnet_filts, c.odim) == \
        (4, 1536, 31, 5, 256, 5, 80)
    assert c.variance("pitch") == (2, 384, 3, 9) and c.variance("energy") == (2, 384, 3, 9)
    assert not c.normalize and c.decoder_config().ff == 1536 and c.ff == 1536
    assert c.postnet_dims() == [(80, 256), (256, 256), (256, 256), (256, 256), (256, 80)]
    s = FS2TTSConfig.from_espnet(_conf(norm="global_mvn", dlayers=2, dunits=256, pitch_predictor_chans=64,
                                       pitch_embed_kernel_size=1, energy_predictor_layers=3, energy_predictor_kernel_size=5,
                                       postnet_layers=0))
    assert (s.dec_blocks, s.dec_ff, s.postnet_layers) == (2, 256, 0) and s.decoder_config().ff == 256 and s.ff == 1536
    assert s.variance("pitch") == (2, 64, 3, 1) and s.variance("energy") == (3, 384, 5, 9)
    assert s.normalize and s.stats_file == R.stats_file() and s.norm_means and s.norm_vars
    # the parent's own config is what it was
    assert FS2DurationConfig.from_espnet(_conf()).dec_blocks == 0 and FS2DurationConfig.from_espnet(_conf()).postnet_layers == 0


@pytest.mark.parametrize("kw,field", [
    (dict(decoder_type="transformer"), "decoder_type"),
    (dict(reduction_factor=2), "reduction_factor"),
    (dict(spks=4), "spks"),
    (dict(langs=2), "langs"),
    (dict(pitch_predictor_kernel_size=4), "pitch_predictor_kernel_size"),
    (dict(energy_predictor_kernel_size=2), "energy_predictor_kernel_size"),
    (dict(pitch_embed_kernel_size=8), "pitch_embed_kernel_size"),
    (dict(energy_embed_kernel_size=4), "energy_embed_kernel_size"),
    (dict(energy_embed_kernel_size=11), "energy_embed_kernel_size"),
    (dict(use_batch_norm=False), "use_batch_norm"),
    (dict(norm="utterance_mvn"), "normalize"),
    (dict(decoder_normalize_before=False), "decoder_normalize_before"),
    (dict(pitch_predictor_chans=1024), "pitch_predictor_chans"),
    (dict(encoder_type="transformer"), "encoder_type"),
])
def test_refusals_name_the_field(kw, field):
    from a3t_amd.fs2_tts import FS2TTSConfig
    with pytest.raises(NotImplementedError, match=field):
        FS2TTSConfig.from_espnet(_conf(**kw))


def test_gst_needs_the_argument_as_the_parent_does():
    from a3t_amd.fs2_tts import FS2TTSConfig
    with pytest.raises(NotImplementedError, match="gst=True"):
        FS2TTSConfig.from_espnet(_conf(use_gst=True))
    assert FS2TTSConfig.from_espnet(_conf(use_gst=True), gst=True).use_gst


# ----------------------------------------------------------------------------------------------------------- key map
@pytest.mark.parametrize("case", ["plain", "xcat", "gst_norm"])
def test_key_map_covers_the_whole_state_dict_and_loads(case):
    """Every tensor of the reference model's state dict has an entry, BatchNorm's num_batches_tracked (training only) aside;
    the store takes them in the layouts the kernels read."""
    from a3t_amd.fs2_tts import FS2TTSConfig, FS2TTSModel, key_map
    meta = R.meta()
    cfg, p = R.checkpoint(meta, case)
    c = FS2TTSConfig.from_espnet(cfg, gst=bool(cfg["tts_conf"].get("use_gst")))
    keys = {k for k, _, _, _ in key_map(c)}
    full = {"tts." + k for k in meta["cases"][case]["shapes"]}
    assert {k for k in full - keys if not k.endswith("num_batches_tracked")} == set()
    assert {k for k in keys - full if not k.endswith("num_batches_tracked")} == set()
    m = FS2TTSModel(c, "cpu").load_state_dict({"tts." + k: v for k, v in p.items()})
    sp = m.store.p
    assert torch.equal(sp["pemb.w"], p["pitch_embed.0.weight"][:, 0, :].t())
    assert torch.equal(sp["eemb.b"], p["energy_embed.0.bias"])
    assert torch.equal(sp["pp.0.w"], p["pitch_predictor.conv.0.0.weight"].permute(0, 2, 1))
    assert torch.equal(sp["ep.lin.w"], p["energy_predictor.linear.weight"].reshape(-1))
    assert torch.equal(sp["dec.1.ff.w1"], p["decoder.encoders.1.feed_forward.w_1.weight"].permute(0, 2, 1))
    assert sp["dec.0.ff.w1"].shape[0] == cfg["tts_conf"]["dunits"] and sp["enc.0.ff.w1"].shape[0] == cfg["tts_conf"]["eunits"]
    assert torch.equal(sp["fout.w"], p["feat_out.weight"])
    assert torch.equal(m.store.buf["post.0.bn.rv"], p["postnet.postnet.0.1.running_var"])
    assert torch.equal(m.store.buf["dec.0.cnv.bn.rm"], p["decoder.encoders.0.conv_module.norm.running_mean"])
    # the folded BatchNorm of the postnet: conv with the folded weights + shift == conv, then BatchNorm
    der = m._tts_derived()
    L = c.postnet_layers - 1
    x = torch.randn(1, c.postnet_dims()[L][0], 9, dtype=torch.float64)
    pre = f"postnet.postnet.{L}."
    want = torch.nn.functional.batch_norm(
        torch.nn.functional.conv1d(x, p[pre + "0.weight"].double(), padding=2), p[pre + "1.running_mean"].double(),
        p[pre + "1.running_var"].double(), p[pre + "1.weight"].double(), p[pre + "1.bias"].double(), False, 0.0, 1e-5)
    got = torch.nn.functional.conv1d(x, der[f"w.{L}"].double().permute(0, 2, 1), der[f"shift.{L}"].double(), padding=2)
    assert float((got - want).abs().max()) <= 1e-6 * R.scale_of(want.numpy())
    bad = {"tts." + k: v for k, v in p.items()}
    bad["tts.postnet.postnet.0.3.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="unexpected"):
        FS2TTSModel(c, "cpu").load_state_dict(bad)
    del bad["tts.postnet.postnet.0.3.weight"], bad["tts.feat_out.bias"]
    with pytest.raises(KeyError, match="feat_out.bias"):
        FS2TTSModel(c, "cpu").load_state_dict(bad)


def test_from_file_reads_config_weights_and_statistics(tmp_path):
    """from_file as the parent's: config.yaml next to the model file, and a relative stats_file next to the config."""
    import shutil
    import yaml
    from a3t_amd.fs2_tts import FS2TTSModel
    meta = R.meta()
    cfg, p = R.checkpoint(meta, "gst_norm")
    shutil.copy(R.stats_file(), tmp_path / "feats_stats.npz")
    cfg["normalize_conf"] = {"stats_file": "feats_stats.npz"}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"tts." + k: v for k, v in p.items()}, tmp_path / "model.pth")
    m = FS2TTSModel.from_file(None, str(tmp_path / "model.pth"), "cpu", gst=True)
    mean, std = R.mvn_mean_std(np.load(R.stats_file()))
    assert m.c.use_gst and m.c.normalize and m.c.dec_blocks == 2 and m.c.odim == 80
    assert np.array_equal(m.mean.numpy(), mean.astype(np.float32)) and np.array_equal(m.std.numpy(), std.astype(np.float32))
    assert torch.equal(m.store.p["fout.b"], p["feat_out.bias"])
    assert m.tokens_to_ids(["sp", "AH0", "nope"]) == [0, meta["token_list"].index("AH0"), 1, len(meta["token_list"]) - 1]


# --------------------------------------------------------------------------------------------------------- GlobalMVN
def test_global_mvn_arithmetic():
    from a3t_amd.fs2_tts import global_mvn_stats
    meta, z = R.meta(), R.arrays()
    stats = np.load(R.stats_file())
    assert sorted(stats.files) == ["count", "sum", "sum_square"]
    mean, std = global_mvn_stats(R.stats_file())
    m2, s2 = R.mvn_mean_std(R.mvn_stats())
    assert np.array_equal(mean, m2) and np.array_equal(std, s2) and mean.dtype == np.float64
    assert global_mvn_stats(R.stats_file(), norm_means=False)[0] is None and global_mvn_stats(R.stats_file(), norm_vars=False)[1] is None
    # a variance below eps is raised to it
    tiny = dict(count=np.array(10), sum=np.full(3, 20.0), sum_square=np.full(3, 40.0))
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"fs2_tts_stats_{os.getpid()}.npz")
    np.savez(path, **tiny)
    try:
        assert np.array_equal(global_mvn_stats(path)[1], np.full(3, 1e-10))
    finally:
        os.remove(path)
    # the fixture's denormalised mel is feat_gen * std + mean in fp32, two roundings, as GlobalMVN.inverse does it
    for tag in meta["cases"]["gst_norm"]["runs"]:
        fg = z[tag + ".feat_gen"]
        assert np.array_equal(fg * std.astype(np.float32) + mean.astype(np.float32), z[tag + ".feat_gen_denorm"]), tag


# --------------------------------------------------------------------------------------------------------- baselines
def test_baseline_mels_bit_for_bit():
    from a3t_amd import tts_baselines as TB
    meta, z = R.meta(), R.arrays()
    n = 0
    for case in MODELS:
        for tag, run in meta["cases"][case]["runs"].items():
            if "baseline" not in run:
                continue
            b = run["baseline"]
            out = {k: torch.from_numpy(z[f"{tag}.{k}"]) for k in ("feat_gen", "feat_gen_denorm", "duration") if f"{tag}.{k}" in z}
            orig = torch.from_numpy(GR.mel_input(meta["orig_frames"], b["orig_seed"]))
            assert TB.old_span_frames(b["mfa_start"], b["span_tobe_replaced"], meta["fs"], meta["hop"]) == b["old_span"]
            b1 = TB.baseline1_mel(out)
            assert b1 is (out["feat_gen_denorm"] if meta["cases"][case]["normalize"] else out["feat_gen"])
            b2 = TB.baseline2_mel(out, orig, b["mfa_start"], b["span_tobe_replaced"], meta["fs"], meta["hop"])
            b3 = TB.baseline3_mel(out, orig, b["mfa_start"], b["span_tobe_replaced"], b["span_tobe_added"], meta["fs"], meta["hop"])
            assert np.array_equal(b2.numpy(), z[tag + ".baseline2"]) and np.array_equal(b3.numpy(), z[tag + ".baseline3"]), tag
            n += 1
    assert n == 8
    # an eos of 0 frames: [:-0] leaves nothing of the target, as the reference writes it
    out = dict(feat_gen=torch.ones(5, 2), duration=torch.tensor([2, 3, 0]))
    assert TB.baseline2_mel(out, torch.zeros(100, 2), [0.0, 0.5, 1.0], [1, 2], 24000, 300).shape[0] == 40 + 0 + 20


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_new_exports_are_declared():
    from a3t_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "a3t_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\(", hdr), name
    for fn in ("fs2_variance_embed", "length_offsets", "length_expand", "fs2_finish", "fs2_mvn"):
        assert callable(getattr(ops, fn))
    from a3t_amd.build import SOURCES
    assert "fs2_tts.hip" in SOURCES
