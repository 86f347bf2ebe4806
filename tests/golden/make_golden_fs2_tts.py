"""Generate tests/golden/fs2_tts.{npz,json} (+ fs2_tts_stages.npz, fs2_tts_stats.npz): FastSpeech2's text-to-mel inference
as the speech-editing driver's TTS baselines run it (espnet2/bin/sedit_inference.py:129-260 through
espnet2/tts/espnet_model.py:223-308 and espnet2/tts/fastspeech2/fastspeech2.py:614-782), run by the REFERENCE itself, in the
build container only.

    python tests/golden/make_golden_fs2_tts.py

The reference is imported through make_golden.install_stubs() and make_golden_fs2._sedit_stubs().  The models are
make_golden_fs2.build_fs2's, with procedural weights and the overrides of tests/fs2_tts_ref.py (recorded in the JSON); inputs
come from seeds (fs2_tts_ref.token_ids, gst_ref.mel_input, make_golden_fs2.speaker_vector) and are not stored.  Stored are the
reference's numeric outputs and its own fp32-vs-fp64 distance F of every stage, which the tests take their bounds from.
fs2_tts_stats.npz is a feats_stats.npz as ESPnet writes one (count, sum, sum_square), drawn from a seed: data.

What the reference's ESPnetTTSModel.inference does around tts.inference -- GlobalMVN on the prompt's log-mel in front,
GlobalMVN.inverse on feat_gen behind -- is done here with the reference's own GlobalMVN module on the reference's own
FastSpeech2.inference (the model class itself needs a feature extractor and a waveform the fixture has no use for: the prompt is
given as its log-mel, the "precalculated feats" branch of :257-259).  The three baseline mels are assembled as the driver's
lines :207, :219-220 and :257-258 assemble them, from a procedural original mel, given mfa_start times and given spans.

Size: fs2_tts.npz holds durations, pitch, energy, feat_gen, feat_gen_denorm and the baselines; fs2_tts_stages.npz holds hs
behind the embeddings, the regulated sequence and `before`.  hs and the regulated sequence are stored for the lengths in
STAGE_LENGTHS only (the regulated sequence is a copy of hs rows), the baselines for BASELINE_LENGTHS (a span needs a few
tokens); everything else for every case.

The generator asserts, for EVERY case (model x length x alpha), and searches the duration predictor's bias / weight scale per
model and the input seed per case until it holds:
  - every token's exp(logd) - offset is >= TIE_MARGIN = 0.02 from a .5 tie (10 x the 1e-4 log-domain bound the duration
    fixtures hold the device to, at the fixture's largest duration -- stated in the JSON), and so are its product with alpha
    and the product of the rounded duration with alpha in the alpha case;
  - at least one token of duration 0 and one of duration >= 3;
  - the pitch / energy embeddings move hs by >= 0.1 of scale, the postnet moves `before` by >= 0.01 of scale."""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import fs2_tts_ref as R                                                                # noqa: E402
import gst_ref as GR                                                                   # noqa: E402
from make_golden_fs2 import _LJ, FS, HOP, TOKEN_LIST, _sedit_stubs, build_fs2, speaker_vector   # noqa: E402

_BASE = dict(_LJ, elayers=2, dlayers=2, dunits=256, postnet_chans=64)
CASES = {
    "plain": dict(_BASE, postnet_layers=5),
    "xadd": dict(_BASE, postnet_layers=2, spk_embed_dim=512, spk_embed_integration_type="add"),
    "xcat": dict(_BASE, postnet_layers=1, spk_embed_dim=512, spk_embed_integration_type="concat", pitch_embed_kernel_size=1,
                 energy_embed_kernel_size=1),
    "gst_norm": dict(_BASE, postnet_layers=2, use_gst=True, gst_conv_layers=4, gst_conv_chans_list=[16, 32, 32, 64],
                     gst_conv_kernel_size=5, gst_gru_units=96, gst_heads=2, gst_tokens=7, spk_embed_dim=512,
                     spk_embed_integration_type="add"),
}
SEEDS = {"plain": 41, "xadd": 42, "xcat": 43, "gst_norm": 44}
NORMALIZE = {"gst_norm"}
STAGE_LENGTHS = {"plain": (2, 7, 33), "xadd": (2, 7), "xcat": (2, 7), "gst_norm": (2, 7)}
BASELINE_LENGTHS = (7, 33)
ORIG_FRAMES = 24                     # the procedural original mel of the baselines: gst_ref.mel_input(ORIG_FRAMES, seed)
DP_GRID = [(1.5, 0.7), (1.5, 0.3), (1.5, 0.5), (2.0, 0.3), (2.0, 0.7), (1.0, 0.7), (1.0, 0.3)]
INPUT_SEEDS, SEARCH_BATCH = 4096, 64
MAX_DURATION = 19                    # TIE_MARGIN = 10 x 1e-4 x (MAX_DURATION + 1)


def load_state(model, state):
    import torch
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    return model


def text_side(tts, ids, style, spembs):
    """exp(logd) - offset and the frames of one phone list (eos included) at alpha = 1; ids [B][T] (lists of one length, so
    that nothing is padded): arrays [B][T]."""
    import torch
    from espnet.nets.pytorch_backend.nets_utils import make_pad_mask
    one = ids.ndim == 1
    ids = ids[None] if one else ids
    text, ilens = torch.from_numpy(ids), torch.full((ids.shape[0],), ids.shape[1], dtype=torch.long)
    with torch.no_grad():
        hs, _ = tts.encoder(text, tts._source_mask(ilens))
        if style is not None:
            hs = hs + style.unsqueeze(1)
        if spembs is not None:
            hs = tts._integrate_with_spk_embed(hs, torch.from_numpy(spembs).to(hs.dtype)[None].expand(hs.shape[0], -1))
        dp = tts.duration_predictor
        x = hs.transpose(1, -1)
        for f in dp.conv:
            x = f(x)
        expm = dp.linear(x.transpose(1, -1)).squeeze(-1).exp() - dp.offset
        frames = dp.inference(hs, make_pad_mask(ilens))
    expm, frames = expm.double().numpy(), frames.numpy()
    return (expm[0], frames[0]) if one else (expm, frames)


def tie(e):
    e = np.asarray(e, np.float64)
    return np.abs(e - np.floor(e) - 0.5)


def durations_ok(expm, frames, alpha):
    if tie(expm).min() < R.TIE_MARGIN or (frames == 0).sum() < 1 or (frames >= 3).sum() < 1 or frames.max() > MAX_DURATION:
        return False
    if alpha != 1.0:
        prod = (frames.astype(np.float32) * np.float32(alpha)).astype(np.float64)
        if tie(expm * alpha).min() < R.TIE_MARGIN or tie(prod).min() < R.TIE_MARGIN:
            return False
        if np.round(prod).sum() < 1:
            return False
    return True


def run_full(tts, gmvn, ids, prompt, spembs, alpha, dtype):
    """The reference's inference with the stages caught by hooks: dict of numpy arrays."""
    import torch
    got = {}
    hooks = [tts.length_regulator.register_forward_hook(lambda m, i, o: got.update(hs_embed=i[0][0], regulated=o[0])),
             tts.feat_out.register_forward_hook(lambda m, i, o: got.update(before=o[0]))]
    with torch.no_grad():
        feats = None
        if prompt is not None:
            feats = torch.from_numpy(prompt.copy()).to(dtype)
            if gmvn is not None:
                feats = gmvn(feats[None])[0][0]
        out = tts.inference(torch.from_numpy(ids[:-1]), feats=feats,
                            spembs=None if spembs is None else torch.from_numpy(spembs).to(dtype), alpha=alpha)
        got.update(feat_gen=out["feat_gen"], duration=out["duration"], pitch=out["pitch"].squeeze(-1),
                   energy=out["energy"].squeeze(-1))
        if gmvn is not None:
            got["feat_gen_denorm"] = gmvn.inverse(out["feat_gen"].clone()[None])[0][0]
    for h in hooks:
        h.remove()
    return {k: v.numpy().copy() for k, v in got.items()}


def baselines(out, orig, mfa_start, span_replaced, span_added):
    """sedit_inference.py:177-183 (baseline 1), :207-220 (baseline 2), :244-258 (baseline 3) on one inference result."""
    import torch
    input_feat = torch.from_numpy(orig)
    out_feat = torch.from_numpy(out["feat_gen_denorm"] if out.get("feat_gen_denorm") is not None else out["feat_gen"])
    dur = out["duration"].tolist()
    old_span = [int(mfa_start[span_replaced[0]] * FS / HOP), int(mfa_start[span_replaced[1]] * FS / HOP)]
    eos_duration = dur[-1]
    target2 = out_feat[:-eos_duration]
    b2 = torch.cat([input_feat[:old_span[0]], target2, input_feat[old_span[1]:]])
    durations = dur[:-1]
    target3 = out_feat[sum(durations[:span_added[0]]):sum(durations[:span_added[1]])]
    b3 = torch.cat([input_feat[:old_span[0]], target3, input_feat[old_span[1]:]])
    return out_feat.numpy(), b2.numpy(), b3.numpy(), old_span


def main():
    import make_golden
    make_golden.install_stubs()
    _sedit_stubs()
    import torch
    from espnet2.layers.global_mvn import GlobalMVN
    torch.use_deterministic_algorithms(False)
    torch.set_num_threads(16)

    np.savez(os.path.join(HERE, "fs2_tts_stats.npz"), **R.mvn_stats())
    gm32 = GlobalMVN(os.path.join(HERE, "fs2_tts_stats.npz"))
    main_arr, stage_arr = {}, {}
    meta = dict(token_list=TOKEN_LIST, lengths=list(R.LENGTHS), alpha_case=list(R.ALPHA_CASE), alpha=R.ALPHA, fs=FS, hop=HOP,
                offset=1.0, tie_margin=R.TIE_MARGIN, prompt_frames=R.PROMPT_FRAMES, orig_frames=ORIG_FRAMES,
                feats_extract_conf=GR.FEATS_CONF, overrides=dict(R.OVERRIDES, var_scale=R.VAR_SCALE, post_scale=R.POST_SCALE),
                stage_lengths={k: list(v) for k, v in STAGE_LENGTHS.items()}, baseline_lengths=list(BASELINE_LENGTHS),
                cases={})
    largest = 0
    for name, conf in CASES.items():
        seed = SEEDS[name]
        model, shapes = build_fs2(conf, seed)
        spk = speaker_vector(conf["spk_embed_dim"]) if conf.get("spk_embed_dim") else None
        prompt = GR.mel_input(R.PROMPT_FRAMES, seed) if conf.get("use_gst") else None
        gmvn = gm32 if name in NORMALIZE else None
        runs = [(T, 1.0) for T in R.LENGTHS] + ([(R.ALPHA_CASE[1], R.ALPHA)] if name == R.ALPHA_CASE[0] else [])
        chosen = None
        for dp_scale, dp_bias in DP_GRID:
            load_state(model, R.build_state(shapes, conf, seed, dp_bias, dp_scale))
            style = None
            if prompt is not None:
                with torch.no_grad():
                    style = model.gst(gm32(torch.from_numpy(prompt.copy())[None])[0] if gmvn is not None
                                      else torch.from_numpy(prompt.copy())[None])
            picks = {}
            for T in sorted(R.LENGTHS, reverse=True):      # the longest is the hardest to satisfy
                alphas = [a for t, a in runs if t == T]
                for s0 in range(0, INPUT_SEEDS, SEARCH_BATCH):
                    cand = np.stack([R.token_ids(T, 1000 * seed + s, len(TOKEN_LIST)) for s in range(s0, s0 + SEARCH_BATCH)])
                    expm, frames = text_side(model, cand, style, spk)
                    good = [k for k in range(SEARCH_BATCH) if all(durations_ok(expm[k], frames[k], a) for a in alphas)]
                    if good:
                        picks[T] = s0 + good[0]
                        break
                if T not in picks:
                    break
            print(name, "dp_scale", dp_scale, "dp_bias", dp_bias, "input seeds", picks, flush=True)
            if len(picks) == len(R.LENGTHS):
                chosen = (dp_scale, dp_bias, picks)
                break
        assert chosen is not None, name
        dp_scale, dp_bias, picks = chosen
        m64 = copy.deepcopy(model).double()
        gm64 = None
        if gmvn is not None:
            gm64 = GlobalMVN(os.path.join(HERE, "fs2_tts_stats.npz"))
        info = dict(tts_conf=conf, seed=seed, shapes=shapes, dp_scale=dp_scale, dp_bias=dp_bias, normalize=name in NORMALIZE,
                    input_seeds={str(T): 1000 * seed + s for T, s in picks.items()}, runs={})
        for T, alpha in runs:
            ids = R.token_ids(T, 1000 * seed + picks[T], len(TOKEN_LIST))
            o32 = run_full(model, gmvn, ids, prompt, spk, alpha, torch.float32)
            o64 = run_full(m64, gm64, ids, None if prompt is None else prompt.astype(np.float64), spk, alpha, torch.float64)
            assert np.array_equal(o32["duration"], o64["duration"]), (name, T, alpha)
            d = o32["duration"]
            assert (d == 0).sum() >= 1 and (d >= 3).sum() >= 1, (name, T, d)
            largest = max(largest, int(d.max()))
            tag = f"{name}.T{T}" + ("" if alpha == 1.0 else f".a{alpha}")
            Fd = {k: float(np.abs(o32[k] - o64[k]).max() / R.scale_of(o64[k])) for k in o32 if k != "duration"}
            # not vacuous: the embeddings move hs, the postnet moves the mel
            expm, _ = text_side(model, ids, None if prompt is None else style, spk)
            with torch.no_grad():
                text, ilens = torch.from_numpy(ids)[None], torch.tensor([T])
                hs, _ = model.encoder(text, model._source_mask(ilens))
                if prompt is not None:
                    hs = hs + style.unsqueeze(1)
                if spk is not None:
                    hs = model._integrate_with_spk_embed(hs, torch.from_numpy(spk)[None])
            moved_embed = float(np.abs(o32["hs_embed"] - hs[0].numpy()).max() / R.scale_of(hs[0].numpy()))
            moved_post = float(np.abs(o32["feat_gen"] - o32["before"]).max() / R.scale_of(o32["before"]))
            assert moved_embed >= 0.1 and moved_post >= 0.01, (name, T, moved_embed, moved_post)
            main_arr[tag + ".duration"] = d
            for k in ("pitch", "energy", "feat_gen", "feat_gen_denorm"):
                if k in o32:
                    main_arr[f"{tag}.{k}"] = o32[k]
            stage_arr[tag + ".before"] = o32["before"]
            if T in STAGE_LENGTHS[name]:
                stage_arr[tag + ".hs_embed"], stage_arr[tag + ".regulated"] = o32["hs_embed"], o32["regulated"]
            run = dict(alpha=alpha, frames=int(o32["feat_gen"].shape[0]), fp64=Fd, tie=float(tie(expm).min()),
                       moved_embed=moved_embed, moved_post=moved_post, zeros=int((d == 0).sum()), long=int((d >= 3).sum()))
            if T in BASELINE_LENGTHS and alpha == 1.0:
                rs = np.random.RandomState(seed * 100 + T)
                n_old = 6
                mfa_start = np.sort(rs.uniform(0.0, (ORIG_FRAMES - 1) * HOP / FS, n_old)).round(3).tolist()
                rep = sorted(rs.choice(n_old, 2, replace=False).tolist())
                add = sorted(rs.choice(T - 1, 2, replace=False).tolist())
                orig = GR.mel_input(ORIG_FRAMES, seed + 7)
                b1, b2, b3, old_span = baselines(o32, orig, mfa_start, rep, add)
                assert np.array_equal(b1, o32.get("feat_gen_denorm", o32["feat_gen"]))
                main_arr[tag + ".baseline2"], main_arr[tag + ".baseline3"] = b2, b3
                run["baseline"] = dict(mfa_start=mfa_start, span_tobe_replaced=rep, span_tobe_added=add, old_span=old_span,
                                       orig_seed=seed + 7)
            info["runs"][tag] = run
            print(tag, "frames", run["frames"], "dur", d[:10].tolist(), "fp64", {k: f"{v:.1e}" for k, v in Fd.items()},
                  "embed", round(moved_embed, 3), "post", round(moved_post, 3), flush=True)
        meta["cases"][name] = info
    meta["largest_duration"] = largest
    # 1e-4 in the log domain moves exp(logd) by 1e-4 * (d + 1) at duration d: the margin is >= 10 x that
    assert R.TIE_MARGIN >= 10 * 1e-4 * (largest + 1), largest
    np.savez_compressed(os.path.join(HERE, "fs2_tts.npz"), **main_arr)
    np.savez_compressed(os.path.join(HERE, "fs2_tts_stages.npz"), **stage_arr)
    with open(os.path.join(HERE, "fs2_tts.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for n in ("fs2_tts.npz", "fs2_tts_stages.npz", "fs2_tts_stats.npz", "fs2_tts.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
