"""Generate tests/golden/fs2_speakers.{npz,json}: FastSpeech2's text-to-mel inference for SEVERAL x-vectors per model, run by
the REFERENCE itself (espnet2/tts/fastspeech2/fastspeech2.py:614-782 FastSpeech2.inference at B = 1), in the build container
only.

    python tests/golden/make_golden_fs2_speakers.py

The models are those of tests/golden/fs2_tts.json that have an x-vector projection (xadd, xcat, gst_norm): the same configs,
seeds, duration predictor overrides, token ids (2, 7 and 33 tokens) and, for the GST model, the same prompt and GlobalMVN
statistics, all read from that fixture, so nothing of them is stored again.  New are three x-vectors per model, drawn from
seeds (fs2_speakers_ref.speaker_vector) on the norms 0.3, 1 and 20, so that F.normalize in front of the projection matters.
Stored per (model, x-vector, length): the reference's log-domain durations (the output of duration_predictor.linear, caught
by a hook), durations, pitch, energy, `before` (for every length: the file stays far below the size limit), feat_gen and,
for the normalising model, feat_gen_denorm; and in the JSON the reference's own fp32-vs-fp64 distance F of every stage,
which the tests take their bounds from.

The tie rule of make_golden_fs2_tts.py holds here too: every token's exp(logd) - offset is >= TIE_MARGIN from a .5 tie and no
duration is above MAX_DURATION (the margin is 10 x the 1e-4 log-domain bound at that duration); an x-vector with which one of
the three lengths misses it is drawn again (JSON: draws).  Also asserted: for every length, any two x-vectors of a model give
different durations or a feat_gen that differs by more than 100 x the tests' bound -- the speaker decides."""
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

import fs2_speakers_ref as SR                                                          # noqa: E402
import fs2_tts_ref as R                                                                # noqa: E402
import gst_ref as GR                                                                   # noqa: E402
from make_golden_fs2 import TOKEN_LIST, _sedit_stubs, build_fs2                        # noqa: E402
from make_golden_fs2_tts import MAX_DURATION, load_state, tie                          # noqa: E402

MAX_DRAWS = 64


def run_full(tts, gmvn, ids, prompt, spembs, dtype):
    """The reference's inference with logd and `before` caught by hooks: dict of numpy arrays."""
    import torch
    got = {}
    hooks = [tts.duration_predictor.linear.register_forward_hook(lambda m, i, o: got.update(logd=o[0].squeeze(-1))),
             tts.feat_out.register_forward_hook(lambda m, i, o: got.update(before=o[0]))]
    with torch.no_grad():
        feats = None
        if prompt is not None:
            feats = torch.from_numpy(prompt.copy()).to(dtype)
            if gmvn is not None:
                feats = gmvn(feats[None])[0][0]
        out = tts.inference(torch.from_numpy(ids[:-1]), feats=feats, spembs=torch.from_numpy(spembs).to(dtype), alpha=1.0)
        got.update(feat_gen=out["feat_gen"], duration=out["duration"], pitch=out["pitch"].squeeze(-1),
                   energy=out["energy"].squeeze(-1))
        if gmvn is not None:
            got["feat_gen_denorm"] = gmvn.inverse(out["feat_gen"].clone()[None])[0][0]
    for h in hooks:
        h.remove()
    return {k: v.numpy().copy() for k, v in got.items()}


def main():
    import make_golden
    make_golden.install_stubs()
    _sedit_stubs()
    import torch
    from espnet2.layers.global_mvn import GlobalMVN
    torch.use_deterministic_algorithms(False)
    torch.set_num_threads(16)

    tts_meta = R.meta()
    assert tts_meta["token_list"] == TOKEN_LIST
    arr = {}
    meta = dict(models=list(SR.MODELS), lengths=list(SR.LENGTHS), norms=list(SR.NORMS), tie_margin=R.TIE_MARGIN,
                max_duration=MAX_DURATION, models_from="fs2_tts.json", cases={})
    assert R.TIE_MARGIN >= 10 * 1e-4 * (MAX_DURATION + 1)
    for name in SR.MODELS:
        mc = tts_meta["cases"][name]
        conf, seed = mc["tts_conf"], mc["seed"]
        model, shapes = build_fs2(conf, seed)
        assert shapes == mc["shapes"], name
        load_state(model, R.build_state(shapes, conf, seed, mc["dp_bias"], mc["dp_scale"]))
        m64 = copy.deepcopy(model).double()
        gm32 = gm64 = None
        if mc["normalize"]:
            gm32, gm64 = GlobalMVN(R.stats_file()), GlobalMVN(R.stats_file())
        prompt = GR.mel_input(tts_meta["prompt_frames"], seed) if conf.get("use_gst") else None
        ids = {T: R.token_ids(T, mc["input_seeds"][str(T)], len(TOKEN_LIST)) for T in SR.LENGTHS}
        info = dict(draws=[], runs={})
        outs = {}
        for k in range(SR.N_SPEAKERS):
            for draw in range(MAX_DRAWS):
                x = SR.speaker_vector(conf["spk_embed_dim"], seed, k, draw)
                o32 = {T: run_full(model, gm32, ids[T], prompt, x, torch.float32) for T in SR.LENGTHS}
                ok = all(tie(np.exp(o["logd"].astype(np.float64)) - 1.0).min() >= R.TIE_MARGIN
                         and o["duration"].max() <= MAX_DURATION and o["duration"].sum() >= 1 for o in o32.values())
                if ok:
                    break
            assert ok, (name, k)
            info["draws"].append(draw)
            assert abs(float(np.linalg.norm(x)) - SR.NORMS[k]) <= 1e-5 * SR.NORMS[k]
            for T in SR.LENGTHS:
                o = o32[T]
                o64 = run_full(m64, gm64, ids[T], None if prompt is None else prompt.astype(np.float64), x, torch.float64)
                assert np.array_equal(o["duration"], o64["duration"]), (name, k, T)
                assert np.array_equal(o["duration"], np.maximum(np.round(np.exp(o["logd"]) - np.float32(1.0)), 0).astype(np.int64))
                Fd = {s: float(np.abs(o[s] - o64[s]).max() / R.scale_of(o64[s])) for s in o if s != "duration"}
                t = SR.tag(name, k, T)
                arr[t + ".duration"] = o["duration"]
                for s in SR.STAGES:
                    if s in o:
                        arr[f"{t}.{s}"] = o[s]
                info["runs"][t] = dict(frames=int(o["feat_gen"].shape[0]), fp64=Fd,
                                       tie=float(tie(np.exp(o["logd"].astype(np.float64)) - 1.0).min()))
                outs[(k, T)] = o
                print(t, "draw", draw, "frames", o["feat_gen"].shape[0], "dur", o["duration"][:10].tolist(),
                      "fp64", {s: f"{v:.1e}" for s, v in Fd.items()}, flush=True)
        # the speaker decides: any two x-vectors differ in the durations, or in feat_gen by > 100 x the tests' bound
        sep = {}
        for T in SR.LENGTHS:
            for a in range(SR.N_SPEAKERS):
                for b in range(a + 1, SR.N_SPEAKERS):
                    oa, ob = outs[(a, T)], outs[(b, T)]
                    if not np.array_equal(oa["duration"], ob["duration"]):
                        sep[f"T{T}.s{a}.s{b}"] = "durations"
                        continue
                    bound = max(SR.mel_bound(info["runs"][SR.tag(name, s, T)]["fp64"]["feat_gen"]) for s in (a, b))
                    dist = float(np.abs(oa["feat_gen"] - ob["feat_gen"]).max() / R.scale_of(oa["feat_gen"]))
                    assert dist > 100 * bound, (name, T, a, b, dist, bound)
                    sep[f"T{T}.s{a}.s{b}"] = dist
        info["separation"] = sep
        print(name, "separation", sep, flush=True)
        meta["cases"][name] = info
    np.savez_compressed(os.path.join(HERE, "fs2_speakers.npz"), **arr)
    with open(os.path.join(HERE, "fs2_speakers.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for n in ("fs2_speakers.npz", "fs2_speakers.json"):
        size = os.path.getsize(os.path.join(HERE, n))
        print(n, size, "bytes")
        assert size < (1 << 20), n


if __name__ == "__main__":
    main()
