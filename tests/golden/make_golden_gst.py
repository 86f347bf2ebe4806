"""Generate tests/golden/gst_duration.{npz,json}: the GST style encoder of a gst+xvector conformer FastSpeech2 and the
duration path behind it (sedit_inference.py:398-425 with use_gst), run by the REFERENCE itself, in the build container only.

    python tests/golden/make_golden_gst.py

The reference is imported through make_golden.install_stubs() and make_golden_fs2._sedit_stubs().  Weights are procedural
(oracle.procedural_state + make_golden_fs2.apply_overrides + tests/gst_ref.py::apply_gst_overrides, all recorded in the JSON);
inputs come from seeds (tests/gst_ref.py: mel_input, waveform, mel_perturbation; make_golden_fs2.token_ids) and are not
stored.  Only the reference's numeric outputs are stored, plus two measurements of the reference against itself that the
tests take their bounds from: the fp32-vs-fp64 distance of every stage, and how far the style embedding moves when its
log-mel input moves by +-2e-4 per element (the bound tests/golden/logmel.npz holds the device extractor to).

The generator asserts that the fixture is not vacuous: every conv layer has 10 .. 90 % non-zero outputs, adding the style
changes frames, and two different prompts get style embeddings >= 0.1 of scale apart that change at least one frame."""
import copy
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gst_ref as R                                                                    # noqa: E402
from make_golden_fs2 import (_LJ, EXTRA_LISTS, FS, HOP, LENGTHS, TOKEN_LIST, _sedit_stubs, build_fs2, speaker_vector,  # noqa: E402
                             token_ids)

_SMALL = dict(_LJ, elayers=2, use_gst=True, gst_conv_layers=4, gst_conv_chans_list=[16, 32, 32, 64], gst_conv_kernel_size=5,
              gst_gru_units=96, gst_heads=2, gst_tokens=7, spk_embed_dim=512, spk_embed_integration_type="add")
CASES = {
    "gst_xadd": dict(_LJ, use_gst=True, spk_embed_dim=512, spk_embed_integration_type="add"),
    "gst_xcat": dict(_LJ, use_gst=True, spk_embed_dim=512, spk_embed_integration_type="concat"),
    "gst_plain": dict(_LJ, use_gst=True),
    "gst_small": _SMALL,
}
SEEDS = {"gst_xadd": 31, "gst_xcat": 32, "gst_plain": 33, "gst_small": 34}


def build(conf, seed):
    """build_fs2 + the GST overrides: (model, {name: shape})."""
    import torch
    from oracle.a3t_oracle import procedural_state
    from make_golden_fs2 import apply_overrides
    model, shapes = build_fs2(conf, seed)
    state = procedural_state({k: tuple(v) for k, v in shapes.items()}, seed)
    apply_overrides(state, conf.get("duration_predictor_layers", 2))
    R.apply_gst_overrides(state, conf.get("gst_conv_layers", 6))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    return model, shapes


def scale_of(a):
    return max(1.0, float(np.abs(np.asarray(a)).max()))


def run_gst(tts, mel):
    """(per-layer non-zero fractions, last conv output [C][T'][F'], ref_embs [H], style [d]) of one mel [T][n_mels]."""
    import torch
    with torch.no_grad():
        x = torch.as_tensor(mel)[None, None]
        nz = []
        for m in tts.gst.ref_enc.convs:
            x = m(x)
            if isinstance(m, torch.nn.ReLU):
                nz.append(float((x > 0).double().mean()))
        ys = torch.as_tensor(mel)[None]
        ref = tts.gst.ref_enc(ys)
        style = tts.gst.stl(ref)
        assert torch.equal(style, tts.gst(ys))
    return nz, x[0].numpy(), ref[0].numpy(), style[0].numpy()


def run_text(tts, ids, style, spembs):
    """duration_predict's tensor path behind the encoder: (logd, exp - offset, frames)."""
    import torch
    from espnet.nets.pytorch_backend.nets_utils import make_pad_mask
    text, ilens = torch.from_numpy(ids)[None], torch.tensor([ids.shape[0]])
    with torch.no_grad():
        hs, _ = tts.encoder(text, tts._source_mask(ilens))
        if style is not None:
            hs = hs + torch.as_tensor(style, dtype=hs.dtype)[None].unsqueeze(1)
        if spembs is not None:
            hs = tts._integrate_with_spk_embed(hs, torch.from_numpy(spembs).to(hs.dtype)[None])
        dp = tts.duration_predictor
        x = hs.transpose(1, -1)
        for f in dp.conv:
            x = f(x)
        logd = dp.linear(x.transpose(1, -1)).squeeze(-1)
        expm = logd.exp() - dp.offset
        frames = dp.inference(hs, make_pad_mask(ilens))
    assert torch.equal(frames, torch.clamp(torch.round(expm), min=0).long())
    return logd[0].numpy(), expm[0].numpy(), frames[0].numpy()


def main():
    import make_golden
    make_golden.install_stubs()
    _sedit_stubs()
    import torch
    import espnet2.bin.sedit_inference as S
    from espnet2.text.token_id_converter import TokenIDConverter
    from espnet2.tts.feats_extract.log_mel_fbank import LogMelFbank
    torch.use_deterministic_algorithms(False)
    torch.set_num_threads(1)

    fe = LogMelFbank(**R.FEATS_CONF)
    assert (R.FEATS_CONF["fs"], R.FEATS_CONF["hop_length"]) == (FS, HOP)
    arrays = {}
    meta = dict(token_list=TOKEN_LIST, lengths=list(LENGTHS), mel_lengths=list(R.MEL_LENGTHS), conv_lengths=list(R.CONV_LENGTHS),
                text_prompt=R.TEXT_PROMPT, wav_samples=R.WAV_SAMPLES, feats_extract_conf=R.FEATS_CONF, fs=FS, hop=HOP, offset=1.0,
                mel_eps=R.MEL_EPS, overrides=R.OVERRIDES, cases={})
    proc = types.SimpleNamespace(token_id_converter=TokenIDConverter(TOKEN_LIST))
    records = []
    wavs = {k: R.waveform(n, seed=i) for i, (k, n) in enumerate(sorted(R.WAV_SAMPLES.items()))}
    for name, conf in CASES.items():
        seed = SEEDS[name]
        model, shapes = build(conf, seed)
        m64 = copy.deepcopy(model).double()
        spk = speaker_vector(conf["spk_embed_dim"]) if conf.get("spk_embed_dim") else None
        if spk is not None:
            arrays[f"{name}.spembs"] = spk
        info = dict(tts_conf=conf, seed=seed, shapes=shapes, fp64={}, nonzero={}, sensitivity={})
        styles = {}
        for L in R.MEL_LENGTHS:
            mel = R.mel_input(L, seed)
            nz, conv, ref, style = run_gst(model, mel)
            _, conv64, ref64, style64 = run_gst(m64, mel.astype(np.float64))
            assert all(0.10 <= v <= 0.90 for v in nz), (name, L, nz)
            p = f"{name}.M{L}."
            if L in R.CONV_LENGTHS:
                arrays[p + "conv"] = conv
            arrays[p + "ref_embs"], arrays[p + "style"] = ref, style
            styles[L] = style
            info["nonzero"][str(L)] = [round(v, 3) for v in nz]
            info["fp64"][str(L)] = dict(conv=float(np.abs(conv - conv64).max() / scale_of(conv64)),
                                        ref_embs=float(np.abs(ref - ref64).max() / scale_of(ref64)),
                                        style=float(np.abs(style - style64).max() / scale_of(style64)))
            print(name, "mel", L, "nonzero", info["nonzero"][str(L)], "fp64", info["fp64"][str(L)])
        # two different prompts: far apart
        a, b = styles[R.TEXT_PROMPT], styles[1003]
        apart = float(np.abs(a - b).max() / scale_of(a))
        assert apart >= 0.1, (name, apart)
        info["prompts_apart"] = apart
        changed_by_style = changed_by_prompt = total = 0
        fp64_logd = 0.0
        for T in LENGTHS:
            ids = token_ids(T, seed)
            logd, expm, frames = run_text(model, ids, a, spk)
            logd64, _, _ = run_text(m64, ids, a.astype(np.float64), None if spk is None else spk)
            _, _, bare = run_text(model, ids, None, spk)
            _, _, other = run_text(model, ids, b, spk)
            p = f"{name}.T{T}."
            arrays[p + "logd"], arrays[p + "expm1"], arrays[p + "frames"] = logd, expm, frames
            changed_by_style += int((frames != bare).sum())
            changed_by_prompt += int((frames != other).sum())
            total += T
            fp64_logd = max(fp64_logd, float(np.abs(logd - logd64).max()))
        assert changed_by_style >= 1 and changed_by_prompt >= 1, (name, changed_by_style, changed_by_prompt)
        info.update(frames_changed_by_style=changed_by_style, frames_changed_by_prompt=changed_by_prompt, frames_total=total)
        info["fp64"]["logd_abs"] = fp64_logd
        print(name, "prompts apart", apart, "frames changed by style", changed_by_style, "by prompt", changed_by_prompt, "of", total)

        # from the waveform: the extractor's mel, its style, the sensitivity to the mel, and duration_predict itself
        fs2 = types.SimpleNamespace(tts=model, feats_extract=fe)
        for w, wav in wavs.items():
            with torch.no_grad():
                ys, _ = fe(torch.from_numpy(wav)[None], torch.tensor([len(wav)]))
                style = model.gst(ys)[0].numpy()
                moved = [model.gst(ys + torch.from_numpy(R.mel_perturbation(tuple(ys.shape[1:]), seed=k))[None])[0].numpy()
                         for k in range(4)]
            arrays[f"{name}.wav_{w}.style"] = style
            logd_moved = 0.0
            for phns in (EXTRA_LISTS if w == "a" else EXTRA_LISTS[:2]):
                out = S.duration_predict(list(phns), FS, HOP, fs2, proc, wav, sid=spk)
                assert all(isinstance(v, float) for v in out)
                # the same call's log-domain output: how close every phone is to a rounding tie, and how far the +-2e-4 mels move it
                ids = np.array(proc.token_id_converter.tokens2ids([q if q != "sp" else "<blank>" for q in phns])
                               + [len(TOKEN_LIST) - 1], np.int64)
                logd, _, frames = run_text(model, ids, style, spk)
                assert ((frames * HOP).astype(np.float32) / np.float32(FS))[:-1].tolist() == out
                ties = np.log(np.arange(0, 400) + 1.5)
                tie_log = np.abs(logd[:-1, None] - ties[None, :]).min(1)
                logd_moved = max([logd_moved] + [float(np.abs(run_text(model, ids, sm, spk)[0] - logd).max()) for sm in moved])
                records.append(dict(model=name, wav=w, spembs=spk is not None, phns=list(phns), seconds=out,
                                    tie_log=[float(v) for v in tie_log]))
            info["sensitivity"][w] = dict(frames=int(ys.shape[1]), logd_moved=logd_moved,
                                          style_moved=max(float(np.abs(sm - style).max()) for sm in moved) / scale_of(style))
            print(name, "wav", w, info["sensitivity"][w])
        meta["cases"][name] = info
    meta["duration_predict"] = records
    np.savez_compressed(os.path.join(HERE, "gst_duration.npz"), **arrays)
    with open(os.path.join(HERE, "gst_duration.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for n in ("gst_duration.npz", "gst_duration.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
