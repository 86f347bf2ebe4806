"""One x-vector per row of a FastSpeech2 batch: the inputs of tests/golden/fs2_speakers.{npz,json} and the CPU restatement of
such a batch.  The restatements themselves are tests/fs2_tts_ref.py's (and, through it, fs2_ragged_ref's and gst_ref's), which
take ONE x-vector per call: here they are called row by row, each row alone at its own length with its own x-vector, which is
what a row of a batch with per-row speakers has to equal.

The fixture reuses the procedural models of tests/golden/fs2_tts.json (xadd, xcat, gst_norm: their configs, seeds, duration
predictor overrides, token ids and, for the GST model, its prompt), so no weights are stored again; per model it adds
N_SPEAKERS x-vectors drawn from seeds, on the scales NORMS -- F.normalize in front of the projection has to matter.  Not a
test module: tests/test_fs2_speakers_host.py and tests/test_gpu_fs2_speakers.py import it, and
tests/golden/make_golden_fs2_speakers.py takes the inputs from here.  Nothing of the reference is imported."""
import json
import os

import numpy as np
import torch

import fs2_tts_ref as R
import gst_ref as GR

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MODELS = ("xadd", "xcat", "gst_norm")
LENGTHS = (2, 7, 33)
NORMS = (0.3, 1.0, 20.0)               # |x| of the three x-vectors of every model
N_SPEAKERS = len(NORMS)
STAGES = ("logd", "pitch", "energy", "before", "feat_gen", "feat_gen_denorm")
MEL_STAGES = ("pitch", "energy", "before", "feat_gen", "feat_gen_denorm")


def speaker_vector(dim, model_seed, k, draw):
    """x-vector k of a model: a standard normal draw scaled to the norm NORMS[k]; `draw` counts the generator's re-draws."""
    v = np.random.RandomState(770000 + 1000 * model_seed + 100 * k + draw).standard_normal(dim)
    return (v * (NORMS[k] / np.linalg.norm(v))).astype(np.float32)


def meta():
    return json.load(open(os.path.join(G, "fs2_speakers.json")))


def arrays():
    return np.load(os.path.join(G, "fs2_speakers.npz"))


def tag(case, k, T):
    return f"{case}.s{k}.T{T}"


def inputs(tts_meta, spk_meta, case):
    """Of one fixture model: ({T: ids int64 [T], eos included}, [x-vector] * N_SPEAKERS, raw prompt mel | None, mean, std)."""
    mc = tts_meta["cases"][case]
    conf = mc["tts_conf"]
    ids = {T: R.token_ids(T, mc["input_seeds"][str(T)], len(tts_meta["token_list"])) for T in LENGTHS}
    draws = spk_meta["cases"][case]["draws"]
    spk = [speaker_vector(conf["spk_embed_dim"], mc["seed"], k, draws[k]) for k in range(N_SPEAKERS)]
    prompt = GR.mel_input(tts_meta["prompt_frames"], mc["seed"]) if conf.get("use_gst") else None
    mean, std = R.mvn_mean_std(np.load(R.stats_file())) if mc["normalize"] else (None, None)
    return ids, spk, prompt, mean, std


def phones(tts_meta, ids):
    """The phone strings whose tokens_to_ids is `ids` (the fixture's ids are never <blank>, <unk> or, but for the last, eos)."""
    return [tts_meta["token_list"][int(i)] for i in ids[:-1]]


def synthesize_rows(p, conf, rows, speakers, prompt=None, mean=None, std=None, dtype=torch.float64):
    """fs2_tts_ref.synthesize for every (ids, x-vector) pair on its own: a list of dicts of numpy arrays trimmed to the row
    (duration, logd, pitch, energy [T]; before, feat_gen, feat_gen_denorm [F][odim])."""
    out = []
    for ids, x in zip(rows, speakers):
        ids = np.asarray(ids, np.int64)
        got = R.synthesize(p, conf, ids[None], [len(ids)], x, prompt, 1.0, mean, std, dtype=dtype)
        row = {k: v[0].numpy() for k, v in got.items() if torch.is_tensor(v)}
        row["logd"] = text_logd(p, conf, ids, x, prompt, mean, std, dtype)
        out.append(row)
    return out


def text_logd(p, conf, ids, x, prompt=None, mean=None, std=None, dtype=torch.float64):
    """The log-domain durations [T] of one row with its x-vector (fs2_tts_ref.ragged_text; a GST model's style from the prompt's
    log-mel normalised as inference normalises it)."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
    style = None
    if conf.get("use_gst"):
        mel = R.normalize_mel(torch.as_tensor(np.asarray(prompt)).to(dtype), mean, std)
        style = GR.style_encoder(p, conf, mel[None])[2]
    ids = torch.as_tensor(np.asarray(ids, np.int64))[None]
    return R.ragged_text(p, conf, ids, [ids.shape[1]], x, style, dtype)[1][0].numpy()


def mel_bound(F):
    """tests/test_gpu_fs2_tts.py's bound on a mel-side stage, of the stage's scale."""
    return max(4 * F, 1e-4)


LOGD_BOUND = 1e-4                      # tests/test_gpu_duration*.py's bound on the log-domain durations (absolute)
