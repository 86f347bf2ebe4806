"""Generate tests/golden/dyneval.{npz,json}: dynamic evaluation and prompt-based TTS of the speech-editing driver
(sedit_inference.py: dynamic_evaluation :748-776, get_mlm_output :673-683, prompt_decoding_fn :685-707) run by the
REFERENCE itself on a tiny model, in the build container only.

    python tests/golden/make_golden_dyneval.py

It regenerates both files bit-identically on the same machine (one torch thread, no global-RNG use after seeding; checked by
running it twice and comparing the files).

The driver is imported through make_golden.install_stubs() and the stubs gen_sedit uses.  Its external programs are replaced by
synthetic stand-ins whose outputs are stored as the fixture's inputs:
  load_model          -> the reference model of oracle.tiny_config() (sega_mlm input layer: segment embeddings on) with
                         procedural weights (oracle.procedural_state, seed MODEL_SEED), built fresh on every call like a
                         checkpoint load
  alignment           -> TIMES2 / WORD2PHNS below (phones of LEX, durations from RandomState(ALIGN_SEED))
  words2phns_yuan     -> phonemise(): LEX look-up, `[MASK]` is its own one-phone word
  preprocessor        -> token_ids(): phone -> id by a fixed rule (the recipe's CommonPreprocessor needs a g2p install)
  librosa.load        -> white noise from RandomState(WAV_SEED), stored
  duration model      -> make_golden.fake_phone_duration
  vocoder             -> zeros of hop * frames samples (only the crop arithmetic of prompt_decoding_fn is recorded)

Stored (data only): the stand-in outputs; every entry of the batch dynamic_evaluation builds; the integer tensors of the
collated batch; the loss of every step; a fixed-seed sample (sample_index) of <= 256 elements of every parameter's gradient
at step 1 and of its total change after STEPS steps; the mel prompt_decoding_fn's decode returns after the adaptation, the
same decode without adaptation, and the span boundaries; and the fp32-vs-fp64 floor of the reference itself: the same
dynamic_evaluation run with the model and the features in float64, per-tensor relative L2 difference of the total change
and the largest difference of the adapted mel relative to its scale.

LR / STEPS: at the reference's default lr = 5e-5 an update lr * g is of the order of one fp32 ulp of the weight it is added
to, so the stored change would mostly be rounding; LR is chosen so that the change is well resolved and the reference's own
losses fall strictly from step to step (asserted below).
"""
import argparse
import importlib.machinery
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

MODEL_SEED = 1
ALIGN_SEED = 17
WAV_SEED = 23
SAMPLE_SEED = 4242
N_SAMPLE = 256
LR = 1e-2
STEPS = 3
LEX = {"THE": ["DH", "AH0"], "CAT": ["K", "AE1", "T"], "SAT": ["S", "AE1", "T"], "ON": ["AA1", "N"], "A": ["AH0"],
       "MAT": ["M", "AE1", "T"], "DOG": ["D", "AO1", "G"], "RAN": ["R", "AE1", "N"], "HOME": ["HH", "OW1", "M"],
       "TODAY": ["T", "AH0", "D", "EY1"]}
OLD_WORDS = ["THE", "CAT", "SAT", "ON", "A", "MAT"]
NEW_WORDS = OLD_WORDS + ["RAN", "HOME"]
SILENCE_AFTER = {-1, 2, 5}         # `sp` in front (-1) and after these word indices


def sample_index(i, numel):
    """Indices of the stored sample of the i-th parameter (state-dict order of the parameters): all of a small tensor."""
    if numel <= N_SAMPLE:
        return np.arange(numel)
    return np.sort(np.random.RandomState(SAMPLE_SEED + i).choice(numel, N_SAMPLE, replace=False))


def token_ids(phns, vocab):
    return np.array([2 + sum(map(ord, ph)) % (vocab - 4) for ph in phns], dtype=np.int64)


def phonemise(line):
    """Stand-in for words2phns_yuan: (phones, {"<i>_<WORD>": [phones]}); `[MASK]` is a word of one phone."""
    phns, w2p = [], {}
    for i, w in enumerate(line.split()):
        w = w if w == "[MASK]" else w.upper()
        ph = [w] if w == "[MASK]" else LEX[w]
        w2p[f"{i}_{w}"] = ph
        phns.extend(ph)
    return phns, w2p


def aligner_output():
    rs = np.random.RandomState(ALIGN_SEED)
    seq = ["sp"] if -1 in SILENCE_AFTER else []
    for i, w in enumerate(OLD_WORDS):
        seq.append(w)
        if i in SILENCE_AFTER:
            seq.append("sp")
    t, times2, word2phns = 0.0, [], {}
    for idx, w in enumerate(seq):
        phs = ["sp"] if w == "sp" else LEX[w]
        word2phns[f"{idx}_{w}"] = " ".join(phs)
        for ph in phs:
            d = round(float(rs.uniform(0.04, 0.11)), 4)
            times2.append([ph, round(t, 4), round(t + d, 4)])
            t = round(t + d, 4)
    return times2, word2phns, t


def _sedit_stubs():
    class _Any:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return True

        def __getattr__(self, k):
            return _Any()

    for n in ["matplotlib", "matplotlib.pylab", "parallel_wavegan", "parallel_wavegan.utils", "ipywidgets", "IPython",
              "IPython.display", "espnet2.tasks.tts", "espnet2.bin.align_english"]:
        m = types.ModuleType(n)
        m.__spec__ = importlib.machinery.ModuleSpec(n, None)
        m.__path__ = []

        def _ga(k):
            if k.startswith("__"):
                raise AttributeError(k)
            return _Any()

        m.__getattr__ = _ga
        sys.modules[n] = m


def main():
    import make_golden
    make_golden.install_stubs()
    _sedit_stubs()
    import torch
    import espnet2.bin.sedit_inference as S
    from espnet2.tasks.mlm import MLMTask
    from espnet2.tts.feats_extract.log_mel_fbank import LogMelFbank
    from oracle import a3t_oracle as O
    torch.use_deterministic_algorithms(False)     # (the driver switches it on at import)
    torch.set_num_threads(1)

    c = O.tiny_config()
    fs, hop = c.fs, c.hop_length
    times2, word2phns, t_end = aligner_output()
    wav = (0.1 * np.random.RandomState(WAV_SEED).standard_normal(int(np.ceil(t_end * fs)) + 137)).astype(np.float32)
    old_str = " ".join(w.lower() for w in OLD_WORDS)
    new_str = " ".join(w.lower() for w in NEW_WORDS)

    # ---- stand-ins
    seen = {}
    real_build_model = MLMTask.build_model.__func__
    MLMTask.build_model = classmethod(lambda cls, a: (seen.__setitem__("args", a), real_build_model(cls, a))[1])
    state = {"double": False, "losses": [], "entries": None, "feats": None, "grads": None, "model": None}

    def load_model(name):
        model, _ = make_golden.build_ref_model(c, c.vocab)
        make_golden.load_procedural(model, c, seed=MODEL_SEED)
        if state["double"]:
            model.double()
        model.register_forward_hook(lambda m, i, o: state["losses"].append(float(o[0].detach().double())))
        state["model"] = model
        args = argparse.Namespace(**vars(seen["args"]))      # (build_model consumes the extractor's settings)
        args.feats_extract = "fbank"
        args.feats_extract_conf = dict(n_fft=c.n_fft, hop_length=c.hop_length, win_length=c.win_length, fs=c.fs, fmin=c.fmin,
                                       fmax=c.fmax, n_mels=c.n_mels)
        model.feats_extract = LogMelFbank(**args.feats_extract_conf)     # (a model built with odim owns none; the driver reads it)
        return model, args

    real_collate = MLMTask.build_collate_fn.__func__

    def build_collate_fn(cls, args, train, epoch=-1):
        fn = real_collate(cls, args, train, epoch)

        def collate(batch):
            if len(batch) > 1:
                state["entries"] = batch
            uids, feats = fn(batch)
            if len(batch) > 1:
                state["feats"] = {k: v.clone() for k, v in feats.items()}
            if state["double"]:
                feats = {k: (v.double() if v.is_floating_point() else v) for k, v in feats.items()}
            return uids, feats
        return collate

    MLMTask.build_collate_fn = classmethod(build_collate_fn)
    MLMTask.build_preprocess_fn = classmethod(
        lambda cls, args, train: (lambda uid, data: {"text": token_ids(data["text"].split(), c.vocab)}))
    real_step = torch.optim.SGD.step

    def sgd_step(self, *a, **k):
        if state["grads"] is None:      # gradients of the first step, before the update
            state["grads"] = [p.grad.detach().clone() for g in self.param_groups for p in g["params"]]
        return real_step(self, *a, **k)

    torch.optim.SGD.step = sgd_step
    S.load_model = load_model
    S.alignment = lambda wav_path, txt: (times2, word2phns)
    S.words2phns_yuan = phonemise
    S.get_fs2_model = lambda path: (None, None)
    S.duration_predict = lambda phns, fs_, hop_, m, pr, w, sid=None: make_golden.fake_phone_duration(phns)
    S.librosa.load = lambda path, sr=None: (wav, sr)
    decoded = {}
    real_decode = S.decode_with_model

    def decode_with_model(*a, **k):
        r = real_decode(*a, **k)
        decoded["r"] = r
        return r

    S.decode_with_model = decode_with_model
    vocoder = lambda feat: torch.zeros(feat.shape[0] * hop)

    def run(double, dynamic_eval):
        state.update(double=double, losses=[], grads=None)
        out = S.prompt_decoding_fn("model", "x.wav", old_str, old_str, new_str, vocoder, "fs2.pth", dynamic_eval=dynamic_eval)
        _, _, feat, old_b, new_b, _, _ = decoded["r"]
        return out, feat.detach(), [int(x) for x in old_b], [int(x) for x in new_b]

    ref0 = {k: v.detach().clone() for k, v in load_model("model")[0].named_parameters()}
    names = list(ref0)
    state["losses"] = []

    # ---- the reference, fp32: unadapted decode, then dynamic evaluation + decode
    _, mel0, _, _ = run(False, (0, 0))
    out, mel, old_b, new_b = run(False, (LR, STEPS))
    losses = list(state["losses"][:STEPS])
    assert len(state["losses"]) == STEPS, state["losses"]      # (inference() does not go through forward)
    assert all(b < a for a, b in zip(losses, losses[1:])), f"the reference's losses do not fall at lr={LR}: {losses}"
    model32 = state["model"]
    grads = state["grads"]
    delta = {k: (v.detach() - ref0[k]) for k, v in model32.named_parameters()}
    entries, feats = state["entries"], state["feats"]
    assert out["new_wav"].shape[0] == hop * (mel.shape[0] - new_b[0])
    bufs_after = {k: v for k, v in model32.named_buffers() if "running" in k or "num_batches" in k}
    fresh = load_model("model")[0]
    for k, v in fresh.named_buffers():
        if k in bufs_after:
            assert torch.equal(v, bufs_after[k]), k         # eval-mode steps leave the BatchNorm buffers alone
    state["losses"] = []

    # ---- the reference, fp64: the floor of the fixture (what fp32 rounding alone does to the trajectory)
    _, mel64, _, _ = run(True, (LR, STEPS))
    losses64 = list(state["losses"][:STEPS])
    delta64 = {k: (v.detach() - ref0[k].double()) for k, v in state["model"].named_parameters()}
    floor_delta = {k: float((delta[k].double() - delta64[k]).norm() / delta64[k].norm().clamp_min(1e-300)) for k in names}
    mel_scale = float(mel64.abs().max())
    floor_mel = float((mel.double() - mel64).abs().max() / mel_scale)

    arrays = {"wav": wav, "mel": mel.numpy(), "mel_unadapted": mel0.numpy(), "losses": np.asarray(losses, np.float64),
              "losses64": np.asarray(losses64, np.float64)}
    for i, (u, e) in enumerate(entries):
        assert u == str(i) and e["speech"].dtype == np.float32 and np.array_equal(e["speech"], wav)
        for k in ("align_start", "align_end", "text", "span_boundary"):
            arrays[f"entry{i}.{k}"] = np.asarray(e[k])
    for k, v in feats.items():
        if not v.is_floating_point():
            arrays["batch." + k] = v.numpy()
    assert feats["speech"].dtype == torch.float32
    for i, k in enumerate(names):
        idx = sample_index(i, ref0[k].numel())
        arrays["grad." + k] = grads[i].reshape(-1)[idx].numpy()
        arrays["delta." + k] = delta[k].reshape(-1)[idx].numpy()
        arrays["gradmax." + k] = np.asarray(float(grads[i].abs().max()), np.float64)
        arrays["deltanorm." + k] = np.asarray(float(delta[k].double().norm()), np.float64)
    meta = dict(fs=fs, hop=hop, lr=LR, steps=STEPS, model_seed=MODEL_SEED, sample_seed=SAMPLE_SEED, n_sample=N_SAMPLE,
                old_str=old_str, new_str=new_str, times2=times2, word2phns=word2phns,
                phonemise={ln: list(phonemise(ln)) for ln in
                           [new_str] + [" ".join(old_str.split()[:i] + ["[MASK]"] + old_str.split()[i + 1:])
                                        for i in range(len(OLD_WORDS) - 1)]},
                token_ids={ph: int(token_ids([ph], c.vocab)[0]) for ph in
                           sorted({p for v in LEX.values() for p in v} | {"sp", "[MASK]"})},
                param_names=names, n_entries=len(entries), old_span_boundary=old_b, new_span_boundary=new_b,
                new_wav_len=int(out["new_wav"].shape[0]), mel_frames=int(mel.shape[0]),
                losses=losses, losses64=losses64, floor_delta=floor_delta,
                # (tensors whose gradient is analytically zero -- linear_k.bias -- change by rounding noise only: no floor)
                floor_delta_max=max(v for k, v in floor_delta.items() if float(delta64[k].norm()) > 1e-6),
                zero_gradient=[k for k in names if float(delta64[k].norm()) <= 1e-6],
                floor_mel=floor_mel, mel_scale=mel_scale,
                mel_moved=float((mel - mel0).abs().max() / mel_scale))
    np.savez_compressed(os.path.join(HERE, "dyneval.npz"), **arrays)
    with open(os.path.join(HERE, "dyneval.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("losses fp32", losses, "fp64", losses64)
    print("floor: delta max", meta["floor_delta_max"], "mel", floor_mel, "| mel moved by adaptation", meta["mel_moved"])
    print("spans", old_b, new_b, "frames", mel.shape[0], "batch", {k: tuple(v.shape) for k, v in feats.items()})
    for n in ("dyneval.npz", "dyneval.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
