"""Latency of dynamic evaluation and prompt-based TTS (a3t_amd/sedit.py: SpeechEditor.dynamic_evaluation / prompt_tts) on
synthetic prompts, and how far the adaptation moves the mel in each compute mode.  Wall time of a whole call including the
collate and the final synchronisation, median over repeated calls after warm-up.  Models: `tiny` (oracle.tiny_config) and
`c2` (BASELINE configs[1]: 6 + 6 blocks, d = 384), procedural weights; the prompt has --words words of three phones each and
about --frames mel frames; prompt_tts appends two words, no vocoder (mel only).

  per SGD step   (median T(steps = 1 + K) - median T(steps = 1)) / K: collate and launch warm-up cancel
  sgd kernel     a3t_sgd_step alone on the model's flat parameter buffer: events around 20 back-to-back launches
  mel moved      max |adapted - unadapted| over the generated span, relative to max |unadapted|, at each --lrs value

    python tools/dyneval_latency.py [--models tiny c2] [--compute f32 bf16] [--calls 50] [--warmup 5] [--lrs 5e-5 1e-2]

Launch counts: `--count-steps N` runs ONE dynamic_evaluation of N steps and nothing else; under
`rocprofv3 --kernel-trace --stats -- python tools/dyneval_latency.py --models c2 --compute bf16 --count-steps N` the
difference of the dispatch counts of N = 3 and N = 1, halved, is the launches of one step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEX = {"THE": ["DH", "AH0", "V"], "CAT": ["K", "AE1", "T"], "SAT": ["S", "AE1", "T"], "MAT": ["M", "AE1", "T"],
       "DOG": ["D", "AO1", "G"], "RAN": ["R", "AE1", "N"], "HOME": ["HH", "OW1", "M"], "TODAY": ["T", "AH0", "D"]}


def phonemise(line):
    phns, w2p = [], {}
    for i, w in enumerate(line.split()):
        w = w if w == "[MASK]" else w.upper()
        ph = [w] if w == "[MASK]" else LEX[w]
        w2p[f"{i}_{w}"] = ph
        phns.extend(ph)
    return phns, w2p


def prompt(words, frames, fs, hop, seed=0):
    rs = np.random.RandomState(seed)
    names = sorted(LEX)
    old = [names[i % len(names)] for i in rs.permutation(words)]
    n_ph = 3 * words
    d = rs.uniform(0.7, 1.3, n_ph)
    d = d / d.sum() * (frames * hop / fs)
    t, times2, w2p, k = 0.0, [], {}, 0
    for i, w in enumerate(old):
        w2p[f"{i}_{w}"] = " ".join(LEX[w])
        for ph in LEX[w]:
            times2.append([ph, round(t, 4), round(t + d[k], 4)])
            t = round(t + d[k], 4)
            k += 1
    wav = (0.1 * rs.standard_normal(int(np.ceil(t * fs)) + 100)).astype(np.float32)
    old_str = " ".join(w.lower() for w in old)
    return wav, times2, w2p, old_str, old_str + " ran home"


def editor(which, compute):
    from a3t_amd.collate import MLMCollateFn
    from a3t_amd.config import A3TConfig
    from a3t_amd.espnet_model import ESPnetMLMEncAsDecoderModel
    from a3t_amd.features import LogMelFbank
    from a3t_amd.sedit import SpeechEditor
    from oracle import a3t_oracle as O
    oc = O.tiny_config() if which == "tiny" else O.A3TConfig(enc_blocks=6, dec_blocks=6)
    c = A3TConfig(**{k: getattr(oc, k) for k in ("idim", "odim", "vocab", "adim", "heads", "ff", "ff_kernel", "enc_blocks",
                                                  "dec_blocks", "enc_kernel", "dec_kernel", "postnet_layers", "postnet_chans",
                                                  "postnet_filts", "max_len", "seg_table", "lsm_weight")})
    model = ESPnetMLMEncAsDecoderModel([f"t{i}" for i in range(oc.vocab)], oc.odim, None, None, c, device="cuda",
                                       compute=compute)
    state = O.procedural_state(O.param_shapes(oc), 3)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()
    fe = LogMelFbank(fs=oc.fs, n_fft=oc.n_fft, win_length=oc.win_length, hop_length=oc.hop_length, n_mels=oc.n_mels,
                     fmin=oc.fmin, fmax=oc.fmax, device="cuda")
    coll = MLMCollateFn(fe, float_pad_value=0.0, int_pad_value=0, mlm_prob=oc.mlm_prob, mean_phn_span=oc.mean_phn_span,
                        sega_emb=True)
    ids = lambda phns: np.array([2 + sum(map(ord, ph)) % (oc.vocab - 4) for ph in phns], dtype=np.int64)
    dur = lambda phns: [0.05 + 0.01 * (sum(map(ord, ph)) % 5) for ph in phns]
    return SpeechEditor(model, coll, None, ids, dur), oc


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def sgd_alone(store, calls):
    from a3t_amd import ops
    g = torch.zeros_like(store.flat)
    reps, ts = 20, []
    for _ in range(calls + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            ops.sgd_step(store.flat, g, 1e-3)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    us = 1e3 * float(np.median(ts[3:]))
    return dict(n=int(store.flat.numel()), us=round(us, 2), tb_per_s=round(12.0 * store.flat.numel() / (us * 1e-6) / 1e12, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["tiny", "c2"])
    ap.add_argument("--compute", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--extra-steps", type=int, default=2)
    ap.add_argument("--lrs", type=float, nargs="*", default=[5e-5, 1e-2])
    ap.add_argument("--moved-steps", type=int, default=3)
    ap.add_argument("--count-steps", type=int, default=0)
    a = ap.parse_args()
    out = {}
    for which in a.models:
        for compute in a.compute:
            ed, oc = editor(which, compute)
            wav, times2, w2p, old_str, new_str = prompt(a.words, a.frames, oc.fs, oc.hop_length)
            dyn = (wav, times2, w2p, old_str, phonemise)
            if a.count_steps:
                ed.dynamic_evaluation(*dyn, lr=1e-3, steps=a.count_steps)
                torch.cuda.synchronize()
                continue
            new_phns, new_w2p = phonemise(new_str)
            tts = (wav, times2, w2p, new_phns, new_w2p, old_str, new_str)
            K = a.extra_steps
            with ed:
                t1 = timed(lambda: ed.dynamic_evaluation(*dyn, lr=1e-6, steps=1), a.calls, a.warmup)
                tk = timed(lambda: ed.dynamic_evaluation(*dyn, lr=1e-6, steps=1 + K), a.calls, a.warmup)
            r = dict(rows=a.words - 1, frames=a.frames, dyneval_1_step_call_ms=round(t1, 3),
                     per_sgd_step_ms=round((tk - t1) / K, 3),
                     prompt_tts_ms=round(timed(lambda: ed.prompt_tts(*tts), a.calls, a.warmup), 3),
                     prompt_tts_dyneval_1_step_ms=round(timed(lambda: ed.prompt_tts(*tts, dynamic_eval=(1e-6, 1),
                                                                                   phonemise_fn=phonemise), a.calls, a.warmup), 3),
                     sgd_kernel=sgd_alone(ed.model.store, a.calls))
            base = ed.prompt_tts(*tts)
            s, e = base["new_span_boundary"]
            ref = base["feat"][s:e]
            moved = {}
            for lr in a.lrs:
                got = ed.prompt_tts(*tts, dynamic_eval=(lr, a.moved_steps), phonemise_fn=phonemise)["feat"][s:e]
                moved[f"{lr:g}"] = float((got - ref).abs().max() / ref.abs().max())
            r["mel_moved"] = dict(steps=a.moved_steps, by_lr=moved)
            out[f"{which}.{compute}"] = r
    if not a.count_steps:
        print(json.dumps({"dyneval_latency": out}))


if __name__ == "__main__":
    main()
