"""Latency of the GST style path of the duration model (a3t_amd/duration.py, csrc/gst.hip) next to the same computation as
torch ops on the same GPU: tests/gst_ref.py, the restatement the kernels are tested against, with its weights on the device.
The model is the fixture's `gst_xadd` (ljspeech conformer shape, default style plan, x-vector add, procedural weights).

    python tools/gst_style_latency.py [--frames 400 1000] [--batch 1 8] [--calls 50] [--warmup 5]

Per (frames, B): wall time of ONE style embedding of B prompts from given log-mel frames, synchronised, in the order A (torch
ops), B (native), A in one process, median of --calls after --warmup; the spread between the two A runs is the noise a
difference has to exceed, and both results are compared.  Then, native only, one full duration call with a prompt --
fn.batch(B phone lists, prompts=B waveforms of that many frames): log-mel, style, the batched duration forward, frames on the
host -- and the same call's style part alone from the waveforms.

Launches: --only torch|native --calls K --warmup 0 runs exactly K style embeddings of the first (frames, B) after the set-up,
so the dispatch counts of two `rocprofv3 --kernel-trace --stats` runs with K = 1 and K = 2 differ by the launches of one.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(call, calls, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def _ms(ts):
    return dict(median_ms=round(1e3 * float(np.median(ts)), 4), min_ms=round(1e3 * float(np.min(ts)), 4),
                max_ms=round(1e3 * float(np.max(ts)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[400, 1000])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["torch", "native"], default=None, help="one leg of the first shape only (kernel traces)")
    a = ap.parse_args()
    import gst_ref as R
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    meta = R.meta()
    cfg, sd = R.checkpoint(meta, "gst_xadd")
    m = FS2DurationModel(FS2DurationConfig.from_espnet(cfg, gst=True), "cuda").load_state_dict({"tts." + k: v for k, v in sd.items()})
    dsd = {k: v.cuda() for k, v in sd.items() if k.startswith("gst.") and v.is_floating_point()}
    tts_conf = cfg["tts_conf"]
    spk = np.random.RandomState(77).standard_normal(512).astype(np.float32)
    fn = m.duration_fn(meta["fs"], meta["hop"], spembs=spk)
    phones = [t for t in meta["token_list"][2:-1]]
    rs = np.random.RandomState(0)
    out = {}
    for F in a.frames:
        for B in a.batch:
            mel = torch.from_numpy(np.stack([R.mel_input(F, seed=b) for b in range(B)])).cuda()
            legs = {"torch": lambda: R.style_encoder(dsd, tts_conf, mel)[2], "native": lambda: m.style_from_mel(mel)}
            if a.only is not None:
                with torch.no_grad():
                    _timed(legs[a.only], a.calls, a.warmup)
                print(json.dumps({"gst_style_trace": dict(leg=a.only, frames=F, B=B, calls=a.calls)}))
                return
            with torch.no_grad():
                want, got = legs["torch"](), legs["native"]()
                row = dict(max_abs_diff=float((want - got).abs().max()))
                for name, leg in (("A1", "torch"), ("B", "native"), ("A2", "torch")):
                    row[name] = _ms(_timed(legs[leg], a.calls, a.warmup))
            a1, a2, b = (row[k]["median_ms"] for k in ("A1", "A2", "B"))
            row["A_spread_ms"] = round(abs(a1 - a2), 4)
            row["B_over_A"] = round(b / (0.5 * (a1 + a2)), 4)
            row["faster_beyond_spread"] = bool(min(a1, a2) - b > abs(a1 - a2))
            # one full duration call with a prompt, and its style part from the waveform (log-mel included)
            wavs = [R.waveform((F - 1) * meta["hop"], seed=b) for b in range(B)]
            lists = [[phones[i] for i in rs.randint(0, len(phones), 60)] for _ in range(B)]
            row["native_duration_call"] = _ms(_timed(lambda: fn.batch(lists, prompts=wavs), a.calls, a.warmup))
            row["native_style_from_wav"] = _ms(_timed(lambda: m.style_embedding_batch(wavs), a.calls, a.warmup))
            row["calls"] = a.calls
            out[f"frames{F}_B{B}"] = row
    print(json.dumps({"gst_style_latency": out}))


if __name__ == "__main__":
    main()
