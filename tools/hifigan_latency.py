"""Latency of the HiFi-GAN generator (a3t_amd/vocoder.py::HiFiGANGeneratorHIP), layer by layer against fused, on the 24 kHz v1
plan (512 channels, scales 5 5 4 3, kernels 3 7 11, dilations 1 3 5) with procedural weights.  A report: no speed is promised.

  A  fused=False: a3t_leaky_relu + the exact-fp32 GEMM for every convolution
  B  fused=True:  the 64- and 32-channel stages on a3t_hfg_conv, the output convolution on a3t_hfg_out
  order A, B, A in one process; wall time of inference() on a mel that is already on the device, median / min / max over
  --calls after warm-up; per stage: HIP events around each stage's residual blocks (`rest`: the input convolution, the four
  transposed convolutions, the output convolution and the tail zeroing).
  workloads: 8 x 1000 frames, and the ragged lengths 1000 / 700 / 500 / 300 x 2 through lengths=.
  context: ParallelWaveGAN v1 (compute f32 and f16) on the same workloads.

    python tools/hifigan_latency.py [--calls 20] [--warmup 3] [--frames 1000] [--out profiles/hifigan_latency.txt]

  --compute f32 f16: the compute-mode leg instead -- fused=True with compute f32, f16, f32 again in one process on the same
  workloads, per-stage block times for all three, f16 over the mean of the two f32 runs per stage, and the f16 blocks' achieved
  TB/s against the byte model of csrc/hifigan_f16.hip (per sample and convolution 4 C bytes for each of: x read, R read, y or acc
  written, acc read with acc_add).  Default --out profiles/hifigan_f16.txt.

    python tools/hifigan_latency.py --compute f32 f16 [--calls 20] [--warmup 3] [--frames 1000] [--out profiles/hifigan_f16.txt]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 3), min_max_ms=[round(min(ts), 3), round(max(ts), 3)])


def series(gen, c, lengths, calls, warmup, stages=False):
    """inference(c, lengths=) `calls` times: wall ms, and with stages=True the HIP-event time of every stage's residual blocks."""
    marks = []
    if stages:
        def wrap(fn):
            def run(st, *a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(st, *a)
                e1.record()
                marks.append((st["C"], e0, e1))
                return out
            return run
        gen._stage_fused, gen._stage_layers = wrap(type(gen)._stage_fused.__get__(gen)), wrap(type(gen)._stage_layers.__get__(gen))
    try:
        for _ in range(warmup):
            y = gen.inference(c, lengths=lengths)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all())
        marks.clear()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            gen.inference(c, lengths=lengths)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
    finally:
        if stages:
            del gen._stage_fused, gen._stage_layers
    out = stats(ts)
    if stages:
        per = {}
        for C, e0, e1 in marks:
            per.setdefault(f"blocks_C{C}_ms", []).append(e0.elapsed_time(e1))
        out["stages"] = {k: round(float(np.median(v)), 3) for k, v in per.items()}
        out["stages"]["rest_ms"] = round(out["median_ms"] - sum(out["stages"].values()), 3)
    return out


def block_bytes(gen, st, samples):
    """HBM bytes of one stage's residual blocks by the kernels' byte model: every convolution reads x and writes y or acc
    (4 C each), the last of a unit reads R, an accumulating one reads acc."""
    per = 0
    for j, blk in enumerate(st["blocks"]):
        for u in range(len(blk["units"])):
            last = u == len(blk["units"]) - 1
            per += (8 if gen.add else 0) + 12 + (4 if last and j > 0 else 0)
    return per * st["C"] * samples


def compute_leg(a):
    """fused=True: compute f32, f16, f32 again."""
    import hifigan_ref as R
    from a3t_amd.vocoder import F16_WIDTHS, HiFiGANGeneratorHIP
    prop = torch.cuda.get_device_properties(0)
    out = {"device": f"{prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)",
           "plan": "24 kHz v1: 512 channels, scales 5 5 4 3, kernels 3 7 11, dilations 1 3 5", "calls": a.calls,
           "order": list(a.compute) + [a.compute[0]], "F16_WIDTHS": list(F16_WIDTHS)}
    state = R.procedural_hifigan_state(R.V1, 41)
    gens = {cm: HiFiGANGeneratorHIP(state, device="cuda", compute=cm, **R.V1) for cm in a.compute}
    base, mode = a.compute
    F = a.frames
    sets = {f"8x{F}": (8, None), "ragged": (8, [F, F * 7 // 10, F // 2, F * 3 // 10] * 2)}
    for name, (B, lengths) in sets.items():
        c = torch.randn(B, F, 80, device="cuda")
        r = dict(lengths=lengths)
        r[f"{base}_first"] = series(gens[base], c, lengths, a.calls, a.warmup, True)
        r[mode] = series(gens[mode], c, lengths, a.calls, a.warmup, True)
        r[f"{base}_again"] = series(gens[base], c, lengths, a.calls, a.warmup, True)
        frames = sum(lengths) if lengths else B * F
        r["valid_samples"] = frames * gens[mode].upsample_factor
        ratio = {"whole": round(2 * r[mode]["median_ms"] / (r[f"{base}_first"]["median_ms"] + r[f"{base}_again"]["median_ms"]), 4)}
        model, rate = {}, 1
        for st in gens[mode].stages:
            rate *= st["s"]
            key = f"blocks_C{st['C']}_ms"
            ratio[key] = round(2 * r[mode]["stages"][key] / (r[f"{base}_first"]["stages"][key] + r[f"{base}_again"]["stages"][key]), 4)
            if st["f16"]:
                nbytes = block_bytes(gens[mode], st, frames * rate)
                model[f"blocks_C{st['C']}"] = dict(model_GB=round(nbytes / 1e9, 3),
                                                    achieved_TBps=round(nbytes / 1e9 / r[mode]["stages"][key], 3))
        r[f"{mode}_over_{base}"] = ratio
        r[f"{mode}_byte_model"] = model
        out[name] = r
        print(json.dumps({name: r}), flush=True)
    with open(a.out, "w") as f:
        f.write("tools/hifigan_latency.py --compute: HiFi-GAN generator, fused=True, compute modes in the order run; ms per call\n")
        f.write(json.dumps({"hifigan_f16": out}, indent=1) + "\n")
    print(json.dumps({"hifigan_f16": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pwg", action="store_true")
    ap.add_argument("--compute", nargs=2, choices=("f32", "f16"), default=None, metavar=("BASE", "MODE"))
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "hifigan_f16.txt" if a.compute else "hifigan_latency.txt")
    if a.compute:
        return compute_leg(a)
    import hifigan_ref as R
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, ParallelWaveGANGeneratorHIP
    prop = torch.cuda.get_device_properties(0)
    out = {"device": f"{prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)",
           "plan": "24 kHz v1: 512 channels, scales 5 5 4 3, kernels 3 7 11, dilations 1 3 5", "calls": a.calls}
    state = R.procedural_hifigan_state(R.V1, 41)
    gens = {False: HiFiGANGeneratorHIP(state, device="cuda", fused=False, **R.V1),
            True: HiFiGANGeneratorHIP(state, device="cuda", fused=True, **R.V1)}
    F = a.frames
    sets = {f"8x{F}": (8, None), "ragged": (8, [F, F * 7 // 10, F // 2, F * 3 // 10] * 2)}
    for name, (B, lengths) in sets.items():
        c = torch.randn(B, F, 80, device="cuda")
        r = dict(lengths=lengths, A_first=series(gens[False], c, lengths, a.calls, a.warmup, True),
                 B=series(gens[True], c, lengths, a.calls, a.warmup, True),
                 A_again=series(gens[False], c, lengths, a.calls, a.warmup))
        A = 0.5 * (r["A_first"]["median_ms"] + r["A_again"]["median_ms"])
        r["B_over_A"] = round(r["B"]["median_ms"] / A, 4)
        r["valid_samples"] = (sum(lengths) if lengths else B * F) * gens[True].upsample_factor
        out[name] = r
        print(json.dumps({name: r}), flush=True)
        if not a.no_pwg:
            from sedit_batch_latency import vocoder_state
            for compute in ("f32", "f16"):
                pwg = ParallelWaveGANGeneratorHIP(vocoder_state(), device="cuda", compute=compute)
                out[f"pwg_{compute}.{name}"] = series(pwg, c, lengths, a.calls, a.warmup)
                print(json.dumps({f"pwg_{compute}.{name}": out[f"pwg_{compute}.{name}"]}), flush=True)
                del pwg
                torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("tools/hifigan_latency.py: HiFi-GAN generator, A = layer by layer (fused=False), B = fused (fused=True); ms per call\n")
        f.write(json.dumps({"hifigan_latency": out}, indent=1) + "\n")
    print(json.dumps({"hifigan_latency": out}))


if __name__ == "__main__":
    main()
