"""Latency of the multi-band MelGAN generator (a3t_amd/vocoder.py::MelGANGeneratorHIP), layer by layer against fused, on the
24 kHz v2 plan (384 channels, scales 5 5 3, 4 stacks, 4 sub-bands, PQMF 62 taps) with procedural weights.  A report: no speed is
promised; the faster of the two modes is the class's default.

  A  fused=False: a3t_leaky_relu + a3t_reflect_pad_rows + the exact-fp32 GEMM for every convolution, a3t_pqmf_synthesis
  B  fused=True:  every ResidualStack on a3t_mgan_stack, the output convolution on a3t_mgan_out, a3t_pqmf_synthesis
  order A, B, A in one process; wall time of inference() on a mel that is already on the device, median / min / max over
  --calls after warm-up.
  workloads: 8 x 1000 frames, and the ragged lengths 1000 / 700 / 500 / 300 x 2 through lengths=.
  for scale, in the same process on the same workloads: HiFiGANGeneratorHIP (v1 plan, fused, f32) and
  ParallelWaveGANGeneratorHIP (v1, f32).

    timeout -k 10 900 python tools/melgan_latency.py [--calls 50] [--warmup 3] [--frames 1000] [--out profiles/melgan_latency.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hifigan_latency import series      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melgan_latency.txt"))
    ap.add_argument("--no-scale", action="store_true", help="leave out the HiFi-GAN and ParallelWaveGAN runs")
    a = ap.parse_args()
    import hifigan_ref as H
    import melgan_ref as R
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, MelGANGeneratorHIP, ParallelWaveGANGeneratorHIP
    prop = torch.cuda.get_device_properties(0)
    out = {"device": f"{prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)",
           "plan": "multi-band MelGAN v2: 384 channels, scales 5 5 3, 4 stacks (dilations 1 3 9 27), 4 sub-bands, PQMF 62 taps",
           "calls": a.calls}
    state = R.procedural_melgan_state(R.V2, 51)
    gens = {f: MelGANGeneratorHIP(state, device="cuda", fused=f, **R.V2) for f in (False, True)}
    F = a.frames
    sets = {f"8x{F}": (8, None), "ragged": (8, [F, F * 7 // 10, F // 2, F * 3 // 10] * 2)}
    for name, (B, lengths) in sets.items():
        c = torch.randn(B, F, 80, device="cuda")
        r = dict(lengths=lengths, A_first=series(gens[False], c, lengths, a.calls, a.warmup),
                 B=series(gens[True], c, lengths, a.calls, a.warmup), A_again=series(gens[False], c, lengths, a.calls, a.warmup))
        r["B_over_A"] = round(r["B"]["median_ms"] / (0.5 * (r["A_first"]["median_ms"] + r["A_again"]["median_ms"])), 4)
        r["valid_samples"] = (sum(lengths) if lengths else B * F) * gens[True].upsample_factor
        out[name] = r
        print(json.dumps({name: r}), flush=True)
        if not a.no_scale:
            from sedit_batch_latency import vocoder_state
            for tag, make in (("hifigan_v1_fused_f32", lambda: HiFiGANGeneratorHIP(H.procedural_hifigan_state(H.V1, 41), device="cuda", **H.V1)),
                              ("pwg_v1_f32", lambda: ParallelWaveGANGeneratorHIP(vocoder_state(), device="cuda"))):
                gen = make()
                out[f"{tag}.{name}"] = series(gen, c, lengths, a.calls, a.warmup)
                print(json.dumps({f"{tag}.{name}": out[f"{tag}.{name}"]}), flush=True)
                del gen
                torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("tools/melgan_latency.py: multi-band MelGAN generator, A = layer by layer (fused=False), B = fused (fused=True); "
                "ms per call\n")
        f.write(json.dumps({"melgan_latency": out}, indent=1) + "\n")
    print(json.dumps({"melgan_latency": out}))


if __name__ == "__main__":
    main()
