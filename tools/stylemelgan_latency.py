"""Latency of the StyleMelGAN generator (a3t_amd/vocoder.py::StyleMelGANGeneratorHIP) on the 24 kHz plan (64 channels, kernel 9,
noise scales 10 2 2 2, upsample scales 5 1 5 1 3 1 2 2 1) with procedural weights.  A report: no speed is promised.

  A  the torch restatement (tests/stylemelgan_ref.py) run as torch ops on the device in fp32: what a user of this package had
     before the class existed.  A dense batch is one batched forward, a ragged one a loop over the rows (the reference's
     inference takes one utterance).
  B  StyleMelGANGeneratorHIP.inference
  order A, B, A in one process; wall time of a call on a mel that is already on the device (the noise is drawn inside, in both),
  median / min / max over --calls after warm-up; for B also the HIP-event time of every TADEResBlock.
  workloads: 8 x 1000 frames, and the ragged lengths 1000 / 700 / 500 / 300 x 2 through lengths=.
  for scale, in the same process on the same workloads: MelGANGeneratorHIP (v2, fused), HiFiGANGeneratorHIP (v1, fused, f32) and
  ParallelWaveGANGeneratorHIP (v1, f32).

    timeout -k 10 900 python tools/stylemelgan_latency.py [--calls 50] [--warmup 3] [--frames 1000] [--out profiles/stylemelgan_latency.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hifigan_latency import series      # noqa: E402


class TorchStyleMelGAN:
    """The restatement on the device, with the interface `series` calls."""

    def __init__(self, state, cfg, R):
        self.R, self.cfg = R, cfg
        self.w = {k: v.cuda() for k, v in R.folded(state, torch.float32).items()}

    @torch.no_grad()
    def inference(self, c, lengths=None):
        R, cfg = self.R, self.cfg
        hop, Fn = R.hop_of(cfg), R.noise_factor(cfg)
        B, T, _ = c.shape
        if lengths is None:
            z = torch.randn(B, cfg["in_channels"], -(-T // Fn), device=c.device)
            return R._row(self.w, cfg, c.transpose(1, 2), z, None).transpose(1, 2)
        out = torch.zeros(B, T * hop, 1, device=c.device)
        for b, n in enumerate(lengths):
            z = torch.randn(1, cfg["in_channels"], -(-n // Fn), device=c.device)
            out[b, :n * hop, 0] = R._row(self.w, cfg, c[b:b + 1, :n].transpose(1, 2), z, None)[0, 0]
        return out


def block_times(gen, c, lengths, calls):
    """Median HIP-event ms of every TADEResBlock over `calls` calls."""
    marks, inner = [], type(gen)._block.__get__(gen)

    def run(blk, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = inner(blk, *a)
        e1.record()
        marks.append((e0, e1))
        return out

    gen._block = run
    try:
        for _ in range(calls):
            gen.inference(c, lengths=lengths)
        torch.cuda.synchronize()
    finally:
        del gen._block
    nb = len(gen.blocks)
    ms = [[marks[i * nb + k][0].elapsed_time(marks[i * nb + k][1]) for i in range(calls)] for k in range(nb)]
    return [round(statistics.median(v), 4) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stylemelgan_latency.txt"))
    ap.add_argument("--no-scale", action="store_true", help="leave out the MelGAN, HiFi-GAN and ParallelWaveGAN runs")
    a = ap.parse_args()
    import hifigan_ref as H
    import melgan_ref as M
    import stylemelgan_ref as R
    from a3t_amd.vocoder import HiFiGANGeneratorHIP, MelGANGeneratorHIP, ParallelWaveGANGeneratorHIP, StyleMelGANGeneratorHIP
    prop = torch.cuda.get_device_properties(0)
    out = {"device": f"{prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)",
           "plan": "StyleMelGAN 24 kHz: 64 channels, kernel 9, dilation 2, noise scales 10 2 2 2, upsample scales 5 1 5 1 3 1 2 2 1",
           "calls": a.calls}
    state = R.case_state("v1_wn")
    A, Bn = TorchStyleMelGAN(state, R.V1, R), StyleMelGANGeneratorHIP(state, device="cuda", **R.V1)
    F = a.frames
    sets = {f"8x{F}": (8, None), "ragged": (8, [F, F * 7 // 10, F // 2, F * 3 // 10] * 2)}
    for name, (B, lengths) in sets.items():
        c = torch.randn(B, F, 80, device="cuda")
        r = dict(lengths=lengths, A_first=series(A, c, lengths, a.calls, a.warmup), B=series(Bn, c, lengths, a.calls, a.warmup),
                 A_again=series(A, c, lengths, a.calls, a.warmup))
        r["B_over_A"] = round(r["B"]["median_ms"] / (0.5 * (r["A_first"]["median_ms"] + r["A_again"]["median_ms"])), 4)
        r["B_block_ms"] = block_times(Bn, c, lengths, min(a.calls, 10))
        r["valid_samples"] = (sum(lengths) if lengths else B * F) * Bn.hop
        out[name] = r
        print(json.dumps({name: r}), flush=True)
        torch.cuda.empty_cache()
        if not a.no_scale:
            from sedit_batch_latency import vocoder_state
            for tag, make in (("melgan_v2_fused", lambda: MelGANGeneratorHIP(M.procedural_melgan_state(M.V2, 51), device="cuda", **M.V2)),
                              ("hifigan_v1_fused_f32", lambda: HiFiGANGeneratorHIP(H.procedural_hifigan_state(H.V1, 41), device="cuda", **H.V1)),
                              ("pwg_v1_f32", lambda: ParallelWaveGANGeneratorHIP(vocoder_state(), device="cuda"))):
                gen = make()
                out[f"{tag}.{name}"] = series(gen, c, lengths, a.calls, a.warmup)
                print(json.dumps({f"{tag}.{name}": out[f"{tag}.{name}"]}), flush=True)
                del gen
                torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("tools/stylemelgan_latency.py: StyleMelGAN generator, A = torch restatement on the device, B = StyleMelGANGeneratorHIP; "
                "ms per call\n")
        f.write(json.dumps({"stylemelgan_latency": out}, indent=1) + "\n")
    print(json.dumps({"stylemelgan_latency": out}))


if __name__ == "__main__":
    main()
