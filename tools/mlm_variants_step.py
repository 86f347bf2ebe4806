"""bf16 training-step time of the model variants at the size of BASELINE configs[1] (B = 32, T_mel = 1000, T_phn = 120, d = 384,
recipe dropout; the step of bench.py: forward + loss + backward + clip + Adam on one GPU):

  A  default      6 encoder + 6 decoder blocks                         (the headline workload)
  B  no_decoder   12 encoder blocks, decoder: no_decoder               ("one flag away" from configs[1])
  C  pre_speech   2 pre-speech + 4 encoder + 6 decoder blocks          (pre_speech_layer: 2; the pre blocks run at T = 1000)

Protocol of the other tools: every model is warmed up, then the median wall time of --steps steps (events around each step) is
taken in the order A, B, C, A; the spread of the two A runs stands next to the results as the noise of the measurement.

    python tools/mlm_variants_step.py [--steps 50] [--warmup 5] [--out profiles/mlm_variants_step.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def models():
    from a3t_amd.config import A3TConfig
    return [("A default 6+6", A3TConfig(enc_blocks=6, dec_blocks=6)),
            ("B 12 + no_decoder", A3TConfig(enc_blocks=12, dec_blocks=0, has_decoder=False)),
            ("C 2 pre + 4 + 6", A3TConfig(pre_blocks=2, enc_blocks=4, dec_blocks=6)),
            ("A default 6+6 (again)", A3TConfig(enc_blocks=6, dec_blocks=6))]


def measure(cfg, B, Tm, Tp, steps, warmup):
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    from a3t_amd.trainer import A3TTrainer
    store = ParamStore(cfg, "cuda")
    xavier_init_(store, seed=0, bn_gamma=1.0)
    tr = A3TTrainer(cfg, store, compute="bf16", lr=1.0, warmup_steps=4000, grad_clip=1.0, dropout=True)
    batch = synthetic_batch(cfg, B, Tm, Tp, seed=1234, device="cuda")
    for _ in range(warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = tr.step(batch)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    paths = dict(tr.engine.attn_path)
    res = dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3), loss=float(loss),
               params=int(store.n_params), attn_path=sorted(set(paths.values())))
    del tr, store, batch
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, nargs=3, default=[32, 1000, 120], metavar=("B", "T_MEL", "T_PHN"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlm_variants_step.txt"))
    a = ap.parse_args()
    B, Tm, Tp = a.batch
    rows = [(name, measure(cfg, B, Tm, Tp, a.steps, a.warmup)) for name, cfg in models()]
    a0, a1 = rows[0][1]["median_ms"], rows[-1][1]["median_ms"]
    spread = abs(a0 - a1)
    base = 0.5 * (a0 + a1)
    lines = [f"bf16 training step, B = {B}, T_mel = {Tm}, T_phn = {Tp}, d = 384, recipe dropout; median of {a.steps} steps after "
             f"{a.warmup} warm-up steps, order A, B, C, A ({torch.cuda.get_device_name(0)})", ""]
    for name, r in rows:
        lines.append(f"  {name:24s} {r['median_ms']:8.3f} ms  (min {r['min_ms']:.3f})  {r['median_ms'] - base:+7.3f} ms against A   "
                     f"{r['params']:>10d} parameters   attention forward: {','.join(r['attn_path'])}")
    lines += ["", f"  spread of the two A runs: {spread:.3f} ms ({100 * spread / base:.2f} % of {base:.3f} ms)"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    print(json.dumps({"mlm_variants_step": {n: r for n, r in rows}, "a_spread_ms": round(spread, 3)}))


if __name__ == "__main__":
    main()
