"""Measurements of the transformer MLM model (`encoder: transformer`), written to profiles/mlm_transformer_step.txt:

  kernel  the band-free fused attention forward (a3t_attn_fwd_plain / a3t_attn_fwd_train_plain) against the existing kernel fed
          qu = qv = q and an all-zero positional table, at (B, H, T, d_k) = (32, 2, 1120, 192), attention dropout 0.2: forward only
          and training (sign-tagged save), in the order A (zero table), B (band-free), A; median of --reps launches each.  The spread
          of the two A runs is the noise of the measurement.
  step    the bf16 training step (forward + loss + backward + clip + Adam, recipe dropout) of a 6 + 6 transformer model at the size of
          BASELINE configs[1] (B = 32, T_mel = 1000, T_phn = 120, d = 384, 2 heads, conv1d FFN k = 3) next to the default conformer
          step, in the same process, order conformer, transformer, conformer; ms and library calls per step (every ops.* call is one
          entry point of liba3t_hip, most of them one launch).

    python tools/mlm_transformer_step.py [--reps 50] [--steps 20] [--warmup 5] [--out profiles/mlm_transformer_step.txt]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


def kernel_ab(reps, B=32, H=2, T=1120, dk=192, drop=(0.2, 12345)):
    from a3t_amd import ops
    d = H * dk
    gen = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * T, 3 * d, generator=gen).to("cuda").bfloat16()
    q = qkv[:, :d].contiguous()
    Z = torch.zeros(T, d, device="cuda", dtype=torch.bfloat16)
    km = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    ctx = torch.empty(B * T, d, device="cuda", dtype=torch.bfloat16)
    lse, rs = torch.empty(B, H, T, device="cuda"), torch.empty(B, H, T, device="cuda")
    probs = torch.empty(B, H, T, T, device="cuda", dtype=torch.bfloat16)
    sc = 1.0 / math.sqrt(dk)
    legs = {
        "forward only": (lambda: ops.attn_fwd(q, q, qkv, Z, km, ctx, lse, B, H, T, sc, drop=drop),
                         lambda: ops.attn_fwd_plain(qkv, km, ctx, lse, B, H, T, sc, drop=drop)),
        "training": (lambda: ops.attn_fwd_train(q, q, qkv, Z, km, ctx, lse, probs, None, rs, B, H, T, sc, drop=drop),
                     lambda: ops.attn_fwd_train_plain(qkv, km, ctx, lse, probs, None, rs, B, H, T, sc, drop=drop)),
    }
    out = {}
    for name, (zero_table, band_free) in legs.items():
        a1, b, a2 = _median_ms(zero_table, reps), _median_ms(band_free, reps), _median_ms(zero_table, reps)
        out[name] = dict(zero_table_ms=[a1, a2], band_free_ms=b, spread_ms=round(abs(a1 - a2), 4),
                         gain_ms=round(min(a1, a2) - b, 4))
    return out


def step(cfg, steps, warmup, B=32, Tm=1000, Tp=120):
    from a3t_amd import _lib
    from a3t_amd.collate import synthetic_batch
    from a3t_amd.init import xavier_init_
    from a3t_amd.params import ParamStore
    from a3t_amd.trainer import A3TTrainer
    store = ParamStore(cfg, "cuda")
    xavier_init_(store, seed=0, bn_gamma=1.0)
    tr = A3TTrainer(cfg, store, compute="bf16", lr=1.0, warmup_steps=4000, grad_clip=1.0, dropout=True)
    batch = synthetic_batch(cfg, B, Tm, Tp, seed=1234, device="cuda")
    ms = _median_ms(lambda: tr.step(batch), steps, warmup)
    calls, orig = [0], _lib.check

    def counting(rc, what=""):
        calls[0] += 1
        return orig(rc, what)
    _lib.check = counting
    try:
        loss = float(tr.step(batch))
    finally:
        _lib.check = orig
    res = dict(median_ms=ms, library_calls_per_step=calls[0], loss=loss, params=int(store.n_params),
               attn_path=sorted(set(tr.engine.attn_path.values())))
    del tr, store, batch
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlm_transformer_step.txt"))
    a = ap.parse_args()
    from a3t_amd.config import A3TConfig
    res = dict(device=torch.cuda.get_device_name(0), kernel=kernel_ab(a.reps))
    conf = A3TConfig(enc_blocks=6, dec_blocks=6)
    trans = A3TConfig(enc_blocks=6, dec_blocks=6, block="transformer")
    res["step"] = [("conformer 6+6", step(conf, a.steps, a.warmup)), ("transformer 6+6", step(trans, a.steps, a.warmup)),
                   ("conformer 6+6 (again)", step(conf, a.steps, a.warmup))]
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as fh:
        fh.write(__doc__.split("\n\n    python")[0] + "\n\n" + text + "\n")


if __name__ == "__main__":
    main()
