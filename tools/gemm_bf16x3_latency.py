"""gemm_f32_kernel against gemm_bf16x3_kernel alone (compute = F32 / BF16X3 of a3t_gemm on the same fp32 operands), at the GEMM
shapes of the speech editor's forward for N = 8 requests x 1000 frames on model c2 (d = 384, 2 heads of 192, FFN 1536 with
k = 3, postnet 5 x k = 5 over 256 channels; T = 1176 tokens per row: 1000 frames + 176 phones):

  linear d x d          M = 8 T, N = 384, K = 384 (the attention output / pointwise projections)
  linear qkv            N = 1152
  ffn conv 1 / 2        implicit im2col, 3 taps: K = 3 x 384 -> 1536 with ReLU, K = 3 x 1536 -> 384 with the residual
  postnet 1 .. 5        M = 8000 frames, 5 taps: 80 -> 256, 256 -> 256 (x 3), 256 -> 80
  scores ac / bd        (q + u) k^T and (q + v) P^T per (request, head): M = N = T, K = 192, batch 16, the strides of the packed
                        qkv tensor and of the shared positional projection
  probs x V             M = T, N = 192, K = T, B = V [k][n] inside qkv

Per shape the two kernels alternate (f32, bf16x3, f32, bf16x3, ...), --repeats windows of --iters launches each over rotating
operand and output buffers, device events around a window; us per launch as median [min, max] over the windows, the ratio of the
medians, the share of the bf16 MFMA peak (2.5 PFLOP/s dense, 256 CUs) that 3 x 2 M N K flops in that time are, and the largest
difference of the two results relative to max |C|.

    python tools/gemm_bf16x3_latency.py [--repeats 3] [--iters 20] [--requests 8] [--frames 1000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from a3t_amd import _lib, ops  # noqa: E402
from a3t_amd._lib import ACT_RELU, BF16X3, F32  # noqa: E402

BF16_PEAK = 2.5e15
NB = 3          # rotating buffer sets


def shapes(B, frames):
    d, H, dk, ff, pc, od = 384, 2, 192, 1536, 256, 80
    T = (frames + 176 + 7) // 8 * 8
    M, Mp = B * T, B * frames
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s, scale=1.0: torch.randn(*s, device="cuda", generator=g) * scale

    def linear(name, M, N, K, **kw):
        xs, W, outs = [rn(M, K) for _ in range(NB)], rn(N, K, scale=K ** -0.5), [torch.empty(M, N, device="cuda") for _ in range(NB)]
        return name, 2.0 * M * N * K, outs, lambda i, c: ops.gemm(xs[i], W, outs[i], M, N, K, K, 1, K, 1, N, compute=c, **kw)

    def conv(name, M, Tseq, Cin, Cout, taps, **kw):
        K = taps * Cin
        xs, W, outs = [rn(M, Cin) for _ in range(NB)], rn(Cout, taps, Cin, scale=K ** -0.5), [torch.empty(M, Cout, device="cuda") for _ in range(NB)]
        if kw.pop("residual", False):
            kw["R"] = rn(M, Cout)
        return name, 2.0 * M * Cout * K, outs, lambda i, c: ops.conv_fwd(xs[i], W, outs[i], Tseq, (taps - 1) // 2, compute=c, **kw)

    out = [linear("linear d x d", M, d, d, bias=rn(d)), linear("linear qkv", M, 3 * d, d, bias=rn(3 * d)),
           conv("ffn conv 1", M, T, d, ff, 3, bias=rn(ff), act=ACT_RELU),
           conv("ffn conv 2", M, T, ff, d, 3, bias=rn(d), alpha=0.5, residual=True),
           conv("postnet 1 (80 -> 256)", Mp, frames, od, pc, 5), conv("postnet 2-4 (256 -> 256)", Mp, frames, pc, pc, 5),
           conv("postnet 5 (256 -> 80)", Mp, frames, pc, od, 5)]
    qkv = [rn(B * T, 3 * d) for _ in range(NB)]
    qu = [rn(B * T, d) for _ in range(NB)]
    P = rn(T, d)
    sc = [torch.empty(B, H, T, T, device="cuda") for _ in range(NB)]
    probs = [torch.softmax(rn(B, H, T, T), -1) for _ in range(NB)]
    ctx = [torch.empty(B * T, d, device="cuda") for _ in range(NB)]
    bh = dict(batch=B * H, batch_inner=H)
    out.append(("scores ac", 2.0 * B * H * T * T * dk, sc, lambda i, c: ops.gemm(
        qu[i], qkv[i].view(-1)[d:], sc[i], T, T, dk, d, 1, 3 * d, 1, T, a_bs=(T * d, dk), b_bs=(T * 3 * d, dk), c_bs=(H * T * T, T * T),
        compute=c, **bh)))
    out.append(("scores bd", 2.0 * B * H * T * T * dk, sc, lambda i, c: ops.gemm(
        qu[i], P, sc[i], T, T, dk, d, 1, d, 1, T, a_bs=(T * d, dk), b_bs=(0, dk), c_bs=(H * T * T, T * T), compute=c, **bh)))
    out.append(("probs x V", 2.0 * B * H * T * T * dk, ctx, lambda i, c: ops.gemm(
        probs[i], qkv[i].view(-1)[2 * d:], ctx[i], T, dk, T, T, 1, 1, 3 * d, d, a_bs=(H * T * T, T * T), b_bs=(T * 3 * d, dk),
        c_bs=(T * d, dk), compute=c, **bh)))
    return out


def window(fn, compute, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k % NB, compute)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1000)
    a = ap.parse_args()
    lib = _lib.load()
    prop = torch.cuda.get_device_properties(0)
    print(f"# {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs); {a.requests} x {a.frames} frames; "
          f"{a.repeats} alternating windows of {a.iters} launches; us per launch: median [min, max]")
    rows = []
    for name, flops, outs, fn in shapes(a.requests, a.frames):
        kern, res = {}, {}
        for c in (F32, BF16X3):                 # warm-up, the kernel each mode runs, and the two results
            for i in range(NB):
                fn(i, c)
            torch.cuda.synchronize()
            kern[c] = lib.a3t_gemm_last_kernel().decode()
            res[c] = outs[0].double().clone()
        diff = float((res[BF16X3] - res[F32]).abs().max()) / max(float(res[F32].abs().max()), 1e-30)
        del res
        ts = {F32: [], BF16X3: []}
        for _ in range(a.repeats):
            for c in (F32, BF16X3):
                ts[c].append(window(fn, c, a.iters))
        m32, m3 = float(np.median(ts[F32])), float(np.median(ts[BF16X3]))
        r = dict(shape=name, f32_kernel=kern[F32], x3_kernel=kern[BF16X3], f32_us=round(m32, 1), f32_min_max_us=[round(min(ts[F32]), 1), round(max(ts[F32]), 1)],
                 x3_us=round(m3, 1), x3_min_max_us=[round(min(ts[BF16X3]), 1), round(max(ts[BF16X3]), 1)], f32_over_x3=round(m32 / m3, 2),
                 ranges_overlap=not (max(ts[BF16X3]) < min(ts[F32]) or max(ts[F32]) < min(ts[BF16X3])),
                 x3_share_of_bf16_peak_3_products=round(3 * flops / (m3 * 1e-6) / BF16_PEAK, 4),
                 f32_tflops=round(flops / (m32 * 1e-6) / 1e12, 1), max_diff_of_max=float(f"{diff:.3e}"))
        rows.append(r)
        print(f"{name:26s} f32 {m32:8.1f} [{min(ts[F32]):8.1f}, {max(ts[F32]):8.1f}]  bf16x3 {m3:8.1f} [{min(ts[BF16X3]):8.1f}, {max(ts[BF16X3]):8.1f}]  "
              f"x{m32 / m3:5.2f}  {100 * r['x3_share_of_bf16_peak_3_products']:5.1f} % of bf16 peak  diff {diff:.2e}  [{kern[BF16X3]}]", flush=True)
    print(json.dumps({"gemm_bf16x3_latency": rows}))


if __name__ == "__main__":
    main()
