"""Latency of one duration_fn call of the native FastSpeech2 duration model (a3t_amd/duration.py): wall time of the
call including the host copy of the frames, median over repeated calls after warm-up, for a few phone counts.  The
model has the ljspeech conformer shape (d=384, 2 heads, ff 1536, 4 blocks, kernel 7, predictor 2 x 256) with
procedural weights.  Launch counts: run under `rocprofv3 --kernel-trace --stats -- python tools/duration_latency.py
--calls 1 --warmup 0` and divide the dispatch count by the number of calls (one per length).

    python tools/duration_latency.py [--phones 60 300] [--calls 50] [--warmup 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phones", type=int, nargs="+", default=[60, 300])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    from oracle import a3t_oracle as O
    phones = ["AA1", "AE1", "AH0", "B", "D", "K", "L", "M", "N", "S", "T", "sp"]
    tl = ["<blank>", "<unk>"] + phones[:-1] + ["<sos/eos>"]
    conf = dict(adim=384, aheads=2, elayers=4, eunits=1536, positionwise_conv_kernel_size=3, encoder_type="conformer",
                conformer_enc_kernel_size=7, duration_predictor_chans=256)
    c = FS2DurationConfig.from_espnet({"tts": "fastspeech2", "tts_conf": conf, "token_list": tl})
    m = FS2DurationModel(c, "cuda")
    shapes = {k: tuple(int(x) for x in np.atleast_1d(np.array(v.shape))) for k, v in m.store.p.items()}
    # procedural weights straight into the store (layout names; the key map is exercised by the tests)
    for k, v in O.procedural_state(shapes, 3).items():
        m.store.p[k].copy_(torch.from_numpy(np.array(v)).reshape(m.store.p[k].shape))
    for k in m.store.buf:
        if k.endswith(".rv"):
            m.store.buf[k].fill_(1.0)
    fn = m.duration_fn(24000, 300)
    rs = np.random.RandomState(0)
    out = {}
    for n in a.phones:
        phns = [phones[i] for i in rs.randint(0, len(phones), n)]
        for _ in range(a.warmup):
            fn(phns)
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn(phns)
            ts.append(time.perf_counter() - t0)
        out[n] = dict(median_ms=round(1e3 * float(np.median(ts)), 3), min_ms=round(1e3 * float(np.min(ts)), 3),
                      calls=a.calls)
    print(json.dumps({"duration_fn_latency": out}))


if __name__ == "__main__":
    main()
