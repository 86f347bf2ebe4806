"""Latency of one duration_fn call of the native FastSpeech2 duration model (a3t_amd/duration.py): wall time of the
call including the host copy of the frames, median over repeated calls after warm-up, for a few phone counts.  The
model has the ljspeech conformer shape (d=384, 2 heads, ff 1536, 4 blocks, kernel 7, predictor 2 x 256) with
procedural weights.  Launch counts: run under `rocprofv3 --kernel-trace --stats -- python tools/duration_latency.py
--calls 1 --warmup 0` and divide the dispatch count by the number of calls (one per length).

    python tools/duration_latency.py [--phones 60 300] [--calls 50] [--warmup 5]

--batch N [N ...]: the batched path instead.  For every N, N distinct lists of 20-120 phones (seeded); wall time per list of
(A) a loop of N single calls and (B) one `.batch` call of the same lists, measured in the order A, B, A in one process,
median of --calls repetitions after --warmup.  The yardstick of B is A in the same run; the spread between the two A runs is
the noise a difference has to exceed.  Every N also checks that B returns what A returns.

    python tools/duration_latency.py --batch 1 2 8 16

Launches of ONE batched forward: --batch N --only B --calls K --warmup 0 makes exactly K `.batch` calls and nothing else after
the model is built, so the dispatch counts of two `rocprofv3 --kernel-trace --stats` runs with K = 1 and K = 2 differ by the
launches of one call (copies to the staging buffers and torch's own kernels included).

--speakers N [N ...]: one x-vector per list.  The model gets an x-vector projection (spk_embed_dim 512, "add"); for every N and
every phone count of --speaker-phones, N lists of that many phones from N different x-vectors; wall time per list of (A) a loop
of N single calls, one per speaker, each on a callable bound to its x-vector ahead of the timing (fn.with_speaker(x): what a
caller without speakers= has to do) and (B) one `.batch(lists, speakers=[...])` call, which computes the N speaker biases inside
the call.  Order A, B, A, median of --calls after --warmup, as above; --out appends the result lines to a file.

    python tools/duration_latency.py --speakers 1 8 --out profiles/fs2_speakers_latency.txt
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


def _timed(call, calls, warmup):
    """Wall times (s) of `calls` repetitions of call() after `warmup`; every call ends with its frames on the host."""
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return ts


def batch_latency(fn, phones, a, rs):
    out = {}
    for n in a.batch:
        lists, seen = [], set()
        while len(lists) < n:
            ph = tuple(phones[i] for i in rs.randint(0, len(phones), rs.randint(20, 121)))
            if ph not in seen:
                seen.add(ph)
                lists.append(list(ph))
        legs = {"A": lambda: [fn(x) for x in lists], "B": lambda: fn.batch(lists)}
        if a.only is not None:
            ts = _timed(legs[a.only], a.calls, a.warmup)
            out[n] = {a.only: dict(median_ms_per_list=round(1e3 * float(np.median(ts)) / n, 4), calls=a.calls)}
            continue
        same = legs["A"]() == legs["B"]()
        row = dict(phones=[len(x) for x in lists], same_result=bool(same))
        for name, leg in (("A1", "A"), ("B", "B"), ("A2", "A")):
            ts = _timed(legs[leg], a.calls, a.warmup)
            row[name] = dict(median_ms_per_list=round(1e3 * float(np.median(ts)) / n, 4),
                             min_ms_per_list=round(1e3 * float(np.min(ts)) / n, 4),
                             max_ms_per_list=round(1e3 * float(np.max(ts)) / n, 4))
        a1, a2, b = (row[k]["median_ms_per_list"] for k in ("A1", "A2", "B"))
        row["A_spread_ms"] = round(abs(a1 - a2), 4)
        row["B_over_A"] = round(b / (0.5 * (a1 + a2)), 4)
        row["faster_beyond_spread"] = bool(min(a1, a2) - b > abs(a1 - a2))
        row["calls"] = a.calls
        out[n] = row
    return out


def speakers_latency(fn, phones, a, rs):
    out = {}
    for n in a.speakers:
        for count in a.speaker_phones:
            lists = [[phones[i] for i in rs.randint(0, len(phones), count)] for _ in range(n)]
            xs = [(rs.standard_normal(512) * s).astype(np.float32) for s in np.linspace(0.3, 20.0, n)]
            bound = [fn.with_speaker(x) for x in xs]
            legs = {"A": lambda: [f(l) for f, l in zip(bound, lists)], "B": lambda: fn.batch(lists, speakers=xs)}
            row = dict(speakers=n, phones=count, same_result=bool(legs["A"]() == legs["B"]()))
            for name, leg in (("A1", "A"), ("B", "B"), ("A2", "A")):
                ts = _timed(legs[leg], a.calls, a.warmup)
                row[name] = dict(median_ms_per_list=round(1e3 * float(np.median(ts)) / n, 4),
                                 min_ms_per_list=round(1e3 * float(np.min(ts)) / n, 4),
                                 max_ms_per_list=round(1e3 * float(np.max(ts)) / n, 4))
            a1, a2, b = (row[k]["median_ms_per_list"] for k in ("A1", "A2", "B"))
            row["A_spread_ms"] = round(abs(a1 - a2), 4)
            row["B_over_A"] = round(b / (0.5 * (a1 + a2)), 4)
            row["B_call_over_one_single_call"] = round(b * n / (0.5 * (a1 + a2)), 4)
            row["faster_beyond_spread"] = bool(min(a1, a2) - b > abs(a1 - a2))
            row["calls"] = a.calls
            out[f"duration_speakers{n}_phones{count}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phones", type=int, nargs="+", default=[60, 300])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, nargs="+", default=None, help="batched path: numbers of lists per call")
    ap.add_argument("--only", choices=["A", "B"], default=None, help="with --batch: run one leg only (for kernel traces)")
    ap.add_argument("--speakers", type=int, nargs="+", default=None, help="one x-vector per list: numbers of lists per call")
    ap.add_argument("--speaker-phones", type=int, nargs="+", default=[30, 130], help="with --speakers: phones per list")
    ap.add_argument("--out", default=None, help="with --speakers: append the result lines to this file")
    a = ap.parse_args()
    from a3t_amd.duration import FS2DurationConfig, FS2DurationModel
    from oracle import a3t_oracle as O
    phones = ["AA1", "AE1", "AH0", "B", "D", "K", "L", "M", "N", "S", "T", "sp"]
    tl = ["<blank>", "<unk>"] + phones[:-1] + ["<sos/eos>"]
    conf = dict(adim=384, aheads=2, elayers=4, eunits=1536, positionwise_conv_kernel_size=3, encoder_type="conformer",
                conformer_enc_kernel_size=7, duration_predictor_chans=256)
    if a.speakers is not None:
        conf.update(spk_embed_dim=512, spk_embed_integration_type="add")
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
    if a.speakers is not None:
        res = speakers_latency(fn, phones, a, rs)
        print(json.dumps({"duration_speakers_latency": res}))
        if a.out:
            with open(a.out, "a") as f:
                for k, row in res.items():
                    f.write(f"{k}: {json.dumps(row)}\n")
        return
    if a.batch is not None:
        print(json.dumps({"duration_batch_latency": batch_latency(fn, phones, a, rs)}))
        return
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
