"""Latency of FastSpeech2 text-to-mel synthesis (a3t_amd/fs2_tts.py, csrc/fs2_tts.hip) next to the same computation as torch
ops on the same GPU: tests/fs2_tts_ref.py, the restatement the model is tested against, with its weights on the device.
The model is the fixture's `plain` (conformer encoder and decoder at d = 384, five postnet layers, procedural weights).

    python tools/fs2_tts_latency.py [--phones 30 130] [--batch 1 8] [--calls 50] [--warmup 5] [--out profiles/fs2_tts_latency.txt]

Per (phones, B): wall time of ONE synthesis of B lists of that many phones (+ eos), synchronised, in the order A (torch ops),
B (native), A in one process, median of --calls after --warmup; the spread between the two A runs is the noise a difference
has to exceed.  Both legs end with their result on the device; both read their frame counts on the host on the way (the
restatement sizes its padded batch with them, the native path its decoder buffers).

Launches: --only torch|native --calls K --warmup 0 runs exactly K syntheses of the first (phones, B) after the set-up, so the
dispatch counts of two `rocprofv3 --kernel-trace --stats` runs with K = 1 and K = 2 differ by the launches of one call.

--speakers N [N ...]: one x-vector per list, on the fixture's `xadd` model.  Per (phones, N): N lists of that many phones from N
different x-vectors; (A) a loop of N single syntheses, one per speaker (synthesize_ids_batch([list], x): what a caller without
speakers= has to do) against (B) one synthesize_ids_batch(lists, speakers=[...]) call; order A, B, A, median of --calls after
--warmup, ms per list.  --out appends the result lines to the file.

    python tools/fs2_tts_latency.py --speakers 1 8 --out profiles/fs2_speakers_latency.txt
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


def speakers_latency(a):
    import fs2_tts_ref as R
    from a3t_amd.fs2_tts import FS2TTSConfig, FS2TTSModel
    meta = R.meta()
    cfg, sd = R.checkpoint(meta, "xadd")
    m = FS2TTSModel(FS2TTSConfig.from_espnet(cfg), "cuda").load_state_dict({"tts." + k: v for k, v in sd.items()})
    vocab, dim = len(meta["token_list"]), cfg["tts_conf"]["spk_embed_dim"]
    rs = np.random.RandomState(0)
    out = {}
    for n in a.phones:
        for N in a.speakers:
            lists = [R.token_ids(n + 1, 50 + b, vocab).tolist() for b in range(N)]
            xs = [(rs.standard_normal(dim) * s).astype(np.float32) for s in np.linspace(0.3, 20.0, N)]
            legs = {"A": lambda: [m.synthesize_ids_batch([l], x)[0] for l, x in zip(lists, xs)],
                    "B": lambda: m.synthesize_ids_batch(lists, speakers=xs)}
            with torch.no_grad():
                one, got = legs["A"](), legs["B"]()
                same = all(torch.equal(o["duration"], g["duration"]) for o, g in zip(one, got))
                row = dict(speakers=N, phones=n, frames=[int(g["feat_gen"].shape[0]) for g in got], same_durations=bool(same))
                if same:
                    row["max_abs_diff"] = max(float((o["feat_gen"] - g["feat_gen"]).abs().max()) for o, g in zip(one, got))
                for name, leg in (("A1", "A"), ("B", "B"), ("A2", "A")):
                    ts = _timed(legs[leg], a.calls, a.warmup)
                    row[name] = {k: round(v / N, 4) for k, v in _ms(ts).items()}       # ms per list
            a1, a2, b = (row[k]["median_ms"] for k in ("A1", "A2", "B"))
            row["A_spread_ms"] = round(abs(a1 - a2), 4)
            row["B_over_A"] = round(b / (0.5 * (a1 + a2)), 4)
            row["B_call_over_one_single_call"] = round(b * N / (0.5 * (a1 + a2)), 4)
            row["faster_beyond_spread"] = bool(min(a1, a2) - b > abs(a1 - a2))
            row["calls"] = a.calls
            out[f"synthesis_speakers{N}_phones{n}"] = row
    print(json.dumps({"fs2_tts_speakers_latency": out}))
    if a.out:
        with open(a.out, "a") as f:
            for k, row in out.items():
                f.write(f"{k}: {json.dumps(row)}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phones", type=int, nargs="+", default=[30, 130])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["torch", "native"], default=None, help="one leg of the first shape only (kernel traces)")
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--speakers", type=int, nargs="+", default=None, help="one x-vector per list: numbers of lists per call")
    a = ap.parse_args()
    if a.speakers is not None:
        return speakers_latency(a)
    import fs2_tts_ref as R
    from a3t_amd.fs2_tts import FS2TTSConfig, FS2TTSModel
    meta = R.meta()
    cfg, sd = R.checkpoint(meta, "plain")
    m = FS2TTSModel(FS2TTSConfig.from_espnet(cfg), "cuda").load_state_dict({"tts." + k: v for k, v in sd.items()})
    dsd = {k: v.cuda() for k, v in sd.items()}
    conf, vocab = cfg["tts_conf"], len(meta["token_list"])
    out = {}
    for n in a.phones:
        for B in a.batch:
            lists = [R.token_ids(n + 1 - (b % 3), 50 + b, vocab).tolist() for b in range(B)]      # lengths n+1, n, n-1, ...
            lens = [len(x) for x in lists]
            ids = torch.zeros(B, max(lens), dtype=torch.int64)
            for b, x in enumerate(lists):
                ids[b, :lens[b]] = torch.tensor(x)
            ids = ids.cuda()
            legs = {"torch": lambda: R.synthesize(dsd, conf, ids, lens)["feat_gen"],
                    "native": lambda: m.synthesize_ids_batch(lists)}
            if a.only is not None:
                with torch.no_grad():
                    _timed(legs[a.only], a.calls, a.warmup)
                print(json.dumps({"fs2_tts_trace": dict(leg=a.only, phones=n, B=B, calls=a.calls)}))
                return
            with torch.no_grad():
                want, got = legs["torch"](), legs["native"]()
                frames = [int(o["feat_gen"].shape[0]) for o in got]
                row = dict(frames=frames, max_abs_diff=max(float((want[b, :frames[b]] - got[b]["feat_gen"]).abs().max())
                                                           for b in range(B)))
                for name, leg in (("A1", "torch"), ("B", "native"), ("A2", "torch")):
                    row[name] = _ms(_timed(legs[leg], a.calls, a.warmup))
            a1, a2, b = (row[k]["median_ms"] for k in ("A1", "A2", "B"))
            row["A_spread_ms"] = round(abs(a1 - a2), 4)
            row["B_over_A"] = round(b / (0.5 * (a1 + a2)), 4)
            row["faster_beyond_spread"] = bool(min(a1, a2) - b > abs(a1 - a2))
            row["calls"] = a.calls
            out[f"phones{n}_B{B}"] = row
    line = json.dumps({"fs2_tts_latency": out})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            for k, row in out.items():
                f.write(f"{k}: {json.dumps(row)}\n")


if __name__ == "__main__":
    main()
