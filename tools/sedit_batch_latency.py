"""Latency of batched speech editing (a3t_amd/sedit.py: SpeechEditor.edit_batch) against a loop of single edits, and of the
ragged ParallelWaveGAN blocks against the padded ones.  Synthetic requests: utterances of --frames-range mel frames, a run of
words in the middle replaced so that the new span has roughly 40 to 200 frames; model `c2` (BASELINE configs[1]: 6 + 6
blocks, d = 384) or `tiny`, procedural weights, PWG v1 vocoder with random noise.  The duration model is a host-side stand-in
(a table look-up), NOT the FastSpeech2 model of duration.py: its leg shows how often and where it is called, not what that
model would cost.

  A       loop of SpeechEditor.edit over the N requests (the single-request path)
  B full  edit_batch(requests): one collate, one infill, one ragged vocoder call over whole utterances
  B span  edit_batch(requests, outputs=("orgin_replaced",)): the vocoder sees span +- margin_frames only
  order A, B full, B span, A again; wall time of the whole call (final copy included), median over --calls after warm-up,
  reported per request.  `legs`: the stages of B run one by one with a synchronisation after each (their sum exceeds the
  whole call, where host and device overlap).

  kernel  the 30 residual blocks alone, B x T frames: a3t_pwg_block, a3t_pwg_block_ragged with all lengths equal (the tile
          list's cost), and ragged lengths (expected near valid / padded samples of the padded run)

  --vocoder-compute f32 f16: the request legs are run once per vocoder compute mode (keys `<model>.<compute>.n<N>` for f32,
          `<model>.<compute>.voc_f16.n<N>` for f16), and --kernel adds `pwg_blocks_f16`: the 30 blocks through a3t_pwg_block_f16
          (one launch per block, x ping-ponging between two buffers) next to the fp32 pair of launches, order f32, f16, f32,
          median of --calls, on the padded 8 x 1000 frames and on the ragged lengths, with the bytes per second the f16 blocks
          reach against their HBM model (x read and written, cu16 read, skips read and written: 1184 B per sample and block).

  --rows batch alone: the rows="alone" path of edit_batch (every row computed as the request alone, fp32 compute only) next to
          the default, keys `<model>.f32.rows.n<N>`: order A, B = edit_batch(requests), C = edit_batch(requests, rows="alone"),
          A again, full and span-only vocoding; the stages of B and of C one by one; and per request the largest distance of
          B's and of C's mel to A's (the request edited alone), relative to the scale max(1, max |mel|), and of the collated
          log-mels.  --compute is not read for these legs.

  --spans: two separate edits in one pass (MultiSpanEditRequest.max_spans), keys `<model>.<compute>.spans.n<N>`.  Every request changes
          two words with three kept words (>= 40 frames) between them, the new words from a dictionary of the tool's own so that
          the word diff has exactly these two runs.  A = edit_batch with max_spans=1 (one span over the hull: the kept words are
          regenerated), B = edit_batch with max_spans=2, C = two sequential passes, one word each (the second pass edits the
          first one's "orgin_replaced"; its transcript and alignment are prepared ahead, outside the timing: an aligner run on
          the intermediate audio is not counted).  Order A, B, C, A, full and span-only vocoding, median of --calls, ms per
          request, and the frames the vocoder was given per request.  `kept_mel_B_to_A`: over the kept middle words B returns
          the recording's mel and A the model's output -- max and RMS of the difference relative to max(1, max |mel|), frame by
          frame from the start of the kept run over the shorter of the two runs.

  --ab R: the compute modes of --compute against each other on one set of requests, keys `<model>.ab.n<N>`: one editor per mode,
          and R times over, mode after mode (f32, bf16x3, bf16, f32, ...): the loop of `edit`, edit_batch(requests) and -- with
          --rows alone, on the modes that have it (f32, bf16x3) -- edit_batch(requests, rows="alone"), each the median of --calls
          calls.  Per mode and leg ms per request as median [min, max] over the R rounds, for every other mode whether its range
          lies clear of f32's, and the distance of its edit_batch mel from the f32 editor's (RMS and worst element over all
          requests, relative to max(1, max |mel|)).

    python tools/sedit_batch_latency.py [--models c2] [--compute bf16 f32 bf16x3] [--n 1 4 8] [--calls 50] [--warmup 5] [--kernel]
                                        [--vocoder-compute f32 f16] [--rows batch alone] [--spans] [--ab 3]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dyneval_latency import LEX, phonemise, prompt  # noqa: E402


def request(frames, k, oc, seed):
    """A `frames`-frame utterance of three-phone words with k words in the middle replaced by k other words."""
    from a3t_amd.sedit import EditRequest
    words = max(k + 4, frames // 17)
    wav, times2, w2p, old_str, _ = prompt(words, frames, oc.fs, oc.hop_length, seed=seed)
    old = old_str.split()
    names = sorted(n.lower() for n in LEX)
    i = (words - k) // 2
    new = old[:i] + [names[(names.index(w) + 1) % len(names)] for w in old[i:i + k]] + old[i + k:]
    new_str = " ".join(new)
    new_phns, new_w2p = phonemise(new_str)
    return EditRequest(wav, times2, w2p, new_phns, new_w2p, old_str, new_str)


def vocoder_state():
    """PWG v1 with procedural weights; the smoothing kernels of the upsampling network normalised like trained ones."""
    from oracle import a3t_oracle as O
    state = O.procedural_state(O.pwg_param_shapes(O.PWGConfig()), seed=4)
    for k in state:
        if "up_layers" in k:
            state[k] = np.abs(state[k]) / np.abs(state[k]).sum()
    return state


def editor(which, compute, vocoder_compute="f32"):
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP
    from dyneval_latency import editor as base
    ed, oc = base(which, compute)
    kw = {} if vocoder_compute == "f32" else dict(compute=vocoder_compute)
    ed.vocoder = ParallelWaveGANGeneratorHIP(vocoder_state(), device="cuda", **kw)
    return ed, oc


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def legs(ed, reqs, span_only, calls, warmup, rows="batch"):
    """The stages of edit_batch one by one, a synchronisation after each; ms per request."""
    from a3t_amd.sedit import plan_batch
    from a3t_amd.vocoder import span_window
    acc = {k: [] for k in ("plan", "duration_model", "collate", "infill", "vocoder", "splice_copy")}
    B, hop = len(reqs), ed.hop
    alone = {"rows": rows} if rows != "batch" else {}
    for it in range(warmup + calls):
        t_dur = [0.0]

        def dur(phns):
            t0 = time.perf_counter()
            out = ed.duration_fn(phns)
            t_dur[0] += time.perf_counter() - t0
            return out

        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())

        plans, data = plan_batch(reqs, ed.fs, hop, dur, ed.token_id_fn)
        lap()
        feats = ed.collate_fn(data, **alone)[1]
        flen = [int(n) for n in feats["speech_mask"].reshape(B, -1).sum(-1).tolist()]
        feats = {k: v.to("cuda") for k, v in feats.items() if k not in ("span_boundary", "speech_lengths", "text_lengths")}
        lap()
        with torch.no_grad():
            mel, _ = ed.model.inference_batch(**feats, span_boundary=[p.new_span_boundary for p in plans], **alone)
        lap()
        if span_only:
            m = ed.vocoder.margin_frames
            win = [span_window(*p.new_span_boundary, flen[b], m) for b, p in enumerate(plans)]
            c = mel.new_zeros(B, max(w1 - w0 for w0, w1 in win), mel.shape[2])
            for b, (w0, w1) in enumerate(win):
                c[b, :w1 - w0] = mel[b, w0:w1]
        else:
            win, c = [(0, n) for n in flen], mel
        wav = ed.vocoder.inference(c, lengths=[w1 - w0 for w0, w1 in win])
        lap()
        wav = wav.reshape(B, -1).cpu().numpy()
        for b, (p, r, (w0, w1)) in enumerate(zip(plans, reqs, win)):
            n0, n1 = p.new_span_boundary
            o0, o1 = p.old_span_boundary
            np.concatenate([r.wav_org[:hop * o0], wav[b, hop * (n0 - w0):hop * (n1 - w0)], r.wav_org[hop * o1:]])
        lap()
        if it >= warmup:
            d = np.diff(t)
            for k, v in zip(("plan", "collate", "infill", "vocoder", "splice_copy"), d):
                acc[k].append(v - (t_dur[0] if k == "plan" else 0.0))
            acc["duration_model"].append(t_dur[0])
    return {k: round(1e3 * float(np.median(v)) / B, 3) for k, v in acc.items()}


def kernel_bench(frames, lengths_sets, reps=5):
    """30 fused residual blocks on B x frames x hop samples: padded, ragged with equal lengths, ragged lengths; ms."""
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP, pwg_tile_list
    gen = ParallelWaveGANGeneratorHIP(vocoder_state(), device="cuda")
    hop, out = gen.upsample_factor, {}
    for name, lengths in lengths_sets.items():
        B, Tw = len(lengths), frames * hop
        # activations of the size the generator sees (first conv of unit noise, log-mel-like aux): x and skips start afresh in
        # every run and the result is checked to be finite, so the gate's exp / rcp work on ordinary numbers
        x0 = 0.1 * torch.randn(B * Tw, 64, device="cuda")
        cu = 1.5 * torch.randn(B * Tw, 80, device="cuda") - 4.0
        scratch = gen._scratch(B * Tw)
        tiles = torch.from_numpy(pwg_tile_list(lengths, hop)).to("cuda")
        equal = all(n == frames for n in lengths)

        def run(ragged):
            x, sk = x0.clone(), torch.zeros(B * Tw, 64, device="cuda")
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gen._blocks(x, cu, sk, B, Tw, tiles=tiles if ragged else None, scratch=scratch)
            b.record()
            torch.cuda.synchronize()
            fin.append(bool(torch.isfinite(x).all()) and bool(torch.isfinite(sk).all()))
            return a.elapsed_time(b)

        fin = []
        run(False), run(True)
        seq = ["padded", "ragged", "padded", "ragged", "padded"]          # padded first, between and last: its own spread
        ts = {k: [] for k in ("padded", "ragged")}
        for _ in range(reps):
            for k in seq:
                ts[k].append(run(k == "ragged"))
        out[name] = dict(lengths=list(lengths), padded_ms=round(float(np.median(ts["padded"])), 3),
                         padded_min_max_ms=[round(min(ts["padded"]), 3), round(max(ts["padded"]), 3)],
                         ragged_ms=round(float(np.median(ts["ragged"])), 3),
                         ragged_min_max_ms=[round(min(ts["ragged"]), 3), round(max(ts["ragged"]), 3)],
                         valid_over_padded=round(sum(lengths) / (B * frames), 3), all_equal=equal, finite=all(fin))
    return out


F16_BLOCK_BYTES = 64 * 4 + 64 * 4 + 80 * 2 + 2 * 64 * 4      # per sample and block: x in, x out, cu16, skips read + write


def kernel_bench_f16(frames, lengths_sets, calls=50, warmup=3):
    """The 30 residual blocks in fp32 (two launches per block) and on the 16-bit MFMA (one launch per block), B x frames x hop
    samples: `8x1000`-like sets (all lengths equal) run the padded entry points, the others the tile list; order f32, f16, f32,
    median / min / max of `calls` runs each, ms."""
    from a3t_amd import ops
    from a3t_amd.vocoder import ParallelWaveGANGeneratorHIP, pwg_tile_list
    gen = ParallelWaveGANGeneratorHIP(vocoder_state(), device="cuda", compute="f16")
    gen32 = ParallelWaveGANGeneratorHIP(vocoder_state(), device="cuda")
    hop, out = gen.upsample_factor, {}
    for name, lengths in lengths_sets.items():
        B, Tw = len(lengths), frames * hop
        x0 = 0.1 * torch.randn(B * Tw, 64, device="cuda")
        cu = 1.5 * torch.randn(B * Tw, 80, device="cuda") - 4.0
        cu16 = torch.empty(B * Tw, 80, dtype=torch.float16, device="cuda")
        ops.cast_f16_sat(cu, cu16)
        scratch32 = gen32._scratch(B * Tw)
        equal = all(n == frames for n in lengths)
        tiles = None if equal else torch.from_numpy(pwg_tile_list(lengths, hop)).to("cuda")
        fin = []

        def run(f16):
            x, sk = x0.clone(), torch.zeros(B * Tw, 64, device="cuda")
            scratch16 = gen._scratch(B * Tw)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if f16:
                gen._blocks(x, cu16, sk, B, Tw, tiles=tiles, scratch=scratch16)
            else:
                gen32._blocks(x, cu, sk, B, Tw, tiles=tiles, scratch=scratch32)
            b.record()
            torch.cuda.synchronize()
            fin.append(bool(torch.isfinite(sk).all()))
            return a.elapsed_time(b)

        def series(f16):
            for _ in range(warmup):
                run(f16)
            ts = [run(f16) for _ in range(calls)]
            return dict(median_ms=round(float(np.median(ts)), 3), min_max_ms=[round(min(ts), 3), round(max(ts), 3)])

        r = dict(lengths=list(lengths), f32_first=series(False), f16=series(True), f32_again=series(False))
        f32 = 0.5 * (r["f32_first"]["median_ms"] + r["f32_again"]["median_ms"])
        valid = sum(lengths) * hop
        r["f16_over_f32"] = round(r["f16"]["median_ms"] / f32, 4)
        r["f16_bytes_per_s_model"] = round(valid * len(gen.blocks) * F16_BLOCK_BYTES / (1e-3 * r["f16"]["median_ms"]), 0)
        r["valid_samples"], r["finite"] = valid, all(fin)
        out[name] = r
    return out


def _of_scale(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max())) if ref.numel() else 0.0


def rows_alone_legs(ed, oc, reqs, calls, warmup):
    """A, B, C, A (module docstring, --rows) on one set of requests, fp32 compute; ms per request and mel distances."""
    from a3t_amd.sedit import plan_batch
    n = len(reqs)
    args = [(r.wav_org, r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str) for r in reqs]
    span = ("orgin_replaced",)

    def loop():
        for x in args:
            ed.edit(*x)

    r = {"A_loop_of_edit_ms": round(timed(loop, calls, warmup) / n, 3),
         "B_full_ms": round(timed(lambda: ed.edit_batch(reqs), calls, warmup) / n, 3),
         "B_span_only_ms": round(timed(lambda: ed.edit_batch(reqs, outputs=span), calls, warmup) / n, 3),
         "C_full_ms": round(timed(lambda: ed.edit_batch(reqs, rows="alone"), calls, warmup) / n, 3),
         "C_span_only_ms": round(timed(lambda: ed.edit_batch(reqs, outputs=span, rows="alone"), calls, warmup) / n, 3),
         "A_again_ms": round(timed(loop, calls, warmup) / n, 3)}
    ed.vocoder, voc = None, ed.vocoder
    one = [ed.edit(*x)["feat"] for x in args]
    got_b, got_c = ed.edit_batch(reqs), ed.edit_batch(reqs, rows="alone")
    ed.vocoder = voc
    r["frames"] = [int(f.shape[0]) for f in one]
    r["span_frames"] = [int(g["new_span_boundary"][1] - g["new_span_boundary"][0]) for g in got_b]
    r["mel_B_to_A_of_scale"] = [float(f"{_of_scale(g['feat'], f):.3e}") for g, f in zip(got_b, one)]
    r["mel_C_to_A_of_scale"] = [float(f"{_of_scale(g['feat'], f):.3e}") for g, f in zip(got_c, one)]
    data = plan_batch(reqs, ed.fs, ed.hop, ed.duration_fn, ed.token_id_fn)[1]
    fb, fc = ed.collate_fn(data)[1]["speech"], ed.collate_fn(data, rows="alone")[1]["speech"]
    lb, lc = [], []
    for i, d in enumerate(data):
        f1 = ed.collate_fn([d])[1]["speech"][0]
        lb.append(float((fb[i, :f1.shape[0]] - f1).abs().max()))
        lc.append(float((fc[i, :f1.shape[0]] - f1).abs().max()))
    r["logmel_B_to_A_max"], r["logmel_C_to_A_max"] = float(f"{max(lb):.3e}"), float(f"{max(lc):.3e}")
    k = max(5, calls // 5)
    r["legs_B_full_ms"], r["legs_C_full_ms"] = legs(ed, reqs, False, k, 2), legs(ed, reqs, False, k, 2, rows="alone")
    return r


def ab_legs(eds, reqs, alone, calls, warmup, rounds):
    """--ab (module docstring): eds = {compute: editor}, f32 among them."""
    n = len(reqs)
    args = [(r.wav_org, r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str) for r in reqs]
    ts = {c: {} for c in eds}
    for _ in range(rounds):
        for c, ed in eds.items():
            def loop():
                for x in args:
                    ed.edit(*x)

            legs_ = {"loop_of_edit": loop, "edit_batch": lambda: ed.edit_batch(reqs)}
            if alone and c != "bf16":
                legs_["edit_batch_rows_alone"] = lambda: ed.edit_batch(reqs, rows="alone")
            for k, fn in legs_.items():
                ts[c].setdefault(k, []).append(timed(fn, calls, warmup) / n)
    out = {}
    for c, legs_ in ts.items():
        out[c] = {k: dict(ms=round(float(np.median(v)), 3), min_max_ms=[round(min(v), 3), round(max(v), 3)]) for k, v in legs_.items()}
        if c != "f32":
            for k, v in legs_.items():
                ref = ts["f32"][k]
                out[c][k]["f32_over_this"] = round(float(np.median(ref)) / float(np.median(v)), 3)
                out[c][k]["range_clear_of_f32"] = bool(max(v) < min(ref) or max(ref) < min(v))
    mel = {}
    for c, ed in eds.items():
        ed.vocoder, voc = None, ed.vocoder
        mel[c] = [g["feat"].double() for g in ed.edit_batch(reqs)]
        ed.vocoder = voc
    for c in eds:
        if c != "f32":
            d = torch.cat([(x - y).reshape(-1) for x, y in zip(mel[c], mel["f32"])])
            scale = max(1.0, max(float(y.abs().max()) for y in mel["f32"]))
            out[c]["edit_batch_mel_to_f32_of_scale"] = dict(rms=float(f"{float(d.pow(2).mean().sqrt()) / scale:.3e}"),
                                                            worst=float(f"{float(d.abs().max()) / scale:.3e}"))
    out["frames"] = [int(f.shape[0]) for f in mel["f32"]]
    return out


SPAN_LEX = {"ZEBRA": ["Z", "IY1", "B"], "PLUM": ["P", "L", "AH1"]}      # in no prompt: the word diff is the two swaps


def two_edit_requests(frames, oc, seed, duration_fn, token_id_fn):
    """A `frames`-frame utterance of three-phone words with word i -> ZEBRA and word i + 4 -> PLUM (three kept words between
    them).  Returns (both edits with max_spans=1, the same with max_spans=2, the first word's edit alone, a function
    intermediate audio -> the second word's edit)."""
    from dataclasses import replace
    from a3t_amd.sedit import EditRequest, MultiSpanEditRequest, plan_batch
    words = max(9, frames // 17)
    wav, times2, w2p, old_str, _ = prompt(words, frames, oc.fs, oc.hop_length, seed=seed)
    old = old_str.split()
    i = (words - 5) // 2

    def swapped(base, swaps):
        new = [swaps.get(k, w) for k, w in enumerate(base)]
        table = [(w.upper(), SPAN_LEX.get(w.upper()) or LEX[w.upper()]) for w in new]
        return ([ph for _, phs in table for ph in phs], {f"{k}_{w}": list(phs) for k, (w, phs) in enumerate(table)}, " ".join(new))

    phns, nw2p, new_str = swapped(old, {i: "zebra", i + 4: "plum"})
    hull = MultiSpanEditRequest(wav, times2, w2p, phns, nw2p, old_str, new_str)
    phns1, nw2p1, mid_str = swapped(old, {i: "zebra"})
    first = EditRequest(wav, times2, w2p, phns1, nw2p1, old_str, mid_str)
    # the second pass: the first pass's plan is its aligner output (prepared once; the audio is swapped in per call)
    plan = plan_batch([first], oc.fs, oc.hop_length, duration_fn, token_id_fn)[0][0]
    t2 = [[ph, s, e] for ph, s, e in zip(plan.phns, plan.align_start, plan.align_end)]
    w2p2 = {k: " ".join(v) for k, v in nw2p1.items()}
    phns2, nw2p2, _ = swapped(mid_str.split(), {i + 4: "plum"})
    second = EditRequest(plan.wav, t2, w2p2, phns2, nw2p2, mid_str, new_str)
    return hull, replace(hull, max_spans=2), first, lambda audio: replace(second, wav_org=audio)


class _CountingVocoder:
    """Passes through to the generator and adds up the frames it is given."""

    def __init__(self, voc):
        self.voc, self.frames = voc, 0
        self.margin_frames = voc.margin_frames

    def __call__(self, feat):
        return self.voc(feat)

    def inference(self, c, z=None, normalize_before=False, lengths=None):
        self.frames += int(sum(lengths)) if lengths is not None else int(c.shape[0] * c.shape[1] if c.dim() == 3 else c.shape[0])
        return self.voc.inference(c, z, normalize_before, lengths=lengths)


def spans_legs(ed, oc, frames_list, calls, warmup):
    """A, B, C, A of --spans on len(frames_list) requests; ms per request, vocoded frames per request, mel distance."""
    n = len(frames_list)
    sets = [two_edit_requests(int(f), oc, 100 + 7 * i, ed.duration_fn, ed.token_id_fn) for i, f in enumerate(frames_list)]
    hull, multi, first, second = ([s[k] for s in sets] for k in range(4))
    ed.vocoder = voc = _CountingVocoder(ed.vocoder)
    r = {}

    def two_passes(outputs):
        one = ed.edit_batch(first, outputs=outputs)
        return ed.edit_batch([mk(o["orgin_replaced"]) for mk, o in zip(second, one)], outputs=outputs)

    for name, outputs in (("full", ("prediction", "orgin_replaced")), ("span_only", ("orgin_replaced",))):
        fns = {"A_hull": lambda: ed.edit_batch(hull, outputs=outputs), "B_max_spans_2": lambda: ed.edit_batch(multi, outputs=outputs),
               "C_two_passes": lambda: two_passes(outputs)}
        for key in ("A_hull", "B_max_spans_2", "C_two_passes", "A_hull"):
            tag = f"{name}.{key}" + ("_again" if f"{name}.{key}_ms" in r else "")
            r[f"{tag}_ms"] = round(timed(fns[key], calls, warmup) / n, 3)
            voc.frames = 0
            fns[key]()
            r[f"{tag}_vocoded_frames"] = round(voc.frames / n, 1)
    ed.vocoder = None
    a, b = ed.edit_batch(hull), ed.edit_batch(multi)
    ed.vocoder = voc.voc
    r["frames"] = [int(g["feat"].shape[0]) for g in b]
    r["spans_B"] = [g["new_spans"] for g in b]
    r["span_A"] = [g["new_span_boundary"] for g in a]
    r["kept_frames_between"] = [int(g["old_spans"][-1][0] - g["old_spans"][0][1]) for g in b]
    dmax, drms = [], []
    for ga, gb in zip(a, b):
        k0, k1 = gb["new_spans"][0][1], gb["new_spans"][1][0]
        m = min(k1, ga["new_span_boundary"][1], ga["feat"].shape[0]) - k0
        x, y = gb["feat"][k0:k0 + m].double(), ga["feat"][k0:k0 + m].double()
        scale = max(1.0, float(x.abs().max()))
        dmax.append(float(f"{float((x - y).abs().max()) / scale:.3e}"))
        drms.append(float(f"{float((x - y).pow(2).mean().sqrt()) / scale:.3e}"))
    r["kept_mel_B_to_A"] = dict(max_of_scale=dmax, rms_of_scale=drms)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=["c2"])      # (none given: the --kernel leg alone)
    ap.add_argument("--compute", nargs="+", default=["bf16", "f32"])
    ap.add_argument("--n", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--frames-range", type=int, nargs=2, default=[300, 1000])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--vocoder-compute", nargs="+", default=["f32"], choices=["f32", "f16"])
    ap.add_argument("--rows", nargs="+", default=["batch"], choices=["batch", "alone"])
    ap.add_argument("--spans", action="store_true")
    ap.add_argument("--ab", type=int, default=0, metavar="ROUNDS")
    a = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    out = {"device": f"{prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)"}
    if a.kernel:
        sets = {"8x1000": [1000] * 8, "ragged": [1000, 700, 500, 300] * 2}
        if "f32" in a.vocoder_compute:
            out["pwg_blocks"] = kernel_bench(1000, sets)
        if "f16" in a.vocoder_compute:
            out["pwg_blocks_f16"] = kernel_bench_f16(1000, sets, a.calls)
            print(json.dumps({"pwg_blocks_f16": out["pwg_blocks_f16"]}), flush=True)
    if a.spans:
        for which in a.models:
            for compute in a.compute:
                ed, oc = editor(which, compute)
                for n in a.n:
                    lo, hi = a.frames_range
                    frames = np.linspace(hi, lo, n).astype(int) if n > 1 else [(lo + hi) // 2]
                    key = f"{which}.{compute}.spans.n{n}"
                    out[key] = spans_legs(ed, oc, frames, a.calls, a.warmup)
                    print(json.dumps({key: out[key]}), flush=True)
        print(json.dumps({"sedit_batch_latency": out}))
        return
    if a.ab:
        if "f32" not in a.compute:
            ap.error("--ab compares against f32: name it in --compute")
        for which in a.models:
            eds = {c: editor(which, c) for c in a.compute}
            oc = eds["f32"][1]
            for n in a.n:
                rs = np.random.RandomState(n)
                lo, hi = a.frames_range
                reqs = [request(int(f), int(k), oc, seed=10 * n + i)
                        for i, (f, k) in enumerate(zip(np.linspace(hi, lo, n).astype(int) if n > 1 else [(lo + hi) // 2],
                                                       rs.randint(3, 11, n)))]
                key = f"{which}.ab.n{n}"
                out[key] = ab_legs({c: e[0] for c, e in eds.items()}, reqs, "alone" in a.rows, a.calls, a.warmup, a.ab)
                print(json.dumps({key: out[key]}), flush=True)
        print(json.dumps({"sedit_batch_latency": out}))
        return
    if "alone" in a.rows:
        for which in a.models:
            ed, oc = editor(which, "f32")
            for n in a.n:
                rs = np.random.RandomState(n)
                lo, hi = a.frames_range
                reqs = [request(int(f), int(k), oc, seed=10 * n + i)
                        for i, (f, k) in enumerate(zip(np.linspace(hi, lo, n).astype(int) if n > 1 else [(lo + hi) // 2],
                                                       rs.randint(3, 11, n)))]
                out[f"{which}.f32.rows.n{n}"] = rows_alone_legs(ed, oc, reqs, a.calls, a.warmup)
                print(json.dumps({f"{which}.f32.rows.n{n}": out[f"{which}.f32.rows.n{n}"]}), flush=True)
        print(json.dumps({"sedit_batch_latency": out}))
        return
    for which in a.models:
        for compute, vc in [(c, v) for c in a.compute for v in a.vocoder_compute]:
            ed, oc = editor(which, compute, vc)
            tag = f"{which}.{compute}" + ("" if vc == "f32" else f".voc_{vc}")
            for n in a.n:
                rs = np.random.RandomState(n)
                lo, hi = a.frames_range
                reqs = [request(int(f), int(k), oc, seed=10 * n + i)
                        for i, (f, k) in enumerate(zip(np.linspace(hi, lo, n).astype(int) if n > 1 else [(lo + hi) // 2],
                                                       rs.randint(3, 11, n)))]
                args = [(r.wav_org, r.times2, r.word2phns, r.new_phns, r.new_word2phns, r.old_str, r.new_str) for r in reqs]

                def loop():
                    for x in args:
                        ed.edit(*x)

                r = {"A_loop_of_edit_ms": round(timed(loop, a.calls, a.warmup) / n, 3),
                     "B_full_ms": round(timed(lambda: ed.edit_batch(reqs), a.calls, a.warmup) / n, 3),
                     "B_span_only_ms": round(timed(lambda: ed.edit_batch(reqs, outputs=("orgin_replaced",)), a.calls,
                                                   a.warmup) / n, 3),
                     "A_again_ms": round(timed(loop, a.calls, a.warmup) / n, 3)}
                got = ed.edit_batch(reqs, outputs=("orgin_replaced",))
                r["frames"] = [int(g["feat"].shape[0]) for g in got]
                r["span_frames"] = [int(g["new_span_boundary"][1] - g["new_span_boundary"][0]) for g in got]
                r["legs_full_ms"] = legs(ed, reqs, False, max(5, a.calls // 5), 2)
                r["legs_span_only_ms"] = legs(ed, reqs, True, max(5, a.calls // 5), 2)
                out[f"{tag}.n{n}"] = r
                print(json.dumps({f"{tag}.n{n}": r}), flush=True)
    print(json.dumps({"sedit_batch_latency": out}))


if __name__ == "__main__":
    main()
