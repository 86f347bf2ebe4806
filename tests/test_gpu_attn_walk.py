"""a3t_attn_bwd_ds against the float64 reference of tests/attn_ref.py while its workgroups WALK: every case of attn_ref.cases()
has more tasks than the 2 x CUs workgroups the launcher starts, so each workgroup carries its three-slot V ring, its prefetched
rows and its counted waits across two or three tasks -- within a query block, into the next one, into the next head and the next
batch row (attn_ref.walk names the transitions; tests/test_attn_ref_host.py checks that the table reaches all of them).

One launch per case on synthetic operands (no forward launch).  dS and dBD start as a sentinel between guard bands: the bands
must come back intact and every element inside written; dS must lie within attn_ref.bound_ds of the reference per element
(printed: `RATIO <case> ds: max error / bound`, a ratio above 1 fails and names the workgroup and transition that produced the
worst element); dBD must be the inverse skew of the dS the kernel wrote, bit for bit; with dbd=None the T zeros in front of each
(b, h) block of dS stay zero; the inputs keep their bits.  Run with `pytest -m gpu -s` on an MI355X.

Measured on an MI355X (256 CUs, 512 workgroups), max error / bound per case; the bf16 rounding term of the bound is reached by
a correct rounding, so a ratio just below 1 is what a correct kernel shows (the fp32 emulations of test_attn_ref_host.py give the
same figures to the third digit; their error before the bf16 store is at most 4 % of the bound's fp32 term):

    case (+ _drop1 / _drop2)         B x H    T   tper  transitions met                                          ratio
    one_tile                        104 x 5   32   2    new-head new-batch nt1->nt1 (idle workgroups)             0.997
    strip_5_1_dk32/64/96/128/192     43 x 3  168   2    same-block                          0.998 0.995 0.992 0.988 0.980
    strip_5_1_dk64_drop1 / _drop2    43 x 3  168   2    same-block                                          0.996 0.995
    strip_5_2 / 5_3 / 5_4            43 x 3 (x 2) 200 / 232 / 264  2  same-block                       0.995 0.995 0.996
    tper3_dk64 / dk192               57 x 2  328   3    same-block                                          0.996 0.983
    tper3_dk192_drop1 / _drop2       57 x 2  328   3    same-block                                          0.981 0.985
    cross_5_1_dk32/64/96/128/192    130 x 2  168   3    same-block new-block new-head new-batch nt1->ntN (short-last)
                                                                                            0.998 0.995 0.993 0.989 0.980
    cross_5_1_dk64_drop1 / _drop2   130 x 2  168   3    as above                                            0.995 0.995
    cross_5_5_1_dk64 / dk192         19 x 3  328   2    same-block new-block new-head new-batch nt1->ntN (short-last)
                                                                                                            0.995 0.982
    cross_5_5_1_dk192_drop1 / _drop2 19 x 3  328   2    as above                                            0.982 0.979
    production (DROP 2, no dBD)     130 x 2  168   3    as cross_5_1                                              0.980

Before the request for the next task's first V tile after a one-tile task was added to the kernel, one_tile, every cross_* case
and production failed here (non-finite or unwritten dS in the task after `nt1->nt1` / `nt1->ntN`); the other cases passed.
"""
import pytest
import torch

import attn_ref as A
from test_gpu_rowkernel_paths import SENT, Bands

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_walking_launch_against_float64(name):
    from a3t_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = {c.name: c for c in A.cases(cus)}[name]
    B, H, T, dk = case.B, case.H, case.T, case.dk
    w = A.walk(B, H, T, cus)
    assert w.geometry.tper == case.tper >= 2
    op = A.case_operands(case)
    dev = {k: op[k].to(DEV) for k in ("dctx", "ctx", "qkv", "probs", "rowscale")}
    before = {k: _bits(v).clone() for k, v in dev.items()}
    bands = Bands()
    sent = torch.tensor(SENT, dtype=torch.bfloat16)
    assert float(sent) == SENT
    if case.dbd is None:
        bs = T * T + T
        init = torch.full((B * H, bs), SENT, dtype=torch.bfloat16, device=DEV)
        init[:, :T] = 0
        blocks = bands.out((B * H, bs), torch.bfloat16, init=init)
        ds_arg, dbd, ds = blocks.view(-1)[T:], None, blocks[:, T:]
    else:
        bs = 0
        ds = ds_arg = bands.out((B, H, T, T), torch.bfloat16)
        dbd = bands.out((H, B, T, T) if case.dbd == "hm" else (B, H, T, T), torch.bfloat16)
    ops.attn_bwd_ds(dev["dctx"], dev["ctx"], dev["qkv"], dev["probs"], dev["rowscale"], ds_arg, dbd, B, H, T, op["scale"],
                    drop=op["drop"], dbd_head_major=case.dbd == "hm", signed_probs=case.mode == 2, ds_bs=bs)
    bands.intact()
    for k, v in dev.items():
        assert torch.equal(_bits(v), before[k]), f"{k} was written"
    got = ds.reshape(B, H, T, T)
    gbits = _bits(got)
    sbits = int(_bits(sent.view(1))[0])
    assert not bool((gbits == sbits).any()), "an element of dS was not written"
    if case.dbd is None:
        assert not bool(blocks[:, :T].any()), "the zeros in front of the blocks are nobody's output"
    # dS against the definition
    d = H * dk
    o = A.ref_bwd_ds(dev["dctx"], dev["ctx"], dev["qkv"][:, 2 * d:], dev["probs"], dev["rowscale"], op["scale"], op["drop"], case.mode)
    g64 = got.to(torch.float64)
    assert bool(torch.isfinite(g64).all())
    assert float(o.ref.abs().max()) > 1e-3 and not bool(g64[2].any())
    q = (g64 - o.ref).abs() / A.bound_ds(o).clamp_min(1e-300)
    ratio = float(q.max())
    trans = "+".join(sorted(A.transition_labels(w)))
    print(f"RATIO {name} ds: max error / bound = {ratio:.3f}   [B{B} H{H} T{T} dk{dk} DROP{case.mode} dbd={case.dbd} tper={case.tper}: {trans}]")
    if ratio > 1.0:
        flat = int(q.argmax())
        bh, i, j = flat // (T * T), (flat // T) % T, flat % T
        bad = (q > 1.0).nonzero()
        tasks = sorted({((int(b) * H + int(h)) * w.geometry.NQB + int(i_) // 128) * w.geometry.NKC + int(j_) // 160
                        for b, h, i_, j_ in bad[:: max(1, len(bad) // 2000)].tolist()})
        raise AssertionError(f"{name}: {len(bad)} elements of dS outside the bound, worst {ratio:.3f} at [bh {bh}][{i}][{j}]: "
                             f"{A.locate(w, bh, i, j)}; tasks hit (sampled): {tasks[:40]}")
    # dBD: the inverse skew of the dS the kernel wrote
    if dbd is not None:
        dbits = _bits(dbd.transpose(0, 1) if case.dbd == "hm" else dbd)
        assert not bool((dbits == sbits).any()), "an element of dBD was not written"
        want = A.inverse_skew(gbits)
        if not torch.equal(dbits, want):
            bad = (dbits != want).nonzero()
            b, h, r, c = bad[0].tolist()
            i, j = (r, c - (T - 1 - r)) if c >= T - 1 - r else (r - 1, c + r + 1)
            raise AssertionError(f"{name}: {len(bad)} elements of dBD differ from the skew of dS, first at [b {b}][h {h}][{r}][{c}] = "
                                 f"dS[{i}][{j}]: {A.locate(w, b * H + h, i, j)}")
