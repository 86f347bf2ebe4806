"""float64 references, error bounds, a host restatement of the persistent tile walk and the case tables for the ParallelWaveGAN
kernels: the fused residual block (csrc/pwg_fused.hip, csrc/pwg_fused_f16.hip) and the layer-by-layer helpers (csrc/misc.hip,
a3t_reflect_pad_rows of csrc/melgan.hip).  No device code: tests/test_pwg_ref_host.py holds every part against torch and the
oracle without a GPU, tests/test_gpu_pwg_blocks.py holds the kernels against it.

Tensors are channels-last like the kernels': x / skips [B][Tw][64], cu [B][Tw][80].  A ragged batch gives each row b its valid
length W[b]; what lies behind it is padding that no reference reads (the tests fill it with NaN).

Tolerance of the fused fp32 block (`allowance`)
-----------------------------------------------
Both the kernel and a CPU fp32 evaluation are fp32 sums of the same 272 + 64 products in different orders, so the kernel is
allowed 4 x F, F = the largest error of the CPU's fp32 evaluation of the same case against float64 (the convention of
hifigan_ref.bound, without its floor: F is taken per case and per output tensor).  On top comes what the CPU evaluation does not
have, the kernel's gate  g = (1 - 2 rcp(1 + e^{2 ya})) * rcp(1 + e^{-yb})  from the hardware exponential and reciprocal
(__expf = v_exp_f32(y * log2 e), __frcp_rn).  An error dg of one gate value reaches output o through wt1[c][o], hence
    |x_out - ref| <= 4 F_x + sqrt(1/2) * R_GATE * sum_c |wt1[c][o]|,        |skips - ref| <= 4 F_s + R_GATE * sum_c |wt1[c][64 + o]|.

R_GATE, first order, in units of u = 2^-24 (half an ulp of a value in [1, 2)); e stands for the exponential, s for the sigmoid:
  * y * log2 e is rounded once (relative u, and as much again for the rounded constant): e is off by 2 |y| u relatively;
    v_exp_f32 is taken at one ulp, at most 2 u relatively.  d s = s (1 - s) * (relative error of e):
    s (1 - s) (2 |y| + 2) u <= 0.95 u (the maximum of s (1 - s)(|y| + 1) is 0.47 near |y| = 1.3).
  * 1 + e is rounded once (relative u) and the reciprocal is taken at one ulp (2 u relatively; a correctly rounded one has u):
    up to 3 s u <= 3 u.  Over all y the two items together stay below 3.3 u for the sigmoid.
  * tanh = 1 - 2 s'(with e^{2 ya}, 2 ya exact): twice the sigmoid's terms at argument 2 ya, 2 s'(1 - s')(2 |2 ya| + 2) u +
    2 (1 - s') 3 u, at most 6.6 u (near 2 ya = -2), plus the final subtraction's rounding 0.5 u: 7.1 u; with a correctly rounded
    reciprocal 5.3 u.
  * the product th * sg: |d th| sg + |th| |d sg| + one rounding u |th sg|.
Each error at an average-sized ulp (0.72 of the worst) and the terms at their own maxima give about 3 u per factor and 6 u for the
product; every rounding at its limit with one sign gives 8.8 u (correctly rounded reciprocal) to 11.4 u (one-ulp reciprocal) on
one channel.  R_GATE = 2^-21 = 8 u.  It enters the bound multiplied by sum_c |wt1[c][o]|, which already assumes that all 64
channels err at once with the sign of their weight: the single-channel corner above (1.4 x R_GATE at most) cannot be reached by all
of them, since the maxima need ya near -1 AND yb large on every channel of a sample.

The layer path's a3t_pwg_gate uses tanhf and 1 / (1 + __expf(-b)) on a = y + c, b = y + c (each sum rounded once):
    |g - ref| <= R_GATE + u (|a| * 1 + |b| / 4)     (the slopes of tanh * sigmoid in a and b are at most 1 and 1/4).
a3t_pwg_res_skip, the paddings and a3t_zero_tail consist of exact fp32 operations or copies: bit for bit.  a3t_pwg_upsample adds
2 scale + 1 products in a fixed order: the fp32 restatement `upsample_ref(dtype=float32)` in the same order is bit for bit too
(the build has -ffp-contract=off)."""
import collections
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
R_GATE = 2.0 ** -21
SQRT_HALF = math.sqrt(0.5)
TILE = 256
SENTINEL = -7777.0
PWG_BLOCK = "conv_layers.3."          # the block of vocoder_state(seed=4) that every block case runs


# ----------------------------------------------------------------------------------------------------------------------
# the fused residual block
# ----------------------------------------------------------------------------------------------------------------------
def gate_perm(gate_channels=128):
    """a3t_amd.vocoder.pwg_gate_perm restated from include/a3t_hip.h: gate channel c (0 .. 63) has its tanh pre-activation in
    column n' = 64 (c / 32) + c % 32 and its sigmoid pre-activation 32 columns further; -> perm[n'] = the convolution's output
    channel in column n' (the sigmoid half of channel c is convolution channel c + gate_channels / 2)."""
    h = gate_channels // 2
    perm = np.empty(gate_channels, dtype=np.int64)
    for c in range(h):
        n = 64 * (c // 32) + c % 32
        perm[n], perm[n + 32] = c, c + h
    return perm


def gate_columns(perm=None):
    """(ia, ib): the columns n' of the packed first product that hold the tanh and the sigmoid pre-activation of gate channel c."""
    perm = gate_perm() if perm is None else np.asarray(perm)
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    h = len(perm) // 2
    return torch.from_numpy(inv[:h].copy()), torch.from_numpy(inv[h:].copy())


def block_ref(x, cu, skips, wt0, b0, wt1, b1, dil, W, dtype=F64):
    """One residual block on the kernel's packed operands (wt0 [272][128] tap-major with gate-permuted columns, b0 permuted the
    same way, wt1 [64][128], b1 [128]) by index gathers, evaluated in `dtype`.  x [B][Tw][64], cu [B][Tw][80], skips [B][Tw][64];
    W[b]: valid samples of row b, a tap outside [0, W[b]) is zero.  -> (x_out, skips_out, absw1): the two tensors hold the
    inputs' own values behind W[b]; absw1[o] = sum_c |wt1[c][o]| in float64."""
    B, Tw, R = x.shape
    wt0, b0, wt1, b1 = (t.to(dtype) for t in (wt0, b0, wt1, b1))
    ia, ib = gate_columns()
    x_out, skips_out = x.to(dtype).clone(), skips.to(dtype).clone()
    half = torch.tensor(SQRT_HALF, dtype=dtype)
    for b in range(B):
        n = int(W[b])
        if n == 0:
            continue
        t = torch.arange(n)
        xb = x[b, :n].to(dtype)
        y = b0 + cu[b, :n].to(dtype) @ wt0[3 * R:]
        for tap in range(3):
            ts = t + (tap - 1) * dil
            ok = (ts >= 0) & (ts < n)
            xs = xb[ts.clamp(0, n - 1)] * ok[:, None].to(dtype)
            y = y + xs @ wt0[tap * R:(tap + 1) * R]
        g = torch.tanh(y[:, ia]) * torch.sigmoid(y[:, ib])
        o = b1 + g @ wt1
        x_out[b, :n] = (o[:, :R] + xb) * half
        skips_out[b, :n] = skips[b, :n].to(dtype) + o[:, R:]
    return x_out, skips_out, wt1.to(F64).abs().sum(0)


def valid_mask(B, Tw, W):
    """bool [B][Tw]: t < W[b]."""
    return torch.arange(Tw)[None, :] < torch.as_tensor([int(w) for w in W])[:, None]


def allowance(ref64, ref32, absw1, W):
    """(allow_x [64], allow_s [64], F_x, F_s) of a block case: ref64 / ref32 = block_ref's (x_out, skips_out) in float64 and in
    float32, compared over the valid samples."""
    B, Tw, _ = ref64[0].shape
    m = valid_mask(B, Tw, W)
    Fx = float((ref32[0].to(F64) - ref64[0])[m].abs().max())
    Fs = float((ref32[1].to(F64) - ref64[1])[m].abs().max())
    return 4.0 * Fx + SQRT_HALF * R_GATE * absw1[:64], 4.0 * Fs + R_GATE * absw1[64:], Fx, Fs


# ----------------------------------------------------------------------------------------------------------------------
# the layer path
# ----------------------------------------------------------------------------------------------------------------------
def gate_ref(y, c):
    """a3t_pwg_gate: y, c [T][2H] (tanh half | sigmoid half) -> (g [T][H] in float64, allowance [T][H])."""
    H = y.shape[1] // 2
    a32 = y + c                                        # the kernel's rounded sums, for the allowance's magnitudes only
    s = y.to(F64) + c.to(F64)
    g = torch.tanh(s[:, :H]) * torch.sigmoid(s[:, H:])
    return g, R_GATE + U * (a32[:, :H].abs().to(F64) + 0.25 * a32[:, H:].abs().to(F64))


def res_skip_ref(o, x, skips, dtype=F64):
    """a3t_pwg_res_skip: o [T][R + S] -> (x_out = (o[:, :R] + x) * sqrt(1/2), skips + o[:, R:]) in `dtype`; float32 is the kernel's
    own arithmetic (one addition, one multiplication by the fp32 constant; one addition)."""
    R = x.shape[1]
    o, x, skips = o.to(dtype), x.to(dtype), skips.to(dtype)
    return (o[:, :R] + x) * torch.tensor(SQRT_HALF, dtype=dtype), skips + o[:, R:]


def _row_lengths(B, full, lens, mul=1):
    return [full if lens is None else max(0, min(full, int(lens[b]) * mul)) for b in range(B)]


def upsample_ref(c, w, scale, lens=None, mul=1, dtype=F64):
    """a3t_pwg_upsample(_ragged): c [B][Tin][C], w [2 scale + 1] -> out [B][Tin * scale][C],
    out[b][t] = sum_j w[j] * c[b][(t + j - scale) // scale] over 0 <= t + j - scale < L_b * scale, added in the order of j, zero
    behind L_b * scale (L_b = Tin, ragged: lens[b] * mul)."""
    B, Tin, C = c.shape
    out = torch.zeros(B, Tin * scale, C, dtype=dtype)
    w = w.to(dtype)
    for b, L in enumerate(_row_lengths(B, Tin, lens, mul)):
        n = L * scale
        if n == 0:
            continue
        t = torch.arange(n)
        cb = c[b, :L].to(dtype)
        acc = torch.zeros(n, C, dtype=dtype)
        for j in range(2 * scale + 1):
            u = t + j - scale
            ok = (u >= 0) & (u < n)
            term = w[j] * cb[torch.div(u.clamp(0, n - 1), scale, rounding_mode="floor")]
            acc = torch.where(ok[:, None], acc + term, acc)
        out[b, :n] = acc
    return out


def replicate_pad_ref(x, pad, lens=None):
    """a3t_replicate_pad(_ragged): x [B][T][C] -> y [B][T + 2 pad][C], y[b][u] = x[b][clamp(u - pad, 0, L_b - 1)], an empty row is
    zero (L_b = T, ragged: lens[b])."""
    B, T, C = x.shape
    y = torch.zeros(B, T + 2 * pad, C, dtype=x.dtype)
    u = torch.arange(T + 2 * pad) - pad
    for b, L in enumerate([T if lens is None else int(lens[b]) for b in range(B)]):
        if L > 0:
            y[b] = x[b][u.clamp(0, L - 1)]
    return y


def zero_tail_ref(x, lens, mul):
    """a3t_zero_tail: x [B][T][C] with the rows t >= lens[b] * mul set to zero."""
    y = x.clone()
    for b in range(x.shape[0]):
        y[b, max(0, int(lens[b]) * mul):] = 0
    return y


def reflect_index(u, L):
    """csrc/wave_conv.h refl(): one reflection at each end of [0, L), what it does not reach clamped into the row."""
    u = u.abs()
    u = torch.where(u >= L, 2 * (L - 1) - u, u)
    return u.clamp(0, L - 1)


def reflect_pad_rows_ref(x, pad, lens=None, mul=1):
    """a3t_reflect_pad_rows(_ragged): x [B][T][C] -> y [B][T + 2 pad][C], y[b][u] = x[b][refl(u - pad)] over the row's own length
    L_b (T, ragged: min(lens[b] * mul, T)); an empty row is zero."""
    B, T, C = x.shape
    y = torch.zeros(B, T + 2 * pad, C, dtype=x.dtype)
    u = torch.arange(T + 2 * pad) - pad
    for b, L in enumerate(_row_lengths(B, T, lens, mul)):
        if L > 0:
            y[b] = x[b][reflect_index(u, L)]
    return y


# ----------------------------------------------------------------------------------------------------------------------
# tiles and the persistent walk
# ----------------------------------------------------------------------------------------------------------------------
def tile_list(W):
    """The contract of csrc/wave_tiles.h written out: int32 [ntiles][4] = {row b, first sample t0, valid samples W[b], 0}, one entry
    per 256-sample tile that holds a valid sample, rows in order."""
    out = [(b, t0, int(w), 0) for b, w in enumerate(W) for t0 in range(0, int(w), TILE)]
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


def check_tile_list(tiles, B, Tw, W):
    """Raises AssertionError unless `tiles` satisfies the contract of wave_tiles.h for rows of W[b] <= Tw samples: every entry
    {0 <= b < B, t0 a multiple of 256, t0 < W_b = W[b] <= Tw, 0}, and every tile that holds a valid sample listed exactly once."""
    seen = set()
    for b, t0, wb, z in np.asarray(tiles).tolist():
        assert 0 <= b < B and z == 0 and t0 % TILE == 0 and 0 <= t0 < wb <= Tw and wb == int(W[b]), (b, t0, wb, z)
        assert (b, t0) not in seen
        seen.add((b, t0))
    assert seen == {(b, t0) for b in range(B) for t0 in range(0, int(W[b]), TILE)}


def walk(ntiles, cus):
    """The persistent loop of pwg_stage_kernel / pwg_f16_kernel: the grid is min(ntiles, cus) workgroups and workgroup g handles
    the tiles g, g + grid, g + 2 grid, ... in that order.  -> one list of tile indices per workgroup."""
    grid = min(ntiles, cus)
    return [list(range(g, ntiles, grid)) for g in range(grid)]


def tile_samples(tiles, Tw):
    """Flat sample indices b * Tw + t of the valid samples of the listed tiles."""
    idx = [torch.arange(b * Tw + t0, b * Tw + min(t0 + TILE, wb)) for b, t0, wb, _ in np.asarray(tiles).tolist()]
    return torch.cat(idx) if idx else torch.zeros(0, dtype=torch.int64)


# ----------------------------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name B Tw W dil ragged seed")


def _case(name, B, Tw, W, dil, seed):
    ragged = W is not None
    return Case(name, B, Tw, tuple(W) if ragged else (Tw,) * B, dil, ragged, seed)


RAGGED_W = (1500, 257, 5)     # a row end one sample into a tile; a row shorter than dilations 8 and 512; 257 < the reach of 512
BLOCK_CASES = tuple(
    [_case(f"dense_d{d}", 3, 1500, None, d, 10 + i) for i, d in enumerate((1, 8, 512))] +
    [_case(f"ragged_d{d}", 3, 1500, RAGGED_W, d, 20 + i) for i, d in enumerate((1, 8, 512))] +
    [_case("dense_T255_d8", 2, 255, None, 8, 30),        # no full tile
     _case("dense_T513_d1", 2, 513, None, 1, 31)])       # the last tile of a row holds one sample


def walk_dense(cus, dil):
    """About 2.25 cus tiles: B = 3 rows of ceil(0.75 cus) full tiles and one tile of a single sample, so a workgroup's second tile
    lies in another row than its first."""
    Tw = TILE * math.ceil(0.75 * cus) + 1
    return _case(f"walk_dense_d{dil}", 3, Tw, None, dil, 40 + dil % 7)


def walk_ragged(cus, dil):
    """Four rows of about 0.9 cus, 0.2 cus, 1 and 1.2 cus tiles: the first ends mid-tile, the third has 5 samples, the fourth one
    sample in its last tile."""
    W = (TILE * math.floor(0.9 * cus) - 100, TILE * math.ceil(0.2 * cus), 5, TILE * math.ceil(1.2 * cus) + 1)
    return _case(f"walk_ragged_d{dil}", 4, max(W), W, dil, 50 + dil % 7)


WALK_DILS = (1, 512)


def walk_cases(cus):
    return tuple(f(cus, d) for f in (walk_dense, walk_ragged) for d in WALK_DILS)


def device_bytes(case):
    """The padded allocation of a case on the device: x, g, skips [B*Tw][64] and cu [B*Tw][80], fp32."""
    return case.B * case.Tw * (64 * 3 + 80) * 4


def case_inputs(case):
    """(x, cu, skips) of a case as fp32 tensors: x = 1.5 N(0, 1), cu = 2 N(0, 1), skips = N(0, 1) in front of W[b]; behind it x and
    cu are NaN and skips holds SENTINEL."""
    rs = np.random.RandomState(case.seed)
    x = torch.full((case.B, case.Tw, 64), float("nan"))
    cu = torch.full((case.B, case.Tw, 80), float("nan"))
    sk = torch.full((case.B, case.Tw, 64), SENTINEL)
    for b, n in enumerate(case.W):
        x[b, :n] = torch.from_numpy((rs.standard_normal((n, 64)) * 1.5).astype(np.float32))
        cu[b, :n] = torch.from_numpy((rs.standard_normal((n, 80)) * 2.0).astype(np.float32))
        sk[b, :n] = torch.from_numpy(rs.standard_normal((n, 64)).astype(np.float32))
    return x, cu, sk


def block_params(pre=PWG_BLOCK, seed=4):
    """The raw parameters of one block of pwg_f16_ref.vocoder_state(seed) as fp32 tensors: (conv.weight, conv.bias,
    conv1x1_aux.weight, conv1x1_out.weight, conv1x1_out.bias)."""
    import pwg_f16_ref
    _, state = pwg_f16_ref.vocoder_state(seed=seed)
    return tuple(torch.from_numpy(np.array(state[pre + k], dtype=np.float32)) for k in
                 ("conv.weight", "conv.bias", "conv1x1_aux.weight", "conv1x1_out.weight", "conv1x1_out.bias"))
