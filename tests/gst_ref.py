"""CPU restatement of the GST style encoder of a gst+xvector FastSpeech2 (espnet2/tts/gst/style_encoder.py) over a padded
batch of log-mel prompts with per-row lengths ("ragged" semantics): the yardstick of a3t_amd/csrc/gst.hip and of
FS2DurationModel.style_from_mel, held to the reference's own outputs in tests/golden/gst_duration.{npz,json}.

Row b of a padded [B][Tmax][n_mels] batch must get what it would get alone at n = lens[b]:
  1. every conv layer reads zeros at time positions >= the row's length in front of that layer and its outputs at
     t' >= n' = (n + 2p - k) // s + 1 are zeroed again: BatchNorm's shift makes them non-zero, and the next layer's taps
     reach over the edge;
  2. the GRU runs n' (of the last layer) steps for the row; the style-token attention is row-wise.
Also here: the procedural inputs of the fixture (mel_input, waveform), generated from seeds and stored nowhere, and the
fixture's documented weight overrides.  Not a test module: tests/test_gst_host.py and tests/test_gpu_gst.py import it, and
tests/golden/make_golden_gst.py takes the inputs and the overrides from here.  Nothing of the reference is imported."""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from oracle import a3t_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the fixture's inputs ----------------------------------------------------------------------------------------------
MEL_LENGTHS = (1, 63, 64, 65, 401, 1003, 2050)        # 64 -> 65: the GRU of the default plan gets its second step
CONV_LENGTHS = (1, 63, 64, 65)                        # the last conv output is stored for these
TEXT_PROMPT = 401                                     # the mel prompt behind the five text lengths of the FS2 fixture
WAV_SAMPLES = {"a": 120000, "b": 39217}               # 401 and 131 frames at hop 300
FEATS_CONF = dict(fs=24000, n_fft=2048, win_length=1200, hop_length=300, n_mels=80, fmin=80, fmax=7600)
MEL_EPS = 2e-4                                        # the bound tests/golden/logmel.npz is held to


def mel_input(T, seed=0, n_mels=80):
    """A log10-mel-like [T][n_mels] float32: a smooth spectral tilt and slow frame-to-frame movement plus noise, in the range
    speech takes under the reference's extractor (about -7 .. 1)."""
    rs = np.random.RandomState(7000 + 13 * T + seed)
    tilt = np.linspace(0.5, -2.5, n_mels)[None, :]
    slow = np.cumsum(rs.standard_normal((T, 1)) * 0.15, axis=0)
    tex = rs.standard_normal((T, n_mels)) * 0.9
    return (-2.0 + tilt + slow + tex).astype(np.float32)


def waveform(n, seed=0, fs=24000):
    """A procedural prompt: three gliding partials under a syllable-rate envelope, plus noise; float32 [n]."""
    rs = np.random.RandomState(9000 + seed)
    t = np.arange(n) / fs
    f0 = 110.0 + 40.0 * rs.rand() + 25.0 * np.sin(2 * np.pi * (0.7 + rs.rand()) * t)
    ph = 2 * np.pi * np.cumsum(f0) / fs
    env = 0.55 + 0.45 * np.sin(2 * np.pi * (3.0 + rs.rand()) * t + rs.rand())
    x = env * (0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 1.0) + 0.12 * np.sin(5 * ph + 2.0))
    return (0.3 * x + 0.02 * rs.standard_normal(n)).astype(np.float32)


def mel_perturbation(shape, seed=0):
    """+-MEL_EPS per element."""
    return (MEL_EPS * np.random.RandomState(11000 + seed).choice([-1.0, 1.0], size=shape)).astype(np.float32)


# ---- the fixture's weights ---------------------------------------------------------------------------------------------
BN_SEED, EMB_SEED = 4321, 4400
Q_SCALE, IH_SCALE, CONV_SCALE = 4.0, 0.25, 1.3
OVERRIDES = {
    "gst.ref_enc.convs.{3i+1}.weight": f"1 + U(-0.2, 0.2), RandomState({BN_SEED} + i): BatchNorm2d gammas (the procedural draw "
                                       "U(-0.1, 0.1) lets BatchNorm's shift drown the signal within three layers)",
    "gst.ref_enc.convs.{3i}.weight": f"x {CONV_SCALE}: keeps the activations' scale through the stride-2 ReLU stack",
    "gst.stl.gst_embs": f"N(0, 1), RandomState({EMB_SEED}): the reference's own init (torch.randn)",
    "gst.stl.mha.linear_q.weight": f"x {Q_SCALE}",
    "gst.ref_enc.gru.weight_ih_l0": f"x {IH_SCALE}: keeps the GRU out of saturation behind conv outputs of scale 10; with the "
                                    "two above the token attention is far from uniform, so two prompts get different "
                                    "style embeddings",
}


def apply_gst_overrides(state, n_conv):
    """The documented overrides on a procedural_state dict keyed by the FastSpeech2 state-dict names."""
    for i in range(n_conv):
        k = f"gst.ref_enc.convs.{3 * i + 1}.weight"
        state[k] = (1.0 + np.random.RandomState(BN_SEED + i).uniform(-0.2, 0.2, state[k].shape)).astype(np.float32)
        k = f"gst.ref_enc.convs.{3 * i}.weight"
        state[k] = (state[k] * np.float32(CONV_SCALE)).astype(np.float32)
    k = "gst.stl.gst_embs"
    state[k] = np.random.RandomState(EMB_SEED).standard_normal(state[k].shape).astype(np.float32)
    state["gst.stl.mha.linear_q.weight"] = (state["gst.stl.mha.linear_q.weight"] * np.float32(Q_SCALE)).astype(np.float32)
    state["gst.ref_enc.gru.weight_ih_l0"] = (state["gst.ref_enc.gru.weight_ih_l0"] * np.float32(IH_SCALE)).astype(np.float32)
    return state


def meta():
    return json.load(open(os.path.join(G, "gst_duration.json")))


def arrays():
    return np.load(os.path.join(G, "gst_duration.npz"))


def checkpoint(m, case):
    """(ESPnet config dict, state dict under the FastSpeech2 names without 'tts.') of a fixture model, overrides applied."""
    mc = m["cases"][case]
    state = O.procedural_state({k: tuple(v) for k, v in mc["shapes"].items()}, mc["seed"])
    if G not in sys.path:
        sys.path.insert(0, G)
    from make_golden_fs2 import apply_overrides      # (imports nothing of the reference)
    apply_overrides(state, mc["tts_conf"].get("duration_predictor_layers", 2))
    apply_gst_overrides(state, mc["tts_conf"].get("gst_conv_layers", 6))
    cfg = {"tts": "fastspeech2", "tts_conf": mc["tts_conf"], "token_list": m["token_list"], "feats_extract": "fbank",
           "feats_extract_conf": m["feats_extract_conf"]}
    return cfg, {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def plan_of(tts_conf):
    """(channel list, kernel, stride, gru units, heads) of a tts_conf, with FastSpeech2's defaults."""
    chans = list(tts_conf.get("gst_conv_chans_list", (32, 32, 64, 64, 128, 128)))
    return chans, tts_conf.get("gst_conv_kernel_size", 3), tts_conf.get("gst_conv_stride", 2), \
        tts_conf.get("gst_gru_units", 128), tts_conf.get("gst_heads", 4)


def out_len(n, k, s):
    return (n + 2 * ((k - 1) // 2) - k) // s + 1


def _time_mask(x, lens):
    """x [B][C][T][F]: zero at t >= lens[b]."""
    if lens is None:
        return x
    keep = torch.arange(x.shape[2], device=x.device)[None, :] < torch.as_tensor(lens, device=x.device)[:, None]
    return torch.where(keep[:, None, :, None], x, torch.zeros((), dtype=x.dtype, device=x.device))


def conv_stack(sd, tts_conf, mel, lens=None, upto=None):
    """The ReferenceEncoder's conv layers over mel [B][T][n_mels] (rows valid for lens[b] frames; None: all T).  Returns
    (hs [B][C][T'][F'], lens') in the reference's channel-first layout; upto: stop after that many layers."""
    chans, k, s, _, _ = plan_of(tts_conf)
    x = mel.unsqueeze(1)
    lens = None if lens is None else [int(n) for n in lens]
    for i in range(len(chans) if upto is None else upto):
        x = _time_mask(x, lens)
        x = F.conv2d(x, sd[f"gst.ref_enc.convs.{3 * i}.weight"].to(x.dtype), stride=s, padding=(k - 1) // 2)
        bn = f"gst.ref_enc.convs.{3 * i + 1}."
        x = F.batch_norm(x, sd[bn + "running_mean"].to(x.dtype), sd[bn + "running_var"].to(x.dtype), sd[bn + "weight"].to(x.dtype),
                         sd[bn + "bias"].to(x.dtype), training=False, eps=1e-5)
        x = torch.relu(x)
        if lens is not None:
            lens = [out_len(n, k, s) for n in lens]
            x = _time_mask(x, lens)
    return x, lens


def gru(sd, xs, lens=None):
    """torch.nn.GRU (one layer, batch_first, gate order r, z, n) over xs [B][T][in]; row b runs lens[b] steps.  Returns the
    rows' last hidden states [B][H]."""
    dt = xs.dtype
    wih, whh = sd["gst.ref_enc.gru.weight_ih_l0"].to(dt), sd["gst.ref_enc.gru.weight_hh_l0"].to(dt)
    bih, bhh = sd["gst.ref_enc.gru.bias_ih_l0"].to(dt), sd["gst.ref_enc.gru.bias_hh_l0"].to(dt)
    B, T, _ = xs.shape
    H = whh.shape[1]
    h = torch.zeros(B, H, dtype=dt, device=xs.device)
    n = torch.full((B,), T, device=xs.device) if lens is None else torch.as_tensor([int(v) for v in lens], device=xs.device)
    for t in range(T):
        gi = xs[:, t] @ wih.t() + bih
        gh = h @ whh.t() + bhh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        c = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        hn = (1 - z) * c + z * h
        h = torch.where((t < n)[:, None], hn, h)
    return h


def style_tokens(sd, tts_conf, ref_embs):
    """StyleTokenLayer: multi-head attention of ref_embs [B][H] over tanh(gst_embs).  Returns [B][adim]."""
    dt = ref_embs.dtype
    heads = plan_of(tts_conf)[4]
    lin = lambda n, x: x @ sd[f"gst.stl.mha.linear_{n}.weight"].to(dt).t() + sd[f"gst.stl.mha.linear_{n}.bias"].to(dt)
    e = torch.tanh(sd["gst.stl.gst_embs"].to(dt))
    q, kk, vv = lin("q", ref_embs), lin("k", e), lin("v", e)
    B, d = q.shape
    dk = d // heads
    q = q.view(B, heads, dk)
    kk, vv = kk.view(-1, heads, dk), vv.view(-1, heads, dk)
    p = torch.softmax(torch.einsum("bhd,khd->bhk", q, kk) / math.sqrt(dk), dim=-1)
    return lin("out", torch.einsum("bhk,khd->bhd", p, vv).reshape(B, d))


def style_encoder(sd, tts_conf, mel, lens=None):
    """StyleEncoder.forward with the ragged rule.  Returns (last conv output [B][C][T'][F'], ref_embs [B][H], style [B][d])."""
    hs, l2 = conv_stack(sd, tts_conf, mel, lens)
    B, C, T, Fq = hs.shape
    ref = gru(sd, hs.transpose(1, 2).reshape(B, T, C * Fq), l2)
    return hs, ref, style_tokens(sd, tts_conf, ref)


def pad_batch(mels, fill=0.0):
    """[B][Tmax][n_mels] float32 tensor of a list of [T_b][n_mels] arrays, `fill` behind every row, and the lengths."""
    lens = [int(m.shape[0]) for m in mels]
    x = torch.full((len(mels), max(lens), mels[0].shape[1]), float(fill), dtype=torch.float32)
    for b, m in enumerate(mels):
        x[b, :lens[b]] = torch.as_tensor(m)
    return x, lens
