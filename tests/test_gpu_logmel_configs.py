"""The log-mel front end (a3t_amd/features.py: the only user of the GEMM's overlapping-row operand) at configurations beside
the golden one: window shorter than n_fft, lengths that straddle a frame boundary, a hop that is no multiple of 4 (scalar loaders)
and an odd n_fft.  Reference: oracle.a3t_oracle.logmel_fbank evaluated in float64 on the CPU."""
import types

import pytest
import torch

from gst_ref import MEL_EPS
from oracle import a3t_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"

#          fs, n_fft,  win, hop, n_mels,    N, lengths
CONFIGS = [(24000, 2048, 1200, 300, 80, 3000, (3000, 2050, 1300)),
           (16000, 1024, 1024, 256, 80, 2311, (2311, 1500)),
           (16000, 512, 400, 160, 40, 1601, (1601, 1600, 1599, 801)),       # hop % 4 == 0, win < n_fft, lengths around a frame boundary
           (22050, 1024, 1024, 256, 80, 1025, (1025,)),
           (16000, 255, 255, 85, 20, 850, (850, 400))]                      # odd n_fft, hop divides N, hop % 4 != 0


@pytest.mark.parametrize("fs,n_fft,win,hop,n_mels,N,lengths", CONFIGS)
def test_logmel_configuration(fs, n_fft, win, hop, n_mels, N, lengths):
    from a3t_amd import _lib
    from a3t_amd.features import LogMelFbank
    lib = _lib.load()
    B = len(lengths)
    g = torch.Generator().manual_seed(n_fft + hop)
    wav = 0.1 * torch.randn(B, N, generator=g)
    lens = torch.tensor(lengths)
    wav[torch.arange(N)[None, :] >= lens[:, None]] = 0.0
    c = types.SimpleNamespace(fs=fs, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, fmin=80, fmax=7600)
    ref, rlens = O.logmel_fbank(wav.double(), lens, c)
    fe = LogMelFbank(fs=fs, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, fmin=80, fmax=7600, device=DEV)
    got, olens = fe(wav, lens)
    torch.cuda.synchronize()
    assert "gemm_f32_kernel<true, true," in lib.a3t_gemm_last_kernel().decode()
    Fr = 1 + (N + 2 * (n_fft // 2) - n_fft) // hop
    assert ref.shape == (B, Fr, n_mels) and tuple(got.shape) == (B, Fr, n_mels) and got.dtype == torch.float32
    assert torch.equal(olens.cpu(), rlens)
    got = got.cpu()
    for b in range(B):
        assert torch.equal(got[b, int(rlens[b]):], torch.zeros(Fr - int(rlens[b]), n_mels)), b
    err = float((got.double() - ref).abs().max())
    print(f"log-mel {fs}/{n_fft}/{win}/{hop}: max |err| {err:.3e}, min log-mel {float(ref[ref != 0].min()):.2f}")
    assert err <= MEL_EPS, err


def test_logmel_stft_runs_on_both_loaders():
    """hop % 4 == 0 frames the padded row for the 16-byte loader, any other hop for the scalar one"""
    from a3t_amd import ops
    from a3t_amd._lib import F32
    for hop, vec in ((160, "true"), (85, "false")):
        xp, basis, S = torch.zeros(1, 2048), torch.zeros(34, 256), torch.zeros(8, 34)
        assert ops.gemm_plan(xp, basis, S, 8, 34, 256, hop, 1, 256, 1, 34, batch=1, a_bs=(2048, 0), c_bs=(8 * 34, 0), compute=F32) == \
            f"gemm_f32_kernel<true, true, {vec}>"


@pytest.mark.parametrize("N,pad,ld", [(10, 4, 18), (10, 4, 24), (7, 6, 20), (1000, 127, 1256)])
def test_reflect_pad_against_index_arithmetic(N, pad, ld):
    from a3t_amd import _lib, ops
    B = 3
    x = torch.arange(B * N, dtype=torch.float32).view(B, N) + 1.0
    out = torch.full((B, ld), -7.0, device=DEV)
    ops.reflect_pad(x.to(DEV), out, pad)
    exp = torch.zeros(B, ld)
    for j in range(N + 2 * pad):
        s = abs(j - pad)
        exp[:, j] = x[:, s if s < N else 2 * (N - 1) - s]
    assert torch.equal(out.cpu(), exp)       # the tail behind N + 2 pad is zero
    assert torch.equal(exp[:, :N + 2 * pad], torch.nn.functional.pad(x[:, None], (pad, pad), mode="reflect")[:, 0])
    for bad in (N, N + 3):
        with pytest.raises(_lib.A3TLibraryError):
            ops.reflect_pad(x.to(DEV), torch.empty(B, N + 2 * bad + 4, device=DEV), bad)
    with pytest.raises(_lib.A3TLibraryError):
        ops.reflect_pad(x.to(DEV), torch.empty(B, N + 2 * pad - 1, device=DEV), pad)


@pytest.mark.parametrize("nb,ld", [(129, 132), (128, 128), (5, 8), (257, 260)])
def test_stft_amp_against_index_arithmetic(nb, ld):
    from a3t_amd import ops
    rows = 37
    g = torch.Generator().manual_seed(nb)
    S = torch.randn(rows, 2 * nb, generator=g)
    S[0, :4] = 0.0
    S[0, nb:nb + 4] = 0.0              # |.|^2 below the 1e-10 clamp
    amp = torch.full((rows, ld), -7.0, device=DEV)
    ops.stft_amp(S.to(DEV), amp, nb)
    got = amp.cpu()
    assert torch.equal(got[:, nb:], torch.zeros(rows, ld - nb))          # columns nb .. ld - 1 are zero
    ref = torch.sqrt(torch.clamp(S[:, :nb].double() ** 2 + S[:, nb:].double() ** 2, min=1e-10))
    assert float(((got[:, :nb].double() - ref).abs() / ref).max()) < 4 * 2.0 ** -24      # u = 2^-24: the sum of the two squares carries 2u, its root half of that plus sqrtf's own 1 ulp = 2u
    assert abs(float(got[0, 0]) - 1e-5) < 1e-11
