"""Shared by the tail-backward tests (test_tail_grad_host.py, test_gpu_tail_grad.py), the golden maker
(golden/make_tail_grad_golden.py) and tools/tail_grad_profile.py:

* ``restated_tail``: the reference's tail (model/model.py:421-441 and the VAD head, :153-179) restated in torch in the
  dtype of its inputs. Float64 autograd through it is the truth the GPU gradients are gated against for shapes too large
  to commit (test_tail_grad_host.py pins it to the reference's own float64 autograd); in float32, in the reference's
  noisy-phase formulation, it is what a trainer runs today, and its error is the yardstick.
* ``closed_form_masks``: the separation path's gradient at the pre-sigmoid masks in closed form,
  the arithmetic csrc/tail_grad.hip implements.
* ``frame_units`` / ``tensor_units``: the gates' error measures, in units of 2^-24.

Gate: the native gradient's error must stay within MARGIN = 2 times the yardstick's error on the same case, under the
same normalisation. The factor covers a different summation order in the 512-point transform and nothing more.
"""
import numpy as np
import torch
import torch.nn.functional as F

NFFT, HOP, NBIN = 512, 256, 257
MARGIN = 2.0
UNIT = 2.0 ** -24
VAD_PARAMS = ("vad.common.conv1_1.weight_g", "vad.common.conv1_1.weight_v", "vad.common.conv1_1.bias",
              "vad.common.relu_1.weight", "vad.common.BN_1.weight", "vad.common.BN_1.bias",
              "vad.output_layer_vad.weight_g", "vad.output_layer_vad.weight_v", "vad.output_layer_vad.bias")
MODES = ("sep", "vad", "both")


def fold(v, g):
    """torch weight_norm (dim 0): w = v g / |v|, the norm over every dimension but the first."""
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))


def vad_head(m, p):
    """model/model.py:173-179 on m [B, 257, T] -> [B, 1, T]; p: the nine parameters by their state_dict names."""
    y = F.conv1d(m, fold(p[VAD_PARAMS[1]], p[VAD_PARAMS[0]]), p[VAD_PARAMS[2]], padding=2)
    y = F.group_norm(F.prelu(y, p[VAD_PARAMS[3]]), 1, p[VAD_PARAMS[4]], p[VAD_PARAMS[5]], eps=1e-8)
    return torch.sigmoid(F.conv1d(y, fold(p[VAD_PARAMS[7]], p[VAD_PARAMS[6]]), p[VAD_PARAMS[8]], padding=1))


def stft_out(x, window):
    """model/model.py:408,410: the spec_output STFT with the DC row zeroed."""
    X = torch.stft(x, NFFT, HOP, NFFT, window=window, center=True, pad_mode="reflect", return_complex=True)
    return torch.cat([torch.zeros_like(X[:, :1]), X[:, 1:]], dim=1)


def restated_tail(x, masks_b, p, win_out, win_inv, noisy_phase=True, with_vad=True):
    """-> (sep [B, 2, N], vad [B, 2, T] or None). x and the windows carry the dtype; masks_b [B, 514, T]."""
    B, N = x.shape
    X = stft_out(x, win_out)
    T = X.shape[-1]
    m = masks_b.reshape(B, 2, NBIN, T)
    vad = torch.cat([vad_head(m[:, s], p) for s in range(2)], dim=1) if with_vad else None
    mask = torch.sigmoid(m)
    if noisy_phase:  # model/model.py:431-437
        est = (X.abs().unsqueeze(1) * mask).to(X.dtype) * torch.exp(1j * X.angle()).unsqueeze(1)
    else:
        est = X.unsqueeze(1) * mask
    sep = torch.istft(est.reshape(2 * B, NBIN, T), NFFT, HOP, NFFT, window=win_inv, center=True, length=N)
    return sep.reshape(B, 2, N), vad


def autograd_grads(x, masks_b, params, win, g_sep, g_vad, dtype, noisy_phase=True):
    """Gradients of <sep, g_sep> + <vad, g_vad> (a None term is left out) through restated_tail in `dtype`:
    dict(masks=[B, 514, T], <parameter name>=...), parameter gradients only with g_vad. `win`: the float32 window
    buffer, whose values every precision uses (as a loaded checkpoint would)."""
    c = lambda t: t.detach().to(dtype)  # noqa: E731
    m = c(masks_b).requires_grad_(True)
    p = {k: c(v).requires_grad_(True) for k, v in params.items()} if params else None
    sep, vad = restated_tail(c(x), m, p, c(win), c(win), noisy_phase, with_vad=g_vad is not None)
    loss = 0
    if g_sep is not None:
        loss = loss + (sep * c(g_sep)).sum()
    if g_vad is not None:
        loss = loss + (vad * c(g_vad)).sum()
    loss.backward()
    out = dict(masks=m.grad)
    if g_vad is not None:
        out.update({k: v.grad for k, v in p.items()})
    return out


def closed_form_masks(x, masks_b, g_sep, win, dtype):
    """The separation gradient at the pre-sigmoid masks, DESIGN.md section 15: g~ = g_sep / env on the centre-padded
    axis, frames u_f = w g~[256 f : 256 f + 512], G_f = (c_k / 512) rfft(u_f), g_m = Re X Re G + Im X Im G, times
    m (1 - m)."""
    x, g_sep, w = x.to(dtype), g_sep.to(dtype), win.to(dtype)
    B, N = x.shape
    X = stft_out(x, w)
    T = X.shape[-1]
    L = HOP * (T + 1)
    env = torch.zeros(L, dtype=dtype)
    for f in range(T):
        env[HOP * f:HOP * f + NFFT] += w * w
    gt = torch.zeros(B, 2, L, dtype=dtype)
    gt[:, :, HOP:HOP + N] = g_sep / env[HOP:HOP + N]
    u = gt.unfold(2, NFFT, HOP) * w                      # [B, 2, T, 512]
    ck = torch.full((NBIN,), 2.0, dtype=dtype)
    ck[0] = ck[-1] = 1.0
    G = torch.fft.rfft(u, dim=-1).transpose(2, 3) * (ck / NFFT).view(1, 1, NBIN, 1)   # [B, 2, 257, T]
    m = torch.sigmoid(masks_b.to(dtype).reshape(B, 2, NBIN, T))
    g = (X.real.unsqueeze(1) * G.real + X.imag.unsqueeze(1) * G.imag) * m * (1 - m)
    return g.reshape(B, 2 * NBIN, T)


def frame_units(g, g64):
    """Worst error of a masks gradient [B, 514, T] in units of 2^-24 of the maximum of |g64| over its (b, speaker, frame)'s
    257 bins (an all-zero frame: the absolute error in 2^-24)."""
    g64 = torch.as_tensor(g64, dtype=torch.float64)
    B, _, T = g64.shape
    d = (torch.as_tensor(g).double().reshape(B, 2, NBIN, T) - g64.reshape(B, 2, NBIN, T)).abs().amax(2)
    scale = g64.reshape(B, 2, NBIN, T).abs().amax(2)
    return float((d / torch.where(scale > 0, scale, torch.ones_like(scale))).max() / UNIT)


def tensor_units(g, g64):
    """Worst error of a parameter gradient in units of 2^-24 of the tensor's maximum."""
    g64 = torch.as_tensor(g64, dtype=torch.float64)
    scale = float(g64.abs().max())
    return float((torch.as_tensor(g).double().reshape(g64.shape) - g64).abs().max() / (scale if scale > 0 else 1.0) / UNIT)


def split_modes(g_sep, g_vad, mode):
    return (g_sep if mode != "vad" else None), (g_vad if mode != "sep" else None)


def seeded_case(B, N, seed, mask_scale=2.0):
    """Inputs of a case too large to commit: (x [B, N], masks_b [B, 514, T], g_sep [B, 2, N], g_vad [B, 2, T]),
    float32, seeded."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = 1 + N // HOP
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    return 0.1 * f(B, N), mask_scale * f(B, 2 * NBIN, T), f(B, 2, N), f(B, 2, T)
