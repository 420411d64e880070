"""Shared by the output-head tests (test_head_grad_host.py, test_gpu_head_grad.py), the golden maker
(golden/make_head_grad_golden.py) and tools/head_grad_profile.py:

* ``restated_head``: the reference's ``TCN.output`` (model/model.py:322-325,357: PReLU -> GroupNorm(1, 256, eps=1e-5) ->
  weight-normed Conv1d(256 -> 514, 1)) restated in torch in the dtype of its inputs. Float64 autograd through it is the
  truth for the shapes too large to commit (test_head_grad_host.py pins it to the reference's own float64 autograd); float32
  autograd through it on the CPU is what a trainer runs today, and its error is the yardstick.
* ``closed_form``: the backward in closed form, the arithmetic csrc/head_grad.hip implements.
* ``frame_units_y``: tail_grad_cases.frame_units for a gradient of 256 channels; the masks and the parameter gradients
  use tail_grad_cases.frame_units / tensor_units themselves.

Gate (tail_grad_cases.MARGIN = 2): the native error stays within 2 times the yardstick's error on the same case under the
same normalisation. g_y: per (b, frame), in units of 2^-24 of that frame's largest float64 gradient; parameter gradients:
in units of 2^-24 of each tensor's maximum.
"""
import numpy as np
import torch
import torch.nn.functional as F

import tail_grad_cases as tc

CH, MOUT = 256, 514
EPS = 1e-5
MARGIN, UNIT = tc.MARGIN, tc.UNIT
HEAD_PARAMS = ("TCN.output.0.weight", "TCN.output.1.weight", "TCN.output.1.bias", "TCN.output.2.weight_g",
               "TCN.output.2.weight_v", "TCN.output.2.bias")
P_ALPHA, P_GAMMA, P_BETA, P_G, P_V, P_BIAS = HEAD_PARAMS
TILE, W_T = 64, 128        # HG_TILE, HG_W_T (csrc/sepvad_internal.h): frames per GEMM tile and per weight-gradient partial
GOLDEN_ROWS = tuple(range(0, MOUT, 64)) + (MOUT - 1,)   # the rows of weight_v's gradient the golden file keeps


def restated_head(y, p):
    """model/model.py:357 on y [B, 256, T] -> masks_b [B, 514, T]; p: the six parameters by their state_dict names."""
    z = F.group_norm(F.prelu(y, p[P_ALPHA]), 1, p[P_GAMMA], p[P_BETA], eps=EPS)
    return F.conv1d(z, tc.fold(p[P_V], p[P_G]), p[P_BIAS])


def head_params(sd):
    return {k: sd[k] for k in HEAD_PARAMS}


def autograd_grads(y, params, G, dtype):
    """Gradients of <masks_b, G> through restated_head in `dtype`: dict(y=[B, 256, T], masks=the forward's output,
    <parameter name>=...)."""
    c = lambda t: t.detach().to(dtype)  # noqa: E731
    yl = c(y).requires_grad_(True)
    p = {k: c(v).requires_grad_(True) for k, v in params.items()}
    m = restated_head(yl, p)
    (m * c(G)).sum().backward()
    out = dict(y=yl.grad, masks=m.detach())
    out.update({k: v.grad for k, v in p.items()})
    return out


def closed_form(y, params, G):
    """DESIGN.md section 16 in float64: dict(y=..., <parameter name>=...), the weight-norm Jacobian included."""
    y, G = y.double(), G.double()
    p = {k: v.double() for k, v in params.items()}
    alpha, gam, bet = p[P_ALPHA], p[P_GAMMA].view(1, CH, 1), p[P_BETA].view(1, CH, 1)
    v, g = p[P_V], p[P_G]
    W = tc.fold(v, g)[:, :, 0]
    pr = torch.where(y > 0, y, alpha * y)
    mu = pr.mean((1, 2), keepdim=True)
    r = 1.0 / torch.sqrt(pr.var((1, 2), unbiased=False, keepdim=True) + EPS)
    zh = (pr - mu) * r
    z = gam * zh + bet
    dz = torch.einsum("mc,bmt->bct", W, G)
    h = gam * dz
    a1, a2 = h.mean((1, 2), keepdim=True), (h * zh).mean((1, 2), keepdim=True)
    dp = r * (h - a1 - zh * a2)
    dW = torch.einsum("bmt,bct->mc", G, z).unsqueeze(-1)
    norm = v.flatten(1).norm(dim=1).view(-1, 1, 1)
    dot = (dW * v).flatten(1).sum(1).view(-1, 1, 1)
    return {"y": dp * torch.where(y > 0, torch.ones_like(y), alpha.expand_as(y)),
            P_ALPHA: (dp * y * (y <= 0)).sum().view(1), P_GAMMA: (dz * zh).sum((0, 2)), P_BETA: dz.sum((0, 2)),
            P_G: dot / norm, P_V: (g / norm) * (dW - dot * v / (norm * norm)), P_BIAS: G.sum((0, 2))}


def frame_units_y(g, g64):
    """Worst error of a trunk gradient [B, 256, T] in units of 2^-24 of the maximum of |g64| over its (b, frame)'s 256
    channels (an all-zero frame: the absolute error in 2^-24)."""
    g64 = torch.as_tensor(g64, dtype=torch.float64)
    d = (torch.as_tensor(g).double() - g64).abs().amax(1)
    scale = g64.abs().amax(1)
    return float((d / torch.where(scale > 0, scale, torch.ones_like(scale))).max() / UNIT)


def units(name, g, g64):
    """The gate's measure of one gradient: y per (b, frame), the forward's masks per (b, speaker, frame), a parameter
    per tensor."""
    return frame_units_y(g, g64) if name == "y" else tc.frame_units(g, g64) if name == "masks" else tc.tensor_units(g, g64)


def seeded_case(B, T, seed, y_scale=1.5):
    """(y [B, 256, T], G [B, 514, T]) float32, seeded; y has both signs, so both PReLU branches are taken."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    return y_scale * f(B, CH, T) + 0.25, f(B, MOUT, T)
