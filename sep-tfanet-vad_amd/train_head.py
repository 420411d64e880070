"""The output head with a backward: from the trunk output to ``masks_b`` (``TCN.output``, ``model/model.py:322-325,357``).

``train_tail.TrainableTail`` ends at ``masks_b.grad``; this module is the stage behind it, ``PReLU -> GroupNorm(1, 256,
eps=1e-5) -> weight-normed Conv1d(256 -> 514, 1)``, as an autograd node whose forward and backward are native
(``sepvad_head_forward``, ``sepvad_head_backward``; csrc/head_grad.hip)::

    head = train_head.TrainableHead(net)          # net: SeparationModel on the device
    tail = train_tail.TrainableTail(net)
    masks_b = head.from_trunk(y)                  # y [B, 256, T]: the trunk output (a leaf, or a torch trunk's output)
    sep, vad = tail.from_masks(x, masks_b)
    loss, *_ = criterion(sep, tgt, vad, labels); loss.backward()
    y.grad, net.TCN.output[2].weight_v.grad, ..., net.vad.common.conv1_1.weight_v.grad, ...

The gradients go to ``y`` and to the head's six parameters (132 611 after the weight-norm fold): the whole mask head can
be fine-tuned on a frozen separator next to the VAD head, and a torch trunk under training receives its gradient from
native code. The node keeps ``y`` and nothing else; the backward recomputes the head's intermediates, so nothing depends
on a forward's workspace. It reads the module's parameters at the time of the call, folded in double, so an optimizer
step needs no ``net.refresh_native()`` for this stage (the tail's forward does: see train_tail). There is no double
backward. The library has no native source of the trunk output yet: ``y`` comes from the caller.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import native as _native
from .train_tail import _fold, _wn_grads

CH, MOUT = 256, 514
_NW = MOUT * CH
HEAD_NPAR = _NW + MOUT + 2 * CH + 1  # SEPVAD_HEAD_NPAR
HEAD_PARAMS = ("TCN.output.0.weight", "TCN.output.1.weight", "TCN.output.1.bias", "TCN.output.2.weight_g",
               "TCN.output.2.weight_v", "TCN.output.2.bias")


def _head_weights(params):
    """The six parameters as hpar: float64, the weight folded, in gpar's layout."""
    alpha, gam, bet, wg, wv, bias = params
    parts = (_fold(wv, wg), bias, gam, bet, alpha)
    return torch.cat([p.detach().double().reshape(-1) for p in parts])


class _Head(torch.autograd.Function):
    """(y, the six parameters) -> masks_b."""

    @staticmethod
    def forward(ctx, y, *params):
        lib, dev = _native.load_library(), y.device
        B, _, T = y.shape
        y32 = y.detach().to(torch.float32).contiguous()
        masks = torch.empty(B, MOUT, T, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            buf, nbytes = _native.scratch_for("sepvad_head_scratch_bytes", dev, B, T)
            hpar = _head_weights(params)
            _native.check(lib.sepvad_head_forward(_native.ptr(y32), B, T, _native.ptr(hpar), _native.ptr(buf), nbytes,
                                                  _native.ptr(masks), _native.stream_ptr(dev)), "sepvad_head_forward")
        ctx.meta = (y.dtype, y.shape)
        ctx.save_for_backward(y32, *params)
        return masks

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y32, *params = ctx.saved_tensors
        lib, dev = _native.load_library(), y32.device
        B, _, T = y32.shape
        want_y, want_p = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:])
        none = (None,) * len(params)
        if g is None or not (want_y or want_p):
            return (None,) + none
        if g.dtype != torch.float32:
            g = g.to(torch.float32)
        _native.require_device("train_head backward", y32, g)
        g_y = torch.empty(B, CH, T, device=dev, dtype=torch.float32) if want_y else None
        gpar = torch.empty(HEAD_NPAR, device=dev, dtype=torch.float64) if want_p else None
        with torch.cuda.device(dev):
            buf, nbytes = _native.scratch_for("sepvad_head_scratch_bytes", dev, B, T)
            hpar = _head_weights(params)
            rc = lib.sepvad_head_backward(_native.ptr(y32), _native.ptr(g), *g.stride(), B, T, _native.ptr(hpar),
                                          _native.ptr(buf), nbytes, _native.ptr(g_y), _native.ptr(gpar),
                                          _native.stream_ptr(dev))
        _native.check(rc, "sepvad_head_backward")
        if g_y is not None:
            g_y = g_y.to(ctx.meta[0]).reshape(ctx.meta[1])
        if not want_p:
            return (g_y,) + none
        # gpar: conv weight (folded) | its bias | GroupNorm weight, bias | PReLU
        alpha, gam, bet, wg, wv, bias = params
        s = gpar[_NW:]
        g_wg, g_wv = _wn_grads(gpar[:_NW].view(MOUT, CH, 1), wv, wg)
        grads = (s[MOUT + 2 * CH:], s[MOUT:MOUT + CH], s[MOUT + CH:MOUT + 2 * CH], g_wg, g_wv, s[:MOUT])
        grads = tuple(q.to(p.dtype).reshape(p.shape) if need else None
                      for q, p, need in zip(grads, params, ctx.needs_input_grad[1:]))
        return (g_y,) + grads


class TrainableHead:
    """The output head of ``net`` (a ``SeparationModel`` on a ROCm device) as an autograd node."""

    def __init__(self, net):
        if net.num_spk != 2:
            raise NotImplementedError("train_head: two speakers only")
        self.net = net

    def _params(self):
        named = dict(self.net.named_parameters())
        return tuple(named[k] for k in HEAD_PARAMS)

    def from_trunk(self, y):
        """-> masks_b [B, 514, T] from the trunk output y [B, 256, T], T >= 2 (a leaf or the output of a torch trunk)."""
        if y.ndim != 3 or y.shape[1] != CH or y.shape[0] < 1 or y.shape[2] < 2:
            raise ValueError(f"train_head: expected y [B, {CH}, T] with T >= 2, got {tuple(y.shape)}")
        params = self._params()
        _native.require_device("train_head", y, *params)
        return _Head.apply(y, *params)
