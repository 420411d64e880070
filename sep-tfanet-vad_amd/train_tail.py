"""The forward's tail with a backward: gradients at the masks and at the VAD head (``model/model.py:421-461``).

``train_criterion.CombinedLoss`` yields ``d loss / d sep`` and ``d loss / d vad``; this module takes them through
``torch.istft``, the mask product, the sigmoid and the VAD head (``model/model.py:153-179``) to ``masks_b`` -- the trunk's
output, where the next stages of the model's backward start -- and to the nine parameters of the VAD head::

    tail = train_tail.TrainableTail(net)          # net: SeparationModel on the device
    sep, vad, masks_b = tail(x)                   # the native forward, once; masks_b is a leaf that requires grad
    loss, *_ = criterion(sep, tgt, vad, labels); loss.backward()
    masks_b.grad, net.vad.common.conv1_1.weight_v.grad, ...
    sep, vad = tail.from_masks(x, masks_b)        # the same node on the caller's pre-sigmoid masks

``tail(x)`` returns the forward's own ``sep`` and ``vad`` tensors (the same bits as ``net(x)``) and builds the node
around them without running anything again. ``from_masks`` computes them from given masks through launches the library
already has (``sepvad_tail_forward``). The backward is ``sepvad_tail_backward`` (csrc/tail_grad.hip). The
node keeps ``x`` and the masks and nothing else: X and the VAD head's forward are recomputed in the backward, so nothing
depends on a forward's workspace surviving. ``est`` is not differentiable, there is no gradient with respect to ``x``,
and a double backward is refused. The forward runs on the weights the native handle was built from: after an
optimizer step call ``net.refresh_native()`` before the next forward, as for any in-place edit of the parameters
(the backward itself reads the module's parameters, folded in double).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import native as _native

NBIN = 257
_NW1 = 4 * NBIN * 5
VAD_PARAMS = ("common.conv1_1.weight_g", "common.conv1_1.weight_v", "common.conv1_1.bias", "common.relu_1.weight",
              "common.BN_1.weight", "common.BN_1.bias", "output_layer_vad.weight_g", "output_layer_vad.weight_v",
              "output_layer_vad.bias")


def _fold(v, g):
    """w = v g / |v| in float64 (torch weight_norm, dim 0)."""
    v64 = v.detach().double()
    return v64 * (g.detach().double() / v64.flatten(1).norm(dim=1).view(-1, 1, 1))


def _vad_weights(params):
    """The nine parameters as sepvad_tail_backward's vadw: float64, folded, in gpar's layout."""
    w1g, w1v, b1, a, gam, bet, w2g, w2v, b2 = params
    parts = (_fold(w1v, w1g), _fold(w2v, w2g), b2, gam, bet, a, b1)
    return torch.cat([p.detach().double().reshape(-1) for p in parts])


def _wn_grads(g_w, v, g):
    """The weight-norm fold w = v g / |v| (norm over every dimension but the first) backwards, in float64:
    (g_g, g_v) from the folded gradient g_w."""
    v64, g64 = v.detach().double(), g.detach().double()
    norm = v64.flatten(1).norm(dim=1).view(-1, 1, 1)
    dot = (g_w * v64).flatten(1).sum(1).view(-1, 1, 1)
    return dot / norm, (g64 / norm) * (g_w - dot * v64 / (norm * norm))


class _Tail(torch.autograd.Function):
    """(masks_b, nine VAD parameters | none, state) -> (sep, vad | nothing). state: dict(handle, x, ldx, outputs)."""

    @staticmethod
    def forward(ctx, masks_b, state, *params):
        h, x = state["handle"], state["x"]
        lib, dev = _native.load_library(), x.device
        B, N = x.shape
        T = 1 + N // 256
        has_vad = bool(h.cfg["final_vad"])
        m32 = masks_b.detach().to(torch.float32).contiguous()
        if state.get("outputs") is not None:  # tail(x): the native forward's own tensors
            sep, vad = state["outputs"]
        else:
            mf = _native.frame_major_masks(m32)
            sep = torch.empty(B, 2, N, device=dev, dtype=torch.float32)
            vad = torch.empty(B, 2, T, device=dev, dtype=torch.float32) if has_vad else None
            buf, nbytes = _native.scratch_for("sepvad_tail_scratch_bytes", dev, B, N)
            _native.check(lib.sepvad_tail_forward(h.raw, _native.ptr(x), state["ldx"], _native.ptr(mf), B, N,
                                                  _native.ptr(buf), nbytes, _native.ptr(sep), _native.ptr(vad),
                                                  _native.stream_ptr(dev)), "sepvad_tail_forward")
        ctx.handle, ctx.ldx, ctx.has_vad = h, state["ldx"], has_vad
        ctx.meta = (masks_b.dtype, masks_b.shape)
        ctx.set_materialize_grads(False)  # an unused output's gradient stays None: zero, nothing computed for it
        ctx.save_for_backward(x, m32, *params)
        return (sep, vad) if has_vad else (sep,)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sep, g_vad=None):
        x, m32, *params = ctx.saved_tensors
        h, lib, dev = ctx.handle, _native.load_library(), x.device
        B, N = x.shape
        T = 1 + N // 256
        want_m = ctx.needs_input_grad[0]
        want_p = ctx.has_vad and g_vad is not None and any(ctx.needs_input_grad[2:])
        none = (None,) * len(params)
        if (g_sep is None and g_vad is None) or not (want_m or want_p):
            return (None, None) + none
        if g_sep is not None and g_sep.dtype != torch.float32:
            g_sep = g_sep.to(torch.float32)
        if g_vad is not None and g_vad.dtype != torch.float32:
            g_vad = g_vad.to(torch.float32)
        _native.require_device("train_tail backward", x, g_sep, g_vad)
        g_masks = torch.empty(B, 2 * NBIN, T, device=dev, dtype=torch.float32) if want_m else None
        gpar = torch.empty(_NW1 + 26, device=dev, dtype=torch.float64) if want_p else None
        buf, nbytes = _native.scratch_for("sepvad_tail_scratch_bytes", dev, B, N)
        vadw = _vad_weights(params) if g_vad is not None else None
        ss = g_sep.stride() if g_sep is not None else (0, 0, 0)
        sv = g_vad.stride() if g_vad is not None else (0, 0, 0)
        rc = lib.sepvad_tail_backward(h.raw, _native.ptr(x), ctx.ldx, _native.ptr(m32), B, N, _native.ptr(g_sep), *ss,
                                      _native.ptr(g_vad), *sv, _native.ptr(vadw), _native.ptr(buf), nbytes,
                                      _native.ptr(g_masks), _native.ptr(gpar), _native.stream_ptr(dev))
        _native.check(rc, "sepvad_tail_backward")
        if g_masks is not None:
            g_masks = g_masks.to(ctx.meta[0]).reshape(ctx.meta[1])
        if not want_p:
            return (g_masks, None) + none
        # gpar: conv1_1 weight (folded) | conv 4 -> 1 weight (folded) | its bias | BN_1 weight, bias | PReLU | conv1_1 bias
        w1g, w1v, b1, a, gam, bet, w2g, w2v, b2 = params
        s = gpar[_NW1:]
        g_w1g, g_w1v = _wn_grads(gpar[:_NW1].view(4, NBIN, 5), w1v, w1g)
        g_w2g, g_w2v = _wn_grads(s[0:12].view(1, 4, 3), w2v, w2g)
        grads = (g_w1g, g_w1v, s[22:26], s[21:22], s[13:17], s[17:21], g_w2g, g_w2v, s[12:13])
        grads = tuple(g.to(p.dtype).reshape(p.shape) if need else None
                      for g, p, need in zip(grads, params, ctx.needs_input_grad[2:]))
        return (g_masks, None) + grads


class TrainableTail:
    """The tail of ``net`` (a ``SeparationModel`` on a ROCm device) as an autograd node."""

    def __init__(self, net):
        if net.final_vad and net.final_vad_masked_speakers:
            raise NotImplementedError("train_tail: final_vad_masked_speakers=True has no backward (the VAD head on the "
                                      "masked spectrum is out of scope)")
        if net.num_spk != 2:
            raise NotImplementedError("train_tail: two speakers only")
        self.net = net

    def _params(self):
        if not self.net.final_vad:
            return ()
        named = dict(self.net.vad.named_parameters())
        return tuple(named[k] for k in VAD_PARAMS)

    def _state(self, x):
        what = "train_tail"
        if x.ndim != 2:
            raise ValueError(f"{what}: expected x [B, N], got {tuple(x.shape)}")
        _native.require_device(what, x)
        if x.requires_grad:
            raise RuntimeError(f"{what}: there is no gradient with respect to x; detach it")
        x, ldx = _native.rows2(x)
        return dict(handle=self.net.native_handle(x.device), x=x, ldx=ldx)

    def _apply(self, masks_b, state):
        out = _Tail.apply(masks_b, state, *self._params())
        return (out[0], out[1]) if self.net.final_vad else (out[0], 0)  # the int 0 of model/model.py:427

    def __call__(self, x, inference_kw=None):
        """-> (sep, vad, masks_b): ``net(x)``'s own sep and vad (the int 0 without final_vad) and the forward's masks_b
        side output [B, 514, T] as a leaf that requires grad."""
        if inference_kw:
            raise ValueError("train_tail: a non-empty inference_kw selects the thresholded inference branch "
                             "(model/model.py:444-457), which has no gradient")
        state = self._state(x)
        with torch.no_grad():
            sep, vad, _est = self.net(state["x"])
            masks_b = self.net.masks_b
        masks_b = masks_b.detach().requires_grad_(True)
        state["outputs"] = (sep, vad if self.net.final_vad else None)
        return self._apply(masks_b, state) + (masks_b,)

    def from_masks(self, x, masks_b):
        """-> (sep, vad) from the caller's pre-sigmoid masks [B, 514, T] (a leaf or the output of a torch head)."""
        state = self._state(x)
        B, N = state["x"].shape
        if tuple(masks_b.shape) != (B, 2 * NBIN, 1 + N // 256):
            raise ValueError(f"train_tail: expected masks_b {(B, 2 * NBIN, 1 + N // 256)}, got {tuple(masks_b.shape)}")
        _native.require_device("train_tail", state["x"], masks_b)
        return self._apply(masks_b, state)
