"""The reference's training criterion on the device, with a backward (``trainer/trainer.py:57-63``).

``train.py:13-14,58-65`` builds ``CombinedLoss(PITLossWrapper(pairwise_neg_sisdr, "pw_mtx"),
PITLossWrapper(BinaryCrossEntropyLoss_Mean(), "pw_pt"), config["combined_loss"])`` from ``model.combined_loss`` and the
trainer calls ``loss.backward()`` on a weighted sum of its first two outputs. This module carries the names ``train.py``
imports from ``model.combined_loss``; its ``CombinedLoss`` is differentiable with respect to ``pred_separation`` and
``pred_vad``. ``combined_loss.CombinedLoss`` and the classes it is built from stay forward-only.

The forward is ``sepvad_eval_separation`` and ``sepvad_eval_vad`` as ``combined_loss`` runs them (the same bits), plus
``sepvad_criterion_coef``: six doubles per estimate row, all the backward keeps beside the inputs. The backward is
``sepvad_criterion_backward`` (csrc/criterion.hip): one pass over the rows, the upstream gradients read on the device.
Nothing is synchronised and nothing is read on the host, in either direction. Two sources, ROCm tensors; no CPU path.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import evaluate as _evaluate
from . import native as _native
from .evaluate import BinaryCrossEntropyLoss_Mean  # noqa: F401  (train.py:62 looks it up here)
from .metrics import calc_sisdr, calc_sisdr_loss  # noqa: F401
from .pit import PITLossWrapper, reorder_source_mse  # noqa: F401  (trainer.py:74)
from .sdr import PairwiseNegSDR

CRIT_COEF = 6  # SEPVAD_CRIT_COEF (include/sepvad.h)


class _Criterion(torch.autograd.Function):
    """(pred_separation, target_separation, pred_vad | None, target_vad | None, settings) ->
    (separation_loss, vad_loss | None, batch_indices)."""

    @staticmethod
    def forward(ctx, est, tgt, vad, labels, sdr_type, zero_mean, take_log, eps):
        lib = _native.load_library()
        dev = est.device
        ctx.est_meta, ctx.vad_meta = (est.dtype, est.shape), None
        est, eld = _native.rows3(est.detach())
        tgt, tld = _native.rows3(tgt)
        B, _, N = est.shape
        r = _evaluate.eval_separation(est, tgt, None, sdr_type, zero_mean, take_log, eps, sheet=False)
        perm, scratch = r["perm"], r["scratch"]  # the moments' partials are in the buffer that call used
        coef = torch.empty(B, 2, CRIT_COEF, dtype=torch.float64, device=dev)
        rc = lib.sepvad_criterion_coef(_native.ptr(est), eld, _native.ptr(tgt), tld, B, N,
                                       _evaluate.SDR_TYPES[sdr_type], int(bool(zero_mean)), int(bool(take_log)),
                                       float(eps), _native.ptr(scratch), scratch.numel(), _native.ptr(perm),
                                       _native.ptr(coef), _native.stream_ptr(dev))
        _native.check(rc, "sepvad_criterion_coef")
        vad_loss = v32 = lab = None
        if vad is not None:
            ctx.vad_meta = (vad.dtype, vad.shape)
            v = _evaluate.eval_vad(vad.detach(), labels, perm)  # labels equal to 2 become 1 in place, as the reference's
            vad_loss, lab = v["bce_mean"], v["labels"]
            v32 = vad.detach().to(torch.float32).contiguous()
        ctx.save_for_backward(est, tgt, coef, perm, v32, lab)
        ctx.mark_non_differentiable(perm)
        return r["means"][0], vad_loss, perm

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sep, g_vad, _g_perm):
        lib = _native.load_library()
        est, tgt, coef, perm, vad, lab = ctx.saved_tensors
        dev = est.device
        B, _, N = est.shape
        want_sep = ctx.needs_input_grad[0]
        want_vad = vad is not None and ctx.needs_input_grad[2]
        grad_est = grad_vad = None
        T = 0
        if want_sep:
            g_sep = g_sep.to(torch.float32).contiguous()
            grad_est = torch.empty(B, 2, N, dtype=torch.float32, device=dev)
        if want_vad:
            g_vad = g_vad.to(torch.float32).contiguous()
            T = vad.shape[2]
            grad_vad = torch.empty(B, 2, T, dtype=torch.float32, device=dev)
        if want_sep or want_vad:
            none = None
            rc = lib.sepvad_criterion_backward(
                B, _native.ptr(est if want_sep else none), est.stride(1), _native.ptr(tgt), tgt.stride(1), N,
                _native.ptr(coef), _native.ptr(g_sep if want_sep else none), _native.ptr(grad_est), N,
                _native.ptr(vad if want_vad else none), _native.ptr(lab), _native.ptr(perm), T,
                _native.ptr(g_vad if want_vad else none), _native.ptr(grad_vad), _native.stream_ptr(dev))
            _native.check(rc, "sepvad_criterion_backward")
        if grad_est is not None:
            grad_est = grad_est.to(ctx.est_meta[0]).reshape(ctx.est_meta[1])
        if grad_vad is not None:
            grad_vad = grad_vad.to(ctx.vad_meta[0]).reshape(ctx.vad_meta[1])
        return grad_est, None, grad_vad, None, None, None, None, None


def _separation_settings(criterion_separation):
    """(sdr_type, zero_mean, take_log, EPS) of PITLossWrapper(sdr.PairwiseNegSDR(...), "pw_mtx"); anything else is not
    built."""
    c = criterion_separation
    if (isinstance(c, PITLossWrapper) and c.pit_from == "pw_mtx" and (c.perm_reduce is None or c.perm_reduce is False)
            and isinstance(c.loss_func, PairwiseNegSDR)):
        f = c.loss_func
        return f.sdr_type, bool(f.zero_mean), bool(f.take_log), float(f.EPS)
    raise NotImplementedError("train_criterion.CombinedLoss: criterion_separation must be this package's "
                              "PITLossWrapper(sdr.PairwiseNegSDR(...), 'pw_mtx') without perm_reduce")


def _check_vad_criterion(criterion_vad):
    c = criterion_vad
    if not (isinstance(c, PITLossWrapper) and c.pit_from == "pw_pt" and (c.perm_reduce is None or c.perm_reduce is False)
            and isinstance(c.loss_func, BinaryCrossEntropyLoss_Mean)):
        raise NotImplementedError("train_criterion.CombinedLoss: criterion_vad must be this package's "
                                  "PITLossWrapper(BinaryCrossEntropyLoss_Mean(), 'pw_pt') without perm_reduce")


class CombinedLoss(nn.Module):
    """model/combined_loss.py:80-118 with a backward. ``weights`` is the config's ``combined_loss`` dict (train.py:65);
    it is read on every call, because the trainer decays ``weight_vad_loss`` in place."""

    def __init__(self, criterion_separation, criterion_vad, weights):
        super().__init__()
        self._settings = _separation_settings(criterion_separation)
        _check_vad_criterion(criterion_vad)
        self.criterion_separation = criterion_separation
        self.criterion_vad = criterion_vad
        self.bce = BinaryCrossEntropyLoss_Mean()
        self.weights = weights
        self.learn_weight_bool = weights["learn_weight_bool"]
        if self.learn_weight_bool:
            self.learn_weight_vadLoss = nn.parameter.Parameter(torch.tensor(0.5))
            self.learn_weight_separationLoss = nn.parameter.Parameter(torch.tensor(0.5))

    @staticmethod
    def _learned(loss, w):
        return loss * (1 / (2 * torch.square(w))) + torch.log(1 + torch.square(w))

    def forward(self, pred_separation, target_separation, pred_vad, target_vad):
        """-> (separation_loss, vad_loss, batch_indices_vad, batch_indices_separation); with a falsy
        ``weight_vad_loss`` the middle two are ``torch.tensor(0)``, as in the reference."""
        what = "train_criterion.CombinedLoss"
        with_vad = bool(self.weights["weight_vad_loss"])
        self.criterion_separation.loss_func.check(pred_separation, target_separation)
        if with_vad and (pred_vad.dim() != 3 or pred_vad.shape[1] != 2 or pred_vad.shape != target_vad.shape
                         or pred_vad.shape[0] != pred_separation.shape[0]):
            raise ValueError(f"{what}: expected pred_vad and target_vad of one shape [B, 2, T] with the batch of "
                             f"pred_separation, got {tuple(pred_vad.shape)} and {tuple(target_vad.shape)}")
        if torch.is_grad_enabled() and (target_separation.requires_grad or (with_vad and target_vad.requires_grad)):
            raise RuntimeError(f"{what}: differentiable with respect to pred_separation and pred_vad only, but a "
                               "target requires grad; detach it")
        _native.require_device(what, pred_separation, target_separation, *((pred_vad, target_vad) if with_vad else ()))
        sdr_type, zero_mean, take_log, eps = self._settings
        separation_loss, vad_loss, batch_indices_separation = _Criterion.apply(
            pred_separation, target_separation, pred_vad if with_vad else None, target_vad if with_vad else None,
            sdr_type, zero_mean, take_log, eps)
        if self.learn_weight_bool:
            separation_loss = self._learned(separation_loss, self.learn_weight_separationLoss)
        if with_vad:
            if self.learn_weight_bool:
                vad_loss = self._learned(vad_loss, self.learn_weight_vadLoss)
            batch_indices_vad = batch_indices_separation
        else:
            vad_loss, batch_indices_vad = torch.tensor(0), torch.tensor(0)
        return separation_loss, vad_loss, batch_indices_vad, batch_indices_separation
