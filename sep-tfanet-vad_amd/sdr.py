"""Pairwise negative SDR losses on the device (reference ``model/sdr.py:7-86``).

``PairwiseNegSDR(sdr_type, zero_mean, take_log, EPS)`` and the three instances the configs name through
``loss_separation.loss_func`` (``pairwise_neg_sisdr``, ``pairwise_neg_sdsdr``, ``pairwise_neg_snr``): est_targets,
targets ``[B, 2, N]`` -> ``[B, 2, 2]``, element ``(b, i, j)`` the loss of estimate i against target j. The arithmetic is
``sepvad_eval_separation`` (csrc/eval.hip): double moments, the reference's EPS placement. Forward-only, two sources.

The reference's other loss classes (``SingleSrcNegSDR``, ``MultiSrcNegSDR``, the emphasized and clipped variants) are
not provided: ``test.py`` builds its criterion from the pairwise ones only.
"""
from __future__ import annotations

from torch import nn

from . import evaluate as _evaluate


class PairwiseNegSDR(nn.Module):
    """model/sdr.py:7-86."""

    def __init__(self, sdr_type, zero_mean=True, take_log=True, EPS=1e-8):
        super().__init__()
        assert sdr_type in ["snr", "sisdr", "sdsdr"]
        self.sdr_type = sdr_type
        self.zero_mean = zero_mean
        self.take_log = take_log
        self.EPS = EPS

    def check(self, est_targets, targets):
        """The reference's shape check (sdr.py:49-52), then what the native path adds: two sources."""
        if targets.size() != est_targets.size() or targets.ndim != 3:
            raise TypeError(
                f"Inputs must be of shape [batch, n_src, time], got {targets.size()} and {est_targets.size()} instead"
            )
        if targets.shape[1] != 2:
            raise NotImplementedError(f"native PairwiseNegSDR: built for 2 sources, got n_src = {targets.shape[1]}")

    def evaluate(self, est_targets, targets, mix=None, sheet=False):
        """The whole result of sepvad_eval_separation for this loss (PITLossWrapper reads pw, min_loss and perm
        from one call)."""
        self.check(est_targets, targets)
        return _evaluate.eval_separation(est_targets, targets, mix, self.sdr_type, self.zero_mean, self.take_log,
                                         self.EPS, sheet=sheet)

    def forward(self, est_targets, targets):
        return self.evaluate(est_targets, targets)["pw"]


pairwise_neg_sisdr = PairwiseNegSDR("sisdr")
pairwise_neg_sdsdr = PairwiseNegSDR("sdsdr")
pairwise_neg_snr = PairwiseNegSDR("snr")
