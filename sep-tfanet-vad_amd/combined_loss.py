"""The reference's evaluation criterion on the device (``model/combined_loss.py:80-138``).

``test.py:13-17`` imports ``CombinedLoss``, ``reorder_source_mse``, ``calc_sisdr`` and ``calc_sisdr_loss`` from
``model.combined_loss`` and looks ``loss_vad.loss_func`` up in it (``test.py:59``); this module carries the same
names, so pointing that import at it is the whole swap. Forward-only.
"""
from __future__ import annotations

import torch
from torch import nn

from . import evaluate as _evaluate
from .evaluate import BinaryCrossEntropyLoss_Mean  # noqa: F401  (test.py:59 looks it up here)
from .metrics import calc_sisdr, calc_sisdr_loss  # noqa: F401  (test.py:16-17)
from .pit import reorder_source_mse  # noqa: F401  (test.py:15)


class CombinedLoss(nn.Module):
    """model/combined_loss.py:80-118. ``weights`` is the config's ``combined_loss`` dict; it may also be given as
    keyword arguments, which is how test.py:64 passes it."""

    def __init__(self, criterion_separation, criterion_vad, weights=None, **kwargs):
        super().__init__()
        if weights is None:
            weights = kwargs
        elif kwargs:
            raise TypeError(f"CombinedLoss: unexpected arguments {sorted(kwargs)}")
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
        _evaluate.refuse_grad("CombinedLoss", pred_separation, target_separation, pred_vad, target_vad)
        separation_loss, batch_indices_separation = self.criterion_separation(pred_separation, target_separation,
                                                                              return_incides=True)
        if self.learn_weight_bool:
            separation_loss = self._learned(separation_loss, self.learn_weight_separationLoss.detach())
        if self.weights["weight_vad_loss"]:
            vad_loss = self.bce(pred_vad, target_vad, batch_indices_separation)
            if self.learn_weight_bool:
                vad_loss = self._learned(vad_loss, self.learn_weight_vadLoss.detach())
            batch_indices_vad = batch_indices_separation
        else:
            vad_loss, batch_indices_vad = torch.tensor(0), torch.tensor(0)
        return separation_loss, vad_loss, batch_indices_vad, batch_indices_separation
