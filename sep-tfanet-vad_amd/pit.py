"""Permutation-invariant L1 matching for the streaming wrapper, on the GPU.

Mirrors the part of the reference's ``PITLossWrapper`` (``model/pit_wrapper.py:7-362``) that the
streaming caller uses — ``PITLossWrapper(loss_func=torch.nn.L1Loss(), pit_from="pw_pt")`` called
with ``return_incides=True`` (``model/online_class_unknown_targets.py:87-91``,
``only_inference.py:84-89``) — and ``reorder_source_mse`` (``model/combined_loss.py:63-78``).
The pairwise losses, the permutation choice and the reordering run in ``libsepvad.so``
(``sepvad_pit_l1``, ``sepvad_stream_append``); there is no CPU path.

``PITLossWrapper`` also carries the two criteria ``test.py:49-61`` builds for evaluation, pairwise negative SDR with
``pw_mtx`` and the weighted VAD BCE with ``pw_pt`` (``sepvad_eval_separation``, ``sepvad_eval_vad``; ``evaluate.py``).

Reference semantics kept on purpose: ``nn.L1Loss()`` (reduction="mean") reduces over the batch as
well as the samples, so ``get_pw_losses`` (``pit_wrapper.py:172-177``) fills every batch row with the
same scalar and the chosen permutation is shared by the whole batch.
"""
from __future__ import annotations

import torch
from torch import nn

from . import native as _native

PIT_SCRATCH_BYTES = 16448  # SEPVAD_PIT_SCRATCH_BYTES (include/sepvad.h)

def pit_l1(est: torch.Tensor, ref: torch.Tensor):
    """(min loss [scalar], batch_indices [B, 2] int64, pairwise [2, 2]) on the device."""
    lib = _native.load_library()
    if est.device.type != "cuda" or ref.device != est.device:
        raise RuntimeError("pit_l1: est and ref must be on the same ROCm device")
    if est.shape != ref.shape:
        raise ValueError(f"pit_l1: shape mismatch {tuple(est.shape)} vs {tuple(ref.shape)}")
    est, eld = _native.rows3(est)
    ref, rld = _native.rows3(ref)
    B, _, L = est.shape
    dev = est.device
    perm = torch.empty(B, 2, dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pw = torch.empty(2, 2, dtype=torch.float32, device=dev)
    scratch = _native.scratch(dev, PIT_SCRATCH_BYTES)
    rc = lib.sepvad_pit_l1(_native.ptr(est), eld, _native.ptr(ref), rld, B, L, _native.ptr(scratch),
                           _native.ptr(perm), _native.ptr(loss), _native.ptr(pw), _native.stream_ptr(dev))
    _native.check(rc, "sepvad_pit_l1")
    return loss, perm, pw


def pit_l1_rows(est: torch.Tensor, ref: torch.Tensor):
    """pit_l1 of every row on its own (sepvad_pit_l1_rows): (loss [B], batch_indices [B, 2] int64, pairwise
    [B, 2, 2]); row b has the bits of pit_l1(est[b:b+1], ref[b:b+1]). For independent live streams, whose
    speakers must not be exchanged by what the other streams of the batch prefer."""
    lib = _native.load_library()
    if est.device.type != "cuda" or ref.device != est.device:
        raise RuntimeError("pit_l1_rows: est and ref must be on the same ROCm device")
    if est.shape != ref.shape:
        raise ValueError(f"pit_l1_rows: shape mismatch {tuple(est.shape)} vs {tuple(ref.shape)}")
    est, eld = _native.rows3(est)
    ref, rld = _native.rows3(ref)
    B, _, L = est.shape
    dev = est.device
    scratch, nbytes = _native.scratch_for("sepvad_pit_l1_rows_scratch_bytes", dev, B, L)
    perm = torch.empty(B, 2, dtype=torch.int64, device=dev)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    pw = torch.empty(B, 2, 2, dtype=torch.float32, device=dev)
    rc = lib.sepvad_pit_l1_rows(_native.ptr(est), eld, _native.ptr(ref), rld, B, L, _native.ptr(scratch), nbytes,
                                _native.ptr(perm), _native.ptr(loss), _native.ptr(pw), _native.stream_ptr(dev))
    _native.check(rc, "sepvad_pit_l1_rows")
    return loss, perm, pw


def pit_l1_sharded(est: torch.Tensor, ref: torch.Tensor, total_rows: int, group=None):
    """pit_l1 for a stream batch sharded over the ranks of `group` (total_rows streams over all ranks): the 4
    pairwise L1 sums of this rank's rows (sepvad_pit_l1_sums) are all-reduced (one 32-byte RCCL all-reduce,
    stream-ordered, no host sync), then every rank makes the batch-global choice of the unsharded call
    (sepvad_pit_l1_choose) with count = total_rows * L."""
    import torch.distributed as dist
    lib = _native.load_library()
    est, eld = _native.rows3(est)
    ref, rld = _native.rows3(ref)
    B, _, L = est.shape
    dev = est.device
    buf = torch.empty(4, dtype=torch.float64, device=dev)
    scratch = _native.scratch(dev, PIT_SCRATCH_BYTES)
    rc = lib.sepvad_pit_l1_sums(_native.ptr(est), eld, _native.ptr(ref), rld, B, L, _native.ptr(scratch),
                                _native.ptr(buf), _native.stream_ptr(dev))
    _native.check(rc, "sepvad_pit_l1_sums")
    if dist.get_backend(group) == "gloo":  # (tests on a shared GPU: gloo reduces host tensors)
        hb = buf.cpu()
        dist.all_reduce(hb, op=dist.ReduceOp.SUM, group=group)
        buf.copy_(hb)
    else:
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    count = float(total_rows) * float(L)
    perm = torch.empty(B, 2, dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pw = torch.empty(2, 2, dtype=torch.float32, device=dev)
    rc = lib.sepvad_pit_l1_choose(_native.ptr(buf), count, B, _native.ptr(perm), _native.ptr(loss), _native.ptr(pw),
                                  _native.stream_ptr(dev))
    _native.check(rc, "sepvad_pit_l1_choose")
    return loss, perm, pw


def pit_sisdr_rows(est: torch.Tensor, ref: torch.Tensor):
    """``PITLossWrapper(calc_sisdr_loss, "pw_pt")`` for two sources (``model/pit_wrapper.py:149-177,287-312`` over
    ``model/combined_loss.py:16-60``): ``calc_sisdr_loss`` returns one loss per row, so the pairwise table and the
    permutation are per row. (mean of the rows' min losses [scalar], batch_indices [B, 2] int64, pairwise [B, 2, 2]
    with estimate i against target j at [b, i, j]) on the device: the four pairs of every row are one ``sepvad_si_sdr``
    call through its index arrays, negated; float32 adds and torch.min's first minimum choose per row."""
    from .metrics import _si_sdr_pairs
    if est.device.type != "cuda" or ref.device != est.device:
        raise RuntimeError("pit_sisdr_rows: est and ref must be on the same ROCm device")
    if est.shape != ref.shape or est.dim() != 3 or est.shape[1] != 2:
        raise ValueError(f"pit_sisdr_rows: expected two [B, 2, L] tensors, got {tuple(est.shape)} and {tuple(ref.shape)}")
    B, _, L = est.shape
    P = est.to(torch.float32).reshape(2 * B, L).contiguous()
    Tg = ref.to(torch.float32).reshape(2 * B, L).contiguous()
    r = torch.arange(4 * B, device=est.device, dtype=torch.int32)  # pair r = 4 b + 2 i + j
    pw = -_si_sdr_pairs(P, Tg, (r >> 2) * 2 + ((r >> 1) & 1), (r >> 2) * 2 + (r & 1), True).reshape(B, 2, 2)
    loss_id, loss_sw = (pw[:, 0, 0] + pw[:, 1, 1]) / 2, (pw[:, 1, 0] + pw[:, 0, 1]) / 2
    swap = (loss_sw < loss_id).to(torch.int64)
    perm = torch.stack([swap, 1 - swap], dim=1)
    return torch.minimum(loss_id, loss_sw).mean(), perm, pw


def stream_append(src: torch.Tensor, s0: int, H: int, perm, dst: torch.Tensor, d0: int):
    """dst[b, i, d0:d0+H] = src[b, perm[b, i], s0:s0+H] (perm None = identity), on the device."""
    lib = _native.load_library()
    src, sld = _native.rows3(src)
    if dst.dim() != 3 or dst.stride(2) != 1 or dst.stride(0) != 2 * dst.stride(1):
        raise ValueError("stream_append: dst must be a [B, 2, L] buffer with unit sample stride")
    B = src.shape[0]
    if perm is not None:
        perm = perm.to(device=src.device, dtype=torch.int64).contiguous()
        if tuple(perm.shape) != (B, 2):
            raise ValueError("stream_append: perm must be [B, 2]")
    rc = lib.sepvad_stream_append(_native.ptr(src), sld, int(s0), B, int(H),
                                  _native.ptr(perm) if perm is not None else None,
                                  _native.ptr(dst), dst.stride(1), int(d0), _native.stream_ptr(src.device))
    _native.check(rc, "sepvad_stream_append")


def reorder_source_mse(preds: torch.Tensor, batch_indices: torch.Tensor) -> torch.Tensor:
    """Reference ``model/combined_loss.py:63-78``: out[b] = preds[b][batch_indices[b]] ([B, 2, L])."""
    out = torch.empty(preds.shape[0], 2, preds.shape[-1], dtype=torch.float32, device=preds.device)
    stream_append(preds, 0, preds.shape[-1], batch_indices, out, 0)
    return out


class PITLossWrapper(nn.Module):
    """``PITLossWrapper(loss_func, pit_from)`` (reference ``model/pit_wrapper.py:66-75``).

    Natively supported, for two sources:

    * ``loss_func`` an ``nn.L1Loss`` with reduction "mean", ``pit_from="pw_pt"`` — the criterion the streaming
      wrapper is built with;
    * ``loss_func`` ``calc_sisdr_loss`` (``metrics`` / ``combined_loss``), ``pit_from="pw_pt"`` — ``si_sdr_loss_similarity``
      of ``test.py:102-105``: per-row losses, a permutation per row (``pit_sisdr_rows``);
    * ``loss_func`` a ``sdr.PairwiseNegSDR``, ``pit_from="pw_mtx"`` — ``loss_separation`` of both shipped configs
      (``test.py:49-56``): a permutation per utterance (``sepvad_eval_separation``);
    * ``loss_func`` a ``combined_loss.BinaryCrossEntropyLoss_Mean``, ``pit_from="pw_pt"`` — ``loss_vad`` and
      ``pit_CE_vad`` (``test.py:59-61``, ``model/metric.py:264``): that loss returns a scalar, so the permutation is
      shared by the batch (``sepvad_eval_vad``), and its labels equal to 2 become 1 in place.

    ``perm_reduce`` may be ``None`` or ``False`` (what ``test.py:50-54`` passes for the configs' ``false``). Other
    combinations raise ``NotImplementedError`` (training losses are out of scope). Forward-only.
    """

    def __init__(self, loss_func, pit_from="pw_mtx", perm_reduce=None):
        super().__init__()
        self.loss_func = loss_func
        self.pit_from = pit_from
        self.perm_reduce = perm_reduce
        if self.pit_from not in ["pw_mtx", "pw_pt", "perm_avg"]:
            raise ValueError("Unsupported loss function type for now. Expected"
                             "one of [`pw_mtx`, `pw_pt`, `perm_avg`]")

    def _native_ok(self):
        return (self.pit_from == "pw_pt" and self.perm_reduce is None and isinstance(self.loss_func, nn.L1Loss)
                and self.loss_func.reduction == "mean")

    def _criterion_forward(self, est_targets, targets, n_src, kwargs):
        """(mean loss, batch_indices [B, 2] int64) of the two evaluation criteria of test.py:49-61."""
        from .evaluate import BinaryCrossEntropyLoss_Mean, eval_vad
        from .metrics import calc_sisdr_loss
        from .sdr import PairwiseNegSDR
        plain = self.perm_reduce is None or self.perm_reduce is False
        if plain and not kwargs and n_src == 2 and self.pit_from == "pw_pt" and self.loss_func is calc_sisdr_loss:
            mean_loss, batch_indices, _ = pit_sisdr_rows(est_targets, targets)
            return mean_loss, batch_indices
        if plain and not kwargs and self.pit_from == "pw_mtx" and isinstance(self.loss_func, PairwiseNegSDR):
            r = self.loss_func.evaluate(est_targets, targets)  # its TypeError / NotImplementedError on bad shapes
            return r["means"][0], r["perm"]
        if (plain and not kwargs and n_src == 2 and self.pit_from == "pw_pt"
                and isinstance(self.loss_func, BinaryCrossEntropyLoss_Mean)):
            pw = eval_vad(est_targets, targets)["pw_ce"]  # [est i][target j], every batch row of get_pw_losses
            # find_best_perm_factorial (pit_wrapper.py:287-312) on that one matrix: float32 adds, the first minimum
            # wins; a few scalar device ops, nothing read on the host
            loss_id, loss_sw = (pw[0, 0] + pw[1, 1]) / 2, (pw[1, 0] + pw[0, 1]) / 2
            swap = (loss_sw < loss_id).to(torch.int64)
            ident = torch.arange(2, device=pw.device)
            return torch.minimum(loss_id, loss_sw), (ident ^ swap).expand(targets.shape[0], 2).contiguous()
        raise NotImplementedError("native PIT: built for 2 sources and PITLossWrapper(nn.L1Loss(), 'pw_pt'), "
                                  "PITLossWrapper(calc_sisdr_loss, 'pw_pt'), "
                                  "PITLossWrapper(sdr.PairwiseNegSDR(...), 'pw_mtx') or "
                                  "PITLossWrapper(combined_loss.BinaryCrossEntropyLoss_Mean(), 'pw_pt'), without "
                                  "perm_reduce or extra arguments")

    def forward(self, est_targets, targets, target_vad=0, return_est=False, return_incides=False,
                reduce_kwargs=None, **kwargs):
        n_src = targets.shape[1]
        assert n_src < 10, f"Expected source axis along dim 1, found {n_src}"
        if self._native_ok() and n_src == 2 and not kwargs:
            mean_loss, batch_indices, _ = pit_l1(est_targets, targets)
        else:
            mean_loss, batch_indices = self._criterion_forward(est_targets, targets, n_src, kwargs)
        if not return_est and not return_incides:
            return mean_loss
        if not return_est and return_incides:
            return mean_loss, batch_indices
        reordered = reorder_source_mse(est_targets, batch_indices)
        if return_est and return_incides:
            return mean_loss, reordered, batch_indices
        return mean_loss, reordered
