"""Separation quality metrics on the device, mirroring the reference's metric surface.

* ``calc_sisdr`` / ``calc_sisdr_loss`` (reference ``model/combined_loss.py:16-60``) and
  ``scale_invariant_signal_distortion_ratio`` (``model/metric.py:61-101``, the same formula):
  ``[..., time]`` -> ``[...]`` SI-SDR in dB, float32 epsilon, optional zero mean.
* ``pit_si_sdr`` (``model/metric.py:258``: torchmetrics ``PIT(scale_invariant_signal_distortion_ratio,
  'max')``): per utterance the best speaker permutation by mean SI-SDR, averaged over the batch.
  torchmetrics is not installed here; its published ``permutation_invariant_training`` (metric matrix
  [B, S, S] -> exhaustive permutations, eval 'max', mean over speakers; the Metric object averages over
  the batch) is restated; parity of that reduction is pinned by the oracle tests, not by torchmetrics.
* ``SI_SDRi`` / ``si_sdri`` (``model/metric.py:145-160``): ``pit_si_sdr(preds, target)`` minus the mean
  SI-SDR of the mixture against each target.
* ``Accuracy_Vad`` (``model/metric.py:163-177``): thresholded (``> 0.5``) VAD label accuracy, overall and per
  speaker; like the reference it thresholds ``preds`` in place (``k_vad_acc``, exact integer counts).
* ``signal_noise_ratio`` (``model/metric.py:104-143``) and ``pit_snr`` (``:255-256``): the SNR of the same row
  pairs (``k_snr``, the moments of ``k_si_sdr`` with another closed form) and the PIT reduction over it.
* ``stoi`` (``model/stoi_metric.py:207-301``, classic STOI; ``extended=True`` draws ``np.random`` noise and is
  refused there: see ``estoi``), the ``Stoi`` module and ``stoi_met`` (``model/metric.py:207-223,276-277``): every
  pair of a batch in one call of ``sepvad_stoi`` (csrc/stoi.hip), float64 results on the device, no host round trip.
* ``estoi``, ``Estoi`` and ``estoi_met``: extended STOI (``stoi_metric.py:177-193,268-271``) with the reference's
  random term left out (it moves the reference's value by 1e-15) and zero-norm rows and columns set to zero;
  ``estoi_pairs`` and ``stoi_both_pairs`` (both metrics from one ``sepvad_stoi_ex`` call) are the row-pair forms.
* ``pit_CE_vad`` (``model/metric.py:264-265``), ``vad_confusion`` (the per-speaker ``confusion_matrix`` of
  ``test.py:164``) and ``calc_vad`` (``Our_utils/utils_test.py:67-73``): ``sepvad_eval_vad`` (csrc/eval.hip);
  ``evaluate.score_batch`` returns all of a ``test.py`` step's numbers from one pass over the rows.

All inputs are ROCm tensors; the arithmetic runs in ``k_si_sdr`` / ``k_snr`` (csrc/metrics.hip), the ``k_stoi_*``
kernels (csrc/stoi.hip) and the ``k_eval_*`` kernels (csrc/eval.hip) through the C ABI. There is no CPU fallback.
"""
from __future__ import annotations

import itertools

import torch

from . import native as _native


def _check_same_shape(preds, target):
    if preds.shape != target.shape:
        raise RuntimeError("Predictions and targets are expected to have the same shape, pred has shape of "
                           f"{preds.shape} and target has shape of {target.shape}")


def _as_rows(x: torch.Tensor) -> torch.Tensor:
    if x.device.type != "cuda":
        raise RuntimeError("sepvad metrics: inputs must be ROCm device tensors")
    return x.to(torch.float32).reshape(-1, x.shape[-1]).contiguous()


def _si_sdr_pairs(P, Tg, pidx=None, tidx=None, zero_mean=True, entry="sepvad_si_sdr"):
    """SI-SDR (or, with entry="sepvad_snr", SNR) of rows P[pidx[r]] vs Tg[tidx[r]] (2-D contiguous float32
    device tensors)."""
    lib = _native.load_library()
    R = len(pidx) if pidx is not None else P.shape[0]
    out = torch.empty(R, device=P.device, dtype=torch.float32)
    pi = torch.as_tensor(pidx, dtype=torch.int32, device=P.device) if pidx is not None else None
    ti = torch.as_tensor(tidx, dtype=torch.int32, device=P.device) if tidx is not None else None
    rc = getattr(lib, entry)(_native.ptr(P), P.shape[1], _native.ptr(Tg), Tg.shape[1], P.shape[1], R,
                             _native.ptr(pi), _native.ptr(ti), int(bool(zero_mean)), _native.ptr(out),
                             _native.stream_ptr(P.device))
    _native.check(rc, entry)
    return out


def _snr_pairs(P, Tg, pidx=None, tidx=None, zero_mean=True):
    return _si_sdr_pairs(P, Tg, pidx, tidx, zero_mean, entry="sepvad_snr")


def scale_invariant_signal_distortion_ratio(preds: torch.Tensor, target: torch.Tensor, zero_mean: bool = True):
    """model/metric.py:61-101 (== model/combined_loss.py:16-56 calc_sisdr)."""
    _check_same_shape(preds, target)
    P, Tg = _as_rows(preds), _as_rows(target)
    return _si_sdr_pairs(P, Tg, zero_mean=zero_mean).reshape(preds.shape[:-1])


calc_sisdr = scale_invariant_signal_distortion_ratio


def calc_sisdr_loss(preds, target, zero_mean: bool = True):
    """model/combined_loss.py:58-60."""
    return -calc_sisdr(preds, target, zero_mean)


def signal_noise_ratio(preds: torch.Tensor, target: torch.Tensor, zero_mean: bool = True):
    """model/metric.py:104-143 (note its default: zero_mean=True, unlike torchmetrics)."""
    _check_same_shape(preds, target)
    P, Tg = _as_rows(preds), _as_rows(target)
    return _snr_pairs(P, Tg, zero_mean=zero_mean).reshape(preds.shape[:-1])


def permutation_invariant_si_sdr(preds: torch.Tensor, target: torch.Tensor, zero_mean: bool = True,
                                 pairwise=_si_sdr_pairs):
    """Per-utterance best permutation for [B, S, time] inputs.

    Returns (best_metric [B], best_perm [B, S] int64): metric matrix m[b, t, p] = SI-SDR(preds[b, p],
    target[b, t]) (or another `pairwise` row-pair metric); perm value = mean_t m[b, t, perm[t]]; the first
    maximum over permutations in itertools order (torchmetrics' exhaustive search)."""
    _check_same_shape(preds, target)
    B, S, N = preds.shape
    P, Tg = _as_rows(preds), _as_rows(target)
    pidx, tidx = [], []
    for b in range(B):
        for t in range(S):
            for p in range(S):
                pidx.append(b * S + p)
                tidx.append(b * S + t)
    mtx = pairwise(P, Tg, pidx, tidx, zero_mean).reshape(B, S, S)
    perms = torch.tensor(list(itertools.permutations(range(S))), device=preds.device)  # [P!, S]
    vals = mtx[:, torch.arange(S, device=preds.device), perms].mean(dim=-1)           # [B, P!]
    best, idx = vals.max(dim=-1)
    return best, perms[idx]


def pit_si_sdr(preds: torch.Tensor, target: torch.Tensor):
    """model/metric.py:258: mean over the batch of the best-permutation SI-SDR."""
    best, _ = permutation_invariant_si_sdr(preds, target, zero_mean=True)
    return best.mean()


def permutation_invariant_snr(preds: torch.Tensor, target: torch.Tensor, zero_mean: bool = True):
    """permutation_invariant_si_sdr over signal_noise_ratio."""
    return permutation_invariant_si_sdr(preds, target, zero_mean, pairwise=_snr_pairs)


def pit_snr(preds: torch.Tensor, target: torch.Tensor):
    """model/metric.py:255-256: mean over the batch of the best-permutation SNR (zero_mean=True)."""
    best, _ = permutation_invariant_snr(preds, target, zero_mean=True)
    return best.mean()


# test.py:149-151 calls `metric.to(device)` and reads `metric.__name__` on every entry of config["metrics"]["separation"]
# (the reference's are torchmetrics objects); the functions here hold no state, so .to returns them unchanged
pit_snr.to = lambda *args, **kwargs: pit_snr
pit_si_sdr.to = lambda *args, **kwargs: pit_si_sdr


def stoi_filter(fs_sig: int):
    """Host design of the STOI front end (sepvad_stoi_filter, no GPU): (taps float32 [ntaps] = h / sum(h) of
    stoi_metric.py:11-52, (up, down), bands int32 [15, 2] = first bin / one past the last bin of OBM, :201)."""
    import ctypes
    import numpy as np
    lib = _native.load_library()
    info = (ctypes.c_int32 * 34)()
    _native.check(lib.sepvad_stoi_filter(int(fs_sig), None, 0, info), "sepvad_stoi_filter")
    taps = np.zeros(info[2], np.float32)
    _native.check(lib.sepvad_stoi_filter(int(fs_sig), taps.ctypes.data_as(ctypes.c_void_p), taps.size, info),
                  "sepvad_stoi_filter")
    return taps, (info[0], info[1]), np.array(info[4:34], np.int32).reshape(15, 2)


def stoi_pairs(X, Y, fs_sig, xidx=None, yidx=None):
    """STOI of clean rows X[xidx[r]] vs estimate rows Y[yidx[r]] (2-D contiguous float32 device tensors of one
    length). Returns (d [R] float64, M [R] int32: spectra left after silence removal; d is exactly 1e-5 where
    M < 30, as the reference returns with a warning)."""
    lib = _native.load_library()
    if X.shape[1] != Y.shape[1]:
        raise RuntimeError(f"x and y should have the same length, found {X.shape[1]} and {Y.shape[1]}")
    N = X.shape[1]
    R = len(xidx) if xidx is not None else X.shape[0]
    dev = X.device
    scratch, _ = _native.scratch_for("sepvad_stoi_scratch_bytes", dev, R, N, int(fs_sig))
    out = torch.empty(R, device=dev, dtype=torch.float64)
    frames = torch.empty(R, device=dev, dtype=torch.int32)
    xi = torch.as_tensor(xidx, dtype=torch.int32, device=dev) if xidx is not None else None
    yi = torch.as_tensor(yidx, dtype=torch.int32, device=dev) if yidx is not None else None
    rc = lib.sepvad_stoi(_native.ptr(X), X.shape[1], _native.ptr(Y), Y.shape[1], N, R, _native.ptr(xi),
                         _native.ptr(yi), int(fs_sig), _native.ptr(scratch), scratch.numel(), _native.ptr(out),
                         _native.ptr(frames), _native.stream_ptr(dev))
    _native.check(rc, "sepvad_stoi")
    return out, frames


STOI_CLASSIC, STOI_EXTENDED = 1, 2  # SEPVAD_STOI_* (include/sepvad.h): the modes of sepvad_stoi_ex


def _stoi_ex(X, Y, fs_sig, xidx, yidx, modes):
    """sepvad_stoi_ex on 2-D contiguous float32 device rows: (stoi or None, estoi or None, M). xidx / yidx: a list
    or a device int tensor (used as it is: no host round trip)."""
    lib = _native.load_library()
    if X.shape[1] != Y.shape[1]:
        raise RuntimeError(f"x and y should have the same length, found {X.shape[1]} and {Y.shape[1]}")
    N = X.shape[1]
    R = len(xidx) if xidx is not None else X.shape[0]
    dev = X.device
    scratch, _ = _native.scratch_for("sepvad_stoi_ex_scratch_bytes", dev, R, N, int(fs_sig), modes)
    d = torch.empty(R, device=dev, dtype=torch.float64) if modes & STOI_CLASSIC else None
    e = torch.empty(R, device=dev, dtype=torch.float64) if modes & STOI_EXTENDED else None
    frames = torch.empty(R, device=dev, dtype=torch.int32)
    xi = torch.as_tensor(xidx, dtype=torch.int32, device=dev).contiguous() if xidx is not None else None
    yi = torch.as_tensor(yidx, dtype=torch.int32, device=dev).contiguous() if yidx is not None else None
    rc = lib.sepvad_stoi_ex(_native.ptr(X), X.shape[1], _native.ptr(Y), Y.shape[1], N, R, _native.ptr(xi),
                            _native.ptr(yi), int(fs_sig), _native.ptr(scratch), scratch.numel(), modes,
                            _native.ptr(d), _native.ptr(e), _native.ptr(frames), _native.stream_ptr(dev))
    _native.check(rc, "sepvad_stoi_ex")
    return d, e, frames


def estoi_pairs(X, Y, fs_sig, xidx=None, yidx=None):
    """Extended STOI of clean rows X[xidx[r]] vs estimate rows Y[yidx[r]], the arguments of ``stoi_pairs``. Returns
    (d [R] float64, M [R] int32); d is exactly 1e-5 where M < 30 and exactly 0 for an all-zero estimate."""
    _, e, frames = _stoi_ex(X, Y, fs_sig, xidx, yidx, STOI_EXTENDED)
    return e, frames


def stoi_both_pairs(X, Y, fs_sig, xidx=None, yidx=None):
    """(stoi [R], estoi [R], M [R]) from one sepvad_stoi_ex call: the front end runs once. The classic values have
    the bits of ``stoi_pairs``, the extended ones those of ``estoi_pairs``."""
    return _stoi_ex(X, Y, fs_sig, xidx, yidx, STOI_CLASSIC | STOI_EXTENDED)


def stoi(x: torch.Tensor, y: torch.Tensor, fs_sig: int, extended: bool = False):
    """model/stoi_metric.py:207-301 with the reference's argument order (x clean, y processed): [..., time] ROCm
    tensors -> [...] float64 on the device. ``extended=True`` is refused here; ``estoi`` is the native form."""
    if extended:
        raise NotImplementedError("stoi(..., extended=True) adds np.random noise in the reference "
                                  "(stoi_metric.py:177-193) and is not reproduced; use metrics.estoi, the same "
                                  "formula with the random term left out")
    if x.shape != y.shape:
        raise RuntimeError(f"x and y should have the same length, found {tuple(x.shape)} and {tuple(y.shape)}")
    X, Y = _as_rows(x), _as_rows(y)
    return stoi_pairs(X, Y, fs_sig)[0].reshape(x.shape[:-1])


def estoi(x: torch.Tensor, y: torch.Tensor, fs_sig: int):
    """Extended STOI (stoi_metric.py:207-301 with extended=True, its random term left out) with ``stoi``'s argument
    order (x clean, y processed): [..., time] ROCm tensors -> [...] float64 on the device."""
    if x.shape != y.shape:
        raise RuntimeError(f"x and y should have the same length, found {tuple(x.shape)} and {tuple(y.shape)}")
    X, Y = _as_rows(x), _as_rows(y)
    return estoi_pairs(X, Y, fs_sig)[0].reshape(x.shape[:-1])


class Stoi(torch.nn.Module):
    """model/metric.py:207-223: preds, targets [B, num_spk, time] -> mean STOI over [B, num_spk] (0-dim float64
    device tensor). The reference hard-codes 16 kHz; fs_sig overrides it. batch_indices_separation is unused
    there as well."""

    def __init__(self, fs_sig: int = 16000):
        super().__init__()
        self.fs_sig = fs_sig

    def forward(self, preds, targets, batch_indices_separation=None):
        _check_same_shape(preds, targets)
        return stoi(targets, preds, self.fs_sig).mean()


stoi_met = Stoi()
stoi_met.__name__ = "stoi_metric"


class Estoi(torch.nn.Module):
    """``Stoi`` with extended STOI: preds, targets [B, num_spk, time] -> mean ESTOI over [B, num_spk] (0-dim float64
    device tensor)."""

    def __init__(self, fs_sig: int = 16000):
        super().__init__()
        self.fs_sig = fs_sig

    def forward(self, preds, targets, batch_indices_separation=None):
        _check_same_shape(preds, targets)
        return estoi(targets, preds, self.fs_sig).mean()


estoi_met = Estoi()
estoi_met.__name__ = "estoi_metric"


class SI_SDRi(torch.nn.Module):
    """model/metric.py:145-160."""

    def forward(self, preds, target, mix):
        mix = mix.unsqueeze(dim=1).repeat(1, preds.shape[1], 1)
        si_sdr_mix_start = torch.mean(scale_invariant_signal_distortion_ratio(mix, target, zero_mean=True))
        return pit_si_sdr(preds, target) - si_sdr_mix_start


si_sdri = SI_SDRi()
si_sdri.__name__ = "si_sdri"


class Accuracy_Vad(torch.nn.Module):
    """model/metric.py:163-177: preds, targets [B, num_spk, T] -> (acc, acc0, acc1) 0-dim float32 tensors.
    preds is thresholded in place (> 0.5 -> 1, <= 0.5 -> 0), as the reference does."""

    def forward(self, preds, targets, batch_indices_vad=None):
        _check_same_shape(preds, targets)
        if preds.device.type != "cuda" or targets.device != preds.device:
            raise RuntimeError("sepvad metrics: inputs must be ROCm device tensors on one device")
        B, S, T = preds.shape
        work = preds if (preds.dtype == torch.float32 and preds.is_contiguous()) else preds.float().contiguous()
        tg = targets.to(torch.float32).contiguous()
        out = torch.empty(1 + S, device=preds.device, dtype=torch.float32)
        lib = _native.load_library()
        rc = lib.sepvad_vad_accuracy(_native.ptr(work), _native.ptr(tg), B, S, T, 1, _native.ptr(out),
                                     _native.stream_ptr(preds.device))
        _native.check(rc, "sepvad_vad_accuracy")
        if work is not preds:
            preds.copy_(work)
        return out[0], out[1], out[2]


vad_accuracy = Accuracy_Vad()  # model/metric.py:270-271
vad_accuracy.__name__ = "vad_accuracy"

# model/metric.py:264-265 (config["metrics"]["vad"], test.py:67,155-156); an nn.Module, so .to exists
from .evaluate import BinaryCrossEntropyLoss_Mean as _BceMean  # noqa: E402
from .pit import PITLossWrapper as _PITLossWrapper  # noqa: E402

pit_CE_vad = _PITLossWrapper(loss_func=_BceMean(), pit_from="pw_pt")
pit_CE_vad.__name__ = "pit_CE_vad"


def vad_confusion(preds: torch.Tensor, labels: torch.Tensor, perm=None):
    """The confusion_matrix(label, pred, labels=[0., 1.]).ravel() of test.py:164 for every utterance and speaker at
    once: preds, labels [B, 2, T] -> [B, 2, 4] int32 (tn, fp, fn, tp) on the device. A prediction is 1 when
    preds > 0.5 (Accuracy_Vad's rule; already thresholded 0 / 1 preds count as they are, a NaN as 0), labels equal to 2 count
    as 1 (labels is not changed), pairs with any other label are left out; perm [B, 2] int64 (device) counts
    preds[b, perm[b, s]] against labels[b, s]."""
    from .evaluate import eval_vad
    _check_same_shape(preds, labels)
    return eval_vad(preds, labels, perm, fix_labels=False)["conf"]


def calc_vad(masks: torch.Tensor):
    """Our_utils/utils_test.py:67-73: post-sigmoid masks [B, 2, 257, T] -> [B, 2, T] int64, 1 where at least a
    quarter of the bins (65 of 257) are >= 0.5."""
    from .evaluate import simple_vad
    return simple_vad(masks)
