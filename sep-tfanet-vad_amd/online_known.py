"""Streaming evaluation with known targets — drop-in for the reference's ``OnlineSaving`` of
``model/online_class_known_targets.py:9-154`` (driven by ``test.py:96-106,117-120,223-269``), on the GPU.

The reference slides the ``max_len`` (3 s) window with hop ``save_sec`` over a padded mixture, orders every window's
speakers by PIT against the target window (``criterion_separation``), optionally re-orders them by a similarity PIT
against the signal stitched so far (``criterion_similarity``), appends the window's last hop, and reports two numbers
per call: ``online_sisdr`` (the stitched signal against the targets) and ``reference_sisdr`` (one whole-file forward
on the same span). Their difference is what streaming costs in dB. This class keeps that algorithm and its
attributes, with the data on the device:

* fused path: all windows of all streams run as window-major ``sepvad_forward_windows`` chunks (``online.py``) and
  each chunk's whole window loop — target PIT, similarity PIT chain, reorder, append — is one ``sepvad_stream_eval``
  call (csrc/stream_eval.hip): a fixed number of launches per chunk instead of about six dependent ones per window.
  It runs when the model is native, the criteria are the supported ones (``PITLossWrapper(PairwiseNegSDR, "pw_mtx")``
  for separation; none, ``PITLossWrapper(nn.L1Loss(), "pw_pt")`` or ``PITLossWrapper(calc_sisdr_loss, "pw_pt")`` for
  similarity) and the window offsets are exactly ``k * hop`` (``online.OnlineSaving._batched_ok``'s rule);
* composed path (``fused_eval = False``, or whenever the fused one does not apply): the reference's loop through the
  criteria and ``sepvad_stream_append``. Same results; it is the cross-check of the fused path.

Both scores take their permutation from ``sepvad_eval_separation`` on strided slices of the padded signals (no
copies); the online score is its score sheet.

Deliberate differences from the reference:

* the forward's 3-tuple is used (the reference unpacks six values, :105,126, and cannot run against its own model);
* a float ``save_sec`` that leaves a remainder pads by ``int(r)`` (the reference hands the float to ``F.pad``, :94-97,
  which raises); the remainder itself, not its complement, is the pad, as in the reference;
* besides the two lists, the per-row scores are kept (``online_sisdr_rows``, ``reference_sisdr_rows``: one ``[B, 2]``
  CPU tensor per call; the reference's mean over the batch hides them), and the last call's per-window permutations
  and pairwise tables (``window_perms`` ``[K, B, 2]``, ``window_perms_target``, ``window_pw_target`` ``[K, B, 2, 2]``,
  ``window_pw_similarity``);
* the wav writes the reference has commented out (:120-122,148-150) are not made;
* streams sharded over ranks are not supported (``process_group`` raises).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import native as _native
from . import pit as _pit
from .online import MAX_WINDOW_UTTS, _slice_bounds

SE_NONE, SE_L1, SE_SISDR = 0, 1, 2  # SEPVAD_SE_* (include/sepvad.h)


def sisdr_under_perm(est, tgt, perm):
    """calc_sisdr(reorder_source_mse(est, perm), tgt) -> [B, 2] (model/combined_loss.py:16-56,63-78) without the
    reordered copy: ``sepvad_si_sdr`` reads the strided rows through index arrays built on the device."""
    lib = _native.load_library()
    est, eld = _native.rows3(est)
    tgt, tld = _native.rows3(tgt)
    B, _, N = est.shape
    dev = est.device
    rows = torch.arange(2 * B, device=dev, dtype=torch.int64)
    pidx = ((rows >> 1) * 2 + perm.reshape(-1)).to(torch.int32)
    tidx = rows.to(torch.int32)
    out = torch.empty(2 * B, device=dev, dtype=torch.float32)
    rc = lib.sepvad_si_sdr(_native.ptr(est), eld, _native.ptr(tgt), tld, N, 2 * B, _native.ptr(pidx),
                           _native.ptr(tidx), 1, _native.ptr(out), _native.stream_ptr(dev))
    _native.check(rc, "sepvad_si_sdr")
    return out.reshape(B, 2)


class StreamEval:
    """The buffers of one signal's ``sepvad_stream_eval`` calls: K windows of B streams, window W, hop H, targets
    ``tgt`` [B, 2, >= (K - 1) H + W]. ``push(sep_w, k0)`` takes the next window-major chunk [n, B, 2, W]; afterwards
    ``online`` [B, 2, K H], ``perm`` [K, B, 2], ``perm_tgt``, ``pw_tgt`` [K, B, 2, 2], ``loss_tgt`` [K, B] and
    ``pw_sim`` [K, G, 2, 2] hold the windows pushed so far."""

    def __init__(self, tgt, K, W, H, mode, sdr_type="sisdr", zero_mean=True, take_log=True, eps=1e-8):
        from .evaluate import SDR_TYPES
        self.lib = _native.load_library()
        self.tgt, self.tgt_ld = _native.rows3(tgt)
        self.B, self.K, self.W, self.H, self.mode = self.tgt.shape[0], int(K), int(W), int(H), int(mode)
        self.crit = (SDR_TYPES[sdr_type], int(bool(zero_mean)), int(bool(take_log)), float(eps))
        dev, B = self.tgt.device, self.B
        self.raw = torch.empty(B, 2, K * H, dtype=torch.float32, device=dev)
        self.online = torch.empty(B, 2, K * H, dtype=torch.float32, device=dev)
        self.perm = torch.empty(K, B, 2, dtype=torch.int64, device=dev)
        self.perm_tgt = torch.empty(K, B, 2, dtype=torch.int64, device=dev) if mode != SE_NONE else self.perm
        self.pw_tgt = torch.empty(K, B, 2, 2, dtype=torch.float32, device=dev)
        self.loss_tgt = torch.empty(K, B, dtype=torch.float32, device=dev)
        G = B if mode == SE_SISDR else 1
        self.pw_sim = torch.empty(K, G, 2, 2, dtype=torch.float32, device=dev) if mode != SE_NONE else None
        self.scratch = None

    def push(self, sep_w, k0):
        n = sep_w.shape[0]
        if tuple(sep_w.shape[1:]) != (self.B, 2, self.W) or sep_w.dtype != torch.float32 or not sep_w.is_contiguous():
            raise ValueError(f"StreamEval.push: expected contiguous float32 [n, {self.B}, 2, {self.W}], got "
                             f"{tuple(sep_w.shape)}")
        nbytes = _native.scratch_bytes("sepvad_stream_eval_scratch_bytes", self.B, n, self.W, self.H, self.mode)
        if self.scratch is None or self.scratch.numel() * 8 < nbytes:
            self.scratch = torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.float64, device=sep_w.device)
        P = _native.ptr
        rc = self.lib.sepvad_stream_eval(
            P(sep_w), self.W, n, int(k0), self.K, self.B, self.W, self.H, P(self.tgt), self.tgt_ld, self.mode,
            *self.crit, P(self.raw), self.raw.stride(1), P(self.online), self.online.stride(1), P(self.perm),
            P(self.perm_tgt) if self.mode != SE_NONE else None, P(self.pw_tgt), P(self.loss_tgt), P(self.pw_sim),
            P(self.scratch), self.scratch.numel() * 8, _native.stream_ptr(sep_w.device))
        _native.check(rc, "sepvad_stream_eval")


class OnlineSaving:
    def __init__(self, criterion_separation, model, save_path, device, criterion_similarity=None) -> None:
        # attributes as in model/online_class_known_targets.py:10-24
        self.indx = 0
        self.fs = 16000
        self.max_len = 3
        self.save_sec = 1
        self.criterion_separation = criterion_separation
        self.model = model
        self.save_path = save_path
        self.online_sisdr = []
        self.reference_sisdr = []
        self.num_save_samples = 2000000
        self.similarity = False
        if criterion_similarity is not None:
            self.similarity = True
            self.criterion_similarity = criterion_similarity
        self.device = device
        self.online_sisdr_rows = []
        self.reference_sisdr_rows = []
        self.one_forward = True   # all windows in window-major forwards when possible (False: a forward per window)
        self.fused_eval = True    # the window loop in sepvad_stream_eval when possible (False: the composed loop)
        self.max_window_utts = MAX_WINDOW_UTTS
        self.used_fused = None    # which path the last calc_online took

    def reset(self):
        self.indx = 0

    def _hop(self) -> int:
        return int(np.floor(self.fs * self.save_sec))

    def update_online_signal(self, est_signals):
        """Reference :29-38 (stand-alone form; calc_online appends into a preallocated buffer)."""
        hop = self._hop()
        tail = est_signals[:, :, est_signals.shape[-1] - hop:]
        self.online_signal = tail if self.indx == 0 else torch.cat((self.online_signal, tail), dim=-1)

    def get_truncated_signal(self, full_signal_mix, target_signal):
        s = int(np.floor(self.fs * self.indx * self.save_sec))
        return full_signal_mix[:, s: s + self.max_len * self.fs], target_signal[:, :, s: s + self.max_len * self.fs]

    def increase_indx(self):
        self.indx += 1

    def get_indx(self):
        return self.indx

    def _fused_mode(self):
        """SEPVAD_SE_* of the similarity criterion when both criteria are ones sepvad_stream_eval restates, else None."""
        from .metrics import calc_sisdr_loss
        from .sdr import PairwiseNegSDR
        cs = self.criterion_separation
        if not (isinstance(cs, _pit.PITLossWrapper) and cs.pit_from == "pw_mtx" and isinstance(cs.loss_func, PairwiseNegSDR)
                and (cs.perm_reduce is None or cs.perm_reduce is False)):
            return None
        if not self.similarity:
            return SE_NONE
        cm = self.criterion_similarity
        if not (isinstance(cm, _pit.PITLossWrapper) and cm.pit_from == "pw_pt" and cm.perm_reduce is None):
            return None
        if isinstance(cm.loss_func, nn.L1Loss) and cm.loss_func.reduction == "mean":
            return SE_L1
        return SE_SISDR if cm.loss_func is calc_sisdr_loss else None

    def _windows_ok(self, n_win: int, hop: int) -> bool:
        """Window-major forwards need the native model and window offsets that are exactly k * hop (:41-42)."""
        if not self.one_forward or not hasattr(self.model, "native_handle"):
            return False
        return all(int(np.floor(self.fs * k * self.save_sec)) == k * hop for k in range(n_win))

    def pad_signals(self, full_signal_mix, target_signal):
        """Reference :86-98: (padded mixture, padded targets, number of windows)."""
        pad = torch.nn.functional.pad
        win = self.fs * self.max_len
        if full_signal_mix.shape[-1] < win:
            full_signal_mix = pad(full_signal_mix, (0, win - full_signal_mix.shape[-1]))
            target_signal = pad(target_signal, (0, win - target_signal.shape[-1]))
        left = int(self.fs * (self.max_len - self.save_sec))
        full_signal_mix = pad(full_signal_mix, (left, 0))
        target_signal = pad(target_signal, (left, 0))
        pad_zero = (full_signal_mix.shape[-1] - win) % (self.fs * self.save_sec)
        if pad_zero:  # the remainder, not its complement (the reference's quirk); int() where it passes a float
            full_signal_mix = pad(full_signal_mix, (0, int(pad_zero)))
            target_signal = pad(target_signal, (0, int(pad_zero)))
        max_indx = np.floor((full_signal_mix.shape[-1] - win) / (self.fs * self.save_sec))
        return full_signal_mix, target_signal, int(max_indx) + 1

    def calc_online(self, full_signal_mix, target_signal, name_folder, sample_indx, inference_kw=None,
                    process_group=None):
        """Reference :85-154. Appends to ``online_sisdr`` / ``reference_sisdr`` (and the ``_rows`` lists) and leaves
        the stitched signal, reordered against the targets (:143), in ``self.online_signal`` ([B, 2, K * hop]).
        name_folder and sample_indx are the reference's arguments (its wav writes are commented out)."""
        if process_group is not None:
            raise NotImplementedError("OnlineSavingKnownTargets: streams sharded over ranks are not supported "
                                      "(per-rank scores would need the batch-global L1 sums all-reduced per window)")
        from .evaluate import eval_separation
        kw = inference_kw or {}
        full_signal_mix, target_signal, n_win = self.pad_signals(full_signal_mix, target_signal)
        full_signal_mix = full_signal_mix.to(torch.float32)
        target_signal = target_signal.to(torch.float32)
        win, hop = self.fs * self.max_len, self._hop()
        B = full_signal_mix.shape[0]
        dev = full_signal_mix.device
        windows = self._windows_ok(n_win, hop)
        mode = self._fused_mode()
        fused = bool(self.fused_eval and windows and mode is not None and hop <= win
                     and (mode == SE_NONE or 2 * hop <= win))
        self.used_fused = fused
        if windows:
            x = full_signal_mix if full_signal_mix.stride(-1) == 1 else full_signal_mix.contiguous()
            wchunk = max(1, int(self.max_window_utts) // max(1, B))
            handle = self.model.native_handle(dev)
        if fused:
            cs = self.criterion_separation.loss_func
            se = StreamEval(target_signal, n_win, win, hop, mode, cs.sdr_type, cs.zero_mean, cs.take_log, cs.EPS)
            for k0 in range(0, n_win, wchunk):
                n = min(wchunk, n_win - k0)
                with torch.no_grad():
                    sep_w = handle.forward_windows(x[:, k0 * hop:], n, hop, win, kw)
                se.push(sep_w, k0)
            self.indx = n_win
            self.online_signal = se.online
            self.window_perms, self.window_perms_target = se.perm, se.perm_tgt
            self.window_pw_target, self.window_pw_similarity = se.pw_tgt, se.pw_sim
        else:
            buf = torch.empty(B, 2, n_win * hop, dtype=torch.float32, device=dev)
            perms, perms_t = [], []
            k_base, sep_w = 0, None
            while self.indx < n_win:
                k = self.indx
                mix_w, tgt_w = self.get_truncated_signal(full_signal_mix, target_signal)
                if windows:
                    if sep_w is None or k >= k_base + sep_w.shape[0]:  # next window-major chunk, one forward
                        k_base, n = k, min(wchunk, n_win - k)
                        with torch.no_grad():
                            sep_w = handle.forward_windows(x[:, k * hop:], n, hop, win, kw)
                    pred = sep_w[k - k_base]
                else:
                    with torch.no_grad():
                        pred = self.model(mix_w, kw)[0]
                _, batch_indices = self.criterion_separation(pred, tgt_w, return_incides=True)   # :106
                perms_t.append(batch_indices)
                L = pred.shape[-1]
                if self.similarity:
                    # the reference seeds online_signal with the un-reordered last hop at indx 0 (:109-111)
                    online = pred[:, :, L - hop:] if k == 0 else buf[:, :, :k * hop]
                    n_on = online.shape[-1]
                    pb, pe = _slice_bounds(L, -hop - n_on, -hop)           # :112
                    ob, oe = _slice_bounds(n_on, -win + hop, None)         # :113
                    _, batch_indices = self.criterion_similarity(pred[:, :, pb:pe], online[:, :, ob:oe],
                                                                 return_incides=True)
                perms.append(batch_indices)
                _pit.stream_append(pred, L - hop, hop, batch_indices, buf, k * hop)   # :118-119
                self.increase_indx()
            self.online_signal = buf
            self.window_perms, self.window_perms_target = torch.stack(perms), torch.stack(perms_t)
            self.window_pw_target = self.window_pw_similarity = None
        self.stitched_signal = self.online_signal  # before the reordering against the targets (:143)

        # the reference score (:126-135): a whole-file forward, its PIT against the whole padded targets, the score on
        # the span the windows emitted
        with torch.no_grad():
            pred_full = self.model(full_signal_mix, kw)[0]
        _, ref_perm = self.criterion_separation(pred_full, target_signal, return_incides=True)
        t0 = int(np.floor(self.fs * (self.max_len - self.save_sec)))
        t1 = int(np.floor(self.fs * (self.max_len + (self.indx - 1) * self.save_sec)))
        target_t = target_signal[:, :, t0:t1]
        ref_rows = sisdr_under_perm(pred_full[:, :, t0:t1], target_t, ref_perm)
        # the online score (:138-145): PIT of the stitched signal against the same span, reorder, calc_sisdr; perm
        # and the reordered estimates' SI-SDR are one sepvad_eval_separation call when the criterion is native
        if mode is not None:
            cs = self.criterion_separation.loss_func
            r = eval_separation(self.online_signal, target_t, None, cs.sdr_type, cs.zero_mean, cs.take_log, cs.EPS)
            on_perm, on_rows = r["perm"], r["sheet"][:, :2]
        else:
            _, on_perm = self.criterion_separation(self.online_signal, target_t, return_incides=True)
            on_rows = sisdr_under_perm(self.online_signal, target_t, on_perm)
        self.online_signal = _pit.reorder_source_mse(self.online_signal, on_perm)
        self.reference_sisdr.append(torch.mean(ref_rows).item())
        self.online_sisdr.append(torch.mean(on_rows).item())
        self.reference_sisdr_rows.append(ref_rows.cpu())
        self.online_sisdr_rows.append(on_rows.cpu())
        self.reset()
