"""One evaluation step of the reference's ``test.py`` on the device.

``test.py:129-181`` scores every utterance with the criterion built from the shipped config
(``CombinedLoss(PITLossWrapper(pairwise_neg_sisdr, "pw_mtx"), PITLossWrapper(BinaryCrossEntropyLoss_Mean(), "pw_pt"))``,
``test.py:49-64``), ``calc_sisdr`` of the reordered estimates and of the mixture, ``pit_si_sdr`` / ``pit_snr`` of both,
``si_sdri``, the per-speaker confusion counts of the VAD track and ``calc_vad`` of the masks. Every one of the
separation numbers is a closed form of 16 sums over the utterance's five rows; ``sepvad_eval_separation``
(csrc/eval.hip) reads the rows once and returns all of them, ``sepvad_eval_vad`` does the VAD track.

* ``eval_separation`` / ``eval_vad``: the two C-ABI entries on torch tensors.
* ``score_batch``: the whole step; dict of device tensors, no host synchronisation.

Forward-only: an input that requires grad under grad mode is refused. Inputs are ROCm tensors; no CPU path.
"""
from __future__ import annotations

import torch

from . import native as _native

SDR_TYPES = {"sisdr": 0, "sdsdr": 1, "snr": 2}  # SEPVAD_SDR_* (include/sepvad.h)
# SEPVAD_EV_* columns of the score sheet
SHEET_COLUMNS = ("si_sdr_speaker0", "si_sdr_speaker1", "si_sdr_start_speaker0", "si_sdr_start_speaker1",
                 "pit_si_sdr", "pit_snr", "pit_si_sdr_start", "pit_snr_start")
MEANS = ("loss", "pit_si_sdr", "pit_snr", "si_sdri")  # SEPVAD_EV_MEAN_*
MASK_BINS = 257


def refuse_grad(what, *tensors):
    """The native criterion has no backward: refuse inputs that would expect one."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what}: forward-only (no backward is built), but an input requires grad; call it under "
                           "torch.no_grad() or detach the inputs")


def eval_separation(est, tgt, mix=None, sdr_type="sisdr", zero_mean=True, take_log=True, eps=1e-8, sheet=True,
                    scratch=None):
    """sepvad_eval_separation: est, tgt [B, 2, N], mix [B, N] or None -> dict of device tensors
    pw [B, 2, 2] (estimate i against target j), min_loss [B], perm [B, 2] int64 (perm[b, j] = the estimate assigned
    to target j), sheet [B, 8] (SHEET_COLUMNS; None when sheet=False), means [4] (MEANS), and scratch: the uint8 buffer
    the call used (the argument, or the stream's shared one), whose moment partials sepvad_criterion_coef reads."""
    what = "eval_separation"
    if sdr_type not in SDR_TYPES:
        raise ValueError(f"{what}: sdr_type must be one of {sorted(SDR_TYPES)}, got {sdr_type!r}")
    if est.dim() != 3 or est.shape != tgt.shape or est.shape[1] != 2:
        raise ValueError(f"{what}: expected est and tgt of one shape [B, 2, N], got {tuple(est.shape)} and "
                         f"{tuple(tgt.shape)}")
    if mix is not None and tuple(mix.shape) != (est.shape[0], est.shape[2]):
        raise ValueError(f"{what}: expected mix [B, N], got {tuple(mix.shape)}")
    dev = _native.require_device(what, est, tgt, mix)
    refuse_grad(what, est, tgt, mix)
    lib = _native.load_library()
    est, eld = _native.rows3(est)
    tgt, tld = _native.rows3(tgt)
    mld = 0
    if mix is not None:
        mix, mld = _native.rows2(mix)
    B, _, N = est.shape
    if scratch is None:
        scratch, _ = _native.scratch_for("sepvad_eval_scratch_bytes", dev, B, N)
    pw = torch.empty(B, 2, 2, dtype=torch.float32, device=dev)
    min_loss = torch.empty(B, dtype=torch.float32, device=dev)
    perm = torch.empty(B, 2, dtype=torch.int64, device=dev)
    sh = torch.empty(B, len(SHEET_COLUMNS), dtype=torch.float32, device=dev) if sheet else None
    means = torch.empty(len(MEANS), dtype=torch.float32, device=dev)
    rc = lib.sepvad_eval_separation(_native.ptr(est), eld, _native.ptr(tgt), tld, _native.ptr(mix), mld, B, N,
                                    SDR_TYPES[sdr_type], int(bool(zero_mean)), int(bool(take_log)), float(eps),
                                    _native.ptr(scratch), scratch.numel(), _native.ptr(pw),
                                    _native.ptr(min_loss), _native.ptr(perm), _native.ptr(sh), _native.ptr(means),
                                    _native.stream_ptr(dev))
    _native.check(rc, "sepvad_eval_separation")
    return dict(pw=pw, min_loss=min_loss, perm=perm, sheet=sh, means=means, scratch=scratch)


def _perm_arg(what, perm, B, dev):
    if perm is None:
        return None
    if perm.device != dev or tuple(perm.shape) != (B, 2):
        raise ValueError(f"{what}: perm must be a [B, 2] tensor on the inputs' device")
    return perm.to(torch.int64).contiguous()


def eval_vad(vad, labels, perm=None, masks=None, fix_labels=True):
    """sepvad_eval_vad: vad, labels [B, 2, T], perm [B, 2] int64 on the device or None, post-sigmoid masks
    [B, 2, 257, T] or None -> dict of device tensors bce_rows [B], bce_mean [], pw_ce [2, 2], conf [B, 2, 4] int32
    (tn, fp, fn, tp), labels (float32, 2 -> 1 when fix_labels: the argument itself if it is a contiguous float32
    tensor, which is then changed in place as the reference changes it), and with masks simple_vad [B, 2, T] int64
    and conf_simple [B, 2, 4]."""
    what = "eval_vad"
    if vad.dim() != 3 or vad.shape[1] != 2 or vad.shape != labels.shape:
        raise ValueError(f"{what}: expected vad and labels of one shape [B, 2, T], got {tuple(vad.shape)} and "
                         f"{tuple(labels.shape)}")
    dev = _native.require_device(what, vad, labels, masks)
    refuse_grad(what, vad, labels, masks)
    B, _, T = vad.shape
    if masks is not None and tuple(masks.shape) != (B, 2, MASK_BINS, T):
        raise ValueError(f"{what}: expected masks [B, 2, {MASK_BINS}, T], got {tuple(masks.shape)}")
    lib = _native.load_library()
    vad = vad.to(torch.float32).contiguous()
    lab = labels.to(torch.float32)  # combined_loss.py:130: the same tensor when it already is float32
    if not lab.is_contiguous():
        lab = lab.contiguous()
    perm = _perm_arg(what, perm, B, dev)
    bce_rows = torch.empty(B, dtype=torch.float32, device=dev)
    bce_mean = torch.empty((), dtype=torch.float32, device=dev)
    pw_ce = torch.empty(2, 2, dtype=torch.float32, device=dev)
    conf = torch.empty(B, 2, 4, dtype=torch.int32, device=dev)
    simple = conf_simple = None
    if masks is not None:
        masks = masks.to(torch.float32).contiguous()
        simple = torch.empty(B, 2, T, dtype=torch.int64, device=dev)
        conf_simple = torch.empty(B, 2, 4, dtype=torch.int32, device=dev)
    rc = lib.sepvad_eval_vad(_native.ptr(vad), _native.ptr(lab), int(bool(fix_labels)), _native.ptr(perm),
                             _native.ptr(masks), B, T, _native.ptr(bce_rows), _native.ptr(bce_mean),
                             _native.ptr(pw_ce), _native.ptr(conf), _native.ptr(simple), _native.ptr(conf_simple),
                             _native.stream_ptr(dev))
    _native.check(rc, "sepvad_eval_vad")
    out = dict(bce_rows=bce_rows, bce_mean=bce_mean, pw_ce=pw_ce, conf=conf, labels=lab)
    if masks is not None:
        out.update(simple_vad=simple, conf_simple=conf_simple)
    return out


class BinaryCrossEntropyLoss_Mean(torch.nn.Module):
    """model/combined_loss.py:120-138 (combined_loss re-exports it): pred_vad, target_vad [B, 2, T] -> the batch
    mean of the per-utterance weighted BCE sums (weight 0.36 for label 1, 0.64 for label 0; labels equal to 2 count
    as 1). A contiguous float32 target_vad is changed in place (2 -> 1), as the reference changes it. ``perm``
    ([B, 2] int64 on the device) scores pred_vad[b, perm[b, s]] against target_vad[b, s] without a reordered copy
    (what CombinedLoss needs)."""

    def forward(self, pred_vad, target_vad, perm=None):
        if pred_vad.dim() != 3 or pred_vad.shape[1] != 2:
            raise NotImplementedError("native BinaryCrossEntropyLoss_Mean: built for [B, 2, T] VAD tracks, got "
                                      f"{tuple(pred_vad.shape)}")
        return eval_vad(pred_vad, target_vad, perm)["bce_mean"]


def simple_vad(masks, perm=None):
    """calc_vad (Our_utils/utils_test.py:67-73) of masks [B, 2, 257, T] reordered by perm: [B, 2, T] int64."""
    what = "calc_vad"
    if masks.dim() != 4 or masks.shape[1] != 2 or masks.shape[2] != MASK_BINS:
        raise NotImplementedError(f"{what}: built for masks [B, 2, {MASK_BINS}, T], got {tuple(masks.shape)}")
    dev = _native.require_device(what, masks)
    refuse_grad(what, masks)
    B, _, _, T = masks.shape
    lib = _native.load_library()
    masks = masks.to(torch.float32).contiguous()
    perm = _perm_arg(what, perm, B, dev)
    simple = torch.empty(B, 2, T, dtype=torch.int64, device=dev)
    rc = lib.sepvad_eval_vad(None, None, 0, _native.ptr(perm), _native.ptr(masks), B, T, None, None, None, None,
                             _native.ptr(simple), None, _native.stream_ptr(dev))
    _native.check(rc, "sepvad_eval_vad")
    return simple


def score_batch(sep, target, mix=None, vad=None, labels=None, masks=None, sdr_type="sisdr", stoi_fs=None):
    """One test.py step (test.py:129-181) for a batch: sep, target [B, 2, N]; mix [B, N]; vad, labels [B, 2, T];
    post-sigmoid masks [B, 2, 257, T]. Returns a dict of device tensors:

    * of ``eval_separation``: pw, min_loss, perm, sheet, means, and the means by name: loss, pit_si_sdr, pit_snr and
      (with mix) si_sdri;
    * sep_reordered [B, 2, N] = reorder_source_mse(sep, perm);
    * with vad and labels, of ``eval_vad`` under that perm: bce_rows, bce_mean, pw_ce, conf, labels; with masks as
      well simple_vad and conf_simple; with masks alone simple_vad;
    * with stoi_fs (the waveforms' sampling rate: 8000, 10000 or 16000), the columns the reference's post-processing
      reads: stoi and estoi [B, 2] float64 (target j against the estimate perm assigns to it) and, with mix,
      initial_stoi and initial_estoi (target j against the mixture), all from one sepvad_stoi_ex call. Without
      stoi_fs the result is what it was before the argument existed.

    Launches: sepvad_eval_separation, the reordering copy (sepvad_stream_append) and, with a VAD track or masks,
    sepvad_eval_vad; nothing is synchronised and no index tensor is built on the host (perm stays on the device)."""
    from .pit import reorder_source_mse
    if (vad is None) != (labels is None):
        raise ValueError("score_batch: vad and labels go together")
    out = eval_separation(sep, target, mix, sdr_type=sdr_type)
    del out["scratch"]
    for i, name in enumerate(MEANS):
        if name != "si_sdri" or mix is not None:
            out[name] = out["means"][i]
    out["sep_reordered"] = reorder_source_mse(sep, out["perm"])
    if vad is not None:
        out.update(eval_vad(vad, labels, out["perm"], masks))
    elif masks is not None:
        out["simple_vad"] = simple_vad(masks, out["perm"])
    if stoi_fs is not None:
        out.update(_stoi_columns(sep, target, mix, out["perm"], stoi_fs))
    return out


def _stoi_columns(sep, target, mix, perm, fs_sig):
    """stoi / estoi [B, 2] (target j against the estimate perm assigns to it) and, with mix, initial_stoi /
    initial_estoi (target j against the mixture), float64, from one sepvad_stoi_ex call over 2B or 4B pairs. The pairs
    are addressed by row indices computed from perm on the device; with mix the estimate rows and the mixtures are
    first joined into one [3B, N] buffer (one base pointer per side), in their own order."""
    from . import metrics
    B, _, N = sep.shape
    dev = sep.device
    X = target.to(torch.float32).reshape(2 * B, N).contiguous()
    Y = sep.to(torch.float32).reshape(2 * B, N).contiguous()
    rows = torch.arange(2 * B, device=dev, dtype=torch.int64)
    yidx = (rows // 2) * 2 + perm.reshape(-1)
    xidx = rows
    if mix is not None:
        Y = torch.cat([Y, mix.to(torch.float32).reshape(B, N)])
        xidx = torch.cat([rows, rows])
        yidx = torch.cat([yidx, 2 * B + rows // 2])
    d, e, _ = metrics.stoi_both_pairs(X, Y, fs_sig, xidx.to(torch.int32), yidx.to(torch.int32))
    res = dict(stoi=d[:2 * B].reshape(B, 2), estoi=e[:2 * B].reshape(B, 2))
    if mix is not None:
        res.update(initial_stoi=d[2 * B:].reshape(B, 2), initial_estoi=e[2 * B:].reshape(B, 2))
    return res
