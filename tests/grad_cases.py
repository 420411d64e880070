"""Shared by the training-criterion tests (test_train_criterion_host.py, test_gpu_train_criterion.py) and
tools/train_criterion_profile.py:

* ``restated_criterion``: the reference's criterion (model/sdr.py:48-86, model/pit_wrapper.py:287-312,
  model/combined_loss.py:93-138) restated element-wise in torch, in the dtype of its inputs: float64 autograd through it
  is the truth the GPU gradients are gated against; in float32 it is the formulation a trainer runs today.
* ``mirror_grad_est`` / ``mirror_grad_vad``: csrc/criterion.hip's closed form in numpy float64 from the same shifted
  moments, rounded once to float32. It shows on a CPU what the kernel's arithmetic can reach.
* ``est_gate`` / ``VAD_GATE``: the gates, set from the number formats (below), never from a GPU result.
* ``regime_grid``: SDR in {0, 20, 40, 60, 80} dB x DC in {0, 100 sigma} at N = 4101.

The gate for grad_est, per row: |g - g_f64| <= rowmax |g_f64| (EST_GATE_ROUND + EST_GATE_CANCEL 10^(SDR_row / 10)).
EST_GATE_ROUND = 2^-22 is four float32 output roundings. EST_GATE_CANCEL = 2^-48 is 16 double ulps times the
cancellation of |n|^2 = <e,e> - 2 a <e,t> + a^2 <t,t>, which loses 10^(SDR / 10) of the moments' precision.
Measured on the mirror (test_mirror_reaches_the_gate prints it): DESIGN.md section 14.
"""
import numpy as np
import torch

PW_CASES = [("sisdr", True, True), ("sisdr", False, True), ("sdsdr", True, True), ("sdsdr", False, True),
            ("snr", True, True), ("snr", False, True), ("sisdr", True, False)]  # make_eval_golden.PW_CASES
EST_GATE_ROUND = 2.0 ** -22
EST_GATE_CANCEL = 2.0 ** -48
VAD_GATE = 2.0 ** -22   # element-wise, relative: four float32 roundings of a quotient evaluated in double
REGIME_SDR_DB = (0, 20, 40, 60, 80)
REGIME_DC_SIGMA = (0, 100)
REGIME_N = 4101


def pw_key(sdr_type, zero_mean, take_log):
    return f"pw_{sdr_type}_zm{int(zero_mean)}" + ("" if take_log else "_nolog")


# ---- the restatement ---------------------------------------------------------------------------------------------

def restated_pw(est, tgt, sdr_type="sisdr", zero_mean=True, take_log=True, eps=1e-8):
    """model/sdr.py:54-86 -> (pw [B, 2, 2], ratio [B, 2, 2] = |proj|^2 / |noise|^2 without EPS, for the gate's SDR)."""
    if zero_mean:
        est, tgt = est - est.mean(2, keepdim=True), tgt - tgt.mean(2, keepdim=True)
    s_t, s_e = tgt.unsqueeze(1), est.unsqueeze(2)
    if sdr_type in ("sisdr", "sdsdr"):
        proj = (s_e * s_t).sum(3, keepdim=True) * s_t / ((s_t ** 2).sum(3, keepdim=True) + eps)
    else:
        proj = s_t.repeat(1, 2, 1, 1)
    noise = s_e - s_t if sdr_type in ("sdsdr", "snr") else s_e - proj
    p, n = (proj ** 2).sum(3), (noise ** 2).sum(3)
    val = p / (n + eps)
    return (-(10 * torch.log10(val + eps)) if take_log else -val), (p / n.clamp(min=1e-300)).detach()


def restated_criterion(est, tgt, vad=None, labels=None, sdr_type="sisdr", zero_mean=True, take_log=True, eps=1e-8):
    """-> dict(sep, vad (or None), perm [B, 2] int64, sdr_db [B, 2]: the SDR of estimate row i against its paired
    target, for the gate). Differentiable with respect to est and vad; the permutation is chosen on the detached
    pairwise matrix rounded to float32, first minimum, as find_best_perm_factorial on the trainer's float32 matrix."""
    pw, ratio = restated_pw(est, tgt, sdr_type, zero_mean, take_log, eps)
    pw32 = pw.detach().float()
    swap = ((pw32[:, 1, 0] + pw32[:, 0, 1]) / 2) < ((pw32[:, 0, 0] + pw32[:, 1, 1]) / 2)
    loss_id, loss_sw = (pw[:, 0, 0] + pw[:, 1, 1]) / 2, (pw[:, 1, 0] + pw[:, 0, 1]) / 2
    sep = torch.where(swap, loss_sw, loss_id).mean()
    perm = torch.where(swap[:, None], torch.tensor([[1, 0]], device=pw.device), torch.tensor([[0, 1]], device=pw.device))
    paired = torch.stack([ratio[:, 0].gather(1, perm[:, :1])[:, 0], ratio[:, 1].gather(1, perm[:, 1:])[:, 0]], 1)
    out = dict(sep=sep, vad=None, perm=perm, sdr_db=10 * torch.log10(paired.double().clamp(min=1e-300)))
    if vad is not None:
        y = torch.where(labels == 2, torch.ones_like(labels), labels).to(vad.dtype)
        pred = torch.stack([vad[b][perm[b]] for b in range(vad.shape[0])])
        w = y * 0.36 + 0.64 * (1 - y)
        bce = torch.nn.functional.binary_cross_entropy(pred, y, reduction="none") * w
        out["vad"] = bce.sum((-1, -2)).mean()
    return out


def autograd_truth(est, tgt, vad=None, labels=None, **kw):
    """float64 autograd of the restatement on float32-valued inputs -> (result dict, grad_est, grad_vad or None)."""
    e = est.double().clone().requires_grad_(True)
    v = vad.double().clone().requires_grad_(True) if vad is not None else None
    r = restated_criterion(e, tgt.double(), v, labels.double() if labels is not None else None, **kw)
    r["sep"].backward()
    if v is not None:
        r["vad"].backward()
    return r, e.grad, (v.grad if v is not None else None)


# ---- the kernel's closed form ------------------------------------------------------------------------------------

def mirror_grad_est(est, tgt, perm, sdr_type="sisdr", zero_mean=True, take_log=True, eps=1e-8, g_sep=1.0):
    """csrc/criterion.hip in numpy: float32 arrays est, tgt [B, 2, N], perm [B, 2] -> float32 grad [B, 2, N]. The
    moments are those of the rows less their first sample, as k_eval_moments takes them."""
    est, tgt = np.asarray(est, np.float32), np.asarray(tgt, np.float32)
    B, _, N = est.shape
    out = np.empty_like(est)
    Nd = float(N)
    for b in range(B):
        for i in range(2):
            j = int(perm[b][i])
            e, t = est[b, i].astype(np.float64), tgt[b, j].astype(np.float64)
            cp, ct = e[0], t[0]
            x, y = e - cp, t - ct
            sp, st, qp, qt, xy = x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum()
            if zero_mean:
                pp, tt, pt = qp - sp * sp / Nd, qt - st * st / Nd, xy - sp * st / Nd
                me, mt = cp + sp / Nd, ct + st / Nd
            else:
                pp = qp + 2 * cp * sp + Nd * cp * cp
                tt = qt + 2 * ct * st + Nd * ct * ct
                pt = xy + cp * st + ct * sp + Nd * cp * ct
                me = mt = 0.0
            pp, tt = max(pp, 0.0), max(tt, 0.0)
            E = tt + eps
            al = 1.0 if sdr_type == "snr" else pt / E
            P = al * al * tt
            noise = max(pp - 2 * al * pt + P if sdr_type == "sisdr" else pp - 2 * pt + tt, 0.0)
            D = noise + eps
            r = P / D
            dl = -(10.0 / np.log(10.0)) / (r + eps) if take_log else -1.0
            c_t = {"sisdr": dl * (2 * al / (E * D)) * (tt + eps * P / D), "sdsdr": dl * 2 * al * tt / (E * D),
                   "snr": 0.0}[sdr_type]
            c_n = -dl * 2 * P / (D * D)
            a_res = al if sdr_type == "sisdr" else 1.0
            G = g_sep / (2.0 * B)
            tp = t - mt
            out[b, i] = ((G * c_n) * ((e - me) - a_res * tp) + (G * c_t) * tp).astype(np.float32)
    return out


def mirror_grad_vad(vad, labels, perm, g_vad=1.0):
    """k_crit_grad_vad in numpy: float32 vad, labels [B, 2, T], perm [B, 2] -> float32 grad [B, 2, T]."""
    vad, labels = np.asarray(vad, np.float32), np.asarray(labels, np.float32)
    B = vad.shape[0]
    out = np.empty_like(vad)
    for b in range(B):
        for s in range(2):
            src = int(perm[b][s])
            p = vad[b, src].astype(np.float64)
            y = labels[b, s].astype(np.float64)
            y = np.where(y == 2, 1.0, y)
            w = y * 0.36 + 0.64 * (1 - y)
            den = np.maximum(p * (1 - p), float(np.float32(1e-12)))
            out[b, src] = ((g_vad / B) * (w * (p - y) / den)).astype(np.float32)
    return out


# ---- gates -------------------------------------------------------------------------------------------------------

def est_gate(grad64, sdr_db):
    """[B, 2, 1]: the allowed |g - g_f64| of every row."""
    rowmax = grad64.abs().amax(-1, keepdim=True)
    return rowmax * (EST_GATE_ROUND + EST_GATE_CANCEL * 10.0 ** (sdr_db.unsqueeze(-1) / 10.0))


def est_error_in_gates(grad, grad64, sdr_db):
    """The worst |g - g_f64| / gate over the rows (0 / 0 = 0: a zero row must be met exactly), and per row the error
    in units of 2^-24 rowmax (for the tables)."""
    d = (torch.as_tensor(grad).double() - grad64).abs().amax(-1, keepdim=True)
    gate = est_gate(grad64, sdr_db)
    ratio = torch.where(d == 0, torch.zeros_like(d), d / gate)
    rowmax = grad64.abs().amax(-1, keepdim=True)
    ulps = torch.where(d == 0, torch.zeros_like(d), d / (rowmax * 2.0 ** -24))
    return float(ratio.max()), ulps[..., 0]


def vad_within_gate(grad, grad64):
    d = (torch.as_tensor(grad).double() - grad64).abs()
    return bool((d <= VAD_GATE * grad64.abs()).all()), float((d / grad64.abs().clamp(min=1e-300)).max())


# ---- regimes -----------------------------------------------------------------------------------------------------

def regime_case(sdr_db, dc_sigma, seed=0, N=REGIME_N):
    """B = 2 (the second utterance's speakers swapped), float32: est = 0.8 t + residual at sdr_db below the projection,
    both on a DC of dc_sigma standard deviations."""
    gen = torch.Generator().manual_seed(1000 * sdr_db + dc_sigma + seed)
    t = torch.randn(2, 2, N, generator=gen, dtype=torch.float64)
    n = torch.randn(2, 2, N, generator=gen, dtype=torch.float64)
    t = t - t.mean(-1, keepdim=True)
    n = n - n.mean(-1, keepdim=True)
    n = n - (n * t).sum(-1, keepdim=True) / (t * t).sum(-1, keepdim=True) * t
    n = n * (0.8 * t.norm(dim=-1, keepdim=True) / n.norm(dim=-1, keepdim=True)) * 10.0 ** (-sdr_db / 20.0)
    est = (0.8 * t + n + dc_sigma).float()
    tgt = (t + dc_sigma).float()
    est[1] = est[1].flip(0)
    return est, tgt


def regime_grid():
    return [(s, d) for s in REGIME_SDR_DB for d in REGIME_DC_SIGMA]
