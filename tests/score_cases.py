"""Shared by test_score_cases_host.py (CPU) and test_gpu_score_regimes.py (device): the inputs that take the scoring
kernels (csrc/metrics.hip k_si_sdr / k_snr, csrc/eval.hip k_eval_moments / k_eval_finish) out of the 7 dB, unit-scale,
DC 0.1 regime of the other tests, their float64 truth, the float32 reference and an emulation of the kernels' arithmetic.

* ``CELLS``: the regime grid. ``make(cell)`` draws the rows (PCG64, fixed seeds, float32):
      t = amp (g + dc),  e = 0.8 t + nl amp g' + 0.5 amp dc   (same_dc: e = 0.8 t + nl amp g'),  mix = t0 + t1 + 0.2 amp g''
  estimate i follows target i, with the speakers of every odd utterance swapped, so both permutations occur and the
  two permutation losses differ by >= 1 dB (the host test asserts it for every cell with ``perm_gap``).
* ``truth(cell)`` / ``ref32(cell)``: the reference's formulas (calc_sisdr, signal_noise_ratio, PairwiseNegSDR and the
  score sheet of test.py) written two-pass and element-wise (centre, project, subtract, then sum), in float64 and in
  float32. ``oracle.torch_ref.si_sdr`` is the float32 SI-SDR itself.
* ``emulate(cell, fixed)``: the kernels' accumulation order on the CPU (per-thread sums over float4 groups in double,
  the xor-shuffle wave sum, the four waves, the chunks of eval.hip in order), then their closed forms; ``fixed=False``
  is the arithmetic as it shipped (raw moments), ``fixed=True`` the moments of the rows less their first sample.
  Products are rounded before they are added (the kernels fuse them); that is below what the emulation is read for.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

TOL_DB = 1e-3                                   # the project's gate for dB values (test_gpu_metrics.py)
EPS32 = float(torch.finfo(torch.float32).eps)   # calc_sisdr / signal_noise_ratio
EPS_PW = 1e-8                                   # PairwiseNegSDR's EPS
EV_CHUNK, THREADS = 4096, 256                   # csrc/sepvad_internal.h EV_CHUNK; SD_THREADS == EV_THREADS
SDR_TYPES = ("sisdr", "sdsdr", "snr")
SHEET_COLUMNS = ("si_sdr_speaker0", "si_sdr_speaker1", "si_sdr_start_speaker0", "si_sdr_start_speaker1",
                 "pit_si_sdr", "pit_snr", "pit_si_sdr_start", "pit_snr_start")


@dataclass(frozen=True)
class Cell:
    name: str
    kind: str            # grid | same_dc | scale | identical | zero | tiny
    N: int
    B: int
    dc: float = 0.0      # DC over the standard deviation of the target
    nl: float = 0.3      # residual level over the standard deviation of the target
    amp: float = 0.01
    same_dc: bool = False
    zero: str = ""       # "est" | "tgt" | "both": all-zero rows
    seed: int = 0
    zm_false: bool = True    # zero_mean=False is scored as well (its truth stays <= 80 dB)
    perm_gap: bool = True    # the two permutation losses differ by >= 1 dB in the truth

    def band(self):
        """The matched, zero-mean SI-SDR the cell is meant to have, dB: (lo, hi)."""
        if self.kind in ("zero", "tiny"):
            return None
        e = self.N * self.amp ** 2
        if self.kind == "identical":
            mid = 10 * math.log10((e + EPS32) / EPS32)
            return mid - 0.2, mid + 0.2
        # the float32 epsilon of calc_sisdr is part of the level: 71.3 dB, not 78, at N = 32 000 and nl = 1e-4
        mid = 10 * math.log10((0.64 * e + EPS32) / (self.nl ** 2 * e + EPS32))
        return mid - 1.5, mid + 1.5


def _cells():
    out, seed = [], 1000
    for N in (32000, 2_000_000):
        B = 2 if N == 32000 else 1
        for dc in (0, 10, 100, 1000):
            for nl in (0.3, 1e-2, 1e-3, 1e-4):
                seed += 1
                out.append(Cell(f"N{N}-dc{dc}-nl{nl:g}", "grid", N, B, dc, nl, seed=seed))
        # zero_mean=False up to 80 dB: the DC is the same multiple of the row on both sides
        for dc, nl in ((10, 0.3), (10, 1e-2), (10, 1e-3), (100, 0.3), (100, 1e-2), (1000, 0.3)):
            seed += 1
            out.append(Cell(f"N{N}-samedc{dc}-nl{nl:g}", "same_dc", N, B, dc, nl, same_dc=True, seed=seed))
    for amp in (1e-4, 3000.0):
        for nl in (0.3, 1e-3):
            seed += 1
            out.append(Cell(f"amp{amp:g}-nl{nl:g}", "scale", 32000, 2, 0, nl, amp=amp, seed=seed))
    for amp in (0.1, 3000.0):
        seed += 1
        # zero_mean=False would be 105 and 195 dB here: out of its 80 dB range
        out.append(Cell(f"identical-amp{amp:g}", "identical", 32000, 2, 0, 0.0, amp=amp, seed=seed, zm_false=False))
    for zero in ("est", "tgt", "both"):
        seed += 1
        out.append(Cell(f"zero-{zero}", "zero", 4097, 2, 0, 0.3, zero=zero, seed=seed, perm_gap=False))
    for N in (1, 2, 3, 5, 4097):
        seed += 1
        # one or two samples: the centred rows are zero or collinear, and the permutation losses tie
        out.append(Cell(f"tiny-N{N}", "tiny", N, 2, 10, 0.3, seed=seed, perm_gap=N >= 3))
    return tuple(out)


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
SMALL = tuple(c for c in CELLS if c.N <= 32000)
LARGE = tuple(c for c in CELLS if c.N > 32000)


@functools.lru_cache(maxsize=2)
def make(cell: Cell):
    """(est [B, 2, N], tgt [B, 2, N], mix [B, N]) float32 numpy arrays; drawn in double, rounded once."""
    rng = np.random.Generator(np.random.PCG64(cell.seed))
    B, N, amp = cell.B, cell.N, cell.amp
    tgt = amp * (rng.standard_normal((B, 2, N)) + cell.dc)
    est = 0.8 * tgt + cell.nl * amp * rng.standard_normal((B, 2, N))
    if not cell.same_dc:
        est += 0.5 * amp * cell.dc
    mix = tgt.sum(1) + 0.2 * amp * rng.standard_normal((B, N))
    est, tgt, mix = est.astype(np.float32), tgt.astype(np.float32), mix.astype(np.float32)
    if cell.kind == "identical":
        est = tgt.copy()
    if cell.zero in ("est", "both"):
        est[:] = 0
    if cell.zero in ("tgt", "both"):
        tgt[:] = 0
    est[1::2] = est[1::2, ::-1].copy()
    for a in (est, tgt, mix):
        a.setflags(write=False)
    return est, tgt, mix


# ---- the reference's formulas, element-wise, in the dtype of choice ----------------------------------------------

def si_sdr(p, t, zero_mean=True):
    """calc_sisdr (model/combined_loss.py:16-56) as oracle.torch_ref.si_sdr states it, float32 epsilon in any dtype."""
    if zero_mean:
        t = t - t.mean(-1, keepdim=True)
        p = p - p.mean(-1, keepdim=True)
    alpha = ((p * t).sum(-1, keepdim=True) + EPS32) / ((t ** 2).sum(-1, keepdim=True) + EPS32)
    ts = alpha * t
    return 10 * torch.log10(((ts ** 2).sum(-1) + EPS32) / (((ts - p) ** 2).sum(-1) + EPS32))


def snr(p, t, zero_mean=True):
    """signal_noise_ratio (model/metric.py:131-143), as _snr_ref of test_gpu_stoi.py."""
    if zero_mean:
        t = t - t.mean(-1, keepdim=True)
        p = p - p.mean(-1, keepdim=True)
    return 10 * torch.log10(((t ** 2).sum(-1) + EPS32) / (((t - p) ** 2).sum(-1) + EPS32))


def pairwise_neg_sdr(est, tgt, sdr_type="sisdr", zero_mean=True, take_log=True, eps=EPS_PW):
    """model/sdr.py:48-86 (ref_pw of test_gpu_eval.py, in the dtype of its inputs): [B, 2, N] -> [B, 2, 2]."""
    if zero_mean:
        est, tgt = est - est.mean(2, keepdim=True), tgt - tgt.mean(2, keepdim=True)
    s_t, s_e = tgt.unsqueeze(1), est.unsqueeze(2)
    if sdr_type in ("sisdr", "sdsdr"):
        proj = (s_e * s_t).sum(3, keepdim=True) * s_t / ((s_t ** 2).sum(3, keepdim=True) + eps)
    else:
        proj = s_t.repeat(1, 2, 1, 1)
    noise = s_e - s_t if sdr_type in ("sdsdr", "snr") else s_e - proj
    val = (proj ** 2).sum(3) / ((noise ** 2).sum(3) + eps)
    return -(10 * torch.log10(val + eps)) if take_log else -val


def best_perm(pw):
    """find_best_perm_factorial on the float32-rounded matrix: (min_loss float32 [B], perm [B, 2], gap [B])."""
    pw = pw.float()
    loss_id, loss_sw = (pw[:, 0, 0] + pw[:, 1, 1]) / 2, (pw[:, 1, 0] + pw[:, 0, 1]) / 2
    swap = loss_sw < loss_id
    perm = torch.where(swap[:, None], torch.tensor([[1, 0]]), torch.tensor([[0, 1]]))
    return torch.minimum(loss_id, loss_sw), perm, (loss_id - loss_sw).abs()


def _pit_max(metric, preds, tgt):
    m = torch.stack([torch.stack([metric(preds[:, p], tgt[:, t]) for p in range(2)], -1) for t in range(2)], 1)
    return torch.maximum((m[:, 0, 0] + m[:, 1, 1]) / 2, (m[:, 0, 1] + m[:, 1, 0]) / 2)


def score_sheet(est, tgt, mix, perm):
    """The score_batch sheet [B, 8] in SHEET_COLUMNS order and (pit_si_sdr, pit_snr, si_sdri) batch means."""
    B = est.shape[0]
    reordered = torch.stack([est[b][perm[b]] for b in range(B)])
    mix2 = mix.unsqueeze(1).repeat(1, 2, 1)
    own, start = si_sdr(reordered, tgt), si_sdr(mix2, tgt)
    sheet = torch.stack([own[:, 0], own[:, 1], start[:, 0], start[:, 1], _pit_max(si_sdr, est, tgt),
                         _pit_max(snr, est, tgt), _pit_max(si_sdr, mix2, tgt), _pit_max(snr, mix2, tgt)], 1)
    return sheet, sheet[:, 4].mean(), sheet[:, 5].mean(), sheet[:, 4].mean() - start.mean()


def _reference(cell: Cell, dtype):
    est, tgt, mix = (torch.tensor(a, dtype=dtype) for a in make(cell))
    out = {}
    for zm in (True, False):
        if not zm and not cell.zm_false:
            continue
        out["si", zm] = si_sdr(est, tgt, zm).double()          # [B, 2]: estimate s against target s
        out["snr", zm] = snr(est, tgt, zm).double()
        for ty in SDR_TYPES:
            out["pw", ty, zm] = pairwise_neg_sdr(est, tgt, ty, zm).double()
    min_loss, perm, gap = best_perm(out["pw", "sisdr", True])
    sheet, pit_si, pit_snr, si_sdri = score_sheet(est, tgt, mix, perm)
    out.update(min_loss=min_loss.double(), perm=perm, gap=gap.double(), sheet=sheet.double(),
               means=torch.stack([min_loss.double().mean(), pit_si.double(), pit_snr.double(), si_sdri.double()]))
    return out


@functools.lru_cache(maxsize=None)
def truth(cell: Cell):
    """Every number the device tests compare, float64, two-pass element-wise. Keys: ("si" | "snr", zero_mean) [B, 2];
    ("pw", sdr_type, zero_mean) [B, 2, 2]; of score_batch (sisdr, zero-mean): min_loss [B], perm [B, 2], gap [B],
    sheet [B, 8], means [4] = (loss, pit_si_sdr, pit_snr, si_sdri)."""
    return _reference(cell, torch.float64)


@functools.lru_cache(maxsize=None)
def ref32(cell: Cell):
    """The same formulas in float32: what the reference itself computes on these rows."""
    return _reference(cell, torch.float32)


# ---- the kernels' accumulation order -----------------------------------------------------------------------------

FLUSH = 4   # float4 groups a thread adds up on their own before they join its running sum (16 samples)


def _block_sum(v, flush=FLUSH):
    """Sum of the terms v [..., n] as one 256-thread workgroup adds them: thread q takes the float4 groups q, q + 256,
    ... in order, `flush` groups at a time into a sum of their own that then joins the thread's running sum (None: every
    term straight into the running sum, as k_si_sdr shipped); the last n % 4 terms go one each to threads 0 .. 2; then
    wave_sum (xor shuffles 32 .. 1) and the four waves in order. A chunk of eval.hip is one such block of 4 groups."""
    lead, n = v.shape[:-1], v.shape[-1]
    n4 = n // 4
    g = flush or 1
    steps = -(-n4 // (THREADS * g)) * g
    body = np.zeros(lead + (steps * THREADS * 4,))
    body[..., :n4 * 4] = v[..., :n4 * 4]
    body = np.moveaxis(body.reshape(lead + (steps, THREADS, 4)), -1, -2).reshape(lead + (steps // g, g * 4, THREADS))
    if steps == 0:
        s = np.zeros(lead + (THREADS,))
    elif flush:
        part = np.zeros(lead + (steps // g, THREADS))
        for j in range(g * 4):
            part = part + body[..., j, :]
        s = np.cumsum(part, axis=-2)[..., -1, :]            # cumsum adds strictly in order
    else:
        s = np.cumsum(body.reshape(lead + (steps * 4, THREADS)), axis=-2)[..., -1, :]
    tail = n - n4 * 4
    s[..., :tail] = s[..., :tail] + v[..., n4 * 4:]
    w = s.reshape(lead + (THREADS // 64, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    tot = np.zeros(lead)
    for i in range(THREADS // 64):
        tot = tot + w[..., i, 0]
    return tot


def _row_sum(v):
    """k_si_sdr / k_snr: one workgroup streams the whole row."""
    return float(_block_sum(v))


def _row_sum_shipped(v):
    return float(_block_sum(v, None))


def _chunked_sum(v):
    """k_eval_moments + k_eval_finish: one workgroup per EV_CHUNK samples, the partials added in chunk order."""
    n = v.shape[0]
    full = n // EV_CHUNK
    parts = list(_block_sum(v[:full * EV_CHUNK].reshape(full, EV_CHUNK))) if full else []
    if n > full * EV_CHUNK:
        parts.append(float(_block_sum(v[full * EV_CHUNK:])))
    tot = 0.0
    for x in parts:
        tot += float(x)
    return tot


def _moments(rows, kp, kt, summer, pivot, memo):
    """(sum p, sum t, <p,p>, <t,t>, <p,t>, pivot of p, pivot of t) of the float32 rows rows[kp], rows[kt] in double;
    memo keeps what a pair shares with the other pairs of its utterance."""
    def shifted(k):
        key = ("x", k, pivot)
        if key not in memo:
            c = float(rows[k][0]) if pivot else 0.0
            memo[key] = (rows[k].astype(np.float64) - c, c)
        return memo[key]

    def single(k):
        key = ("s", k, pivot, summer)
        if key not in memo:
            x = shifted(k)[0]
            memo[key] = (summer(x), summer(x * x))
        return memo[key]
    key = ("m", kp, kt, pivot, summer)
    if key not in memo:
        (x, cp), (y, ct) = shifted(kp), shifted(kt)
        (sp, pp), (st, tt) = single(kp), single(kt)
        memo[key] = (sp, st, pp, tt, summer(x * y), cp, ct)
    return memo[key]


def _centred(m, N, zero_mean, undo):
    """<p,p>, <t,t>, <p,t> of the (zero-mean) rows from the moments of the shifted rows. undo: zero_mean=False
    takes the shift out again in closed form (eval.hip); k_si_sdr does not shift there."""
    sp, st, pp, tt, pt, cp, ct = m
    if zero_mean:
        return pp - sp * sp / N, tt - st * st / N, pt - sp * st / N
    if undo:  # one expression for all three: identical rows keep <p,p> == <t,t> == <p,t> to the bit
        def raw(xy, sx, sy, cx, cy):
            return cx * sy + (cy * sx + (N * cx * cy + xy))
        return raw(pp, sp, sp, cp, cp), raw(tt, st, st, ct, ct), raw(pt, sp, st, cp, ct)
    return pp, tt, pt


def _log10(x):
    return math.log10(x) if x > 0 else -math.inf


def closed_si_sdr(pp, tt, pt):
    """k_si_sdr, and EVK_SI of eval.hip."""
    alpha = (pt + EPS32) / (tt + EPS32)
    sig = alpha * alpha * tt
    noise = max(sig - 2.0 * alpha * pt + pp, 0.0)
    return 10.0 * _log10((sig + EPS32) / (noise + EPS32))


def closed_snr(pp, tt, pt):
    """k_snr, and EVK_SNR of eval.hip."""
    noise = max(tt - 2.0 * pt + pp, 0.0)
    return 10.0 * _log10((tt + EPS32) / (noise + EPS32))


def closed_pw(sdr_type, pp, tt, pt, eps=EPS_PW):
    """ev_score of eval.hip for one PairwiseNegSDR cell (take_log)."""
    al = 1.0 if sdr_type == "snr" else pt / (tt + eps)
    proj = al * al * tt
    noise = max(pp - 2.0 * al * pt + proj if sdr_type == "sisdr" else pp - 2.0 * pt + tt, 0.0)
    return -10.0 * _log10(proj / (noise + eps) + eps)


@functools.lru_cache(maxsize=None)
def emulate(cell: Cell, fixed: bool):
    """The device's numbers by emulation, float64 before the float32 store: ("si" | "snr", zero_mean) [B, 2] of
    k_si_sdr / k_snr; ("pw", sdr_type, zero_mean) [B, 2, 2] and ("sheet_si" | "sheet_snr") [B, 2, 2] (target t,
    estimate p; zero-mean) of k_eval_moments / k_eval_finish."""
    est, tgt, _ = make(cell)
    B, N = cell.B, cell.N
    zms = (True, False) if cell.zm_false else (True,)
    out = {(k, zm): np.zeros((B, 2)) for k in ("si", "snr") for zm in zms}
    out.update({("pw", ty, zm): np.zeros((B, 2, 2)) for ty in SDR_TYPES for zm in zms})
    out.update(sheet_si=np.zeros((B, 2, 2)), sheet_snr=np.zeros((B, 2, 2)))
    for b in range(B):
        rows, memo = {("e", 0): est[b, 0], ("e", 1): est[b, 1], ("t", 0): tgt[b, 0], ("t", 1): tgt[b, 1]}, {}
        for s in range(2):
            for zm in zms:
                # k_si_sdr / k_snr shift by the rows' first samples only where they centre
                m = _moments(rows, ("e", s), ("t", s), _row_sum if fixed else _row_sum_shipped, fixed and zm, memo)
                c = _centred(m, N, zm, False)
                out["si", zm][b, s], out["snr", zm][b, s] = closed_si_sdr(*c), closed_snr(*c)
        for i in range(2):
            for j in range(2):
                m = _moments(rows, ("e", i), ("t", j), _chunked_sum, fixed, memo)
                for zm in zms:
                    c = _centred(m, N, zm, True)
                    for ty in SDR_TYPES:
                        out["pw", ty, zm][b, i, j] = closed_pw(ty, *c)
                c = _centred(m, N, True, True)
                out["sheet_si"][b, j, i], out["sheet_snr"][b, j, i] = closed_si_sdr(*c), closed_snr(*c)
    return out
