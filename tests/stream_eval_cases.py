"""Plain-torch restatement of the reference's streaming evaluation with known targets
(``model/online_class_known_targets.py:85-154``): the padding, the window loop with its three similarity modes, the
stitched signal and both scores. Test infrastructure only; pinned to the reference's own run by
``tests/golden/golden_stream_eval_*.npz`` (``tests/golden/make_stream_eval_golden.py``).

The window loop is computed in the dtype of its inputs, so the same functions give the float32 restatement and the
float64 values the kernel tests compare against; the two scores are taken in float64 on the signals as they are.
Also the fixture's readers (inputs regenerated from the seed, the reference's stitched signal, which decisions count).
"""
from __future__ import annotations

import hashlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FS, MAX_LEN = 16000, 3
MODES = ("none", "l1", "sisdr")
MODE_ID = {"none": 0, "l1": 1, "sisdr": 2}  # SEPVAD_SE_*

# The fixture's cases: (name, N, save_sec, seed). make_batch(2, N, seed) mixtures and their sources.
CASES = (("rem", 70000, 1, 4100), ("short", 30000, 1, 4300), ("half", 64000, 0.5, 4250))


def pad_signals(mix, tgt, save_sec, fs=FS, max_len=MAX_LEN):
    """Reference :86-98 -> (padded mixture, padded targets, K, W, H, P)."""
    pad = torch.nn.functional.pad
    W = fs * max_len
    if mix.shape[-1] < W:
        mix, tgt = pad(mix, (0, W - mix.shape[-1])), pad(tgt, (0, W - tgt.shape[-1]))
    P = int(fs * (max_len - save_sec))
    mix, tgt = pad(mix, (P, 0)), pad(tgt, (P, 0))
    r = (mix.shape[-1] - W) % (fs * save_sec)
    if r:
        mix, tgt = pad(mix, (0, int(r))), pad(tgt, (0, int(r)))
    K = int(np.floor((mix.shape[-1] - W) / (fs * save_sec))) + 1
    return mix, tgt, K, W, int(np.floor(fs * save_sec)), P


def si_sdr(preds, target):
    """calc_sisdr (model/combined_loss.py:16-56), zero_mean=True; eps of float32 whatever the dtype, as the device has it."""
    eps = torch.finfo(torch.float32).eps
    target = target - target.mean(dim=-1, keepdim=True)
    preds = preds - preds.mean(dim=-1, keepdim=True)
    alpha = ((preds * target).sum(-1, keepdim=True) + eps) / ((target ** 2).sum(-1, keepdim=True) + eps)
    ts = alpha * target
    return 10 * torch.log10(((ts ** 2).sum(-1) + eps) / (((ts - preds) ** 2).sum(-1) + eps))


def pairwise_neg_sisdr(est, tgt, eps=1e-8):
    """PairwiseNegSDR("sisdr") (model/sdr.py:48-86): [B, 2, 2], estimate i against target j."""
    tgt = tgt - tgt.mean(dim=2, keepdim=True)
    est = est - est.mean(dim=2, keepdim=True)
    s_t, s_e = tgt.unsqueeze(1), est.unsqueeze(2)
    dot = (s_e * s_t).sum(3, keepdim=True)
    proj = dot * s_t / ((s_t ** 2).sum(3, keepdim=True) + eps)
    sdr = (proj ** 2).sum(3) / (((s_e - proj) ** 2).sum(3) + eps)
    return -10 * torch.log10(sdr + eps)


def best_perm(pw):
    """find_best_perm_factorial (model/pit_wrapper.py:287-312) for two sources: (min loss [B], perm [B, 2], the
    identity's loss minus the swap's [B]); the first minimum wins, so a tie keeps the identity."""
    loss_id, loss_sw = (pw[:, 0, 0] + pw[:, 1, 1]) / 2, (pw[:, 1, 0] + pw[:, 0, 1]) / 2
    swap = (loss_sw < loss_id).to(torch.int64)
    return torch.minimum(loss_id, loss_sw), torch.stack([swap, 1 - swap], dim=1), loss_id - loss_sw


def pw_l1(est, ref):
    """get_pw_losses with nn.L1Loss() (model/pit_wrapper.py:149-177): one scalar per pair, over batch and samples ->
    [1, 2, 2]."""
    return torch.stack([torch.stack([(est[:, e] - ref[:, t]).abs().mean() for t in range(2)]) for e in range(2)])[None]


def pw_sisdr(est, ref):
    """get_pw_losses with calc_sisdr_loss: per-row losses -> [B, 2, 2]."""
    return torch.stack([torch.stack([-si_sdr(est[:, e], ref[:, t]) for t in range(2)], dim=1) for e in range(2)], dim=1)


def reorder(x, perm):
    return torch.stack([x[b][perm[b]] for b in range(x.shape[0])])


def window_loop(preds, tgt, H, mode):
    """Reference :101-123 on the windows' separations preds [K, B, 2, W] (window k starts at sample k H of the padded
    targets tgt). Returns perm [K, B, 2] (what each window is appended under), perm_tgt, pw_tgt [K, B, 2, 2],
    gap_tgt [K, B], pw_sim [K, G, 2, 2] and gap_sim [K, G] (G = B for "sisdr", 1 for "l1"; None for "none") and the
    stitched signal online [B, 2, K H]."""
    K, B, _, W = preds.shape
    online = None
    out = dict(perm=[], perm_tgt=[], pw_tgt=[], gap_tgt=[], pw_sim=[], gap_sim=[])
    for k in range(K):
        pred = preds[k]
        pw = pairwise_neg_sisdr(pred, tgt[:, :, k * H: k * H + W])
        _, perm, gap = best_perm(pw)
        out["perm_tgt"].append(perm); out["pw_tgt"].append(pw); out["gap_tgt"].append(gap)
        if mode != "none":
            if k == 0:
                online = pred[:, :, W - H:]                      # the un-reordered seed (:109-111)
            n_on = online.shape[-1]
            pred_sim = pred[:, :, max(0, W - H - n_on): W - H]   # :112
            online_sim = online[:, :, max(0, n_on - (W - H)):]   # :113
            pws = pw_l1(pred_sim, online_sim) if mode == "l1" else pw_sisdr(pred_sim, online_sim)
            _, perm, gap = best_perm(pws)
            perm = perm.expand(B, 2)
            out["pw_sim"].append(pws); out["gap_sim"].append(gap)
        out["perm"].append(perm)
        tail = reorder(pred, perm)[:, :, W - H:]
        online = tail if k == 0 else torch.cat((online, tail), dim=-1)
    res = {k: (torch.stack(v) if v else None) for k, v in out.items()}
    res["online"] = online
    return res


def calc_online(forward, mix, tgt, save_sec, mode):
    """The whole of calc_online (:85-154) on a forward callable x [B, N] -> sep [B, 2, N]: window_loop's dict plus
    reference_rows / online_rows [B, 2] (calc_sisdr of both scores), their means, and the padded signals."""
    mix, tgt, K, W, H, P = pad_signals(mix, tgt, save_sec)
    offs = [int(np.floor(FS * k * save_sec)) for k in range(K)]
    assert offs == [k * H for k in range(K)]
    preds = torch.stack([forward(mix[:, o: o + W]) for o in offs])
    res = window_loop(preds, tgt, H, mode)
    full = forward(mix)
    _, perm, _ = best_perm(pairwise_neg_sisdr(full, tgt))
    t1 = int(np.floor(FS * (MAX_LEN + (K - 1) * save_sec)))
    tgt_t = tgt[:, :, P:t1]
    # the two scores in float64 on the signals as they are: what is left is the forward's own rounding
    res["reference_rows"] = si_sdr(reorder(full, perm)[:, :, P:t1].double(), tgt_t.double())
    _, perm, _ = best_perm(pairwise_neg_sisdr(res["online"], tgt_t))
    res["online_final"] = reorder(res["online"], perm)
    res["online_rows"] = si_sdr(res["online_final"].double(), tgt_t.double())
    res["reference_sisdr"], res["online_sisdr"] = res["reference_rows"].mean(), res["online_rows"].mean()
    res.update(mix=mix, tgt=tgt, K=K, W=W, H=H, P=P)
    return res


def align_hop0(a, b, H, per_batch):
    """The stitched signal a [B, 2, L] with its speakers exchanged wherever that brings its first hop closer to b's
    (per row, or for the whole batch when the similarity PIT is batch-global): window 0's similarity decision sits on
    a near-tie in the reference itself (the left pad leaves the window silent before its last hop), and every later
    window follows it."""
    a, b = np.asarray(a), np.asarray(b)
    d_id = np.abs(a[:, :, :H] - b[:, :, :H]).reshape(a.shape[0], -1).max(axis=1)
    d_sw = np.abs(a[:, ::-1, :H] - b[:, :, :H]).reshape(a.shape[0], -1).max(axis=1)
    swap = d_sw < d_id
    if per_batch:
        swap = np.full_like(swap, d_sw.max() < d_id.max())
    out = a.copy()
    out[swap] = a[swap][:, ::-1]
    return out, swap


def synthetic_windows(B, W, H, K, seed, swaps=None, noise=0.05):
    """Windows cut from target + noise with chosen per-window swaps, so that every PIT gap is wide: returns
    (preds [K, B, 2, W], tgt [B, 2, (K - 1) H + W]) float32. swaps [K, B] bool: the window's speakers exchanged."""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = (K - 1) * H + W
    t = np.arange(L)
    tgt = np.stack([np.stack([np.sin(2 * np.pi * (0.011 + 0.004 * b) * t + b) * (1 + 0.3 * np.sin(0.002 * t)),
                              0.8 * np.sign(np.sin(2 * np.pi * (0.0037 + 0.001 * b) * t)) * np.cos(0.05 * t)])
                    for b in range(B)]).astype(np.float32)
    tgt += (0.02 * rng.standard_normal(tgt.shape)).astype(np.float32)
    preds = np.empty((K, B, 2, W), np.float32)
    for k in range(K):
        w = tgt[:, :, k * H: k * H + W] + (noise * rng.standard_normal((B, 2, W))).astype(np.float32)
        if swaps is not None:
            w[swaps[k]] = w[swaps[k]][:, ::-1]
        preds[k] = w
    return torch.from_numpy(preds), torch.from_numpy(tgt)


# ---- the fixture ----------------------------------------------------------------------------------------------

def load_case(name):
    return np.load(os.path.join(GOLDEN, f"golden_stream_eval_{name}.npz"))


def case_inputs(g):
    """The fixture's inputs, regenerated from its seed and checked against its SHA-256."""
    from sep_tfanet_vad_amd import synth
    mix, srcs = synth.make_batch(2, int(g["N"]), int(g["seed"]))
    mix, srcs = mix.astype(np.float32), srcs.astype(np.float32)
    assert hashlib.sha256(np.ascontiguousarray(mix).tobytes()).hexdigest() == str(g["mix_sha256"])
    assert hashlib.sha256(np.ascontiguousarray(srcs).tobytes()).hexdigest() == str(g["sources_sha256"])
    return torch.from_numpy(mix), torch.from_numpy(srcs)


def stitched_of(g, mode):
    """The reference's stitched signal of a mode: the fixture's un-permuted hops under that mode's permutations."""
    perm, raw = g[f"{mode}_perm_f32"], g["raw"]
    K = perm.shape[0]
    hops = raw.reshape(2, 2, K, -1)
    out = np.empty_like(hops)
    for k in range(K):
        for b in range(2):
            out[b, :, k] = hops[b, perm[k, b], k]
    return out.reshape(2, 2, -1)


def gap_of(pw):
    return np.abs((pw[..., 0, 0] + pw[..., 1, 1]) / 2 - (pw[..., 1, 0] + pw[..., 0, 1]) / 2)


def check_perms(g, mode, perm, perm_tgt, swap):
    """Decided decisions are equal: every target PIT, and the similarity PIT of windows >= 1 once the rows whose
    window 0 fell the other way (swap [B]) are exchanged throughout. The fixture's maker asserts that these are all
    decided (gaps >= l1_gap_min / db_gap_min)."""
    assert gap_of(g[f"{mode}_pw_tgt_f32"]).min() >= float(g["db_gap_min"])
    assert np.array_equal(np.asarray(perm_tgt), g[f"{mode}_perm_tgt_f32"])
    if mode == "none":
        assert np.array_equal(np.asarray(perm), g["none_perm_f32"])
        return
    lim = float(g["l1_gap_min"]) if mode == "l1" else float(g["db_gap_min"])
    assert gap_of(g[f"{mode}_pw_sim_f32"])[1:].min() >= lim
    want = g[f"{mode}_perm_f32"]
    want = np.where(swap[None, :, None], 1 - want, want)
    assert np.array_equal(np.asarray(perm)[1:], want[1:])
