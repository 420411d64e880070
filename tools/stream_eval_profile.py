#!/usr/bin/env python
"""Cost of the streaming evaluation's window loop (model/online_class_known_targets.py:101-123): the fused entry
sepvad_stream_eval (online_known.StreamEval) against the same loop composed from the existing entries, window by
window (sepvad_eval_separation, sepvad_pit_l1 or four sepvad_si_sdr pairs per row, sepvad_stream_append), as
OnlineSavingKnownTargets runs it with fused_eval = False.

Two shapes, both at the 160 ms hop (W = 48 000, H = 2 560) with the class's padding:

  * cfg 3's batch: 256 streams x 4 s -> K = 25 windows;
  * one 60 s file: B = 1 -> K = 375 windows.

The windows' separations are synthetic (target + noise; the forward is not part of either side). For each similarity
mode (none, L1, SI-SDR) both sides run on the same device arrays; their stitched signals and permutations are compared
bit for bit before anything is timed. Device events around one whole loop (enqueue included: the composed side is
a few thousand small launches), `--warmup` untimed loops of each side first, `--repeats` loops of each, alternating;
the median and the range are reported. The fused side is pushed in window-major chunks of `--max-window-utts`
window-utterances, as calc_online pushes them.

usage: python tools/stream_eval_profile.py [--out profiles/stream_eval_profile.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEV = "cuda"
FS, W, H = 16000, 48000, 2560
SHAPES = (("cfg 3: 256 streams x 4 s", 256, 64000), ("one 60 s file", 1, 960000))
MODES = (("none", 0), ("l1", 1), ("sisdr", 2))


def n_windows(N):
    total = max(N, W) + (W - H)
    total += (total - W) % H
    return (total - W) // H + 1


def make_inputs(B, K, seed=0):
    """Targets [B, 2, (K - 1) H + W] and windows cut from target + noise, every third window's speakers exchanged."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    tgt = torch.randn(B, 2, (K - 1) * H + W, device=DEV, generator=gen)
    sep = torch.empty(K, B, 2, W, device=DEV)
    for k in range(K):
        w = tgt[:, :, k * H: k * H + W] + 0.3 * torch.randn(B, 2, W, device=DEV, generator=gen)
        sep[k] = w.flip(1) if k % 3 == 1 else w
    return sep, tgt


def fused(sep, tgt, mode, chunk):
    from sep_tfanet_vad_amd.online_known import StreamEval
    K = sep.shape[0]
    se = StreamEval(tgt, K, W, H, mode)
    for k0 in range(0, K, chunk):
        se.push(sep[k0: k0 + chunk], k0)
    return se.online, se.perm


def composed(sep, tgt, mode):
    from sep_tfanet_vad_amd import evaluate, pit
    K, B = sep.shape[:2]
    buf = torch.empty(B, 2, K * H, device=DEV)
    perms = []
    for k in range(K):
        pred = sep[k]
        perm = evaluate.eval_separation(pred, tgt[:, :, k * H: k * H + W], sheet=False)["perm"]
        if mode:
            online = pred[:, :, W - H:] if k == 0 else buf[:, :, :k * H]
            n_on = online.shape[-1]
            a, b = pred[:, :, max(0, W - H - n_on): W - H], online[:, :, max(0, n_on - (W - H)):]
            perm = (pit.pit_l1(a, b) if mode == 1 else pit.pit_sisdr_rows(a, b))[1]
        perms.append(perm)
        pit.stream_append(pred, W - H, H, perm, buf, k * H)
    return buf, torch.stack(perms)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)  # ms per loop


def profile(B, N, warmup, repeats, max_window_utts):
    K = n_windows(N)
    sep, tgt = make_inputs(B, K)
    chunk = max(1, max_window_utts // B)
    rows = []
    for name, mode in MODES:
        fns = dict(fused=lambda: fused(sep, tgt, mode, chunk), composed=lambda: composed(sep, tgt, mode))
        (on_f, perm_f), (on_c, perm_c) = fns["fused"](), fns["composed"]()
        torch.cuda.synchronize()
        assert torch.equal(on_f, on_c) and torch.equal(perm_f, perm_c), f"{name}: fused and composed disagree"
        for fn in fns.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(repeats):  # alternate the sides within one run: other work shares the machine
            for k, fn in fns.items():
                times[k].append(timed(fn))
        rows.append((name, {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}))
    return K, chunk, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_eval_profile.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--max-window-utts", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_eval_profile: needs a ROCm device (timings are not taken on a CPU)")
    lines = [f"stream_eval_profile: {torch.cuda.get_device_name(0)}; device events around one whole window loop "
             f"(enqueue included), median of {args.repeats} alternating loops (min .. max), {args.warmup} warm-up loops "
             f"each; W = {W}, H = {H}; fused pushed in chunks of {args.max_window_utts} window-utterances",
             "command: python tools/stream_eval_profile.py", ""]
    for title, B, N in SHAPES:
        K, chunk, rows = profile(B, N, args.warmup, args.repeats, args.max_window_utts)
        lines.append(f"{title}: B = {B}, N = {N}, K = {K} windows ({-(-K // chunk)} sepvad_stream_eval calls); stitched "
                     f"signals and permutations of the two sides equal to the bit")
        for name, t in rows:
            f, c = t["fused"], t["composed"]
            lines.append(f"  {name:6s} fused {f[0]:9.3f} ms ({f[1]:.3f} .. {f[2]:.3f})   composed {c[0]:9.3f} ms "
                         f"({c[1]:.3f} .. {c[2]:.3f})   composed / fused = {c[0] / f[0]:.2f}x")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
