#!/usr/bin/env python
"""Cost of one evaluation step's separation scores: evaluate.score_batch against the separate metric calls.

At B = 64, N = 32 000 (a training-sized batch of 2 s) and B = 1, N = 960 000 (test.py's batch of one 60 s file):

  * score_batch(sep, target, mix): sepvad_eval_separation (k_eval_moments, k_eval_finish, k_eval_means) and the
    reordering copy; also eval_separation alone;
  * the same numbers composed from the separate entries, as a test.py step calls them (test.py:134-152,179-181):
    the mixture repeated as both estimates, calc_sisdr x2, pit_si_sdr x2, pit_snr x2, si_sdri.

Device events around `--inner` back-to-back calls (enqueue included: both sides are small launches), `--warmup`
untimed calls of each first, `--repeats` windows of each, alternating; the median and the spread of the per-call
time are reported. The outputs of the two sides are compared before anything is timed.

With --kernel-stats BxN=FILE (a rocprofv3 --kernel-trace --stats CSV of `--loop BxN`, taken in a run of its own) the
table also gives k_eval_moments' kernel time and its achieved GB/s against the 20 N B bytes it must read.

usage: python tools/eval_profile.py [--out profiles/eval_profile.txt] [--kernel-stats 64x32000=stats.csv ...]
       rocprofv3 --kernel-trace --stats ... -- python tools/eval_profile.py --loop 64x32000
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ((64, 32000), (1, 960000))
DEV = "cuda"


def make_inputs(B, N, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    tgt = torch.randn(B, 2, N, device=DEV, generator=gen)
    sep = 0.7 * tgt + 0.3 * torch.randn(B, 2, N, device=DEV, generator=gen) + 0.1
    sep[1::2] = sep[1::2].flip(1)
    mix = tgt.sum(1) + 0.2 * torch.randn(B, N, device=DEV, generator=gen)
    return sep, tgt, mix


def make_vad_inputs(B, N, seed=1):
    """The VAD track and the masks of the same utterances: T = 1 + N / 256 frames (the model's)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    T = 1 + N // 256
    vad = torch.rand(B, 2, T, device=DEV, generator=gen)
    labels = torch.randint(0, 3, (B, 2, T), device=DEV, generator=gen).float()
    masks = torch.rand(B, 2, 257, T, device=DEV, generator=gen)
    return vad, labels, masks


def composed(sep, tgt, mix, perm):
    """The parent's separate calls of one test.py step, on estimates already reordered by perm."""
    from sep_tfanet_vad_amd import metrics
    from sep_tfanet_vad_amd.pit import reorder_source_mse
    out_sep = reorder_source_mse(sep, perm)                 # test.py:131
    mix2 = mix.unsqueeze(1).repeat(1, 2, 1)                 # test.py:139-140
    return dict(si_sdr_spk=metrics.calc_sisdr(out_sep, tgt), si_sdr_spk_start=metrics.calc_sisdr(mix2, tgt),
                pit_snr=metrics.pit_snr(out_sep, tgt), pit_snr_start=metrics.pit_snr(mix2, tgt),
                pit_si_sdr=metrics.pit_si_sdr(out_sep, tgt), pit_si_sdr_start=metrics.pit_si_sdr(mix2, tgt),
                si_sdri=metrics.si_sdri(out_sep, tgt, mix))


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # us per call


def profile(B, N, warmup, repeats, inner):
    from sep_tfanet_vad_amd import evaluate
    sep, tgt, mix = make_inputs(B, N)
    r = evaluate.score_batch(sep, tgt, mix)
    c = composed(sep, tgt, mix, r["perm"])
    col = {name: r["sheet"][:, i] for i, name in enumerate(evaluate.SHEET_COLUMNS)}
    diffs = dict(
        si_sdr_spk=(torch.stack([col["si_sdr_speaker0"], col["si_sdr_speaker1"]], 1) - c["si_sdr_spk"]).abs().max(),
        si_sdr_spk_start=(torch.stack([col["si_sdr_start_speaker0"], col["si_sdr_start_speaker1"]], 1)
                          - c["si_sdr_spk_start"]).abs().max(),
        pit_si_sdr=(r["pit_si_sdr"] - c["pit_si_sdr"]).abs(), pit_snr=(r["pit_snr"] - c["pit_snr"]).abs(),
        pit_si_sdr_start=(col["pit_si_sdr_start"].double().mean() - c["pit_si_sdr_start"]).abs(),
        pit_snr_start=(col["pit_snr_start"].double().mean() - c["pit_snr_start"]).abs(),
        si_sdri=(r["si_sdri"] - c["si_sdri"]).abs())
    worst = max(float(v) for v in diffs.values())
    assert worst <= 2e-3, f"score_batch and the composed calls disagree: {diffs}"
    vad, labels, masks = make_vad_inputs(B, N)
    fns = dict(score_batch=lambda: evaluate.score_batch(sep, tgt, mix),
               eval_separation=lambda: evaluate.eval_separation(sep, tgt, mix),
               composed=lambda: composed(sep, tgt, mix, r["perm"]),
               score_batch_vad=lambda: evaluate.score_batch(sep, tgt, mix, vad, labels),
               score_batch_vad_masks=lambda: evaluate.score_batch(sep, tgt, mix, vad, labels, masks),
               eval_vad=lambda: evaluate.eval_vad(vad, labels, r["perm"]),
               eval_vad_masks=lambda: evaluate.eval_vad(vad, labels, r["perm"], masks))
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):  # alternate the sides within one run: other work shares the machine
        for k, fn in fns.items():
            times[k].append(window(fn, inner))
    res = dict(B=B, N=N, T=vad.shape[2], max_abs_diff_db=worst, bytes_moments=20 * N * B,
               bytes_masks=4 * masks.numel())
    for k, v in times.items():
        res[f"{k}_us"] = statistics.median(v)
        res[f"{k}_us_min"] = min(v)
        res[f"{k}_us_max"] = max(v)
    return res


def kernel_rows(path):
    with open(path, newline="") as f:
        return {row["Name"]: row for row in csv.DictReader(f)}


def loop(B, N, iters):
    """eval_separation back to back, for a kernel trace."""
    from sep_tfanet_vad_amd import evaluate
    sep, tgt, mix = make_inputs(B, N)
    vad, labels, masks = make_vad_inputs(B, N)
    for _ in range(iters):
        r = evaluate.eval_separation(sep, tgt, mix)
        evaluate.eval_vad(vad, labels, r["perm"], masks)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_profile.txt"))
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--loop", default=None, help="BxN: only run eval_separation --iters times (under rocprofv3)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernel-stats", action="append", default=[], help="BxN=CSV of rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_profile: needs a ROCm GPU (nothing is measured without one)")
    if args.loop:
        B, N = (int(v) for v in args.loop.split("x"))
        loop(B, N, args.iters)
        return
    stats = dict(s.split("=", 1) for s in args.kernel_stats)
    lines = [f"eval_profile: {torch.cuda.get_device_name(0)}; device events around {args.inner} calls, median of "
             f"{args.repeats} alternating windows (min .. max), {args.warmup} warm-up calls each", ""]
    for B, N in SHAPES:
        res = profile(B, N, args.warmup, args.repeats, args.inner)
        print(json.dumps(res))
        lines.append(f"B = {B}, N = {N}  (k_eval_moments reads 20 N B = {res['bytes_moments'] / 1e6:.1f} MB; "
                     f"max |score_batch - composed| = {res['max_abs_diff_db']:.2e} dB)")
        for k in ("score_batch", "eval_separation", "composed"):
            lines.append(f"  {k:<22s} {res[k + '_us']:9.1f} us per call   ({res[k + '_us_min']:.1f} .. {res[k + '_us_max']:.1f})")
        lines.append(f"  composed / score_batch = {res['composed_us'] / res['score_batch_us']:.2f}x")
        lines.append(f"  with the VAD track [B, 2, T = {res['T']}] and the masks [B, 2, 257, T] ({res['bytes_masks'] / 1e6:.1f} MB); "
                     "the package had no device counterpart to compose these from")
        for k in ("score_batch_vad", "score_batch_vad_masks", "eval_vad", "eval_vad_masks"):
            lines.append(f"  {k:<22s} {res[k + '_us']:9.1f} us per call   ({res[k + '_us_min']:.1f} .. {res[k + '_us_max']:.1f})")
        key = f"{B}x{N}"
        if key in stats:
            for name, row in kernel_rows(stats[key]).items():
                if "k_eval_" not in name:
                    continue
                short = re.search(r"k_eval_\w+", name).group(0)
                avg_us = float(row["AverageNs"]) / 1e3
                line = f"  kernel {short:<17s} {avg_us:9.2f} us avg over {row['Calls']} calls ({float(row['MinNs']) / 1e3:.2f} .. {float(row['MaxNs']) / 1e3:.2f})"
                if short == "k_eval_moments":
                    line += f"   {res['bytes_moments'] / (avg_us * 1e-6) / 1e9:.0f} GB/s of its 20 N B bytes"
                if short == "k_eval_simple_vad":
                    line += f"   {res['bytes_masks'] / (avg_us * 1e-6) / 1e9:.0f} GB/s of the masks"
                lines.append(line)
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
