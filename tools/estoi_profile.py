"""Device time of extended STOI next to classic STOI (STOI section), at the two shapes of its table:
128 pairs (64 two-speaker utterances, sources against the mixture) of N = 32000 at fs_sig 8000 and of N = 64000 at
fs_sig 16000.

    python tools/estoi_profile.py [--out profiles/estoi_profile.txt]

Per shape, event-timed milliseconds per call after warm-up (the counts of tools/stoi_profile.py: 10 + 50):
the ``Stoi`` call, the ``Estoi`` call, both metrics from one ``sepvad_stoi_ex`` call (``stoi_both_pairs``), and the two
separate calls back to back (``stoi_pairs`` then ``estoi_pairs``). One JSON line per shape.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stoi_profile import timed  # noqa: E402
from sep_tfanet_vad_amd import metrics, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for name, B, N, fs in (("cfg2_8k", 64, 32000, 8000), ("16k", 64, 64000, 16000)):
        x, srcs = synth.make_batch(B, N, 10_000)
        tgt = torch.from_numpy(srcs).to(dev)
        preds = torch.from_numpy(x).to(dev).unsqueeze(1).repeat(1, 2, 1)
        X, Y = tgt.reshape(2 * B, N), preds.reshape(2 * B, N)
        stoi_met, estoi_met = metrics.Stoi(fs_sig=fs), metrics.Estoi(fs_sig=fs)

        def separate():
            metrics.stoi_pairs(X, Y, fs)
            metrics.estoi_pairs(X, Y, fs)

        res = dict(case=name, pairs=2 * B, N=N, fs_sig=fs, warmup=a.warmup, steps=a.steps)
        res["stoi"] = timed(lambda: stoi_met(preds, tgt, None), a.warmup, a.steps)
        res["estoi"] = timed(lambda: estoi_met(preds, tgt, None), a.warmup, a.steps)
        res["both_one_call"] = timed(lambda: metrics.stoi_both_pairs(X, Y, fs), a.warmup, a.steps)
        res["two_separate_calls"] = timed(separate, a.warmup, a.steps)
        d, e, frames = metrics.stoi_both_pairs(X, Y, fs)
        res.update(stoi_value=d.mean().item(), estoi_value=e.mean().item(),
                   mean_spectra_kept=float(frames.double().mean().item()))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
