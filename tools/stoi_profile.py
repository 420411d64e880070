"""Device time of the STOI metric next to the forward that produces its inputs (STOI section).

    python tools/stoi_profile.py --case cfg2     # 64-utterance forward (N = 32000) + Stoi(fs_sig=8000) on its 128 pairs
    python tools/stoi_profile.py --case 16k      # Stoi(fs_sig=16000) on 128 pairs of N = 64000 (sources vs mixtures)

Plain run: event-timed milliseconds per call after warm-up, one JSON line. Under
``rocprofv3 --kernel-trace --stats -- python tools/stoi_profile.py --case ...`` the per-kernel averages of the
same loop (one shape per run, so the k_stoi_* rows are not a blend of shapes).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sep_tfanet_vad_amd as pkg  # noqa: E402
from sep_tfanet_vad_amd import metrics, synth  # noqa: E402


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)])
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["cfg2", "16k"], required=True)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda:0"
    res = dict(case=a.case, warmup=a.warmup, steps=a.steps)
    if a.case == "cfg2":
        B, N, fs = 64, 32000, 8000
        x, srcs = synth.make_batch(B, N, 10_000)
        net = pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
        sd = synth.make_state_dict(pkg.CONFIG_WITH_VAD, 1234)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net = net.eval().to(dev)
        xd, tgt = torch.from_numpy(x).to(dev), torch.from_numpy(srcs).to(dev)
        met = metrics.Stoi(fs_sig=fs)
        with torch.no_grad():
            sep, _, _ = net(xd)
            res["forward"] = timed(lambda: net(xd), a.warmup, a.steps)
            res["stoi"] = timed(lambda: met(sep, tgt, None), a.warmup, a.steps)
            res["stoi_value"] = met(sep, tgt, None).item()
    else:
        B, N, fs = 64, 64000, 16000
        x, srcs = synth.make_batch(B, N, 10_000)
        tgt = torch.from_numpy(srcs).to(dev)
        preds = torch.from_numpy(x).to(dev).unsqueeze(1).repeat(1, 2, 1)
        met = metrics.Stoi(fs_sig=fs)
        res["stoi"] = timed(lambda: met(preds, tgt, None), a.warmup, a.steps)
        res["stoi_value"] = met(preds, tgt, None).item()
    _, frames = metrics.stoi_pairs(tgt.reshape(2 * B, N), tgt.reshape(2 * B, N), fs)
    res.update(pairs=2 * B, N=N, fs_sig=fs, mean_spectra_kept=float(frames.double().mean().item()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
