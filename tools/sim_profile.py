"""Device time of the scene simulation (csrc/sim.hip) for a BASELINE cfg 4 batch, stage by stage, and the wall time
of synth.make_reverb_batch_device next to the host path synth.make_reverb_batch (scene simulation).

    python tools/sim_profile.py                  # 64 utterances of 64 000 samples, responses at T60 * fs, seed 40 000
    python tools/sim_profile.py --batch 4 --samples 16384 --host-repeats 1   # a rehearsal size

Stages are timed with HIP events after warm-up (median of --steps); the two end-to-end paths with a host clock around
calls that end in a device synchronise, alternating, after one warm-up call each. One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sep_tfanet_vad_amd import native, rirgen, simulate, synth  # noqa: E402


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


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--seed", type=int, default=40000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N = a.batch, a.samples

    t0 = time.perf_counter()
    draws = [synth._reverb_scene_draws(N, a.seed + b) for b in range(B)]
    host_draws_s = time.perf_counter() - t0
    rir_jobs, dry_jobs = [], []
    for d in draws:
        for p in d["pos"]:
            job = dict(roomMeasures=list(d["room"]), sourcePosition=list(p), receiverPositions=list(d["mic"]),
                       nSamples=d["n_rir"])
            rir_jobs.append(dict(job, reverbTime=d["t60"]))
            dry_jobs.append(dict(job, reverbTime=0.0))
    t0 = time.perf_counter()
    table, lens = rirgen.prepare_jobs(rir_jobs + dry_jobs)
    prepare_s = time.perf_counter() - t0
    J, ld = len(lens), max(lens)
    images = [8 * (2 * t.n1 + 1) * (2 * t.n2 + 1) * (2 * t.n3 + 1) for t in table]
    tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    h = torch.empty(J, ld, device=dev, dtype=torch.float64)
    lib = native.load_library()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def rir():
        native._check(lib.sepvad_rir_generate_device(native._ptr(tab), J, native._ptr(h), ld, None, 0, stream),
                      "sepvad_rir_generate_device")

    res = dict(batch=B, samples=N, seed=a.seed, jobs=J, rir_ld=ld, mean_rir_samples=float(np.mean(lens)),
               lattice_images_total=int(sum(images)), warmup=a.warmup, steps=a.steps,
               host_draws_s=host_draws_s, prepare_jobs_s=prepare_s)
    res["rir"] = timed(rir, a.warmup, a.steps)
    src = torch.from_numpy(np.stack([np.stack(d["sources"]) for d in draws]).astype(np.float32)).to(dev)
    noise = torch.from_numpy(np.stack([d["noise"] for d in draws]).astype(np.float32)).to(dev)
    snr = torch.tensor([d["snr"] for d in draws], dtype=torch.float64, device=dev)
    klen = torch.tensor(lens, dtype=torch.int32, device=dev)
    xidx = (torch.arange(J, device=dev, dtype=torch.int32) % (2 * B)).contiguous()
    x = src.reshape(2 * B, N)
    res["convolve"] = timed(lambda: simulate.fir_convolve(x, h, N, klen=klen, xidx=xidx), a.warmup, a.steps)
    # one fused multiply-add per (output, tap that exists and reaches a sample of x)
    fmas = sum(k * N - k * (k - 1) // 2 for k in lens)
    res["convolve_fma"] = int(fmas)
    res["convolve_tflops"] = 2 * fmas / (res["convolve"]["median_ms"] * 1e-3) / 1e12
    y = simulate.fir_convolve(x, h, N, klen=klen, xidx=xidx)
    rev, dry = y[:2 * B].view(B, 2, N), y[2 * B:].view(B, 2, N)
    res["mix"] = timed(lambda: simulate.scene_mix(rev, noise, snr, 1.8, 0.9, 1), a.warmup, a.steps)
    _, stats = simulate.scene_mix(rev, noise, snr, 1.8, 0.9, 1)
    res["targets"] = timed(lambda: simulate.scene_targets(dry, stats, 1, 1.8, 0.9), a.warmup, a.steps)
    n512 = N // 512 * 512
    act = (src[:, :, :n512].abs() > 0.05).to(torch.uint8).contiguous()
    res["vad_labels"] = timed(lambda: simulate.vad_frame_labels(act, 0), a.warmup, a.steps)
    res["stages_total_ms"] = sum(res[k]["median_ms"] for k in ("rir", "convolve", "mix", "targets", "vad_labels"))

    # end to end, the same arguments on both paths, alternating after one warm-up of the device path
    wall(lambda: synth.make_reverb_batch_device(min(B, 2), N, a.seed, device=dev))
    dev_s, host_s, err = [], [], None
    for _ in range(a.host_repeats):
        td, (mix_d, tg_d) = wall(lambda: synth.make_reverb_batch_device(B, N, a.seed, device=dev))
        th, (mix_h, tg_h) = wall(lambda: synth.make_reverb_batch(B, N, a.seed))
        dev_s.append(td)
        host_s.append(th)
        err = [float(np.abs(mix_d.cpu().numpy() - mix_h).max()), float(np.abs(tg_d.cpu().numpy() - tg_h).max())]
    res.update(device_path_s=dev_s, host_path_s=host_s, host_over_device=float(np.median(host_s) / np.median(dev_s)),
               max_abs_diff_mix_targets=err, host_path_threads=8)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
