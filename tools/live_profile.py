#!/usr/bin/env python
"""Cost of a live session (live.LiveSeparator) per hop-sized push, against the offline one-forward calc_online.

For each stream count: fill the 3 s window, warm up, then time hop-sized pushes (one window each):
  * device time per push from events around the push, split by events around its forward_windows call into the
    forward and the rest (ring push + PIT + stitch, three or four small launches);
  * host time per push: the enqueue alone (no synchronise) and the wall time until the device is done;
  * back-to-back pushes without a synchronise in between (throughput), wall time over the count;
  * the real-time factor: hop duration / wall time until done;
  * windows/s of OnlineSaving.calc_online (all 7 windows of a 4 s recording in ONE forward) on the same streams.
Every push must issue exactly one forward: counted and asserted. Prints one JSON line per stream count and a table.

usage: python tools/live_profile.py [--streams 1,64,256] [--steps 60] [--warmup 10] [--save-sec 0.16]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


class TimedHandle:
    """The native handle with device events around forward_windows (and a call count)."""

    def __init__(self, handle):
        self._handle = handle
        self.calls = 0
        self.events = []

    def __getattr__(self, name):
        return getattr(self._handle, name)

    def forward_windows(self, *a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = self._handle.forward_windows(*a, **kw)
        e1.record()
        self.calls += 1
        self.events.append((e0, e1))
        return out


def med(v):
    return float(statistics.median(v))


def profile(net, B, save_sec, steps, warmup, dev):
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    ikw = dict(pkg.INFERENCE_KW_DEFAULTS)
    base = synth.make_batch(min(B, 8), 64000, 7000)[0]
    x = torch.from_numpy(np.tile(base, ((B + base.shape[0] - 1) // base.shape[0], 1))[:B]).to(dev)
    live = pkg.LiveSeparator(net, B, save_sec=save_sec, inference_kw=ikw)
    hop, win = live.hop, live.win
    th = TimedHandle(live._h)
    live._h = th
    n_chunks = (x.shape[1] - hop) // hop

    def chunk(i):
        o = (i % n_chunks) * hop
        return x[:, o: o + hop]

    live.push(x[:, :win])
    for i in range(warmup):
        live.push(chunk(i))
    torch.cuda.synchronize()
    th.calls, th.events = 0, []
    dev_ms, enq_ms, wall_ms = [], [], []
    for i in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        sep, _, perm = live.push(chunk(i))
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert perm.shape[0] == 1 and sep.shape[-1] == hop
        dev_ms.append(e0.elapsed_time(e1))
        enq_ms.append((t1 - t0) * 1e3)
        wall_ms.append((t2 - t0) * 1e3)
    assert th.calls == steps, f"{th.calls} forwards for {steps} hop-sized pushes"
    forwards_per_push = th.calls / steps
    fwd_ms = [a.elapsed_time(b) for a, b in th.events]
    rest_ms = [d - f for d, f in zip(dev_ms, fwd_ms)]
    th.events = []
    t0 = time.perf_counter()
    for i in range(steps):
        live.push(chunk(i))
    torch.cuda.synchronize()
    b2b_ms = (time.perf_counter() - t0) * 1e3 / steps
    th.events = []
    # the offline path on the same streams: 7 windows of every stream in one forward + the sequential PIT chain
    ons = pkg.OnlineSaving(net, "/nonexistent", pkg.PITLossWrapper(loss_func=torch.nn.L1Loss(), pit_from="pw_pt"))
    ons.save_sec = save_sec
    n_win = ons.n_windows(x.shape[1])
    off_ms = []
    for r in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ons.calc_online(x, "s", 10 ** 6, ikw)
        torch.cuda.synchronize()
        if r >= 2:
            off_ms.append((time.perf_counter() - t0) * 1e3)
    hop_ms = 1e3 * hop / live.fs
    res = dict(
        n_streams=B, save_sec=save_sec, steps=steps, warmup=warmup, forwards_per_push=forwards_per_push,
        device_ms_per_push=med(dev_ms), device_ms_min=min(dev_ms), device_ms_max=max(dev_ms),
        forward_ms=med(fwd_ms), rest_ms=med(rest_ms), rest_share=med(rest_ms) / med(dev_ms),
        host_enqueue_ms=med(enq_ms), wall_ms_per_push=med(wall_ms), wall_ms_min=min(wall_ms), wall_ms_max=max(wall_ms),
        back_to_back_ms_per_push=b2b_ms, real_time_factor=hop_ms / med(wall_ms),
        live_windows_per_s=B / (med(wall_ms) * 1e-3), live_windows_per_s_back_to_back=B / (b2b_ms * 1e-3),
        calc_online_windows=B * n_win, calc_online_ms=med(off_ms), calc_online_windows_per_s=B * n_win / (med(off_ms) * 1e-3),
    )
    live._h = th._handle
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,64,256")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--save-sec", type=float, default=0.16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("live_profile: needs a ROCm device (there is nothing to measure without one)")
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    dev = torch.device("cuda", 0)
    net = pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
    sd = synth.make_state_dict(pkg.CONFIG_WITH_VAD, 1234)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.eval().to(dev)
    rows = []
    for B in [int(s) for s in args.streams.split(",")]:
        r = profile(net, B, args.save_sec, args.steps, args.warmup, dev)
        rows.append(r)
        print(json.dumps(r), flush=True)
    print(f"\n{'streams':>7} {'device ms':>10} {'forward':>9} {'rest':>8} {'rest %':>7} {'enqueue':>8} {'wall ms':>8} "
          f"{'b2b ms':>8} {'RTF':>7} {'live win/s':>11} {'calc_online win/s':>18}")
    for r in rows:
        print(f"{r['n_streams']:>7} {r['device_ms_per_push']:>10.3f} {r['forward_ms']:>9.3f} {r['rest_ms']:>8.3f} "
              f"{100 * r['rest_share']:>7.1f} {r['host_enqueue_ms']:>8.3f} {r['wall_ms_per_push']:>8.3f} "
              f"{r['back_to_back_ms_per_push']:>8.3f} {r['real_time_factor']:>7.1f} {r['live_windows_per_s']:>11.0f} "
              f"{r['calc_online_windows_per_s']:>18.0f}")


if __name__ == "__main__":
    main()
