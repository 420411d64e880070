"""Forward + backward of the native tail (train_tail.TrainableTail.from_masks) against the formulation a trainer runs
today (tests/tail_grad_cases.restated_tail: model/model.py:421-441 and the VAD head in torch, float32 autograd) on the same
GPU, and the achieved bytes/s of the backward's hot kernel.

    python tools/tail_grad_profile.py [--out profiles/tail_grad_profile.txt] [--reps 30]

Shapes: a training batch (B = 64, N = 32 000) and one 60 s file (B = 1, N = 480 000), T = 1 + N // 256. Every shape is
warmed up; a repetition is timed by device events around `inner` steps that end in a synchronise; the two implementations
alternate repetition by repetition, and the median and the quartiles over the repetitions are reported. The backward
alone: sepvad_tail_backward, `inner` calls back to back between two events (launch gaps included: an upper bound), once
whole (both upstream gradients, masks and parameter gradients) and once as k_tail_grad_masks alone (g_sep only), over the
bytes that kernel must move: g_sep and x read once, the masks read once and their gradient written once. No speed-up was
set in advance; what is measured is reported beside that floor. A GPU is required; nothing is estimated.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import tail_grad_cases as tc  # noqa: E402

SHAPES = ((64, 32000), (1, 480000))
COPY_RATE_TBS = 6.3


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per step


def quartiles(x):
    return tuple(float(v) for v in np.percentile(np.asarray(x), [25, 50, 75]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tail_grad_profile.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tail_grad_profile: needs a ROCm GPU")
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import native, synth, train_tail
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(pkg.CONFIG_WITH_VAD, 1234).items()}
    net = pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
    net.load_state_dict(sd, strict=True)
    net = net.eval().to(dev)
    tail = train_tail.TrainableTail(net)
    lib, h = native.load_library(), net.native_handle(dev)
    params = {k: v.to(dev).requires_grad_(True) for k, v in sd.items() if k in tc.VAD_PARAMS}
    win = sd["inv_spec.window"].to(dev)
    lines = [f"tail_grad_profile: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, libsepvad "
             f"{native.build_id()}; reps {args.reps} x inner {args.inner}, device events, us per step",
             "(native: train_tail.TrainableTail.from_masks + backward; torch f32: the reference formulation, float32 "
             "autograd)"]
    for B, N in SHAPES:
        T = 1 + N // 256
        x, masks0, g_sep, g_vad = (t.to(dev) for t in tc.seeded_case(B, N, seed=B + N))
        masks = masks0.clone().requires_grad_(True)

        def native_step():
            masks.grad = None
            net.zero_grad()
            sep, vad = tail.from_masks(x, masks)
            torch.autograd.backward([sep, vad], [g_sep, g_vad])

        def torch_step():
            masks.grad = None
            for p in params.values():
                p.grad = None
            sep, vad = tc.restated_tail(x, masks, params, win, win)
            torch.autograd.backward([sep, vad], [g_sep, g_vad])

        buf, nbytes = native.scratch_for("sepvad_tail_scratch_bytes", dev, B, N)
        g_masks = torch.empty(B, 514, T, device=dev)
        gpar = torch.empty(5166, device=dev, dtype=torch.float64)
        vadw = train_tail._vad_weights(tail._params())
        m32 = masks0.contiguous()

        def backward(whole):
            def run():
                native.check(lib.sepvad_tail_backward(
                    h.raw, native.ptr(x), N, native.ptr(m32), B, N, native.ptr(g_sep), *g_sep.stride(),
                    native.ptr(g_vad if whole else None), *g_vad.stride(), native.ptr(vadw if whole else None),
                    native.ptr(buf), nbytes, native.ptr(g_masks), native.ptr(gpar if whole else None),
                    native.stream_ptr(dev)), "sepvad_tail_backward")
            return run

        steps = dict(native=native_step, torch=torch_step, bwd=backward(True), hot=backward(False))
        for fn in steps.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in steps}
        for _ in range(args.reps):
            for k, fn in steps.items():
                t[k].append(timed(fn, args.inner))
        q = {k: quartiles(v) for k, v in t.items()}
        moved = 4.0 * (B * 2 * N + B * N + 2 * B * 514 * T)
        floor_us = moved / (COPY_RATE_TBS * 1e12) * 1e6
        lines += [f"B = {B}, N = {N}, T = {T}:",
                  f"  forward + backward  native {q['native'][1]:9.1f} us (quartiles {q['native'][0]:.1f} .. "
                  f"{q['native'][2]:.1f})   torch f32 {q['torch'][1]:9.1f} us ({q['torch'][0]:.1f} .. {q['torch'][2]:.1f})"
                  f"   ratio {q['torch'][1] / q['native'][1]:.2f}x",
                  f"  sepvad_tail_backward, both gradients, masks and parameters: {q['bwd'][1]:9.1f} us "
                  f"({q['bwd'][0]:.1f} .. {q['bwd'][2]:.1f})",
                  f"  k_tail_grad_masks alone (g_sep only): {q['hot'][1]:9.1f} us ({q['hot'][0]:.1f} .. {q['hot'][2]:.1f}); "
                  f"{moved / 1e6:.1f} MB to move: {moved / q['hot'][1] / 1e6:.2f} TB/s achieved, floor {floor_us:.1f} us at "
                  f"the {COPY_RATE_TBS} TB/s copy rate"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
