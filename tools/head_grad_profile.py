"""The output head's native forward and backward (train_head.TrainableHead; sepvad_head_forward, sepvad_head_backward)
and a whole fine-tuning step of the mask head, against the same step in torch float32 autograd on the same GPU.

    python tools/head_grad_profile.py [--out profiles/head_grad_profile.txt] [--reps 20]

Shapes: a training batch (B = 64, N = 32 000) and one 60 s file (B = 1, N = 480 000), T = 1 + N // 256. Every shape is
warmed up; a repetition is timed by device events around `inner` steps; the implementations alternate repetition by
repetition, and the median and the quartiles over the repetitions are reported. The step: head.from_trunk(y) ->
tail.from_masks(x, masks_b) -> train_criterion.CombinedLoss -> backward, with y a leaf (there is no native source of the
trunk output yet); in torch: tests/head_grad_cases.restated_head -> tail_grad_cases.restated_tail ->
grad_cases.restated_criterion in float32 autograd. The entries alone: `inner` calls back to back between two events
(launch gaps included: an upper bound). The backward's floor: its two products, 4 B T 514 256 FLOP, at the f64 MFMA
peak (v_mfma_f64_16x16x4_f64, 78.6 TFLOP/s; the library has no other kernel of that form to take a reached rate from) plus
the bytes it must move (y and G read, g_y written, the weight partials written and read) at the copy rate of DESIGN.md
section 4d. Also timed: net.refresh_native() followed by the handle's rebuild, which an optimizer step costs today before
the next native forward. No speed-up was set in advance. A GPU is required; nothing is estimated.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import grad_cases as gc  # noqa: E402
import head_grad_cases as hc  # noqa: E402
import tail_grad_cases as tc  # noqa: E402

SHAPES = ((64, 32000), (1, 480000))
COPY_RATE_TBS = 6.3
F64_MFMA_TFLOPS = 78.6   # v_mfma_f64_16x16x4_f64 peak of the part
W_T = hc.W_T


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_grad_profile.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_grad_profile: needs a ROCm GPU")
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import combined_loss, native, pit, sdr, synth, train_criterion, train_head, train_tail
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(pkg.CONFIG_WITH_VAD, 1234).items()}
    net = pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
    net.load_state_dict(sd, strict=True)
    net = net.eval().to(dev)
    head, tail = train_head.TrainableHead(net), train_tail.TrainableTail(net)
    crit = train_criterion.CombinedLoss(
        pit.PITLossWrapper(sdr.PairwiseNegSDR("sisdr", zero_mean=True, take_log=True), pit_from="pw_mtx"),
        pit.PITLossWrapper(combined_loss.BinaryCrossEntropyLoss_Mean(), pit_from="pw_pt"),
        dict(weight_separation_loss=0.99, weight_vad_loss=0.01, learn_weight_bool=False)).to(dev)
    lib = native.load_library()
    names = hc.HEAD_PARAMS + tc.VAD_PARAMS
    params = {k: v.to(dev).requires_grad_(True) for k, v in sd.items() if k in names}
    win = sd["inv_spec.window"].to(dev)
    lines = [f"head_grad_profile: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, libsepvad "
             f"{native.build_id()}; reps {args.reps} x inner {args.inner}, device events, us per step",
             "(native: head.from_trunk -> tail.from_masks -> train_criterion.CombinedLoss -> backward; torch f32: the "
             "restatements of the same three stages, float32 autograd on the device)"]
    for B, N in SHAPES:
        T = 1 + N // 256
        x, _, tgt, _ = (t.to(dev) for t in tc.seeded_case(B, N, seed=B + N))
        y, G = (t.to(dev) for t in hc.seeded_case(B, T, seed=B + T))
        labels = (torch.rand(B, 2, T, device=dev) > 0.5).float()
        yl = y.clone().requires_grad_(True)

        def native_step():
            yl.grad = None
            net.zero_grad()
            sep, vad = tail.from_masks(x, head.from_trunk(yl))
            sl, vl, _, _ = crit(sep, tgt, vad, labels)
            (0.99 * sl + 0.01 * vl).backward()

        def torch_step():
            yl.grad = None
            for p in params.values():
                p.grad = None
            sep, vad = tc.restated_tail(x, hc.restated_head(yl, params), params, win, win)
            r = gc.restated_criterion(sep, tgt, vad, labels)
            (0.99 * r["sep"] + 0.01 * r["vad"]).backward()

        buf, nbytes = native.scratch_for("sepvad_head_scratch_bytes", dev, B, T)
        hpar = train_head._head_weights(head._params())
        masks = torch.empty(B, 514, T, device=dev)
        g_y = torch.empty(B, 256, T, device=dev)
        gpar = torch.empty(train_head.HEAD_NPAR, device=dev, dtype=torch.float64)

        def fwd():
            native.check(lib.sepvad_head_forward(native.ptr(y), B, T, native.ptr(hpar), native.ptr(buf), nbytes,
                                                 native.ptr(masks), native.stream_ptr(dev)), "sepvad_head_forward")

        def bwd():
            native.check(lib.sepvad_head_backward(native.ptr(y), native.ptr(G), *G.stride(), B, T, native.ptr(hpar),
                                                  native.ptr(buf), nbytes, native.ptr(g_y), native.ptr(gpar),
                                                  native.stream_ptr(dev)), "sepvad_head_backward")

        steps = dict(native=native_step, torch=torch_step, fwd=fwd, bwd=bwd)
        for fn in steps.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in steps}
        for _ in range(args.reps):
            for k, fn in steps.items():
                t[k].append(timed(fn, args.inner))
        q = {k: quartiles(v) for k, v in t.items()}
        flop = 4.0 * B * T * 514 * 256
        nw = B * ((T + W_T - 1) // W_T)
        moved = 4.0 * (2 * B * 256 * T + B * 514 * T) + 2 * 8.0 * nw * 514 * 256
        floor_us = flop / (F64_MFMA_TFLOPS * 1e12) * 1e6 + moved / (COPY_RATE_TBS * 1e12) * 1e6
        lines += [f"B = {B}, N = {N}, T = {T}:",
                  f"  whole step  native {q['native'][1]:9.1f} us (quartiles {q['native'][0]:.1f} .. "
                  f"{q['native'][2]:.1f})   torch f32 {q['torch'][1]:9.1f} us ({q['torch'][0]:.1f} .. {q['torch'][2]:.1f})"
                  f"   ratio {q['torch'][1] / q['native'][1]:.2f}x",
                  f"  sepvad_head_forward:  {q['fwd'][1]:9.1f} us ({q['fwd'][0]:.1f} .. {q['fwd'][2]:.1f})",
                  f"  sepvad_head_backward, g_y and parameters: {q['bwd'][1]:9.1f} us ({q['bwd'][0]:.1f} .. {q['bwd'][2]:.1f}); "
                  f"floor {floor_us:.1f} us ({flop / 1e9:.2f} GFLOP at {F64_MFMA_TFLOPS} TFLOP/s + {moved / 1e6:.1f} MB at "
                  f"{COPY_RATE_TBS} TB/s): {q['bwd'][1] / floor_us:.1f}x the floor"]
    rebuild = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.refresh_native()
        net.native_handle(dev)
        torch.cuda.synchronize()
        rebuild.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"net.refresh_native() + the handle's rebuild (host clock, 5 runs): median {np.median(rebuild):.1f} ms "
                 f"(min {min(rebuild):.1f}, max {max(rebuild):.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
