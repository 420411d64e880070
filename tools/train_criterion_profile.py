"""Forward + backward of the native training criterion (train_criterion.CombinedLoss) against the formulation a trainer
runs today (tests/grad_cases.restated_criterion: the reference's model/sdr.py:48-86 and model/combined_loss.py:93-138
in torch, float32 autograd) on the same GPU, and the achieved bytes/s of k_crit_grad_sep.

    python tools/train_criterion_profile.py [--out profiles/train_criterion_profile.txt] [--reps 30]

Shapes: a training batch (B = 64, N = 32 000) and one 60 s file (B = 1, N = 480 000), T = 1 + N // 256. Every shape is
warmed up; a repetition is timed by device events around `inner` forward + backward steps that end in a synchronise; the
two implementations alternate repetition by repetition, and the median and the quartiles over the repetitions are
reported. k_crit_grad_sep: sepvad_criterion_backward's separation part alone, `inner` launches back to back between two
events (launch gaps included: an upper bound of the kernel's time), over the bytes it must move (16 B read and 8 B
written per sample of an utterance). A GPU is required; nothing is estimated.
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
import grad_cases as gc  # noqa: E402

WEIGHTS = dict(weight_separation_loss=0.99, weight_vad_loss=0.01, learn_weight_bool=False)
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_criterion_profile.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_criterion_profile: needs a ROCm GPU")
    from sep_tfanet_vad_amd import combined_loss, evaluate, native, pit, sdr, train_criterion
    dev = torch.device("cuda:0")
    lib = native.load_library()
    lines = [f"train_criterion_profile: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, libsepvad "
             f"{native.build_id()}; reps {args.reps} x inner {args.inner}, device events, us per forward + backward",
             "(native: train_criterion.CombinedLoss; torch f32: the reference formulation, float32 autograd)"]
    for B, N in SHAPES:
        T = 1 + N // 256
        gen = torch.Generator().manual_seed(B + N)
        tgt = torch.randn(B, 2, N, generator=gen).to(dev)
        est0 = (0.8 * tgt + 0.1 * torch.randn(B, 2, N, generator=gen).to(dev))
        est0[1::2] = est0[1::2].flip(1)
        lab = torch.randint(0, 2, (B, 2, T), generator=gen).float().to(dev)
        vad0 = torch.rand(B, 2, T, generator=gen).clamp(0.01, 0.99).to(dev)
        est, vad = est0.clone().requires_grad_(True), vad0.clone().requires_grad_(True)
        crit = train_criterion.CombinedLoss(pit.PITLossWrapper(sdr.pairwise_neg_sisdr, pit_from="pw_mtx"),
                                            pit.PITLossWrapper(combined_loss.BinaryCrossEntropyLoss_Mean(), pit_from="pw_pt"),
                                            dict(WEIGHTS))

        def native_step():
            est.grad = vad.grad = None
            s, v, _, _ = crit(est, tgt, vad, lab)
            (s * 0.99 + v * 0.01).backward()

        def torch_step():
            est.grad = vad.grad = None
            r = gc.restated_criterion(est, tgt, vad, lab)
            (r["sep"] * 0.99 + r["vad"] * 0.01).backward()

        native_step()
        g_native = est.grad.clone()
        torch_step()
        g_torch = est.grad.clone()
        rowmax = g_native.abs().amax(-1, keepdim=True)
        agree = float(((g_native - g_torch).abs() / rowmax).max())
        for _ in range(3):
            timed(native_step, args.inner), timed(torch_step, args.inner)
        tn, tt = [], []
        for _ in range(args.reps):
            tn.append(timed(native_step, args.inner))
            tt.append(timed(torch_step, args.inner))
        qn, qt = quartiles(tn), quartiles(tt)
        # k_crit_grad_sep alone
        with torch.no_grad():
            r = evaluate.eval_separation(est0, tgt, sheet=False)
            scratch = r["scratch"]
            coef = torch.empty(B, 2, train_criterion.CRIT_COEF, dtype=torch.float64, device=dev)
            P, stream = native.ptr, native.stream_ptr(dev)
            native._check(lib.sepvad_criterion_coef(P(est0), N, P(tgt), N, B, N, 0, 1, 1, 1e-8, P(scratch),
                                                    scratch.numel(), P(r["perm"]), P(coef), stream), "coef")
            one, grad = torch.ones((), device=dev), torch.empty(B, 2, N, device=dev)

            def grad_sep():
                native._check(lib.sepvad_criterion_backward(B, P(est0), N, P(tgt), N, N, P(coef), P(one), P(grad), N,
                                                            None, None, None, 0, None, None, stream), "backward")
            for _ in range(3):
                timed(grad_sep, 200)
            qk = quartiles([timed(grad_sep, 200) for _ in range(args.reps)])
        nbytes = 24 * B * N
        lines += ["",
                  f"B = {B}, N = {N}, T = {T}  (max |native - torch f32| / rowmax of grad_est: {agree:.1e})",
                  f"  native     forward + backward: median {qn[1]:9.1f} us  (quartiles {qn[0]:.1f} .. {qn[2]:.1f})",
                  f"  torch f32  forward + backward: median {qt[1]:9.1f} us  (quartiles {qt[0]:.1f} .. {qt[2]:.1f})",
                  f"  ratio of the medians: {qt[1] / qn[1]:.2f}",
                  f"  k_crit_grad_sep, 200 launches back to back: median {qk[1]:.2f} us per launch (quartiles "
                  f"{qk[0]:.2f} .. {qk[2]:.2f}); {nbytes / 1e6:.1f} MB moved -> {nbytes / qk[1] / 1e6:.2f} TB/s "
                  f"(copy rate of DESIGN section 4d: {COPY_RATE_TBS} TB/s; the inputs of this shape "
                  f"{'fit' if 16 * B * N < 256 << 20 else 'do not fit'} in the 256 MiB Infinity Cache)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
