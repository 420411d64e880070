"""Golden vectors of the reference's own autograd through the forward's tail (run where the reference tree is, never on
the GPU box).

    python tests/golden/make_tail_grad_golden.py

Imports the reference as make_golden.import_reference does and runs the real ``SeparationModel.forward``
(``model/model.py:402-461``) with ``masks_b`` as a leaf that retains its gradient, in float32 and with ``torch.float32``
and ``torch.complex64`` bound to their double-width types (make_eval_golden.as64's binding, extended by the complex type
that ``model/model.py:437`` names). The masks of both runs are the float32 run's own TCN output: a forward hook on
``TCN`` hands the later stages those values as a leaf, so both precisions differentiate the same function at the same
point. The float64 run is the float32 module converted (``.double()``), so it uses the float32 window buffer's values, as
a loaded checkpoint would.

Cases: B = 2, N in {257, 700, 2816} (T = 2, 3, 12). N = 257 is the shortest input the reference accepts: torch.stft's
reflect padding of 256 needs N > 256 (asserted below for N = 255). For each case and each of the three upstream
choices (g_sep only, g_vad only, both): ``masks_b.grad`` and the nine VAD-head parameter gradients in float64, and the
float32 run's error against them in the gates' units (tail_grad_cases.frame_units / tensor_units): the yardstick.
Only seeded inputs and the reference's outputs are written (golden_tail_grad.npz).
"""
from __future__ import annotations

import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import tail_grad_cases as tc  # noqa: E402
from make_eval_golden import as64  # noqa: E402
from make_golden import SEED_W, import_reference  # noqa: E402

import sep_tfanet_vad_amd as pkg  # noqa: E402
from sep_tfanet_vad_amd import synth  # noqa: E402

CASES = (("n257", 257, 61), ("n700", 700, 62), ("n2816", 2816, 63))
B = 2


def run(net, x, masks, g_sep, g_vad, dt):
    """One forward and backward of the reference in dtype dt with the TCN's output replaced by the leaf `masks`."""
    leaf = masks.detach().to(dt, copy=True).requires_grad_(True)
    hook = net.TCN.register_forward_hook(lambda mod, inp, out: leaf)
    try:
        net.zero_grad()
        sep, vad, _est = net(x.to(dt))
    finally:
        hook.remove()
    assert net.masks_b is leaf and sep.dtype == dt and vad.dtype == dt
    loss = 0
    if g_sep is not None:
        loss = loss + (sep * g_sep.to(dt)).sum()
    if g_vad is not None:
        loss = loss + (vad * g_vad.to(dt)).sum()
    loss.backward()
    out = dict(masks=leaf.grad.detach().clone())
    if g_vad is not None:
        sd = dict(net.named_parameters())
        out.update({k: sd[k].grad.detach().clone() for k in tc.VAD_PARAMS})
    return out, sep.detach(), vad.detach()


def main():
    ref_model, _, _ = import_reference()
    cfg = pkg.CONFIG_WITH_VAD
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, SEED_W).items()}
    net32 = ref_model.SeparationModel(**cfg)
    net32.load_state_dict(sd, strict=True)
    net32.eval()
    net64 = ref_model.SeparationModel(**cfg)
    net64.load_state_dict(sd, strict=True)
    net64.eval().double()
    assert torch.equal(net64.inv_spec.window, net32.inv_spec.window.double())
    try:
        net32(torch.zeros(1, 255))
        raise AssertionError("the reference accepted N = 255")
    except RuntimeError as e:
        print("N = 255:", str(e).splitlines()[0])
    out = dict(weights_seed=np.int64(SEED_W))
    for tag, N, seed in CASES:
        T = 1 + N // 256
        rng = np.random.Generator(np.random.PCG64(seed))
        x = torch.from_numpy((0.1 * rng.standard_normal((B, N))).astype(np.float32))
        g_sep = torch.from_numpy(rng.standard_normal((B, 2, N)).astype(np.float32))
        g_vad = torch.from_numpy(rng.standard_normal((B, 2, T)).astype(np.float32))
        with torch.no_grad():
            net32(x)
        masks = net32.masks_b.detach().clone()
        assert masks.shape == (B, 514, T) and masks.dtype == torch.float32
        out[f"{tag}_x"], out[f"{tag}_masks"] = x.numpy(), masks.numpy()
        out[f"{tag}_g_sep"], out[f"{tag}_g_vad"] = g_sep.numpy(), g_vad.numpy()
        for mode in tc.MODES:
            gs, gv = tc.split_modes(g_sep, g_vad, mode)
            r32, sep32, vad32 = run(net32, x, masks, gs, gv, torch.float32)
            with mock.patch.object(torch, "complex64", torch.complex128):
                r64, sep64, vad64 = as64(lambda: run(net64, x, masks, gs, gv, torch.float64))
            assert r64["masks"].dtype == torch.float64 and bool(torch.isfinite(r64["masks"]).all())
            if mode == "both":
                out[f"{tag}_sep_f64"], out[f"{tag}_vad_f64"] = sep64.numpy(), vad64.numpy()
            out[f"{tag}_{mode}_masks_f64"] = r64["masks"].numpy()
            out[f"{tag}_{mode}_yard_masks"] = np.float64(tc.frame_units(r32["masks"], r64["masks"]))
            print(tag, mode, "yardstick (2^-24 of the frame maximum), masks:", out[f"{tag}_{mode}_yard_masks"])
            if mode == "sep":
                assert not r64["masks"].reshape(B, 2, 257, T)[:, :, 0].any()  # the DC row of X is zero
            if gv is not None:
                for k in tc.VAD_PARAMS:
                    if mode == "vad":  # g_sep adds nothing to a parameter gradient: stored once
                        out[f"{tag}_{k}_f64"] = r64[k].numpy()
                    out[f"{tag}_{mode}_yard_{k}"] = np.float64(tc.tensor_units(r32[k], r64[k]))
                    print("   ", k, out[f"{tag}_{mode}_yard_{k}"])
    fn = os.path.join(HERE, "golden_tail_grad.npz")
    np.savez_compressed(fn, **out)
    size = os.path.getsize(fn)
    print(len(out), "arrays,", size, "bytes")
    assert size <= 1 << 20, size


if __name__ == "__main__":
    main()
