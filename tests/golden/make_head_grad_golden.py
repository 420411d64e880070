"""Golden vectors of the reference's own autograd through its output head (run where the reference tree is, never on the
GPU box).

    python tests/golden/make_head_grad_golden.py

Imports the reference as make_golden.import_reference does, loads the recipe weights into the real ``SeparationModel``
and runs ``net.TCN.output`` (``model/model.py:322-325,357``) on its own input: a forward pre-hook on that module records the
trunk output y of a float32 forward of a seeded mixture. The module is then called on y as a leaf, in float32 and, converted
with ``.double()``, in float64, and <masks_b, G> is differentiated for a seeded G.

Cases: B = 2, N in {257, 700, 2600} (T = 2, 3, 11). Per case: y, G, the float64 masks_b, the float64 gradients at y and at
the six parameters, and the float32 run's error against them in the gates' units (head_grad_cases.units): the yardstick.
The gradient of ``weight_v`` [514, 256, 1] is kept for the rows head_grad_cases.GOLDEN_ROWS only (its yardstick is
measured on those rows, normalised by their maximum), which keeps the file small. Only seeded inputs and the
reference's outputs are written (golden_head_grad.npz).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import head_grad_cases as hc  # noqa: E402
from make_golden import SEED_W, import_reference  # noqa: E402

import sep_tfanet_vad_amd as pkg  # noqa: E402
from sep_tfanet_vad_amd import synth  # noqa: E402

CASES = (("t2", 257, 71), ("t3", 700, 72), ("t11", 2600, 73))
B = 2
PREFIX = "TCN.output."


def run(head, y, G, dt):
    """-> (masks_b, dict(y=..., <parameter name>=...)) of the reference's head in dtype dt."""
    leaf = y.detach().to(dt, copy=True).requires_grad_(True)
    head.zero_grad()
    m = head(leaf)
    assert m.dtype == dt
    (m * G.to(dt)).sum().backward()
    out = dict(y=leaf.grad.detach().clone())
    named = dict(head.named_parameters())
    out.update({k: named[k[len(PREFIX):]].grad.detach().clone() for k in hc.HEAD_PARAMS})
    return m.detach(), out


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
    assert net32.TCN.output[1].eps == hc.EPS and net32.TCN.output[1].num_groups == 1
    rows = list(hc.GOLDEN_ROWS)
    out = dict(weights_seed=np.int64(SEED_W))
    for tag, N, seed in CASES:
        T = 1 + N // 256
        rng = np.random.Generator(np.random.PCG64(seed))
        x = torch.from_numpy((0.1 * rng.standard_normal((B, N))).astype(np.float32))
        G = torch.from_numpy(rng.standard_normal((B, hc.MOUT, T)).astype(np.float32))
        seen = []
        hook = net32.TCN.output.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].detach().clone()))
        try:
            with torch.no_grad():
                net32(x)
        finally:
            hook.remove()
        (y,) = seen
        assert y.shape == (B, hc.CH, T) and y.dtype == torch.float32
        m32, r32 = run(net32.TCN.output, y, G, torch.float32)
        m64, r64 = run(net64.TCN.output, y, G, torch.float64)
        assert torch.equal(m32, net32.masks_b)  # the head on the recorded y is the forward's own head
        out[f"{tag}_y"], out[f"{tag}_G"], out[f"{tag}_masks_f64"] = y.numpy(), G.numpy(), m64.numpy()
        out[f"{tag}_yard_masks"] = np.float64(hc.units("masks", m32, m64))
        print(tag, "y: min", float(y.min()), "max", float(y.max()), "share <= 0:", float((y <= 0).float().mean()))
        print(tag, "yardstick masks (forward):", out[f"{tag}_yard_masks"])
        for k in ("y",) + hc.HEAD_PARAMS:
            a32, a64 = r32[k], r64[k]
            if k == hc.P_V:
                a32, a64 = a32[rows], a64[rows]
            assert a64.dtype == torch.float64 and bool(torch.isfinite(a64).all())
            out[f"{tag}_{k}_f64"] = a64.numpy()
            out[f"{tag}_yard_{k}"] = np.float64(hc.units(k, a32, a64))
            print("   ", k, "yardstick:", out[f"{tag}_yard_{k}"])
    fn = os.path.join(HERE, "golden_head_grad.npz")
    np.savez_compressed(fn, **out)
    size = os.path.getsize(fn)
    print(len(out), "arrays,", size, "bytes")
    assert size <= 400 << 10, size


if __name__ == "__main__":
    main()
