"""tail_grad_cases' restatement and closed form against the reference's own float64 autograd (no GPU).

tests/golden/golden_tail_grad.npz holds ``masks_b.grad`` and the nine VAD-head parameter gradients of the real reference
``SeparationModel`` (golden/make_tail_grad_golden.py). The restatement's float64 gradients must equal them to 1e-9 of each
tensor's maximum, and so must the closed form of the separation path; pinned this way, the restatement is the truth for
the shapes too large to commit (test_gpu_tail_grad.py).
"""
import os

import numpy as np
import pytest
import torch

import tail_grad_cases as tc
from conftest import GOLDEN

TAGS = ("n257", "n700", "n2816")
TOL = 1e-9


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_tail_grad.npz"))


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def inputs(g, tag):
    return t_(g[f"{tag}_x"]), t_(g[f"{tag}_masks"]), t_(g[f"{tag}_g_sep"]), t_(g[f"{tag}_g_vad"])


def vad_params(sd):
    return {k: sd[k] for k in tc.VAD_PARAMS}


def close(a, ref, where):
    ref = t_(ref).double()
    err = float((a.double().reshape(ref.shape) - ref).abs().max())
    scale = float(ref.abs().max())
    print(where, "max error / tensor max:", err / scale if scale else err)
    assert err <= TOL * scale, where


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference(g, state_dicts, tag, mode):
    sd = state_dicts["with_vad"]
    x, masks, g_sep, g_vad = inputs(g, tag)
    gs, gv = tc.split_modes(g_sep, g_vad, mode)
    r = tc.autograd_grads(x, masks, vad_params(sd), sd["inv_spec.window"], gs, gv, torch.float64)
    close(r["masks"], g[f"{tag}_{mode}_masks_f64"], f"{tag} {mode} masks")
    if gv is not None:
        for k in tc.VAD_PARAMS:
            close(r[k], g[f"{tag}_{k}_f64"], f"{tag} {mode} {k}")


@pytest.mark.parametrize("tag", TAGS)
def test_restated_forward_equals_the_reference(g, state_dicts, tag):
    sd = state_dicts["with_vad"]
    x, masks, _, _ = inputs(g, tag)
    w = sd["inv_spec.window"].double()
    p = {k: v.double() for k, v in vad_params(sd).items()}
    sep, vad = tc.restated_tail(x.double(), masks.double(), p, w, w)
    close(sep, g[f"{tag}_sep_f64"], f"{tag} sep")
    close(vad, g[f"{tag}_vad_f64"], f"{tag} vad")


@pytest.mark.parametrize("tag", TAGS)
def test_closed_form_equals_the_reference(g, state_dicts, tag):
    x, masks, g_sep, _ = inputs(g, tag)
    cf = tc.closed_form_masks(x, masks, g_sep, state_dicts["with_vad"]["inv_spec.window"], torch.float64)
    close(cf, g[f"{tag}_sep_masks_f64"], f"{tag} closed form")
    B, _, T = masks.shape
    assert not bool(cf.reshape(B, 2, tc.NBIN, T)[:, :, 0].any())  # bin 0 receives the VAD term only


def test_the_three_windows_are_one(state_dicts):
    """The restatement takes one window for the STFT and its inverse: the recipe's three buffers are equal."""
    sd = state_dicts["with_vad"]
    assert torch.equal(sd["inv_spec.window"], sd["spec_output.window"])
    assert torch.equal(sd["inv_spec.window"], sd["spec_input.spec.window"])


def test_linear_in_the_upstream_gradients(g, state_dicts):
    """The 'both' gradient is the sum of the two parts (what the GPU tests rely on when they gate the three modes)."""
    tag = "n700"
    both = t_(g[f"{tag}_both_masks_f64"])
    parts = t_(g[f"{tag}_sep_masks_f64"]) + t_(g[f"{tag}_vad_masks_f64"])
    assert float((both - parts).abs().max()) <= 1e-12 * float(both.abs().max())


def test_float32_closed_form_is_within_the_margin_of_the_yardstick(g, state_dicts):
    """On the CPU, the closed form evaluated in float32 stays within the gate of the float32 autograd yardstick: the gate
    is reachable by the arithmetic the kernel implements."""
    for tag in TAGS:
        x, masks, g_sep, _ = inputs(g, tag)
        cf = tc.closed_form_masks(x, masks, g_sep, state_dicts["with_vad"]["inv_spec.window"], torch.float32)
        units, yard = tc.frame_units(cf, g[f"{tag}_sep_masks_f64"]), float(g[f"{tag}_sep_yard_masks"])
        print(tag, "float32 closed form:", units, "yardstick:", yard)
        assert units <= tc.MARGIN * yard
