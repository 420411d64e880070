"""The architecture variants the native path accepts beyond the two shipped configs (config.native_support_error):
one table shared by tests/golden/make_variant_golden.py, tests/test_oracle_variants.py and tests/test_gpu_variants.py.

Each variant names the config it departs from (W = CONFIG_WITH_VAD, WO = CONFIG_WITHOUT_VAD) and the switches it
changes; `ctor_defaults` is the reference constructor's own defaults (model/model.py:362-366) with weight_norm on.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

WEIGHTS_SEED = 1234
# the two golden inputs, synth.make_batch(B, N, seed): T = 32 (one workgroup per utterance) and T = 49 (odd, two
# workgroups, a partial last tile)
INPUTS = {"t32": (2, 8000, 100), "t49": (2, 12345, 200)}
# the inference_kw of tests/golden/make_golden.py (masked_vad's ikw_sep / ikw_vad)
IKW = dict(filter_signals_by_smo_vad=True, filter_signals_by_unsmo_vad=False, length_smoothing_filter=3,
           threshold_activated_vad=0.5, return_smoothed_vad=True)

# name -> (base, overrides); base None: the overrides alone over the constructor defaults
_TABLE = {
    "masked_vad": ("W", dict(final_vad_masked_speakers=True)),
    "masked_no_phase": ("W", dict(final_vad_masked_speakers=True, noisy_phase=False)),
    "no_final_vad": ("W", dict(final_vad=False)),
    "no_activity": ("W", dict(activity_input_bool=False)),
    "plain_phase": ("W", dict(noisy_phase=False)),
    "both_ln": ("W", dict(apply_residual_ln=True)),
    "layer5_stack2": ("W", dict(layer=5, stack=2)),
    "layer3_stack1": ("WO", dict(layer=3, stack=1)),
    "ctor_defaults": (None, dict(weight_norm=True)),
}
NAMES = tuple(_TABLE)
# variants whose forward returns the int 0 for vad (model/model.py:424-427,434)
NO_VAD = ("masked_no_phase", "no_final_vad")
# mathematically equal to their base config given the same tensors for the shared keys
EQUAL_TO_BASE = ("plain_phase", "both_ln")


def base_name(name):
    return _TABLE[name][0]


def overrides(name):
    return dict(_TABLE[name][1])


def base_config(name):
    """The shipped config variant `name` departs from (ctor_defaults: W, the nearest shipped one)."""
    import sep_tfanet_vad_amd as pkg
    return dict(pkg.CONFIG_WITHOUT_VAD if _TABLE[name][0] == "WO" else pkg.CONFIG_WITH_VAD)


def config(name):
    base, over = _TABLE[name]
    return dict(over) if base is None else dict(base_config(name), **over)


def make_input(iname):
    """The golden input `iname` as float32 numpy [B, N], regenerated from its seed."""
    from sep_tfanet_vad_amd import synth
    B, N, seed = INPUTS[iname]
    return synth.make_batch(B, N, seed)[0]


def state_dict(name, seed=WEIGHTS_SEED):
    """Recipe weights of variant `name` as float32 torch tensors."""
    import torch
    from sep_tfanet_vad_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(config(name), seed).items()}


def golden_path(name):
    return os.path.join(GOLDEN, f"golden_variant_{name}.npz")


def load_golden(name):
    return dict(np.load(golden_path(name)))


def load_manifest():
    with open(os.path.join(GOLDEN, "VARIANTS_MANIFEST.json")) as f:
        return json.load(f)


def input_sha(x):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float32).tobytes()).hexdigest()
