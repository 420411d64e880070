"""Reference goldens for the architecture variants of tests/variants.py (CPU only; needs the reference tree).

    python tests/golden/make_variant_golden.py

Per variant: golden_variant_<name>.npz with the REFERENCE's sep and vad (a 0-d 0 where it returns the int 0) for the
two inputs of variants.INPUTS, the sha256 of each input (the tests regenerate the inputs from their seeds), the weight
seed and sha, and for masked_vad the outputs under make_golden.py's inference_kw on the first input. Also the
reference's state_dict key contract per variant (state_dict_keys_variant_<name>.json) and VARIANTS_MANIFEST.json: per
variant and input the reference's VAD margin min |p - 0.5|, the fp32-reference-to-fp64-oracle distance on sep and on
vad (the noise terms of the GPU gates), and the fixture sizes. Only data is written; the fixtures of make_golden.py
are left alone.

Input condition (checked here, on the reference alone): every VAD margin >= 1e-3 and >= 4x that input's fp32-vs-fp64
VAD distance, so the bit-exact label checks of the GPU tests have room above rounding.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import SEED_W, build, import_reference, run_case, weights_sha  # noqa: E402
import variants  # noqa: E402
from oracle.torch_ref import OracleModel  # noqa: E402

MAX_FILE = 400 * 1024  # bytes per fixture
MAX_SET = 3584 * 1024  # bytes for the set (3.5 MiB)
MIN_MARGIN = 1e-3
MARGIN_OVER_NOISE = 4.0


def main():
    assert SEED_W == variants.WEIGHTS_SEED
    ref_model, _, _ = import_reference()
    torch.set_num_threads(8)
    manifest = dict(weights_seed=SEED_W, seeds_changed=None, min_margin=MIN_MARGIN, margin_over_noise=MARGIN_OVER_NOISE,
                    inputs={k: dict(B=v[0], N=v[1], seed=v[2]) for k, v in variants.INPUTS.items()}, variants={})
    xs = {iname: variants.make_input(iname) for iname in variants.INPUTS}
    bad, total = [], 0
    for name in variants.NAMES:
        cfg = variants.config(name)
        net, sd = build(ref_model, cfg)
        with open(os.path.join(HERE, f"state_dict_keys_variant_{name}.json"), "w") as f:
            json.dump([[k, list(v.shape)] for k, v in net.state_dict().items()], f)
        o64 = OracleModel(cfg, sd, torch.float64)
        keep = dict(weights_seed=np.array(SEED_W), weights_sha256=np.array(weights_sha(sd)))
        entry = dict(base=variants.base_name(name), overrides=variants.overrides(name), inputs={})
        for iname, x in xs.items():
            out = run_case(net, x)
            sep, vad = out["sep"], out["vad"]
            s64, v64, _ = o64(torch.from_numpy(x))
            keep[f"sep_{iname}"] = sep
            keep[f"vad_{iname}"] = vad
            keep[f"x_sha256_{iname}"] = np.array(variants.input_sha(x))
            rec = dict(sep_f32_vs_f64=float(np.abs(sep - s64.numpy()).max()), vad_margin=None, vad_f32_vs_f64=None)
            assert (vad.ndim == 0) == (name in variants.NO_VAD), (name, vad.shape)
            if vad.ndim:
                rec["vad_margin"] = float(np.abs(vad - 0.5).min())
                rec["vad_f32_vs_f64"] = float(np.abs(vad - v64.numpy()).max())
                if rec["vad_margin"] < MIN_MARGIN or rec["vad_margin"] < MARGIN_OVER_NOISE * rec["vad_f32_vs_f64"]:
                    bad.append(f"{name}/{iname}: margin {rec['vad_margin']:.3g}, fp32-vs-fp64 {rec['vad_f32_vs_f64']:.3g}")
            entry["inputs"][iname] = rec
            print(name, iname, rec)
        if name == "masked_vad":
            o2 = run_case(net, xs["t32"], inference_kw=dict(variants.IKW))
            keep.update(ikw_sep=o2["sep"], ikw_vad=o2["vad"])
        fn = variants.golden_path(name)
        np.savez_compressed(fn, **keep)
        entry["bytes"] = os.path.getsize(fn)
        total += entry["bytes"]
        if entry["bytes"] > MAX_FILE:
            bad.append(f"{name}: fixture of {entry['bytes']} bytes")
        manifest["variants"][name] = entry
    manifest["total_bytes"] = total
    if total > MAX_SET:
        bad.append(f"fixture set of {total} bytes")
    with open(os.path.join(HERE, "VARIANTS_MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    if bad:
        sys.exit("input condition not met: " + "; ".join(bad))
    print("input condition holds for every entry;", total, "bytes")


if __name__ == "__main__":
    main()
