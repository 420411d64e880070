"""Reference goldens for the weight profiles and the silence input of tests/weight_profiles.py (CPU only; needs the
reference tree).

    python tests/golden/make_profile_golden.py

Per profile x {with_vad, without_vad}: golden_profile_<profile>_<config>.npz with the REFERENCE's sep and vad (profile
weights loaded strict=True) on one T = 32 and one T = 49 input, the input seeds and sha256 (the tests regenerate the
inputs), and the weights' sha256. Per silence config (recipe weights; with_vad, without_vad, no_activity):
golden_silence_<config>.npz with the reference's sep and vad on the silence input. PROFILES_MANIFEST.json: per entry
and input the fp32-reference-to-fp64-oracle distance on sep, vad and masks_b (the noise terms of the GPU gates), the
VAD margin min |p - 0.5| (per row for the silence fixtures), the chosen seeds / cuts, the fixture sizes, and per
profile and config |mean| / std (over channels and frames, averaged over the batch rows; fp64 oracle, the T = 49
input) of the tensors entering reg2 and ln_first_modules / ln_modules at the first and the last block, for the profile
and for the recipe weights. Only data is written, and no number of the native code goes in.

Input condition (checked here, on the reference alone; exit status non-zero if unmet): every VAD margin >= 1e-3 and
>= 4x that input's fp32-vs-fp64 VAD distance (make_variant_golden.py's rule). Inputs: seeds 100, 110, ... (T = 32) and
200, 210, ... (T = 49), the first that satisfies the condition, per (profile, config). For `offset` the T = 49 seed
must also give |mean| / std entering reg2 >= 3x the recipe's on that input, at the first and at the last block, so
the profile does what it claims (without_vad: 2.97x at the last block on seed 200, where the recipe's own ratio is
0.493; the profile's is 1.46 on every seed). Silence: seeds 200, 210, ..., and for each the cut pairs of
weight_profiles.SILENCE_CUTS in order; the first (seed, cuts) that satisfies the condition on all three configs, so
they share one input. The all-zero row of no_activity is exempt (listed under "exempt_vad_rows"): its TCN input is
constant, GroupNorm sees zero variance, and the reference's own fp32 and fp64 VAD disagree there. Each fixture
<= 400 KiB, the set <= 3.5 MiB. The choices must equal the tables of weight_profiles.py (INPUT_SEEDS, SILENCE_CHOICE).
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
from make_golden import import_reference, run_case  # noqa: E402
import weight_profiles as wp  # noqa: E402
import oracle.torch_ref as torch_ref  # noqa: E402
from oracle.torch_ref import OracleModel  # noqa: E402

MAX_FILE = 400 * 1024  # bytes per fixture
MAX_SET = 3584 * 1024  # bytes for the set (3.5 MiB)
MIN_MARGIN = 1e-3
MARGIN_OVER_NOISE = 4.0
OFFSET_RATIO = 3.0
MAX_TRIES = 10


def ref_net(ref_model, cfg, sd_np):
    net = ref_model.SeparationModel(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return net.eval()


def measure(net, o64, x, rows=None):
    """The reference's outputs on x and their distances from the fp64 oracle; `rows`: the rows the VAD and masks_b
    terms cover (all by default)."""
    out = run_case(net, x)
    s64, v64, _ = o64(torch.from_numpy(x))
    rows = list(range(x.shape[0])) if rows is None else rows
    vad, v64 = out["vad"], v64.numpy()
    rec = dict(sep_f32_vs_f64=float(np.abs(out["sep"] - s64.numpy()).max()),
               vad_f32_vs_f64=float(np.abs(vad - v64)[rows].max()),
               masks_b_f32_vs_f64=float(np.abs(out["masks_b"] - o64.masks_b.numpy())[rows].max()),
               vad_margin=float(np.abs(vad - 0.5)[rows].min()),
               vad_margin_rows=[float(np.abs(vad[b] - 0.5).min()) for b in range(x.shape[0])],
               vad_f32_vs_f64_rows=[float(np.abs(vad[b] - v64[b]).max()) for b in range(x.shape[0])])
    return out, rec


def condition(rec):
    return rec["vad_margin"] >= MIN_MARGIN and rec["vad_margin"] >= MARGIN_OVER_NOISE * rec["vad_f32_vs_f64"]


def mean_over_std(cfg, sd_np, x):
    """|mean| / std of the inputs of reg2 and of ln_first_modules (recursive LN) or ln_modules (residual LN) at the
    first and the last block, fp64 oracle: every GroupNorm call of the TCN is recorded in call order (TCN.LN, then per
    block reg1, reg2 and the block's LN calls)."""
    calls = []
    orig = torch_ref.gn1

    def rec_gn1(xx, weight, bias, eps):
        m = xx.mean(dim=(1, 2))
        s = xx.std(dim=(1, 2), unbiased=False)
        calls.append(float((m.abs() / s).mean()))
        return orig(xx, weight, bias, eps)

    torch_ref.gn1 = rec_gn1
    try:
        OracleModel(cfg, sd_np, torch.float64)(torch.from_numpy(x))
    finally:
        torch_ref.gn1 = orig
    per = 4 if cfg["apply_recursive_ln"] else 3
    nblk = cfg["layer"] * cfg["stack"]
    ln = "ln_first" if cfg["apply_recursive_ln"] else "ln_modules"
    out = {}
    for tag, i in (("first", 0), ("last", nblk - 1)):
        out[f"reg2_{tag}"] = calls[1 + per * i + 1]
        out[f"{ln}_{tag}"] = calls[1 + per * i + 2]
    return out


def main():
    ref_model, _, _ = import_reference()
    torch.set_num_threads(8)
    from sep_tfanet_vad_amd import synth
    manifest = dict(weights_seed=wp.WEIGHTS_SEED, min_margin=MIN_MARGIN, margin_over_noise=MARGIN_OVER_NOISE,
                    input_shapes={k: dict(B=v[0], N=v[1], first_seed=v[2]) for k, v in wp.INPUT_SHAPES.items()},
                    profiles={}, silence={})
    bad, total = [], 0

    for profile, cname in wp.PAIRS:
        cfg = wp.config(cname)
        sd, _ = wp.state_dict_np(cfg, profile)
        net = ref_net(ref_model, cfg, sd)
        recipe_sd = synth.make_state_dict(cfg, wp.WEIGHTS_SEED)
        o64 = OracleModel(cfg, sd, torch.float64)
        keep = dict(weights_seed=np.array(wp.WEIGHTS_SEED), weights_sha256=np.array(wp.weights_sha(sd)))
        entry = dict(inputs={})
        for iname, (_, _, seed0) in wp.INPUT_SHAPES.items():
            for seed in range(seed0, seed0 + 10 * MAX_TRIES, 10):
                x = wp.make_input(iname, seed)
                out, rec = measure(net, o64, x)
                print(profile, cname, iname, seed, {k: v for k, v in rec.items() if not k.endswith("_rows")})
                ok = condition(rec)
                if ok and iname == "t49":  # the input the |mean| / std figures are taken on
                    mos = dict(profile=mean_over_std(cfg, sd, x), recipe=mean_over_std(cfg, recipe_sd, x))
                    print(profile, cname, seed, "mean/std", mos)
                    if profile == "offset":
                        ok = all(mos["profile"][t] >= OFFSET_RATIO * mos["recipe"][t] for t in ("reg2_first", "reg2_last"))
                if ok:
                    break
            else:
                bad.append(f"{profile}/{cname}/{iname}: no seed of {MAX_TRIES} meets the input condition")
            del rec["vad_margin_rows"], rec["vad_f32_vs_f64_rows"]
            rec["seed"] = seed
            if seed != wp.input_seed(profile, cname, iname):
                bad.append(f"{profile}/{cname}/{iname}: chose seed {seed}, weight_profiles.INPUT_SEEDS says "
                           f"{wp.input_seed(profile, cname, iname)}")
            keep[f"sep_{iname}"] = out["sep"]
            keep[f"vad_{iname}"] = out["vad"]
            keep[f"x_seed_{iname}"] = np.array(seed)
            keep[f"x_sha256_{iname}"] = np.array(wp.input_sha(x))
            entry["inputs"][iname] = rec
        entry["mean_over_std"] = mos
        fn = wp.golden_path("profile", profile, cname)
        np.savez_compressed(fn, **keep)
        entry["bytes"] = os.path.getsize(fn)
        total += entry["bytes"]
        if entry["bytes"] > MAX_FILE:
            bad.append(f"{profile}/{cname}: fixture of {entry['bytes']} bytes")
        manifest["profiles"][f"{profile}/{cname}"] = entry

    # ---- silence: one (seed, cuts) for the three configs ---------------------------------------------------------
    nets = {}
    for cname in wp.SILENCE_CONFIGS:
        cfg = wp.config(cname)
        sd = synth.make_state_dict(cfg, wp.WEIGHTS_SEED)
        nets[cname] = (ref_net(ref_model, cfg, sd), OracleModel(cfg, sd, torch.float64), wp.weights_sha(sd))
    exempt = {c: ([wp.SILENCE_ZERO_ROW] if c == "no_activity" else []) for c in wp.SILENCE_CONFIGS}
    chosen = None
    for seed in wp.SILENCE_SEEDS:
        for cuts in wp.SILENCE_CUTS:
            x = wp.silence_input(seed, cuts)
            res, ok = {}, True
            for cname, (net, o64, _) in nets.items():
                rows = [b for b in range(wp.SILENCE_B) if b not in exempt[cname]]
                res[cname] = measure(net, o64, x, rows)
                print("silence", cname, seed, cuts, res[cname][1])
                ok = ok and condition(res[cname][1])
            if ok:
                chosen = (seed, cuts)
                break
        if chosen:
            break
    if chosen is None:
        bad.append("silence: no (seed, cuts) meets the input condition on every config")
    elif any(tuple(wp.SILENCE_CHOICE[c]) != chosen for c in wp.SILENCE_CONFIGS):
        bad.append(f"silence: chose {chosen}, weight_profiles.SILENCE_CHOICE says {wp.SILENCE_CHOICE}")
    for cname, (out, rec) in res.items():
        if not np.isfinite(out["sep"]).all() or not np.isfinite(out["vad"]).all():
            bad.append(f"silence/{cname}: the reference is not finite")
        if np.abs(out["sep"][wp.SILENCE_ZERO_ROW]).max() != 0.0:
            bad.append(f"silence/{cname}: the reference's sep on the all-zero row is not exactly 0")
        fn = wp.golden_path("silence", cname)
        np.savez_compressed(fn, sep=out["sep"], vad=out["vad"], x_sha256=np.array(wp.input_sha(x)),
                            x_seed=np.array(seed), x_cuts=np.array(cuts), weights_seed=np.array(wp.WEIGHTS_SEED),
                            weights_sha256=np.array(nets[cname][2]))
        rec.update(seed=seed, cuts=list(cuts), exempt_vad_rows=exempt[cname], bytes=os.path.getsize(fn))
        total += rec["bytes"]
        if rec["bytes"] > MAX_FILE:
            bad.append(f"silence/{cname}: fixture of {rec['bytes']} bytes")
        manifest["silence"][cname] = rec

    manifest["total_bytes"] = total
    if total > MAX_SET:
        bad.append(f"fixture set of {total} bytes")
    with open(os.path.join(HERE, "PROFILES_MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    if bad:
        sys.exit("input condition not met: " + "; ".join(bad))
    print("input condition holds for every entry;", total, "bytes")


if __name__ == "__main__":
    main()
