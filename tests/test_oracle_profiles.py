"""The oracle (oracle/torch_ref.py) pinned against the reference under the weight profiles and on the silence input of
tests/weight_profiles.py, so that tests/test_gpu_profiles.py may use it (fp32 and fp64) as the yardstick there too.
Goldens: tests/golden/make_profile_golden.py (the reference's own sep / vad).

Bounds are those of test_oracle_variants.py (sep 2e-6, VAD probabilities 2e-5, labels equal). Each profile golden must
also be able to fail: the recipe weights miss it by more than 100x the sep gate.
"""
import os

import numpy as np
import pytest
import torch

import weight_profiles as wp
from oracle.torch_ref import OracleModel
from test_gpu_fused import SEP_TOL

INAMES = tuple(wp.INPUT_SHAPES)
CASES = [(p, c, i) for p, c in wp.PAIRS for i in INAMES]

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _golden(kind, *parts):
    return _cached(("golden", kind) + parts, lambda: wp.load_golden(kind, *parts))


def _x(profile, cname, iname):
    seed = wp.input_seed(profile, cname, iname)
    return _cached(("x", iname, seed), lambda: torch.from_numpy(wp.make_input(iname, seed)))


def _sd(profile, cname):
    return _cached(("sd", profile, cname), lambda: wp.state_dict(wp.config(cname), profile))


def _recipe_sd(cname):
    from sep_tfanet_vad_amd import synth
    return _cached(("recipe", cname), lambda: {k: torch.from_numpy(v) for k, v in
                                               synth.make_state_dict(wp.config(cname), wp.WEIGHTS_SEED).items()})


def _run(cname, sd, x):
    sep, vad, _ = OracleModel(wp.config(cname), sd, torch.float32)(x)
    return sep.numpy(), vad.numpy()


@pytest.mark.parametrize("profile,cname", wp.PAIRS)
def test_fixture_inputs_and_weights_regenerate(profile, cname):
    """Neither inputs nor weights are stored: the seeds of weight_profiles.INPUT_SEEDS and the profile's edit of the
    recipe reproduce what the reference ran, and the manifest names the same seeds."""
    g = _golden("profile", profile, cname)
    man = wp.load_manifest()["profiles"][f"{profile}/{cname}"]
    assert int(g["weights_seed"]) == wp.WEIGHTS_SEED
    assert str(g["weights_sha256"]) == wp.weights_sha(_sd(profile, cname))
    for iname in INAMES:
        assert int(g[f"x_seed_{iname}"]) == man["inputs"][iname]["seed"] == wp.input_seed(profile, cname, iname)
        assert str(g[f"x_sha256_{iname}"]) == wp.input_sha(_x(profile, cname, iname).numpy())


@pytest.mark.parametrize("cname", wp.SILENCE_CONFIGS)
def test_silence_fixture_regenerates(cname):
    g = _golden("silence", cname)
    man = wp.load_manifest()["silence"][cname]
    seed, cuts = wp.SILENCE_CHOICE[cname]
    assert (int(g["x_seed"]), tuple(int(c) for c in g["x_cuts"])) == (seed, tuple(cuts)) == (man["seed"], tuple(man["cuts"]))
    x = wp.chosen_silence_input(cname)
    assert str(g["x_sha256"]) == wp.input_sha(x)
    assert str(g["weights_sha256"]) == wp.weights_sha(_recipe_sd(cname))
    # the input is what it claims: exact zeros where cut, signal elsewhere, and frames wholly inside the zeros
    assert not x[0, :cuts[0]].any() and not x[1].any() and not x[2, cuts[1]:].any()
    assert np.abs(x[0, cuts[0]:]).max() > 0.1 and np.abs(x[2, :cuts[1]]).max() > 0.1
    sil = wp.silent_frames(x)
    assert sil[1].all() and 5 <= sil[0].sum() < sil.shape[1] and 5 <= sil[2].sum() < sil.shape[1]
    assert sil[0, 0] and not sil[0, -1] and sil[2, -1] and not sil[2, 0]


def test_manifest_input_condition():
    """Every stored VAD margin is >= 1e-3 and >= 4x the input's fp32-vs-fp64 VAD distance (the rule of
    test_oracle_variants.py::test_manifest_input_condition); the all-zero row of no_activity, and only it, is exempt.
    `offset` raises |mean| / std entering reg2 to >= 3x the recipe's. Each fixture <= 400 KiB, the set <= 3.5 MiB."""
    man = wp.load_manifest()
    assert set(man["profiles"]) == {f"{p}/{c}" for p, c in wp.PAIRS}
    assert set(man["silence"]) == set(wp.SILENCE_CONFIGS)
    total = 0
    for profile, cname in wp.PAIRS:
        entry = man["profiles"][f"{profile}/{cname}"]
        size = os.path.getsize(wp.golden_path("profile", profile, cname))
        assert size == entry["bytes"] and size <= 400 * 1024
        total += size
        g = _golden("profile", profile, cname)
        for iname in INAMES:
            rec = entry["inputs"][iname]
            assert rec["vad_margin"] == float(np.abs(g[f"vad_{iname}"] - 0.5).min())
            assert rec["vad_margin"] >= 1e-3 and rec["vad_margin"] >= 4.0 * rec["vad_f32_vs_f64"], (profile, cname, rec)
        if profile == "offset":
            mos = entry["mean_over_std"]
            for tag in ("reg2_first", "reg2_last"):
                assert mos["profile"][tag] >= 3.0 * mos["recipe"][tag], (cname, tag, mos)
    for cname in wp.SILENCE_CONFIGS:
        rec = man["silence"][cname]
        size = os.path.getsize(wp.golden_path("silence", cname))
        assert size == rec["bytes"] and size <= 400 * 1024
        total += size
        assert rec["exempt_vad_rows"] == ([wp.SILENCE_ZERO_ROW] if cname == "no_activity" else [])
        vad = _golden("silence", cname)["vad"]
        rows = [b for b in range(wp.SILENCE_B) if b not in rec["exempt_vad_rows"]]
        for b in range(wp.SILENCE_B):
            assert rec["vad_margin_rows"][b] == float(np.abs(vad[b] - 0.5).min())
        assert rec["vad_margin"] == min(rec["vad_margin_rows"][b] for b in rows)
        assert rec["vad_f32_vs_f64"] == max(rec["vad_f32_vs_f64_rows"][b] for b in rows)
        assert rec["vad_margin"] >= 1e-3 and rec["vad_margin"] >= 4.0 * rec["vad_f32_vs_f64"], (cname, rec)
    assert total == man["total_bytes"] <= 3584 * 1024


@pytest.mark.parametrize("profile,cname,iname", CASES)
def test_oracle_fp32_matches_profile_golden(profile, cname, iname):
    g = _golden("profile", profile, cname)
    sep, vad = _cached(("out", profile, cname, iname),
                       lambda: _run(cname, _sd(profile, cname), _x(profile, cname, iname)))
    d_sep = np.abs(sep - g[f"sep_{iname}"]).max()
    d_vad = np.abs(vad - g[f"vad_{iname}"]).max()
    print(f"{profile} {cname} {iname}: oracle fp32 vs reference sep {d_sep:.2e} vad {d_vad:.2e}")
    assert np.isfinite(sep).all() and np.isfinite(vad).all()
    assert d_sep <= 2e-6
    assert d_vad <= 2e-5
    assert np.array_equal(vad >= 0.5, g[f"vad_{iname}"] >= 0.5)


@pytest.mark.parametrize("cname", wp.SILENCE_CONFIGS)
def test_oracle_fp32_matches_silence_golden(cname):
    """On every row the manifest does not exempt: the bounds above. On the all-zero row sep is exactly 0 in the
    reference and in the oracle, in every config; where the row is exempt its VAD probabilities are not compared."""
    g = _golden("silence", cname)
    exempt = wp.load_manifest()["silence"][cname]["exempt_vad_rows"]
    rows = [b for b in range(wp.SILENCE_B) if b not in exempt]
    sep, vad = _run(cname, _recipe_sd(cname), torch.from_numpy(wp.chosen_silence_input(cname)))
    assert np.isfinite(g["sep"]).all() and np.isfinite(g["vad"]).all()
    assert np.isfinite(sep).all() and np.isfinite(vad[rows]).all()
    assert not g["sep"][wp.SILENCE_ZERO_ROW].any() and not sep[wp.SILENCE_ZERO_ROW].any()
    d_sep = np.abs(sep - g["sep"]).max()
    d_vad = np.abs(vad - g["vad"])[rows].max()
    print(f"silence {cname}: oracle fp32 vs reference sep {d_sep:.2e} vad {d_vad:.2e} (rows {rows})")
    assert d_sep <= 2e-6
    assert d_vad <= 2e-5
    assert np.array_equal(vad[rows] >= 0.5, g["vad"][rows] >= 0.5)


@pytest.mark.parametrize("profile,cname,iname", CASES)
def test_recipe_weights_miss_profile_golden(profile, cname, iname):
    """A fixture must not be satisfiable by the wrong weights: the oracle with the recipe weights, on the same input,
    misses the golden's sep by more than 100x the GPU test's sep gate."""
    g = _golden("profile", profile, cname)
    rec = wp.load_manifest()["profiles"][f"{profile}/{cname}"]["inputs"][iname]
    sep, _ = _run(cname, _recipe_sd(cname), _x(profile, cname, iname))
    gate = max(SEP_TOL, 2.0 * rec["sep_f32_vs_f64"])
    miss = np.abs(sep - g[f"sep_{iname}"]).max()
    print(f"{profile} {cname} {iname}: recipe weights miss the golden's sep by {miss:.3g} (gate {gate:.3g})")
    assert miss > 100 * gate


@pytest.mark.parametrize("profile,cname", wp.PAIRS)
def test_state_dict_deterministic_and_local(profile, cname):
    """weight_profiles.state_dict is deterministic, keeps the recipe's keys, shapes and dtype, edits only the kinds
    its row of the table names, leaves every other tensor bit-identical to the recipe, and does edit what it names."""
    from sep_tfanet_vad_amd.config import param_spec
    cfg = wp.config(cname)
    a, edited = wp.state_dict_np(cfg, profile)
    b, _ = wp.state_dict_np(cfg, profile)
    rec = _recipe_sd(cname)
    assert list(a) == list(rec)
    kinds = {k: (kind, tuple(shape)) for k, shape, kind in param_spec(cfg)}
    allowed = dict(signed=("wn_g", "gn_w", "prelu"), offset=("bias", "gn_b"), sparse=("wn_g", "gn_w"),
                   spread=("gn_w", "wn_g", "wn_v"))[profile]
    for k, v in a.items():
        assert v.dtype == np.float32 and v.shape == tuple(rec[k].shape) and np.array_equal(v, b[k])
        assert np.isfinite(v).all()
        if k in edited:
            assert kinds[k][0] in allowed, k
            if profile != "signed" or v.size >= 64:  # a handful of +-1 draws may all come out +1
                assert not np.array_equal(v, rec[k].numpy()), k
        else:
            assert np.array_equal(v, rec[k].numpy()), k
    assert edited
    ek = lambda kind: [k for k in edited if kinds[k][0] == kind]  # noqa: E731
    if profile == "signed":
        g = np.concatenate([a[k].ravel() for k in ek("wn_g") + ek("gn_w")])
        assert 0.4 < (g < 0).mean() < 0.6
        slopes = np.concatenate([a[k].ravel() for k in ek("prelu")])
        assert set(np.unique(slopes)) == set(np.float32(wp.SLOPES))
        assert len(ek("prelu")) == sum(1 for v in kinds.values() if v[0] == "prelu")
    elif profile == "offset":
        assert all(k.startswith("TCN.") for k in edited)
        assert all(np.array_equal(a[k], rec[k].numpy() + np.float32(3.0 if kinds[k][0] == "bias" else 2.0)) for k in edited)
    elif profile == "sparse":
        for k in ek("wn_g"):
            z = np.flatnonzero(a[k].ravel() == 0)
            assert len(z) == 40 and set(range(32, 64)) <= set(z)
        assert all((a[k] == 0).sum() == 16 for k in ek("gn_w"))
        assert ek("wn_g") and ek("gn_w")
    else:
        for k in ek("wn_v"):
            r = a[k] / rec[k].numpy()  # one factor in (2^-3, 1] per input column
            assert np.allclose(r, r[:1]) and r.max() <= 1.0 and r.min() >= 0.125 and r.min() < 0.25
        for k in ek("wn_g"):
            r = (a[k] / rec[k].numpy()).ravel()
            assert r.min() < 0.25 and r.max() > 4.0
        assert ek("wn_v") and ek("wn_g") and ek("gn_w")
