"""Every architecture switch the native path accepts (config.native_support_error), not only the two shipped configs:
the nine variants of tests/variants.py through SeparationModel at the default f16x3 precision, on the fused, the
two-slice and the multi-kernel schedule, against the reference's own outputs (tests/golden/golden_variant_*.npz,
pinned to the oracle on the CPU by tests/test_oracle_variants.py).

Gates. sep: max(SEP_TOL, 2 x the reference's fp32-vs-fp64 distance on that input) -- the rule
test_gpu_parity.py::test_forward_matches_reference uses for side attributes; the short stacks amplify fp32 rounding
(layer3_stack1 at T = 49: the fp32 reference is 8.6e-5 from fp64), so a flat 1e-4 would not be a fair bound for them.
VAD probabilities: max(VAD_PROB_TOL, 2 x the fp32-vs-fp64 VAD distance); labels bit-exact (check_vad_labels; every
golden margin is >= 1e-3 and >= 4x that distance, VARIANTS_MANIFEST.json). Schedules against each other at
test_gpu_fused.py's SCHED_TOL / VAD_SCHED_TOL / LO8_TOL. Each test prints its errors beside the gate and noise term.

Measured on an MI355X (max-abs against the golden, the T=258 rows against the fp32 oracle; noise = the fp32
reference's distance from fp64 on that input, gate = the larger of the flat bound and 2 x noise). Between schedules,
over all rows: fused (fp16 lo plane) vs multi-kernel sep <= 3.8e-7 (SCHED_TOL 1e-5), vad <= 2.2e-5 (VAD_SCHED_TOL
1e-4); int8 vs fp16 lo plane sep <= 3.2e-6 (LO8_TOL 4e-5), vad <= 6.5e-5 (VAD_PROB_TOL 1e-3). Side attributes
(B = 1, N = 32000): spectrum 3.0e-4 (bound 1.0e-3, noise 1.9e-4); ctor_defaults masks_b 5.8e-5 (bound 2e-4, noise
1.5e-5), mask_per_speaker 1.4e-5 (bound 5e-5, noise 3.1e-6).
variant          input  schedule       sep err  gate     noise    | vad err  gate     noise
masked_vad       t32    fused          7.2e-07  1.0e-04  1.5e-07  | 6.8e-06  1.0e-03  2.2e-06
masked_vad       t49    fused          8.3e-07  1.0e-04  1.0e-06  | 8.6e-06  1.0e-03  5.7e-06
masked_no_phase  t32    fused          7.2e-07  1.0e-04  1.5e-07  | vad is the int 0
masked_no_phase  t49    fused          8.6e-07  1.0e-04  1.0e-06  | vad is the int 0
no_final_vad     t32    fused          6.9e-07  1.0e-04  2.1e-07  | vad is the int 0
no_final_vad     t49    fused          2.2e-06  1.0e-04  3.5e-06  | vad is the int 0
no_activity      t32    fused          9.4e-07  1.0e-04  2.0e-07  | 2.1e-05  1.0e-03  4.8e-06
no_activity      t49    fused          4.5e-06  1.0e-04  6.4e-06  | 3.3e-05  1.0e-03  4.0e-05
plain_phase      t32    fused          7.2e-07  1.0e-04  1.5e-07  | 2.3e-05  1.0e-03  2.0e-06
plain_phase      t49    fused          8.6e-07  1.0e-04  1.0e-06  | 1.4e-05  1.0e-03  2.1e-05
both_ln          t32    fused          1.3e-06  1.0e-04  1.2e-06  | 3.9e-05  1.0e-03  9.9e-06
both_ln          t49    fused          4.1e-05  1.2e-04  6.0e-05  | 1.5e-04  1.0e-03  2.2e-04
layer5_stack2    t32    fused          8.3e-07  1.0e-04  5.0e-07  | 2.6e-05  1.0e-03  7.8e-06
layer5_stack2    t49    fused          3.9e-05  1.1e-04  5.6e-05  | 2.0e-04  1.0e-03  2.8e-04
layer3_stack1    t32    fused          3.3e-06  1.0e-04  1.9e-06  | 5.4e-05  1.0e-03  4.7e-05
layer3_stack1    t49    fused          5.9e-05  1.7e-04  8.6e-05  | 5.4e-04  1.6e-03  7.9e-04
ctor_defaults    t32    fused          1.9e-06  1.0e-04  4.6e-07  | 4.4e-05  1.0e-03  1.2e-05
ctor_defaults    t49    fused          1.2e-05  1.0e-04  1.8e-05  | 2.2e-04  1.0e-03  2.9e-04
masked_vad       t32    multi-kernel   1.8e-07  1.0e-04  1.5e-07  | 2.0e-06  1.0e-03  2.2e-06
masked_vad       t49    multi-kernel   7.5e-07  1.0e-04  1.0e-06  | 4.8e-06  1.0e-03  5.7e-06
masked_no_phase  t32    multi-kernel   2.1e-07  1.0e-04  1.5e-07  | vad is the int 0
masked_no_phase  t49    multi-kernel   7.7e-07  1.0e-04  1.0e-06  | vad is the int 0
no_final_vad     t32    multi-kernel   3.0e-07  1.0e-04  2.1e-07  | vad is the int 0
no_final_vad     t49    multi-kernel   2.3e-06  1.0e-04  3.5e-06  | vad is the int 0
no_activity      t32    multi-kernel   3.5e-07  1.0e-04  2.0e-07  | 5.4e-06  1.0e-03  4.8e-06
no_activity      t49    multi-kernel   4.4e-06  1.0e-04  6.4e-06  | 2.6e-05  1.0e-03  4.0e-05
plain_phase      t32    multi-kernel   2.1e-07  1.0e-04  1.5e-07  | 3.3e-06  1.0e-03  2.0e-06
plain_phase      t49    multi-kernel   7.7e-07  1.0e-04  1.0e-06  | 1.6e-05  1.0e-03  2.1e-05
both_ln          t32    multi-kernel   1.3e-06  1.0e-04  1.2e-06  | 2.4e-05  1.0e-03  9.9e-06
both_ln          t49    multi-kernel   4.1e-05  1.2e-04  6.0e-05  | 1.5e-04  1.0e-03  2.2e-04
layer5_stack2    t32    multi-kernel   5.0e-07  1.0e-04  5.0e-07  | 5.3e-06  1.0e-03  7.8e-06
layer5_stack2    t49    multi-kernel   3.9e-05  1.1e-04  5.6e-05  | 1.9e-04  1.0e-03  2.8e-04
layer3_stack1    t32    multi-kernel   3.1e-06  1.0e-04  1.9e-06  | 4.8e-05  1.0e-03  4.7e-05
layer3_stack1    t49    multi-kernel   5.9e-05  1.7e-04  8.6e-05  | 5.5e-04  1.6e-03  7.9e-04
ctor_defaults    t32    multi-kernel   7.5e-07  1.0e-04  4.6e-07  | 1.0e-05  1.0e-03  1.2e-05
ctor_defaults    t49    multi-kernel   1.2e-05  1.0e-04  1.8e-05  | 2.0e-04  1.0e-03  2.9e-04
masked_vad       T=258  fused          1.9e-06  1.0e-04  3.2e-07  | 1.3e-05  1.0e-03  2.2e-06
masked_vad       T=258  multi-kernel   7.6e-07  1.0e-04  3.2e-07  | 3.1e-06  1.0e-03  2.2e-06
no_activity      T=258  fused          2.8e-06  1.0e-04  5.2e-07  | 2.7e-05  1.0e-03  1.2e-05
no_activity      T=258  multi-kernel   7.7e-07  1.0e-04  5.2e-07  | 1.5e-05  1.0e-03  1.2e-05
ctor_defaults    t49    fp32 fused     1.2e-05  1.0e-04  1.8e-05  | 2.0e-04  1.0e-03  2.9e-04
both_ln          t49    fp32 fused     4.1e-05  1.2e-04  6.0e-05  | 1.6e-04  1.0e-03  2.2e-04
"""
import numpy as np
import pytest
import torch

import variants
from conftest import check_vad_labels
from test_gpu_fused import LO8_TOL, SCHED_TOL, SEP_TOL, VAD_PROB_TOL, VAD_SCHED_TOL, _run, _run_slices

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(n, i) for n in variants.NAMES for i in variants.INPUTS]

_NETS, _ORACLE, _GOLDEN, _X = {}, {}, {}, {}


def _net(name):
    """SeparationModel of variant `name` with its recipe weights (strict=True), f16x3, cached for the module."""
    if name not in _NETS:
        import sep_tfanet_vad_amd as pkg
        net = pkg.SeparationModel(**variants.config(name))
        net.load_state_dict(variants.state_dict(name), strict=True)
        net = net.eval().to(DEV)
        net.native_precision = "f16x3"
        _NETS[name] = net
    return _NETS[name]


def _golden(name):
    if name not in _GOLDEN:
        _GOLDEN[name] = variants.load_golden(name)
    return _GOLDEN[name]


def _x(iname):
    """Golden input `iname` (regenerated from its seed, checked against the sha every fixture stores)."""
    if iname not in _X:
        x = variants.make_input(iname)
        for name in variants.NAMES:
            assert str(_golden(name)[f"x_sha256_{iname}"]) == variants.input_sha(x)
        _X[iname] = torch.from_numpy(x)
    return _X[iname]


def _oracle(name, key, x):
    """fp32 and fp64 oracle runs of variant `name` on x, cached per (variant, input key): dict with sep / vad (numpy;
    vad the int 0 where the forward returns it) and the side attributes of both, computed once and left unchanged."""
    if (name, key) not in _ORACLE:
        from oracle.torch_ref import OracleModel
        out = {}
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            om = OracleModel(variants.config(name), variants.state_dict(name), dt)
            sep, vad, _ = om(x)
            out[tag] = dict(sep=sep.numpy(), vad=vad.numpy() if torch.is_tensor(vad) else vad,
                            spectrum=om.spectrum.numpy(), masks_b=om.masks_b.numpy(),
                            mask_per_speaker=om.mask_per_speaker.numpy())
        _ORACLE[(name, key)] = out
    return _ORACLE[(name, key)]


def _gates(sep_noise, vad_noise):
    return max(SEP_TOL, 2.0 * sep_noise), max(VAD_PROB_TOL, 2.0 * (vad_noise or 0.0))


def _golden_gates(name, iname):
    rec = variants.load_manifest()["variants"][name]["inputs"][iname]
    return _gates(rec["sep_f32_vs_f64"], rec["vad_f32_vs_f64"]) + (rec["sep_f32_vs_f64"], rec["vad_f32_vs_f64"])


def _check_outputs(where, sep, vad, sep_ref, vad_ref, sep_gate, vad_gate, sep_noise, vad_noise):
    """sep and vad of one GPU forward against a reference: gates as in the module docstring; vad must be the int 0
    exactly where the reference's is."""
    err = float(np.abs(sep.cpu().numpy() - sep_ref).max())
    print(f"{where}: sep max-abs {err:.3e} (gate {sep_gate:.3e}, fp32-vs-fp64 noise {sep_noise:.3e})")
    if np.ndim(vad_ref) == 0:
        assert isinstance(vad, int) and vad == 0 and vad_ref == 0, f"{where}: vad is {type(vad)}, the reference returns 0"
    else:
        assert torch.is_tensor(vad) and tuple(vad.shape) == vad_ref.shape
        v = vad.cpu().numpy()
        verr = float(np.abs(v - vad_ref).max())
        print(f"{where}: vad max-abs {verr:.3e} (gate {vad_gate:.3e}, fp32-vs-fp64 noise {vad_noise:.3e})")
        check_vad_labels(v, vad_ref, where=where)
        assert verr <= vad_gate, f"{where}: vad max-abs {verr} > {vad_gate}"
    assert err <= sep_gate, f"{where}: sep max-abs {err} > {sep_gate}"


def _vdiff(a, b):
    """max-abs distance of two vad results; both the int 0 counts as 0."""
    if isinstance(a, int) or isinstance(b, int):
        assert isinstance(a, int) and isinstance(b, int) and a == b == 0
        return 0.0
    return (a - b).abs().max().item()


def _check_schedules(where, net, x, sf, vf, ikw=None):
    """test_gpu_fused._check_schedules for variants (vad may be the int 0): the fused kernel with the fp16 weight lo
    plane vs the multi-kernel schedule at SCHED_TOL / VAD_SCHED_TOL, the default int8 lo plane (sf, vf) vs it at
    LO8_TOL / VAD_PROB_TOL. Returns the multi-kernel sep, vad."""
    s16, v16, _, used = _run(net, x, True, ikw, wlo="f16")
    assert used, "the fused TCN did not run"
    sm, vm, _, used_m = _run(net, x, False, ikw)
    assert not used_m
    d = ((s16 - sm).abs().max().item(), _vdiff(v16, vm), (sf - s16).abs().max().item(), _vdiff(vf, v16))
    print(f"{where}: fused(f16 lo) vs multi-kernel sep {d[0]:.3e} (<= {SCHED_TOL:g}) vad {d[1]:.3e} (<= {VAD_SCHED_TOL:g}); "
          f"fused(i8 lo) vs fused(f16 lo) sep {d[2]:.3e} (<= {LO8_TOL:g}) vad {d[3]:.3e} (<= {VAD_PROB_TOL:g})")
    assert d[0] <= SCHED_TOL and d[1] <= VAD_SCHED_TOL and d[2] <= LO8_TOL and d[3] <= VAD_PROB_TOL
    return sm, vm


# ---- the matrix: every variant x both golden inputs x the three schedules ------------------------------------------
@pytest.mark.parametrize("name,iname", PAIRS)
def test_fused_matches_variant_golden(name, iname):
    g = _golden(name)
    sep, vad, _, used = _run(_net(name), _x(iname).to(DEV), True)
    assert used, "the fused TCN did not run"
    _check_outputs(f"{name} {iname} fused", sep, vad, g[f"sep_{iname}"], g[f"vad_{iname}"], *_golden_gates(name, iname))


@pytest.mark.parametrize("name,iname", PAIRS)
def test_multikernel_matches_variant_golden_and_fused(name, iname):
    g = _golden(name)
    net, x = _net(name), _x(iname).to(DEV)
    sf, vf, _, used = _run(net, x, True)
    assert used
    sm, vm = _check_schedules(f"{name} {iname}", net, x, sf, vf)
    _check_outputs(f"{name} {iname} multi-kernel", sm, vm, g[f"sep_{iname}"], g[f"vad_{iname}"],
                   *_golden_gates(name, iname))


@pytest.mark.parametrize("name", variants.NAMES)
def test_two_slices_bitwise_equal_one_slice(name, monkeypatch):
    """T = 49 forced to two-slice workgroups (one workgroup of 64 frames instead of two of 32): every statistic is
    reduced in the one-slice order, so sep, vad and est are bitwise equal -- on every variant's instantiation."""
    net, x = _net(name), _x("t49").to(DEV)
    s1, v1, e1, u1 = _run_slices(net, x, 1, monkeypatch)
    s2, v2, e2, u2 = _run_slices(net, x, 2, monkeypatch)
    assert (u1, u2) == (1, 2)
    assert torch.equal(s1, s2) and torch.equal(e1, e2)
    assert torch.equal(v1, v2) if torch.is_tensor(v1) else (isinstance(v2, int) and v1 == v2 == 0)


# ---- specific paths ------------------------------------------------------------------------------------------------
# seed chosen on the CPU: the fp64 oracle's VAD margin min |p - 0.5| on synth.make_batch(2, 66000, seed) is 2.3e-3
# (masked_vad) and 3.8e-3 (no_activity); of the seeds 700, 710 .. 750 only 700 and 710 keep both above 1e-3
LONG_SEED = {"masked_vad": 700, "no_activity": 700}


@pytest.mark.parametrize("name", ["masked_vad", "no_activity"])
def test_t258_vs_oracle_both_schedules(name):
    """T = 258 (N = 66000, G = 9): several k_vad1 row blocks per (utterance, speaker) for masked_vad; for no_activity
    the T > 256 side of the VAD-feature switch (k_vad_feat instead of the taps finished in k_istft_pair). B = 2,
    both schedules against the fp32 oracle; noise term: the fp32 oracle's distance from the fp64 oracle."""
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(2, 66000, LONG_SEED[name])[0])
    o = _oracle(name, "t258", x)
    assert float(np.abs(o["f64"]["vad"] - 0.5).min()) >= 1e-3
    sn = float(np.abs(o["f32"]["sep"] - o["f64"]["sep"]).max())
    vn = float(np.abs(o["f32"]["vad"] - o["f64"]["vad"]).max())
    gates = _gates(sn, vn) + (sn, vn)
    net = _net(name)
    sf, vf, _, used = _run(net, x.to(DEV), True)
    assert used
    _check_outputs(f"{name} T=258 fused", sf, vf, o["f32"]["sep"], o["f32"]["vad"], *gates)
    sm, vm = _check_schedules(f"{name} T=258", net, x.to(DEV), sf, vf)
    _check_outputs(f"{name} T=258 multi-kernel", sm, vm, o["f32"]["sep"], o["f32"]["vad"], *gates)


@pytest.mark.parametrize("fused", [True, False])
def test_masked_vad_inference_kw(fused):
    """The smoothed-VAD branch (model/model.py:444-457) fed by k_vad1's masked-spectrum probabilities: the {0, 1}
    smoothed VAD bit-equal to the reference's, the filtered sep within the gate."""
    g = _golden("masked_vad")
    sep, vad, _, used = _run(_net("masked_vad"), _x("t32").to(DEV), fused, dict(variants.IKW))
    assert bool(used) == fused
    assert tuple(vad.shape) == g["ikw_vad"].shape  # [B, 2, 1, T]
    assert np.array_equal(vad.cpu().numpy(), g["ikw_vad"])
    sep_gate, _, sn, _ = _golden_gates("masked_vad", "t32")
    err = float(np.abs(sep.cpu().numpy() - g["ikw_sep"]).max())
    print(f"masked_vad inference_kw fused={fused}: sep max-abs {err:.3e} (gate {sep_gate:.3e}, noise {sn:.3e})")
    assert err <= sep_gate


@pytest.mark.parametrize("fused", [True, False])
def test_masked_vad_batch_rows_bitwise(fused):
    """k_vad1 indexes (utterance, speaker) pairs: row 1 forwarded alone equals row 1 of the batch forward, bitwise."""
    net, x = _net("masked_vad"), _x("t49").to(DEV)
    sb, vb, eb, _ = _run(net, x, fused)
    s1, v1, e1, _ = _run(net, x[1:2], fused)
    assert torch.equal(sb[1:2], s1) and torch.equal(vb[1:2], v1) and torch.equal(eb[1:2], e1)
    assert not torch.equal(vb[0], vb[1])


@pytest.mark.parametrize("name", variants.NO_VAD)
@pytest.mark.parametrize("fused", [True, False])
def test_no_vad_variants_ignore_inference_kw(name, fused):
    """Pinned native behaviour: without a VAD output inference_kw changes nothing -- sep bitwise
    equal to the run without it and vad the int 0. The reference skips the branch for final_vad=False
    (model/model.py:444) and raises for masked_no_phase (its output_vad is the int 0 there)."""
    net, x = _net(name), _x("t49").to(DEV)
    s0, v0, e0, _ = _run(net, x, fused)
    s1, v1, e1, _ = _run(net, x, fused, dict(variants.IKW))
    assert isinstance(v0, int) and isinstance(v1, int) and v0 == v1 == 0
    assert torch.equal(s0, s1) and torch.equal(e0, e1)


SIDE_INPUT = (1, 32000, 300)  # the input of test_gpu_parity.py::test_side_attributes_tight (the "cfg" golden's)


@pytest.mark.parametrize("name,attrs", [("no_activity", ("spectrum",)),
                                        ("ctor_defaults", ("spectrum", "masks_b", "mask_per_speaker"))])
def test_side_attributes_vs_oracle(name, attrs):
    """The side attributes without the activity gate (the plain dB spectrum of k_stft_gate / the side pass), lazily
    materialised and through return_aux, against the fp32 oracle at test_side_attributes_tight's bounds: spectrum
    within 1e-5 of its range on bins with |X| > 1e-2, masks_b within 2e-4, mask_per_speaker within 5e-5."""
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(*SIDE_INPUT)[0])
    ref = _oracle(name, "side", x)["f32"]
    n64 = _oracle(name, "side", x)["f64"]
    net = _net(name)
    with torch.no_grad():
        net(x.to(DEV))
    lazy = {a: getattr(net, a).cpu().numpy() for a in attrs}
    aux = net.native_handle(DEV).forward(x.to(DEV), return_aux=True)
    X = torch.stft(x, 512, 256, 512, torch.hann_window(512), center=True, pad_mode="reflect", return_complex=True)
    ok = (X.abs() > 1e-2).numpy()
    ok[:, 0, :] = True  # DC: exactly -100 dB in both
    tol = dict(spectrum=1e-5 * float(np.abs(ref["spectrum"]).max()), masks_b=2e-4, mask_per_speaker=5e-5)
    for a in attrs:
        assert np.array_equal(lazy[a], aux[a].cpu().numpy()), f"{a}: return_aux differs from the side attribute"
        d, noise = np.abs(lazy[a] - ref[a]), np.abs(ref[a] - n64[a])
        if a == "spectrum":
            d, noise = d[ok], noise[ok]
        print(f"{name} {a}: max-abs vs fp32 oracle {d.max():.3e} (bound {tol[a]:.3e}, fp32-vs-fp64 noise {noise.max():.3e})")
        assert d.max() <= tol[a], f"{a}: {d.max()} > {tol[a]}"
    if name == "no_activity":  # ungated: the spectrum is the plain dB of |X|^2
        db = 10.0 * torch.log10(torch.clamp(X.abs() ** 2, min=1e-10)).numpy()
        assert np.abs(ref["spectrum"][:, 1:] - db[:, 1:])[ok[:, 1:]].max() <= tol["spectrum"]


@pytest.mark.parametrize("name", ["no_final_vad", "masked_vad"])
@pytest.mark.parametrize("N", [32000, 53120])
def test_streaming_one_forward_equals_window_loop(name, N, tmp_path):
    """OnlineSaving with every window in one forward (sepvad_forward_windows: a null VAD pointer for no_final_vad,
    k_vad1 over window-major rows for masked_vad) equals the window loop bitwise. B = 2, save_sec = 0.16; 32 000
    samples are padded to the 3 s window (one window), 53 120 give three. masked_vad runs under the golden's
    inference_kw, so k_vad1's smoothed labels gate the stitched signal."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(2, N, 4300 + N)[0]).to(DEV)
    ikw = dict(variants.IKW) if name == "masked_vad" else dict(pkg.INFERENCE_KW_DEFAULTS)
    crit = pkg.PITLossWrapper(loss_func=torch.nn.L1Loss(), pit_from="pw_pt")
    outs = []
    for one in (True, False):
        ons = pkg.OnlineSaving(_net(name), str(tmp_path), crit)
        ons.save_sec = 0.16
        ons.one_forward = one
        ons.calc_online(x, "s", 10 ** 6, ikw)
        outs.append(ons.online_signal.clone())
    assert outs[0].shape == (2, 2, (1 if N == 32000 else 3) * 2560)
    assert torch.isfinite(outs[0]).all()
    # 32 000 samples: the one stitched hop is the window's last 160 ms, all padding -- exact zeros; the longer input
    # stitches separated signal
    assert (outs[0].abs().max().item() > 1e-3) == (N != 32000)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name", ["ctor_defaults", "both_ln"])
def test_fp32_arm(name):
    """The exact-fp32 k_tcn instantiations of LD_ADD (ctor_defaults) and of recursive LN with the closed-form
    statistics (both_ln) at T = 49: fused, within the same gates of the golden, and within SCHED_TOL of the
    multi-kernel fp32 schedule (as test_gpu_fused.py::test_fp32_gemms_run_fused)."""
    g = _golden(name)
    net, x = _net(name), _x("t49").to(DEV)
    net.native_precision = "fp32"
    try:
        sf, vf, _, used = _run(net, x, True)
        assert used, "the fused TCN did not run"
        sm, vm, _, used_m = _run(net, x, False)
        assert not used_m
    finally:
        net.native_precision = "f16x3"
    _check_outputs(f"{name} t49 fp32 fused", sf, vf, g["sep_t49"], g["vad_t49"], *_golden_gates(name, "t49"))
    d_s, d_v = (sf - sm).abs().max().item(), _vdiff(vf, vm)
    print(f"{name} t49 fp32: fused vs multi-kernel sep {d_s:.3e} (<= {SCHED_TOL:g}) vad {d_v:.3e} (<= {VAD_SCHED_TOL:g})")
    assert d_s <= SCHED_TOL and d_v <= VAD_SCHED_TOL
