"""OnlineSavingKnownTargets (online_known.py) end to end against the reference's own run of
model/online_class_known_targets.OnlineSaving (tests/golden/golden_stream_eval_*.npz): the fixture's three cases and
three similarity modes.

* the stitched signal within 1e-4 of the reference's, up to one exchange of the speakers fixed on hop 0 (per row, or
  for the batch with L1: window 0's similarity decision sits on a near-tie in the reference itself);
* every decided permutation equal (stream_eval_cases.check_perms);
* both scores within the dB change that a 1e-4 per-sample error of the scored signal can cause, derived per row from
  the reference signals' own signal and residual energies (score_bound below), plus the reference's float32-vs-float64
  difference;
* the fused path (sepvad_stream_eval) bitwise equal to the composed one, chunked forwards included; indx back at 0;
  the lists grow by one per call.
"""
import numpy as np
import pytest
import torch

import stream_eval_cases as sc
from conftest import config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
WAVE_TOL = 1e-4   # the project's gate for the forward's waveforms (test_gpu_parity.py)


@pytest.fixture(scope="module")
def net(state_dicts):
    import sep_tfanet_vad_amd as pkg
    m = pkg.SeparationModel(**config_of("with_vad"))
    m.load_state_dict(state_dicts["with_vad"], strict=True)
    return m.eval().to(DEV)


@pytest.fixture(scope="module")
def oracle_full(state_dicts):
    """The CPU oracle's whole-file forward of a case's padded mixture (the signal the reference score is taken on;
    the fixture stores that score only), once per case."""
    from oracle.torch_ref import OracleModel
    om = OracleModel(config_of("with_vad"), state_dicts["with_vad"], torch.float32)
    cache = {}

    def full(name, mix):
        if name not in cache:
            cache[name] = om(mix)[0]
        return cache[name]
    return full


def criteria(mode):
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import metrics, sdr
    sep = pkg.PITLossWrapper(sdr.pairwise_neg_sisdr, pit_from="pw_mtx")
    sim = {"none": None, "l1": pkg.PITLossWrapper(torch.nn.L1Loss(), pit_from="pw_pt"),
           "sisdr": pkg.PITLossWrapper(metrics.calc_sisdr_loss, pit_from="pw_pt")}[mode]
    return sep, sim


def score_bound(est, tgt, d=WAVE_TOL):
    """How far calc_sisdr(est, tgt) [B, 2] can move when every sample of est moves by at most d, in dB per row. With
    s = alpha t the projection of the zero-mean estimate on the target and e = est - s, SI-SDR = 20 log10(|s| / |e|).
    A perturbation of norm at most r = d sqrt(n) moves |s| and |e| by at most r each (projections do not lengthen a
    vector), so the score moves by at most 20 log10((1 + r / |s|) / (1 - r / |e|))."""
    est, tgt = est.double(), tgt.double()
    est, tgt = est - est.mean(-1, keepdim=True), tgt - tgt.mean(-1, keepdim=True)
    s = (est * tgt).sum(-1, keepdim=True) / (tgt ** 2).sum(-1, keepdim=True) * tgt
    ns, ne = s.norm(dim=-1), (est - s).norm(dim=-1)
    r = d * np.sqrt(est.shape[-1])
    assert bool((r < 0.5 * ne).all())
    return 20 * torch.log10((1 + r / ns) / (1 - r / ne))


def run(net, mix, srcs, save_sec, mode, fused=True, max_window_utts=None):
    import sep_tfanet_vad_amd as pkg
    sep, sim = criteria(mode)
    ons = pkg.OnlineSavingKnownTargets(sep, net, "unused", DEV, sim)
    ons.save_sec = save_sec
    ons.fused_eval = fused
    if max_window_utts:
        ons.max_window_utts = max_window_utts
    ons.calc_online(mix.to(DEV), srcs.to(DEV), "case", 0)
    assert ons.used_fused == fused and ons.indx == 0
    assert len(ons.online_sisdr) == len(ons.reference_sisdr) == 1
    assert len(ons.online_sisdr_rows) == len(ons.reference_sisdr_rows) == 1
    return ons


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("name,N,save_sec,seed", sc.CASES)
def test_against_reference_run(net, oracle_full, name, N, save_sec, seed, mode):
    g = sc.load_case(name)
    mix, srcs = sc.case_inputs(g)
    ons = run(net, mix, srcs, save_sec, mode)
    pmix, ptgt, K, W, H, P = sc.pad_signals(mix, srcs, save_sec)
    ref = sc.stitched_of(g, mode)
    got, swap = sc.align_hop0(ons.stitched_signal.cpu().numpy(), ref, H, per_batch=(mode == "l1"))
    d = np.abs(got - ref).max()
    print(f"{name} {mode}: stitched max abs vs reference {d:.2e}, hop-0 exchange {swap.tolist()}")
    assert d <= WAVE_TOL
    assert not (mode == "none" and swap.any())
    sc.check_perms(g, mode, ons.window_perms.cpu().numpy(), ons.window_perms_target.cpu().numpy(), swap)
    # the scores: the bound of a WAVE_TOL error on the reference's own signals, plus the reference's rounding
    tgt_t = ptgt[:, :, P: P + K * H]
    _, perm, _ = sc.best_perm(sc.pairwise_neg_sisdr(torch.from_numpy(ref), tgt_t))
    bound_on = score_bound(sc.reorder(torch.from_numpy(ref), perm), tgt_t)
    full = oracle_full(name, pmix)
    _, perm, _ = sc.best_perm(sc.pairwise_neg_sisdr(full, ptgt))
    bound_ref = score_bound(sc.reorder(full, perm)[:, :, P: P + K * H], tgt_t)
    for key, bound, rows in (("online_sisdr", bound_on, ons.online_sisdr_rows[0]),
                             ("reference_sisdr", bound_ref, ons.reference_sisdr_rows[0])):
        f32, f64 = float(g[f"{mode}_{key}_f32"]), float(g[f"{mode}_{key}_f64"])
        tol = float(bound.mean()) + abs(f32 - f64)
        val = getattr(ons, key)[0]
        print(f"{name} {mode} {key}: {val:.6f} dB, reference {f64:.6f} dB, |diff| {abs(val - f64):.2e}, bound {tol:.2e}")
        assert abs(val - f64) <= tol
        assert tuple(rows.shape) == (2, 2) and abs(float(rows.mean()) - val) <= 1e-6
    # the online signal is left reordered against the targets (:143)
    _, perm, _ = sc.best_perm(sc.pairwise_neg_sisdr(ons.stitched_signal.cpu(), tgt_t))
    assert torch.equal(ons.online_signal.cpu(), sc.reorder(ons.stitched_signal.cpu(), perm))


@pytest.mark.parametrize("mode", sc.MODES)
def test_fused_equals_composed(net, mode):
    """The half-second case (K = 8): one sepvad_stream_eval call, three chunked forwards (max_window_utts = 6: three
    windows of two streams per call) and the composed loop give the same bits; a second call appends a second score."""
    name, N, save_sec, seed = sc.CASES[2]
    mix, srcs = sc.case_inputs(sc.load_case(name))
    fused = run(net, mix, srcs, save_sec, mode)
    chunked = run(net, mix, srcs, save_sec, mode, max_window_utts=6)
    comp = run(net, mix, srcs, save_sec, mode, fused=False)
    for other in (chunked, comp):
        assert torch.equal(fused.stitched_signal, other.stitched_signal)
        assert torch.equal(fused.window_perms, other.window_perms)
        assert torch.equal(fused.window_perms_target, other.window_perms_target)
        assert torch.equal(fused.online_signal, other.online_signal)
        assert fused.online_sisdr == other.online_sisdr and fused.reference_sisdr == other.reference_sisdr
    assert torch.equal(fused.window_pw_target, chunked.window_pw_target)
    fused.calc_online(mix.to(DEV), srcs.to(DEV), "case", 1)
    assert len(fused.online_sisdr) == len(fused.reference_sisdr) == 2 and fused.indx == 0
    assert fused.online_sisdr[1] == fused.online_sisdr[0] and fused.reference_sisdr[1] == fused.reference_sisdr[0]


def test_per_window_forward_path_matches(net):
    """one_forward = False: a forward per window and the composed loop (what a non-native model gets)."""
    import sep_tfanet_vad_amd as pkg
    name, N, save_sec, seed = sc.CASES[1]
    mix, srcs = sc.case_inputs(sc.load_case(name))
    fused = run(net, mix, srcs, save_sec, "l1")
    sep, sim = criteria("l1")
    ons = pkg.OnlineSavingKnownTargets(sep, net, "unused", DEV, sim)
    ons.one_forward = False
    ons.calc_online(mix.to(DEV), srcs.to(DEV), "case", 0)
    assert ons.used_fused is False
    assert torch.equal(ons.window_perms, fused.window_perms)
    assert float((ons.stitched_signal - fused.stitched_signal).abs().max()) <= 1e-5
    assert abs(ons.online_sisdr[0] - fused.online_sisdr[0]) <= 1e-4
