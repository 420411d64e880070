"""On-device STOI and SNR (csrc/stoi.hip, k_snr in csrc/metrics.hip) vs outputs of the reference itself
(model/stoi_metric.py:207-301 stoi, model/metric.py:104-143 signal_noise_ratio; tests/golden/golden_stoi.npz,
written by tests/golden/make_stoi_golden.py).

The STOI gate is |d - d_ref| <= 1e-5. A CPU emulation with the resampler, framing, FFT and band sums in float32 and
the segment statistics in double stays within 1.1e-7 of the reference; the arithmetic chosen here (float32 only for
the store of the resampled signal, double elsewhere; make_stoi_golden.py --emulate restates it in numpy) stays
within 1.6e-8 over the 108 golden pairs. The gate leaves two to three orders of magnitude for the device's FFT
ordering, FMA contraction and double transcendentals, and is far below the third decimal STOI is reported to.
Pairs on the 1e-5 branch (M < 30) and all-zero estimates must be exact; every golden pair has a keep / drop
threshold margin >= 0.1 dB, so M must be exact too."""
import itertools

import numpy as np
import pytest
import torch

import stoi_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
GATE = 1e-5
N_SETS = 12
TOL_DB = 1e-3


@pytest.fixture(scope="module")
def cases():
    g, sets = stoi_cases.load_sets()
    assert len(sets) == N_SETS
    return g, sets


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _set_pairs(s):
    from sep_tfanet_vad_amd import metrics
    clean, est = stoi_cases.set_rows(s)
    d, frames = metrics.stoi_pairs(_dev(clean), _dev(est), s["fs"])
    return d, frames


@pytest.mark.parametrize("i", range(N_SETS))
def test_stoi_matches_reference(cases, i):
    g, sets = cases
    s = sets[i]
    d, frames = _set_pairs(s)
    assert d.dtype == torch.float64 and frames.dtype == torch.int32 and d.device.type == "cuda"
    d, frames = d.cpu().numpy(), frames.cpu().numpy()
    for row, (p, c, kind) in enumerate(s["pairs"]):
        ref, M = float(g["pair_stoi"][p]), int(g["pair_M"][p])
        print(f"set {i} fs {s['fs']} N {s['mix'].size} spk {c} {kind:8s} M {frames[row]} (ref {M}) "
              f"d {d[row]:.9f} ref {ref:.9f} diff {abs(d[row] - ref):.2e}")
    for row, (p, c, kind) in enumerate(s["pairs"]):
        ref, M = float(g["pair_stoi"][p]), int(g["pair_M"][p])
        assert frames[row] == M
        if M < 30:
            assert ref == 1e-5 and d[row] == 1e-5
        elif kind == "zeros":
            assert ref == 0.0 and d[row] == 0.0
        else:
            assert abs(d[row] - ref) <= GATE
            if kind == "self":
                assert abs(d[row] - 1.0) <= GATE


def test_stoi_python_surface_shapes(cases):
    """stoi(x, y, fs) keeps the leading dimensions ([2, 2, N] -> [2, 2]) and the reference's argument order."""
    from sep_tfanet_vad_amd import metrics
    g, sets = cases
    s = sets[1]
    x = np.stack([s["srcs"], s["srcs"]])                               # clean [2, 2, N]
    y = np.stack([np.stack([s["mix"], s["mix"]]), s["srcs"][::-1]])    # mixture, other
    d = metrics.stoi(_dev(x), _dev(y), s["fs"])
    assert d.shape == (2, 2) and d.dtype == torch.float64
    want = {(c, k): float(g["pair_stoi"][p]) for p, c, k in s["pairs"]}
    ref = np.array([[want[0, "mixture"], want[1, "mixture"]], [want[0, "other"], want[1, "other"]]])
    assert np.abs(d.cpu().numpy() - ref).max() <= GATE


def test_stoi_bitwise_deterministic(cases):
    _, sets = cases
    a, fa = _set_pairs(sets[3])
    b, fb = _set_pairs(sets[3])
    assert torch.equal(a, b) and torch.equal(fa, fb)


def test_stoi_batch_invariant(cases):
    """Pair r alone gives the bits it gives inside R = 16 (with other pairs around it, in another block order)."""
    from sep_tfanet_vad_amd import metrics
    _, sets = cases
    s = sets[2]  # N = 23457 at 16 kHz
    clean, est = stoi_cases.set_rows(s)
    rows = [(k * 5) % len(clean) for k in range(16)]
    C, E = _dev(clean[rows]), _dev(est[rows])
    d16, f16 = metrics.stoi_pairs(C, E, s["fs"])
    for r in range(16):
        d1, f1 = metrics.stoi_pairs(C[r:r + 1], E[r:r + 1], s["fs"])
        assert torch.equal(d1[0], d16[r]) and torch.equal(f1[0], f16[r])


def test_stoi_index_arrays_equal_gathered_rows(cases):
    from sep_tfanet_vad_amd import metrics
    _, sets = cases
    s = sets[7]  # 8 kHz, odd length
    X = _dev(s["srcs"])
    Y = _dev(np.stack([s["noisy"], s["mix"], s["srcs"][0], s["srcs"][1]]))
    xidx = [0, 1, 0, 1, 0, 1, 1]
    yidx = [0, 1, 1, 3, 3, 2, 0]
    d, f = metrics.stoi_pairs(X, Y, s["fs"], xidx, yidx)
    dg, fg = metrics.stoi_pairs(X[xidx].contiguous(), Y[yidx].contiguous(), s["fs"])
    assert torch.equal(d, dg) and torch.equal(f, fg)


def test_stoi_on_a_side_stream(cases):
    _, sets = cases
    s = sets[9]  # 10 kHz: the inputs are read in place
    d0, f0 = _set_pairs(s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d1, f1 = _set_pairs(s)
    side.synchronize()
    assert torch.equal(d0, d1) and torch.equal(f0, f1)


def test_stoi_module_on_model_outputs(state_dicts):
    """Stoi()(preds, targets, _) on the separated outputs of a B = 3 forward at 16 kHz == the mean of the per-pair
    stoi(target, pred, 16000) values (model/metric.py:207-223)."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import metrics, synth
    from conftest import config_of
    x, srcs = synth.make_batch(3, 16000, 321)
    net = pkg.SeparationModel(**config_of("with_vad"))
    net.load_state_dict(state_dicts["with_vad"], strict=True)
    net = net.eval().to(DEV)
    with torch.no_grad():
        sep, _, _ = net(torch.from_numpy(x).to(DEV))
    tgt = torch.from_numpy(srcs).to(DEV)
    v = metrics.stoi_met(sep, tgt, None)
    assert v.dim() == 0 and v.dtype == torch.float64 and v.device.type == "cuda"
    per = [metrics.stoi(tgt[b, s], sep[b, s], 16000) for b in range(3) for s in range(2)]
    assert all(p.dim() == 0 for p in per)
    assert abs(v.item() - float(np.mean([p.item() for p in per]))) <= 1e-15
    assert -0.1 < v.item() <= 1.0 + 1e-9
    assert torch.equal(metrics.Stoi(fs_sig=16000)(sep, tgt, None), v)


def _snr_ref(preds, target, zero_mean=True):
    """signal_noise_ratio (model/metric.py:131-143) restated in float64."""
    preds, target = preds.double(), target.double()
    eps = torch.finfo(torch.float32).eps
    if zero_mean:
        target = target - target.mean(-1, keepdim=True)
        preds = preds - preds.mean(-1, keepdim=True)
    noise = target - preds
    return 10 * torch.log10(((target ** 2).sum(-1) + eps) / ((noise ** 2).sum(-1) + eps))


def test_snr_matches_reference_golden(cases):
    from sep_tfanet_vad_amd import metrics
    g, sets = cases
    s = sets[int(g["snr_set"])]
    preds = np.stack([s["noisy"] + g["snr_offset"], s["mix"], s["srcs"][1]]).astype(np.float32)
    tgt = np.stack([s["srcs"][0], s["srcs"][1], s["srcs"][0]])
    for zm in (0, 1):
        v = metrics.signal_noise_ratio(_dev(preds), _dev(tgt), zero_mean=bool(zm))
        assert v.shape == (3,) and v.dtype == torch.float32
        print(f"zero_mean {zm}: device {v.cpu().numpy()} reference {g[f'snr_zm{zm}']}")
        assert np.abs(v.cpu().numpy() - g[f"snr_zm{zm}"]).max() <= 1e-4  # fp32 reference vs moments in double
        again = metrics.signal_noise_ratio(_dev(preds), _dev(tgt), zero_mean=bool(zm))
        assert torch.equal(v, again)
    # the docstring's example (model/metric.py:122-125, torchmetrics' value with zero_mean False)
    e = metrics.signal_noise_ratio(torch.tensor([2.5, 0.0, 2.0, 8.0], device=DEV),
                                   torch.tensor([3.0, -0.5, 2.0, 7.0], device=DEV), zero_mean=False).item()
    assert abs(e - 16.1805) < 1e-3


def test_pit_snr_on_model_outputs(state_dicts):
    """pit_snr of the separated outputs of a B = 6 forward vs torchmetrics' permutation_invariant_training
    (eval 'max') restated on the float64 SNR."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import metrics, synth
    from conftest import config_of
    x, srcs = synth.make_batch(6, 16000, 321)
    net = pkg.SeparationModel(**config_of("with_vad"))
    net.load_state_dict(state_dicts["with_vad"], strict=True)
    net = net.eval().to(DEV)
    with torch.no_grad():
        sep, _, _ = net(torch.from_numpy(x).to(DEV))
    tgt = torch.from_numpy(srcs)
    preds = sep.cpu()
    B, S, _ = preds.shape
    mtx = torch.empty(B, S, S, dtype=torch.float64)
    for t in range(S):
        for p in range(S):
            mtx[:, t, p] = _snr_ref(preds[:, p], tgt[:, t])
    perms = list(itertools.permutations(range(S)))
    vals = torch.stack([mtx[:, torch.arange(S), torch.tensor(pm)].mean(-1) for pm in perms], -1)
    rbest, ridx = vals.max(-1)
    best, perm = metrics.permutation_invariant_snr(sep, tgt.to(DEV))
    assert (best.cpu().double() - rbest).abs().max().item() <= TOL_DB
    gap = (vals[:, 0] - vals[:, 1]).abs() > 0.05  # permutations are only comparable away from ties
    assert torch.equal(perm.cpu()[gap], torch.tensor(perms)[ridx][gap])
    v = metrics.pit_snr(sep, tgt.to(DEV))
    assert v.dim() == 0 and abs(v.item() - rbest.mean().item()) <= TOL_DB
