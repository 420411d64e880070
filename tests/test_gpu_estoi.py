"""Extended STOI on the device (k_stoi_ex_corr / k_stoi_ex_finish in csrc/stoi.hip, sepvad_stoi_ex) vs the reference's own
``stoi(..., extended=True)`` (tests/golden/golden_estoi.npz: mean over 8 seeds of its random term) and vs the numpy
restatement of the device path (tests/estoi_cases.py).

Gate: classic STOI's |d - d_ref| <= 1e-5; the restatement is within 1.9e-8 of the reference, which
leaves the gate's margin to the device's FFT ordering, FMA contraction and reduction order. Pairs where the reference
defines no value (a zero-norm row or column: it normalises its own noise there) are compared with the restatement
only; M < 30 must give exactly 1e-5, an all-zero estimate exactly 0, and M must be exact everywhere.
Measured on the MI355X: device to reference 1.92e-8 over the 76 non-degenerate pairs, device to restatement 5.2e-11
over all 116 pairs."""
import numpy as np
import pytest
import torch

import estoi_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
GATE = estoi_cases.GATE
N_SETS = 13
LONG = 12  # N = 32000 at 8 kHz: J = 249 and 213 segments, four workgroups per pair with a partial last chunk


@pytest.fixture(scope="module")
def cases():
    g, sets = estoi_cases.load_sets()
    assert len(sets) == N_SETS
    return g, sets


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(s):
    clean, est = estoi_cases.set_rows(s)
    return _dev(clean), _dev(est)


@pytest.fixture(scope="module")
def device_values(cases):
    """estoi_pairs of every set, one call per set: (d [P], M [P]) in the golden's pair order."""
    from sep_tfanet_vad_amd import metrics
    g, sets = cases
    d, M = np.zeros(len(g["pair_M"])), np.zeros(len(g["pair_M"]), np.int64)
    for s in sets:
        C, E = _rows(s)
        dd, ff = metrics.estoi_pairs(C, E, s["fs"])
        assert dd.dtype == torch.float64 and ff.dtype == torch.int32 and dd.device.type == "cuda"
        idx = [p for p, _, _ in s["pairs"]]
        d[idx], M[idx] = dd.cpu().numpy(), ff.cpu().numpy()
    return d, M


def test_estoi_matches_reference_and_restatement(cases, device_values):
    g, sets = cases
    d, M = device_values
    n_old = int(g["n_stoi_pairs"])
    kinds = {p: (i, c, k) for i, s in enumerate(sets) for p, c, k in s["pairs"]}
    for p in range(len(M)):
        i, c, k = kinds[p]
        print(f"set {i:2d} spk {c} {k:8s} M {M[p]:4d} (ref {int(g['pair_M'][p])}) d {d[p]: .9f} ref {g['pair_estoi_mean'][p]: .9f} "
              f"restated {g['pair_estoi_restated'][p]: .9f} zero-norm {int(g['pair_degenerate'][p])}")
    assert np.array_equal(M, g["pair_M"])
    compared = (M >= 30) & (g["pair_degenerate"] == 0)
    to_ref = np.abs(d - g["pair_estoi_mean"])[compared].max()
    to_rest = np.abs(d - g["pair_estoi_restated"]).max()
    print(f"device vs reference mean over {compared.sum()} non-degenerate pairs: max {to_ref:.3e}; device vs "
          f"restatement over all {len(M)} pairs: max {to_rest:.3e}")
    assert compared[:n_old].sum() >= 70
    assert to_ref <= GATE
    assert to_rest <= GATE
    selfs = np.array([kinds[p][2] == "self" for p in range(len(M))]) & (M >= 30)
    assert np.abs(d[selfs] - 1.0).max() <= GATE


def test_estoi_degenerate_and_short_pairs(cases, device_values):
    g, sets = cases
    d, M = device_values
    kinds = {p: k for s in sets for p, _, k in s["pairs"]}
    zeros = np.array([kinds[p] == "zeros" for p in range(len(M))])
    assert (M < 30).sum() >= 5 and (zeros & (M >= 30)).sum() >= 20
    assert np.all(d[M < 30] == 1e-5)
    assert np.all(d[zeros & (M >= 30)] == 0.0)
    assert np.all(np.isfinite(d))
    # the boundary: M = 30 is one segment (J = 1) and is scored, M = 29 is not
    at30 = (M == 30) & ~zeros
    assert at30.sum() >= 2 and (M == 29).sum() >= 2
    assert np.all(d[at30] != 1e-5) and np.abs(d[at30] - g["pair_estoi_restated"][at30]).max() <= GATE


@pytest.mark.parametrize("i", [3, 7, 9, LONG])
def test_both_from_one_call_have_the_separate_calls_bits(cases, i):
    from sep_tfanet_vad_amd import metrics
    _, sets = cases
    s = sets[i]
    C, E = _rows(s)
    d0, f0 = metrics.stoi_pairs(C, E, s["fs"])
    e0, g0 = metrics.estoi_pairs(C, E, s["fs"])
    d1, e1, f1 = metrics.stoi_both_pairs(C, E, s["fs"])
    assert torch.equal(d0, d1) and torch.equal(e0, e1) and torch.equal(f0, f1) and torch.equal(g0, f1)
    again = metrics.stoi_both_pairs(C, E, s["fs"])
    assert all(torch.equal(a, b) for a, b in zip(again, (d1, e1, f1)))
    assert torch.equal(metrics.estoi_pairs(C, E, s["fs"])[0], e0)  # a second run


@pytest.mark.parametrize("i", [2, LONG])
def test_estoi_batch_invariant(cases, i):
    """Pair r alone gives the bits it gives among R pairs (other pairs around it, other grid, other block order):
    N = 23457 at 16 kHz with R = 16, and the long set, whose pairs span four workgroups with a partial last chunk."""
    from sep_tfanet_vad_amd import metrics
    _, sets = cases
    s = sets[i]
    clean, est = estoi_cases.set_rows(s)
    rows = [(k * 5) % len(clean) for k in range(16)] if i == 2 else list(range(len(clean)))
    C, E = _dev(clean[rows]), _dev(est[rows])
    dR, eR, fR = metrics.stoi_both_pairs(C, E, s["fs"])
    for r in range(len(rows)):
        e1, f1 = metrics.estoi_pairs(C[r:r + 1], E[r:r + 1], s["fs"])
        assert torch.equal(e1[0], eR[r]) and torch.equal(f1[0], fR[r])


def test_estoi_index_arrays_equal_gathered_rows(cases):
    from sep_tfanet_vad_amd import metrics
    _, sets = cases
    s = sets[7]  # 8 kHz, odd length
    X = _dev(s["srcs"])
    Y = _dev(np.stack([s["noisy"], s["mix"], s["srcs"][0], s["srcs"][1]]))
    xidx = [0, 1, 0, 1, 0, 1, 1]
    yidx = [0, 1, 1, 3, 3, 2, 0]
    d, f = metrics.estoi_pairs(X, Y, s["fs"], xidx, yidx)
    dg, fg = metrics.estoi_pairs(X[xidx].contiguous(), Y[yidx].contiguous(), s["fs"])
    assert torch.equal(d, dg) and torch.equal(f, fg)
    # device index tensors are taken as they are
    dt, ft = metrics.estoi_pairs(X, Y, s["fs"], torch.tensor(xidx, device=DEV), torch.tensor(yidx, device=DEV))
    assert torch.equal(d, dt) and torch.equal(f, ft)


def test_estoi_on_a_side_stream(cases):
    from sep_tfanet_vad_amd import metrics
    _, sets = cases
    s = sets[9]  # 10 kHz: the inputs are read in place
    C, E = _rows(s)
    d0, f0 = metrics.estoi_pairs(C, E, s["fs"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d1, f1 = metrics.estoi_pairs(C, E, s["fs"])
    side.synchronize()
    assert torch.equal(d0, d1) and torch.equal(f0, f1)


def test_estoi_python_surface_shapes(cases):
    """estoi(x, y, fs) keeps the leading dimensions ([2, 2, N] -> [2, 2]) and the reference's argument order; Estoi is
    the mean over the batch with (preds, targets) swapped into it."""
    from sep_tfanet_vad_amd import metrics
    g, sets = cases
    s = sets[1]
    x = np.stack([s["srcs"], s["srcs"]])                               # clean [2, 2, N]
    y = np.stack([np.stack([s["mix"], s["mix"]]), s["srcs"][::-1]])    # mixture, other
    d = metrics.estoi(_dev(x), _dev(y), s["fs"])
    assert d.shape == (2, 2) and d.dtype == torch.float64
    want = {(c, k): float(g["pair_estoi_restated"][p]) for p, c, k in s["pairs"]}
    ref = np.array([[want[0, "mixture"], want[1, "mixture"]], [want[0, "other"], want[1, "other"]]])
    assert np.abs(d.cpu().numpy() - ref).max() <= GATE
    v = metrics.Estoi(fs_sig=s["fs"])(_dev(y), _dev(x), None)
    assert v.dim() == 0 and v.dtype == torch.float64 and torch.equal(v, d.mean())


def _score_case(s):
    srcs, mix = s["srcs"], s["mix"]
    a, b = srcs[0], srcs[1]
    sep = np.stack([np.stack([0.8 * a + 0.2 * b, 0.8 * b + 0.2 * a]),      # estimates in target order
                    np.stack([0.8 * b + 0.1 * a, 0.9 * a + 0.2 * b]),      # exchanged
                    np.stack([mix, b])]).astype(np.float32)
    tgt = np.stack([srcs, srcs, srcs])
    return _dev(sep), _dev(tgt), _dev(np.stack([mix, mix, 0.5 * mix]).astype(np.float32))


def test_score_batch_without_stoi_fs_is_unchanged(cases):
    from sep_tfanet_vad_amd import evaluate
    _, sets = cases
    sep, tgt, mix = _score_case(sets[1])
    a = evaluate.score_batch(sep, tgt, mix)
    b = evaluate.score_batch(sep, tgt, mix, stoi_fs=None)
    assert set(a) == set(b) and not {"stoi", "estoi", "initial_stoi", "initial_estoi"} & set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_score_batch_stoi_columns(cases):
    """The four columns equal, bitwise, stoi_pairs / estoi_pairs on explicitly reordered rows; every other key keeps
    its bits; without a mixture only stoi and estoi are added."""
    from sep_tfanet_vad_amd import evaluate, metrics
    _, sets = cases
    s = sets[1]  # N = 12000 at 16 kHz
    sep, tgt, mix = _score_case(s)
    B, _, N = sep.shape
    base = evaluate.score_batch(sep, tgt, mix)
    r = evaluate.score_batch(sep, tgt, mix, stoi_fs=s["fs"])
    assert set(r) == set(base) | {"stoi", "estoi", "initial_stoi", "initial_estoi"}
    for k in base:
        assert torch.equal(base[k], r[k]), k
    perm = r["perm"].cpu()
    assert perm[0].tolist() == [0, 1] and perm[1].tolist() == [1, 0]
    reordered = torch.stack([sep[b][r["perm"][b]] for b in range(B)]).reshape(2 * B, N).contiguous()
    T = tgt.reshape(2 * B, N).contiguous()
    mixrows = mix.unsqueeze(1).expand(B, 2, N).reshape(2 * B, N).contiguous()
    for key, fn, Y in (("stoi", metrics.stoi_pairs, reordered), ("estoi", metrics.estoi_pairs, reordered),
                       ("initial_stoi", metrics.stoi_pairs, mixrows), ("initial_estoi", metrics.estoi_pairs, mixrows)):
        want = fn(T, Y, s["fs"])[0].reshape(B, 2)
        assert r[key].shape == (B, 2) and r[key].dtype == torch.float64 and r[key].device.type == "cuda"
        assert torch.equal(r[key], want), key
    nomix = evaluate.score_batch(sep, tgt, stoi_fs=s["fs"])
    assert "initial_stoi" not in nomix and "initial_estoi" not in nomix
    assert torch.equal(nomix["stoi"], r["stoi"]) and torch.equal(nomix["estoi"], r["estoi"])
