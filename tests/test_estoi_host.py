"""Host side of extended STOI (no GPU): the numpy restatement of the device path (tests/estoi_cases.py) against the
reference's own ``stoi(..., extended=True)`` (tests/golden/golden_estoi.npz, make_estoi_golden.py: mean and spread over
8 seeds of its random term), the refusals of sepvad_stoi_ex / sepvad_stoi_ex_scratch_bytes, and the Python layer.

The gate is classic STOI's: |d - d_ref| <= 1e-5. The reference defines no value where a
normalised row or column has zero norm (it normalises its own noise there): only those pairs, counted in the golden
from a float64 evaluation, are left out of the comparison, and they must be the 21 known ones of the 108 classic pairs
(20 all-zero estimates, one `other` pair with stretches of exact zeros)."""
import ctypes

import numpy as np
import pytest
import torch

import estoi_cases
import stoi_cases

E_ARG = -1
GATE = estoi_cases.GATE


@pytest.fixture(scope="module")
def restated():
    """(golden, sets, d [P], M [P]) of estoi_cases.restate on the rebuilt inputs, computed once."""
    g, sets = estoi_cases.load_sets()
    gs = np.load(stoi_cases.GOLDEN_FILE)
    d, M = np.zeros(len(g["pair_M"])), np.zeros(len(g["pair_M"]), np.int64)
    for s in sets:
        clean, est = estoi_cases.set_rows(s)
        for row, (p, _, _) in enumerate(s["pairs"]):
            d[p], M[p] = estoi_cases.restate(clean[row], est[row], s["fs"], gs[f"taps_{s['fs']}"], gs[f"bands_{s['fs']}"])
    return g, sets, d, M


def test_golden_holds_the_required_cases():
    g, sets = estoi_cases.load_sets()
    n_old = int(g["n_stoi_pairs"])
    assert n_old == 108 and len(sets) == 13 and int(g["seeds"]) == 8
    assert sum(len(s["pairs"]) for s in sets) == len(g["pair_M"]) == len(g["pair_estoi_mean"])
    # the long set: more than three workgroups' worth of segments, with a partial last chunk
    J = g["pair_M"][n_old:] - estoi_cases.SEG + 1
    assert len(J) >= 8 and np.all(J >= 3 * estoi_cases.CHUNK) and np.all(J % estoi_cases.CHUNK != 0)
    assert sets[-1]["mix"].size == 32000 and sets[-1]["fs"] == 8000
    assert 30 in g["pair_M"] and 29 in g["pair_M"]                     # J = 1 and the 1e-5 branch
    assert np.all(g["pair_estoi_restated"][g["pair_M"] < 30] == 1e-5)
    assert np.all(g["pair_estoi_mean"][g["pair_M"] < 30] == 1e-5)      # the reference returns before the branch


def test_restatement_reproduces_the_golden(restated):
    g, _, d, M = restated
    assert np.array_equal(M, g["pair_M"])
    diff = np.abs(d - g["pair_estoi_restated"])
    print(f"restatement vs stored restatement: max {diff.max():.2e}")
    assert diff.max() <= 1e-12  # the same numpy code; summation order inside numpy may differ between builds


def test_restatement_matches_the_reference(restated):
    g, sets, d, M = restated
    n_old = int(g["n_stoi_pairs"])
    deg, mean, spread = g["pair_degenerate"], g["pair_estoi_mean"], g["pair_estoi_spread"]
    compared = (M >= 30) & (deg == 0)
    left_out = (M >= 30) & ~compared
    kinds = {p: k for s in sets for p, _, k in s["pairs"]}
    # only degenerate pairs are left out; on the 108 classic pairs they are 20 `zeros` and one `other`
    assert np.all(deg[left_out] != 0)
    old_left = [kinds[p] for p in np.nonzero(left_out[:n_old])[0]]
    assert sorted(old_left) == ["other"] + ["zeros"] * 20
    assert compared[:n_old].sum() >= 70
    assert all(kinds[n_old + p] == "zeros" for p in np.nonzero(left_out[n_old:])[0])
    worst = np.abs(d - mean)[compared].max()
    print(f"restated device path vs reference mean over {compared.sum()} pairs: max {worst:.3e} "
          f"(stored {float(g['restated_vs_reference_max']):.3e}); seed spread <= {spread[compared].max():.2e}")
    assert spread[compared].max() < 1e-12
    assert worst <= GATE
    # where the reference has no value the rule gives one: an all-zero estimate scores exactly 0
    zeros = np.array([kinds[p] == "zeros" for p in range(len(M))])
    assert np.all(d[zeros & (M >= 30)] == 0.0) and np.all(d[M < 30] == 1e-5)
    assert np.all(np.isfinite(d)) and np.abs(d).max() <= 1.0 + 1e-9


def test_scratch_size_query():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    q, q0 = lib.sepvad_stoi_ex_scratch_bytes, lib.sepvad_stoi_scratch_bytes
    for R, N, fs in ((1, 32000, 16000), (16, 32000, 8000), (3, 8337, 10000), (128, 64000, 16000)):
        classic = q0(R, N, fs)
        assert q(R, N, fs, 1) == classic                       # the classic stage alone: the classic size
        assert q(R, N, fs, 3) == q(R, N, fs, 2) >= classic + R * 8
        assert q(R, N, fs, 3) % 256 == 0
    # one double per pair and chunk of 64 segments, sized for every frame kept: N = 32000 at 8 kHz has 311 frames
    assert q(4, 32000, 8000, 2) - q0(4, 32000, 8000) >= 4 * 8 * -(-(311 - 1 - 29) // estoi_cases.CHUNK)
    assert q(1, 32000, 16000, 0) == E_ARG and b"modes" in lib.sepvad_last_error()
    assert q(1, 32000, 16000, 4) == E_ARG and q(1, 32000, 16000, -1) == E_ARG
    assert q(1, 32000, 44100, 3) == E_ARG and b"fs_sig" in lib.sepvad_last_error()
    assert q(0, 32000, 16000, 3) == E_ARG and q(70000, 32000, 16000, 3) == E_ARG
    assert q(1, 256, 10000, 2) == E_ARG and q(1, 257, 10000, 2) > 0


def test_stoi_ex_entry_refuses_bad_arguments_without_gpu():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    f = lib.sepvad_stoi_ex
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before any device call
    big = 1 << 24
    need = lib.sepvad_stoi_ex_scratch_bytes(1, 1000, 16000, 3)
    assert 0 < need < big

    def call(X=one, x_ld=1000, Y=one, y_ld=1000, N=1000, R=1, fs=16000, scratch=one, nbytes=big, modes=3,
             out=one, out_ex=one):
        return f(X, x_ld, Y, y_ld, N, R, None, None, fs, scratch, nbytes, modes, out, out_ex, None, None)

    assert call(X=None) == E_ARG and call(Y=None) == E_ARG and call(scratch=None) == E_ARG
    assert call(x_ld=999) == E_ARG and call(y_ld=999) == E_ARG and call(N=0) == E_ARG
    assert call(fs=44100) == E_ARG and b"fs_sig" in lib.sepvad_last_error()
    for modes in (0, 4, -1, 7):
        assert call(modes=modes) == E_ARG and b"modes" in lib.sepvad_last_error()
    # an output pointer missing for a requested mode
    assert call(modes=1, out=None) == E_ARG and b"output pointer" in lib.sepvad_last_error()
    assert call(modes=2, out_ex=None) == E_ARG
    assert call(modes=3, out=None) == E_ARG and call(modes=3, out_ex=None) == E_ARG
    assert call(R=0) == E_ARG and call(R=70000) == E_ARG
    assert call(N=409, x_ld=409, y_ld=409) == E_ARG            # 256 samples at 10 kHz: no frame
    assert call(nbytes=need - 1) == E_ARG and b"scratch too small" in lib.sepvad_last_error()
    # the extended partials count: the classic size is too small for modes 2 and 3 (and an unrequested mode's missing
    # pointer is not what refuses the call)
    classic = lib.sepvad_stoi_scratch_bytes(1, 1000, 16000)
    assert classic < need
    assert call(modes=2, out=None, nbytes=classic) == E_ARG and b"scratch too small" in lib.sepvad_last_error()
    assert call(modes=1, out_ex=None, nbytes=classic - 1) == E_ARG and b"scratch too small" in lib.sepvad_last_error()
    assert call(scratch=ctypes.c_void_p(264)) == E_ARG and b"aligned" in lib.sepvad_last_error()


def test_python_layer():
    from sep_tfanet_vad_amd import metrics
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.estoi(x, x, 16000)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.Estoi()(x.reshape(1, 2, 4000), x.reshape(1, 2, 4000), None)
    with pytest.raises(RuntimeError, match="same length"):
        metrics.estoi(x, torch.zeros(2, 3000), 16000)
    with pytest.raises(NotImplementedError, match="estoi"):
        metrics.stoi(x, x, 16000, extended=True)
    assert metrics.estoi_met.__name__ == "estoi_metric" and metrics.estoi_met.fs_sig == 16000
    assert metrics.Estoi(fs_sig=8000).fs_sig == 8000
    assert (metrics.STOI_CLASSIC, metrics.STOI_EXTENDED) == (1, 2)


def test_mode_constants_match_the_header():
    import os
    import re
    from sep_tfanet_vad_amd import metrics
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sepvad.h")).read()
    c = dict(re.findall(r"^#define[ \t]+(SEPVAD_STOI_(?:CLASSIC|EXTENDED))[ \t]+(\d+)[ \t]*$", src, flags=re.M))
    assert (int(c["SEPVAD_STOI_CLASSIC"]), int(c["SEPVAD_STOI_EXTENDED"])) == (metrics.STOI_CLASSIC, metrics.STOI_EXTENDED)
