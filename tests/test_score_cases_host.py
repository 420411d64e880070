"""The regime grid of score_cases.py on the CPU: the cells are what they claim to be, and the emulation of the scoring
kernels' arithmetic (k_si_sdr / k_snr of csrc/metrics.hip, k_eval_moments / k_eval_finish of csrc/eval.hip) says why
the moments are taken on the rows less their first sample. No GPU: test_gpu_score_regimes.py holds the device to the
same truth.

Worst |emulation - float64 truth| in dB over a cell's numbers (SI-SDR, SNR, PairwiseNegSDR of the three kinds, both
zero_mean values), for the arithmetic as it shipped (raw moments, every term straight into a thread's running sum)
and as it is now; fp32 ref is the reference's own float32 arithmetic. Cells not listed stay below 2e-5 dB shipped and
below 2e-7 dB fixed (zero_mean=False cells near 78 dB: 1e-5 dB in both; they are not shifted):

    cell                        truth SI-SDR   shipped    fixed     fp32 ref
    N32000-dc100-nl0.001           57.9 dB     1.3e-4     1.4e-9    2.8e-4
    N32000-dc100-nl0.0001          71.4 dB     3.0e-3     5.5e-8    4.0e-2
    N32000-dc1000-nl0.01           38.1 dB     1.7e-4     1.1e-8    4.9e-4
    N32000-dc1000-nl0.001          57.8 dB     1.7e-2     1.3e-8    7.6e-2
    N32000-dc1000-nl0.0001         71.3 dB     3.7e-1     7.2e-8    5.5
    N2000000-dc10-nl0.0001         77.8 dB     1.5e-3     1.3e-6    1.9e-4
    N2000000-dc100-nl0.001         58.1 dB     1.5e-3     8.8e-9    4.3e-4
    N2000000-dc100-nl0.0001        77.8 dB     1.4e-1     8.8e-7    4.0e-2
    N2000000-dc1000-nl0.01         38.1 dB     1.5e-3     8.7e-7    5.7e-4
    N2000000-dc1000-nl0.001        58.1 dB     1.5e-1     8.7e-7    5.6e-2
    N2000000-dc1000-nl0.0001       77.3 dB     5.8        8.2e-7    5.3e-1

The shift alone leaves 1.8e-4 dB at N2000000-dc10-nl0.0001 in k_si_sdr: squares of shifted floats are integers
(0 or 1 mod 4) on a common grid, and a running sum of thousands of them rounds downwards more often than upwards.
Sums of 16 terms that then join the running sum (FLUSH of score_cases.py) bring it to 2e-7 dB.
"""
import numpy as np
import pytest

import score_cases as sc

TOL_DB = sc.TOL_DB


def _num(v):
    return v.numpy() if hasattr(v, "numpy") else np.asarray(v)


def _worst(a, b, keys):
    return max(float(np.abs(_num(a[k]) - _num(b[k])).max()) for k in keys)


def _keys(cell):
    zms = (True, False) if cell.zm_false else (True,)
    return [(k, zm) for k in ("si", "snr") for zm in zms] + [("pw", ty, zm) for ty in sc.SDR_TYPES for zm in zms]


def test_the_grid_covers_the_stated_regimes():
    names = [c.name for c in sc.CELLS]
    assert len(set(names)) == len(names)
    grid = [c for c in sc.CELLS if c.kind == "grid"]
    assert {(c.N, c.dc, c.nl) for c in grid} == {(N, dc, nl) for N in (32000, 2_000_000) for dc in (0, 10, 100, 1000)
                                                  for nl in (0.3, 1e-2, 1e-3, 1e-4)}
    assert all(c.B == (2 if c.N == 32000 else 1) and c.amp == 0.01 for c in grid)
    assert {(c.amp, c.nl) for c in sc.CELLS if c.kind == "scale"} == {(a, n) for a in (1e-4, 3000.0) for n in (0.3, 1e-3)}
    assert {c.amp for c in sc.CELLS if c.kind == "identical"} == {0.1, 3000.0}
    assert {c.zero for c in sc.CELLS if c.kind == "zero"} == {"est", "tgt", "both"}
    assert {c.N for c in sc.CELLS if c.kind == "tiny"} == {1, 2, 3, 5, 4097}
    est, tgt, mix = sc.make(sc.BY_NAME["N32000-dc100-nl0.001"])
    again = sc.make.__wrapped__(sc.BY_NAME["N32000-dc100-nl0.001"])
    assert est.dtype == tgt.dtype == mix.dtype == np.float32 and all(np.array_equal(a, b) for a, b in zip((est, tgt, mix), again))


@pytest.mark.parametrize("cell", sc.CELLS, ids=lambda c: c.name)
def test_cell(cell):
    tr, r32 = sc.truth(cell), sc.ref32(cell)
    keys = _keys(cell)
    # the truth is finite, and the matched zero-mean SI-SDR lies in the cell's band
    for k in keys + ["sheet", "means", "min_loss"]:
        assert bool(np.isfinite(_num(tr[k])).all()), k
    si = float(tr["si", True][0, 0])
    if cell.band():
        lo, hi = cell.band()
        assert lo <= si <= hi, (si, lo, hi)
    # zero_mean=False is scored up to 80 dB only
    if cell.zm_false:
        top = max(float(tr["si", False].max()), float(tr["snr", False].max()),
                  *(-float(tr["pw", ty, False].min()) for ty in sc.SDR_TYPES))
        assert top <= 80.0 + TOL_DB, top   # all-zero targets give exactly 80 in float64 up to its rounding
    # the permutation is decided by >= 1 dB; utterance 1 has its speakers swapped
    gap = _num(tr["gap"])
    if cell.perm_gap:
        assert bool((gap >= 1.0).all()), gap
        assert _num(tr["perm"]).tolist() == [[0, 1], [1, 0]][:cell.B]
    else:  # all-zero rows, one sample: an exact tie keeps the identity; two samples: collinear rows, < 1 dB apart
        assert bool((gap < 1.0).all())
        assert all(p == [0, 1] for p, g in zip(_num(tr["perm"]).tolist(), gap) if g == 0)
    # the float32 reference: within max(TOL_DB, 2 |ref32 - truth|) by construction; recorded for the table
    e32 = _worst(r32, tr, keys)
    assert e32 <= max(TOL_DB, 2 * e32)
    fixed, shipped = sc.emulate(cell, True), sc.emulate(cell, False)
    e_fix, e_ship = _worst(fixed, tr, keys), _worst(shipped, tr, keys)
    print(f"{cell.name:28s} {si:9.3f} dB   shipped {e_ship:8.1e}   fixed {e_fix:8.1e}   fp32 ref {e32:8.1e}")
    assert e_fix <= TOL_DB / 8, e_fix
    # the sheet's SI-SDR / SNR (eval.hip's sums) against the same pairs of k_si_sdr / k_snr: the two kernels add in
    # different orders, so the device agrees to rounding, not to the bit
    for b in range(cell.B):
        for s in range(2):
            assert abs(fixed["sheet_si"][b, s, s] - fixed["si", True][b, s]) <= 1e-5
            assert abs(fixed["sheet_snr"][b, s, s] - fixed["snr", True][b, s]) <= 1e-5


@pytest.mark.parametrize("name", ["N32000-dc100-nl0.0001", "N2000000-dc100-nl0.0001"])
def test_shipped_arithmetic_breaks_the_gate(name):
    """Why the moments are shifted: the raw-moment closed form misses TOL_DB where the DC is 100 standard deviations
    and the residual 1e-4 of one, at the production length already; k_si_sdr and eval.hip's PairwiseNegSDR both."""
    cell = sc.BY_NAME[name]
    tr, shipped = sc.truth(cell), sc.emulate(cell, False)
    e_si = _worst(shipped, tr, [("si", True)])
    e_pw = _worst(shipped, tr, [("pw", "sisdr", True)])
    print(f"{name}: shipped k_si_sdr {e_si:.2e} dB, shipped PairwiseNegSDR sisdr {e_pw:.2e} dB")
    assert e_si > TOL_DB and e_pw > TOL_DB
