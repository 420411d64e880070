"""Golden vectors of the reference's extended STOI (run where the reference tree exists, never on the GPU box).

    python tests/golden/make_estoi_golden.py     writes golden_estoi.npz and prints the measurements of DESIGN.md

The reference's ``stoi(x, y, fs_sig, extended=True)`` (model/stoi_metric.py:207-301; row_col_normalize :177-193) adds
``EPS * np.random.standard_normal`` before each centring, so it is run under SEEDS seeds of ``np.random.seed`` and the
file stores, per pair, the mean and the spread (max - min) over the seeds. Cases: every pair of golden_stoi.npz in its
order, then the long sets of LONG_SETS (tests/estoi_cases.py). Also stored per pair: M; the number of zero-norm rows
and columns (exactly zero, or the rounding remainder of one: ``estoi_cases.row_col_normalize``) that the reference's
own float64 front end gives the noise-free formula (where it is not zero the reference normalises pure noise and its
value is a random draw); the noise-free float64 formula's value; and the value of the numpy restatement of the device
path (``estoi_cases.restate``). Recorded numbers only.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import estoi_cases  # noqa: E402
import stoi_cases  # noqa: E402
from make_stoi_golden import MIN_MARGIN_DB, frames_and_margin, load_reference  # noqa: E402

SEEDS = 8
LONG_SETS = [(8000, 32000, 38)]  # (fs_sig, samples, synth seed)


def f64_formula(ref, x, y, fs):
    """(noise-free extended STOI on the reference's own float64 front end, zero-norm rows + columns, M)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if fs != ref.FS:
        x, y = ref.resample_oct(x, ref.FS, fs), ref.resample_oct(y, ref.FS, fs)
    x, y = ref.remove_silent_frames(x, y, ref.DYN_RANGE, ref.N_FRAME, ref.N_FRAME // 2)
    xs = ref.stft(x, ref.N_FRAME, ref.NFFT, overlap=2).transpose()
    ys = ref.stft(y, ref.N_FRAME, ref.NFFT, overlap=2).transpose()
    M = xs.shape[-1]
    if M < ref.N:
        return 1e-5, 0, M
    tob = np.stack([np.sqrt(np.matmul(ref.OBM, np.square(np.abs(s)))) for s in (xs, ys)])
    d, deg = estoi_cases.estoi_tail(tob)
    return d, deg, M


def main():
    ref, _ = load_reference()
    warnings.simplefilter("ignore", RuntimeWarning)  # the 1e-5 branch warns; pure-noise rows divide by tiny norms
    gs, sets = stoi_cases.load_sets()
    n_old = len(gs["pair_M"])
    longs = []
    for fs, n, seed in LONG_SETS:
        srcs, mix = stoi_cases.set_inputs(n, seed)
        pairs = [(-1, c, kind) for c in (0, 1) for kind in estoi_cases.LONG_KINDS]
        sets.append(dict(fs=fs, srcs=srcs, mix=mix, noisy=None, pairs=pairs))
        longs.append((fs, n, seed, stoi_cases.inputs_sha(srcs, mix)))
    mean, spread, pM, deg, f64, rest, kinds = [], [], [], [], [], [], []
    for i, s in enumerate(sets):
        taps, bands = gs[f"taps_{s['fs']}"], gs[f"bands_{s['fs']}"]
        clean, est = stoi_cases.set_rows(s)
        for row, (p, c, kind) in enumerate(s["pairs"]):
            x, y = clean[row], est[row]
            M, margin = frames_and_margin(ref, x, s["fs"])
            if margin < MIN_MARGIN_DB:
                raise RuntimeError(f"set {i} speaker {c}: threshold margin {margin:.3g} dB is below {MIN_MARGIN_DB}")
            if p >= 0:
                assert M == int(gs["pair_M"][p])
            else:
                J = M - estoi_cases.SEG + 1
                if J < 3 * estoi_cases.CHUNK or J % estoi_cases.CHUNK == 0:
                    raise RuntimeError(f"long set {i}: J = {J} does not span three chunks with a partial last one")
            vals = []
            for seed in range(SEEDS):
                np.random.seed(1000 + seed)
                vals.append(float(ref.stoi(x, y, s["fs"], extended=True)))
            d64, ndeg, M64 = f64_formula(ref, x, y, s["fs"])
            dr, Mr = estoi_cases.restate(x, y, s["fs"], taps, bands)
            assert M64 == M == Mr, (M64, M, Mr)
            mean.append(float(np.mean(vals))); spread.append(float(np.max(vals) - np.min(vals)))
            pM.append(M); deg.append(ndeg); f64.append(d64); rest.append(dr); kinds.append(kind)
            print(f"set {i:2d} fs {s['fs']} N {len(x)} spk {c} {kind:8s} M {M:4d} zero-norm {ndeg:4d}  ref mean "
                  f"{mean[-1]: .9f} spread {spread[-1]:.2e}  f64 {d64: .9f}  restated {dr: .9f}")
    mean, spread, pM, deg, f64, rest = (np.array(v) for v in (mean, spread, pM, deg, f64, rest))
    ok = (pM >= estoi_cases.SEG) & (deg == 0)
    old = np.arange(len(pM)) < n_old
    left = (pM >= estoi_cases.SEG) & (deg != 0)
    worst = float(np.abs(rest - mean)[ok].max())
    print(f"pairs {len(pM)} ({n_old} of golden_stoi.npz), M >= 30: {(pM >= 30).sum()} ({(pM[old] >= 30).sum()}), "
          f"non-degenerate: {ok.sum()} ({(ok & old).sum()})")
    print(f"non-degenerate pairs: reference spread over {SEEDS} seeds <= {spread[ok].max():.2e}; noise-free float64 "
          f"formula vs reference mean <= {np.abs(f64 - mean)[ok].max():.2e}; restated device path vs reference mean "
          f"<= {worst:.3e}")
    print(f"degenerate pairs: {left.sum()} ({[k for k, m in zip(kinds, left) if m].count('zeros')} zeros); reference "
          f"spread {spread[left].min():.1e} .. {spread[left].max():.2e}, |mean| <= {np.abs(mean[left]).max():.2e}")
    out = dict(n_stoi_pairs=np.int32(n_old), seeds=np.int32(SEEDS),
               long_fs=np.array([t[0] for t in longs], np.int32), long_n=np.array([t[1] for t in longs], np.int32),
               long_seed=np.array([t[2] for t in longs], np.int32), long_sha=np.array([t[3] for t in longs]),
               pair_estoi_mean=mean, pair_estoi_spread=spread, pair_M=pM.astype(np.int32),
               pair_degenerate=deg.astype(np.int32), pair_estoi_f64=f64, pair_estoi_restated=rest,
               restated_vs_reference_max=np.float64(worst))
    np.savez_compressed(estoi_cases.GOLDEN_FILE, **out)
    print(len(pM), "pairs,", os.path.getsize(estoi_cases.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
