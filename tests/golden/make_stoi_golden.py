"""Golden vectors of the reference's STOI and SNR (run where the reference tree exists, never on the GPU box).

    python tests/golden/make_stoi_golden.py            writes golden_stoi.npz
    python tests/golden/make_stoi_golden.py --emulate  CPU restatement of the device arithmetic vs the reference
    python tests/golden/make_stoi_golden.py --time     seconds per call of the reference's numpy stoi on this CPU

Imports the reference's ``model/stoi_metric.py`` (``stoi``, :207-301) and ``model/metric.py``
(``signal_noise_ratio``, :104-143) through ``make_golden.import_reference`` and the ``torchmetrics`` stand-in of
make_metric_golden.py. Inputs are rebuilt from ``tests/stoi_cases.py``; the file holds the set parameters, the
noisy estimates, and the reference's outputs: ``stoi`` per pair (float64), M = spectra left after silence removal,
the keep / drop threshold margin min_i |max - 40 - e_i| in dB, SNR for both ``zero_mean`` values, and per rate the
reference's resampling taps h / sum(h) and the OBM band edges [first bin, one past the last].
A case whose threshold margin is below 0.1 dB is refused: the keep / drop decision must be out of rounding's reach.
"""
from __future__ import annotations

import os
import sys
import time
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import stoi_cases  # noqa: E402

MIN_MARGIN_DB = 0.1
RATES = (16000, 8000, 10000)
SEED = 5


def load_reference():
    import_reference()

    class _PitStandIn:  # metric.py:255-258 instantiate PIT(...) at import; never called here
        def __init__(self, *args, **kwargs):
            pass
    sys.modules.setdefault("torchmetrics", types.SimpleNamespace(PIT=_PitStandIn, PermutationInvariantTraining=_PitStandIn))
    import model.metric as ref_metric
    import model.stoi_metric as ref_stoi
    return ref_stoi, ref_metric


def frames_and_margin(ref, x, fs):
    """M and the threshold margin of clean signal x, with the reference's own functions (stoi_metric.py:238-248)."""
    if fs != ref.FS:
        x = ref.resample_oct(x, ref.FS, fs)
    w = np.hanning(ref.N_FRAME + 2)[1:-1]
    fr = np.array([w * x[i:i + ref.N_FRAME] for i in range(0, len(x) - ref.N_FRAME, ref.N_FRAME // 2)])
    e = 20 * np.log10(np.linalg.norm(fr, axis=1) + ref.EPS)
    margin = float(np.abs(np.max(e) - ref.DYN_RANGE - e).min())
    xs, _ = ref.remove_silent_frames(x, x, ref.DYN_RANGE, ref.N_FRAME, ref.N_FRAME // 2)
    M = ref.stft(xs, ref.N_FRAME, ref.NFFT, overlap=2).shape[0]
    return M, margin


def find_length(ref, want_M, fs=16000, start=8000, stop=16000):
    """The first N (source 0 of seed SEED) that leaves exactly want_M spectra with a safe threshold margin."""
    for n in range(start, stop, 16):
        srcs, _ = stoi_cases.set_inputs(n, SEED)
        M, margin = frames_and_margin(ref, srcs[0], fs)
        if M == want_M and margin >= MIN_MARGIN_DB:
            return n
    raise RuntimeError(f"no length with M = {want_M}")


def set_table(ref):
    """(fs, n, seed, zero_at, zero_len)."""
    t = [(16000, n, SEED, 0, 0) for n in (9000, 12000, 23457, 32000)]
    t += [(16000, find_length(ref, 30), SEED, 0, 0), (16000, find_length(ref, 29), SEED, 0, 0)]
    t += [(8000, 6000, SEED + 1, 0, 0), (8000, 7001, SEED + 2, 0, 0)]
    t += [(10000, 7000, SEED + 8, 0, 0), (10000, 8337, SEED + 4, 0, 0)]
    t += [(16000, 12000, SEED + 5, 6000, 8000),   # 0.5 s of exact zeros in the middle
          (16000, 10000, SEED + 6, 0, 4000)]      # leading zeros
    return t


def ref_design(ref, fs):
    if fs == ref.FS:
        taps = np.zeros(0)
    else:
        g = np.gcd(ref.FS, fs)
        h = ref._resample_window_oct(ref.FS // g, fs // g)
        taps = h / np.sum(h)
    bands = np.array([[np.nonzero(row)[0][0], np.nonzero(row)[0][-1] + 1] for row in ref.OBM], np.int32)
    assert all(ref.OBM[b, lo:hi].all() and ref.OBM[b].sum() == hi - lo for b, (lo, hi) in enumerate(bands))
    return taps, bands


def emulate(x, y, fs, taps, bands):
    """The device path's arithmetic restated in numpy (csrc/stoi.hip): polyphase sum in double stored as float32,
    everything after it in double, spectrum m rebuilt from kept frames m-1, m, m+1. Returns (d, M)."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    if len(taps):
        g = np.gcd(10000, fs)
        up, down = 10000 // g, fs // g
        half = (len(taps) - 1) // 2
        L = -(-len(x) * up // down)

        def rs(v):
            vu = np.zeros(len(v) * up)
            vu[::up] = v
            full = np.convolve(vu, up * taps)
            return full[half + down * np.arange(L)].astype(np.float32).astype(np.float64)
        x, y = rs(x), rs(y)
    else:
        x, y = x.astype(np.float64), y.astype(np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(256) + 1) / 257)
    L = len(x)
    nF = -(-(L - 256) // 128) if L > 256 else 0
    e = np.array([np.sum((w * x[i * 128:i * 128 + 256]) ** 2) for i in range(nF)])
    db = 20 * np.log10(np.sqrt(e) + np.finfo(float).eps)
    kept = np.nonzero((db.max() - 40 - db) < 0)[0]
    M = len(kept) - 1
    if M < 30:
        return 1e-5, M
    tob = np.zeros((2, 15, M))
    for s, v in enumerate((x, y)):
        for m in range(M):
            c = np.zeros(256)
            for h in (0, 1):
                c[h * 128:(h + 1) * 128] = w[:128] * v[kept[m + h] * 128:kept[m + h] * 128 + 128]
                if m + h >= 1:
                    c[h * 128:(h + 1) * 128] += w[128:] * v[kept[m + h - 1] * 128 + 128:kept[m + h - 1] * 128 + 256]
            p = np.abs(np.fft.rfft(c * w, 512)) ** 2
            tob[s, :, m] = [np.sqrt(p[lo:hi].sum()) for lo, hi in bands]
    eps = np.finfo(float).eps
    J = M - 29
    acc = 0.0
    for b in range(15):
        for j in range(J):
            xs, ys = tob[0, b, j:j + 30], tob[1, b, j:j + 30]
            c = np.sqrt(np.sum(xs * xs)) / (np.sqrt(np.sum(ys * ys)) + eps)
            ys = np.minimum(ys * c, xs * (1 + 10 ** (15 / 20)))
            u, v = xs - xs.mean(), ys - ys.mean()
            acc += np.sum(u * v) / ((np.sqrt(np.sum(u * u)) + eps) * (np.sqrt(np.sum(v * v)) + eps))
    return acc / (J * 15), M


def main():
    ref, ref_metric = load_reference()
    warnings.simplefilter("ignore", RuntimeWarning)  # the reference warns on its 1e-5 branch
    table = set_table(ref)
    out = dict(set_fs=np.array([t[0] for t in table], np.int32), set_n=np.array([t[1] for t in table], np.int32),
               set_seed=np.array([t[2] for t in table], np.int32), set_zero_at=np.array([t[3] for t in table], np.int32),
               set_zero_len=np.array([t[4] for t in table], np.int32))
    rng = np.random.Generator(np.random.PCG64(20240))
    shas, pset, pclean, pest, pstoi, pM, pmargin = [], [], [], [], [], [], []
    designs = {fs: ref_design(ref, fs) for fs in RATES}
    worst = 0.0
    do_emulate = "--emulate" in sys.argv
    for i, (fs, n, seed, zat, zlen) in enumerate(table):
        srcs, mix = stoi_cases.set_inputs(n, seed, zat, zlen)
        shas.append(stoi_cases.inputs_sha(srcs, mix))
        t = srcs[0]
        noisy = (0.8 * t + 0.05 * np.abs(t).max() * rng.standard_normal(t.shape)).astype(np.float32)
        out[f"noisy_{i}"] = noisy
        for c in (0, 1):
            M, margin = frames_and_margin(ref, srcs[c], fs)
            if margin < MIN_MARGIN_DB:
                raise RuntimeError(f"set {i} speaker {c}: threshold margin {margin:.3g} dB is below {MIN_MARGIN_DB}")
            for k, kind in enumerate(stoi_cases.EST_KINDS):
                if kind == "noisy" and c != 0:
                    continue
                est = stoi_cases.estimate(kind, c, srcs, mix, noisy)
                d = float(ref.stoi(srcs[c], est, fs))
                pset.append(i); pclean.append(c); pest.append(k); pstoi.append(d); pM.append(M); pmargin.append(margin)
                line = f"set {i} fs {fs} N {len(t)} spk {c} {kind:8s} M {M:4d} margin {margin:7.3f} dB  stoi {d:.9f}"
                if do_emulate:
                    de, Me = emulate(srcs[c], est, fs, *designs[fs])
                    assert Me == M, (Me, M)
                    worst = max(worst, abs(de - d))
                    line += f"  emulated {de:.9f} (diff {abs(de - d):.2e})"
                print(line)
    if do_emulate:
        print(f"emulation of the device arithmetic vs the reference: max |d - d_ref| = {worst:.3e} over {len(pstoi)} pairs")
        return
    out.update(set_sha=np.array(shas), pair_set=np.array(pset, np.int32), pair_clean=np.array(pclean, np.int32),
               pair_est=np.array(pest, np.int32), pair_stoi=np.array(pstoi, np.float64), pair_M=np.array(pM, np.int32),
               pair_margin=np.array(pmargin, np.float64))
    for fs in RATES:
        out[f"taps_{fs}"], out[f"bands_{fs}"] = designs[fs]
    # signal_noise_ratio (metric.py:104-143) on the rows of set 1: preds [noisy 0, mixture, other] vs targets [0, 1, 0]
    srcs, mix = stoi_cases.set_inputs(*table[1][1:])
    preds = np.stack([out["noisy_1"] + np.float32(0.01), mix, srcs[1]])
    tgt = np.stack([srcs[0], srcs[1], srcs[0]])
    out.update(snr_set=np.int32(1), snr_offset=np.float32(0.01))
    for zm in (True, False):
        out[f"snr_zm{int(zm)}"] = ref_metric.signal_noise_ratio(torch.from_numpy(preds), torch.from_numpy(tgt), zm).numpy()
    fn = stoi_cases.GOLDEN_FILE
    np.savez_compressed(fn, **out)
    print({k: out[k] for k in ("set_n", "snr_zm0", "snr_zm1")}, len(pstoi), "pairs,", os.path.getsize(fn), "bytes")


def time_reference():
    ref, _ = load_reference()
    for fs, n in ((8000, 32000), (16000, 64000)):
        srcs, mix = stoi_cases.set_inputs(n, SEED)
        ref.stoi(srcs[0], mix, fs)
        t0 = time.perf_counter()
        reps = 10
        for _ in range(reps):
            ref.stoi(srcs[0], mix, fs)
        dt = (time.perf_counter() - t0) / reps
        print(f"reference stoi, fs_sig {fs}, N {n}: {dt * 1e3:.2f} ms per pair on this CPU ({128 * dt:.2f} s per 128 pairs)")


if __name__ == "__main__":
    if "--time" in sys.argv:
        time_reference()
    else:
        main()
