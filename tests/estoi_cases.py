"""Inputs and the numpy restatement of the extended-STOI golden cases (tests/golden/golden_estoi.npz), shared by the
generator (tests/golden/make_estoi_golden.py) and the tests.

The cases are every pair of tests/golden/golden_stoi.npz (rebuilt through ``stoi_cases.load_sets``) followed by the
pairs of the *long* sets that golden_estoi.npz adds: (fs_sig, length, seed) again from ``synth.make_batch``, with the
estimate kinds mixture, self, other and zeros for both clean speakers (no stored noisy copy, so the file stays small).
A long set has more than three times the segments one workgroup of k_stoi_ex_corr takes, and not a multiple of them.

``restate`` is the device path's arithmetic in numpy (csrc/stoi.hip): the front end of
``make_stoi_golden.emulate`` (polyphase sum in double stored as float32, everything after it in double, spectrum m
rebuilt from kept frames m - 1, m, m + 1) and the extended tail without the reference's random term: per window of 30
spectra the band rows are centred and divided by their norm, then the frame columns; a row or column whose norm is
zero, exactly or up to the rounding of its centring, becomes zeros.
"""
import os

import numpy as np

import stoi_cases

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_estoi.npz")
LONG_KINDS = ("mixture", "self", "other", "zeros")
SEG = 30          # spectra per window
BANDS = 15
CHUNK = 64        # segments per workgroup of k_stoi_ex_corr (ST_EX_CHUNK)
GATE = 1e-5       # the gate of classic STOI


def load_sets():
    """(golden_estoi.npz, sets): stoi_cases' sets followed by the long ones, each dict(fs, srcs, mix, noisy, pairs =
    [(pair index into the pair_* arrays of golden_estoi.npz, clean speaker, kind)])."""
    g = np.load(GOLDEN_FILE)
    gs, sets = stoi_cases.load_sets()
    n_old = len(gs["pair_M"])
    assert np.array_equal(g["pair_M"][:n_old], gs["pair_M"]) and int(g["n_stoi_pairs"]) == n_old
    p = n_old
    for i in range(len(g["long_fs"])):
        srcs, mix = stoi_cases.set_inputs(g["long_n"][i], g["long_seed"][i])
        assert stoi_cases.inputs_sha(srcs, mix) == str(g["long_sha"][i]), f"long set {i}: inputs changed"
        pairs = []
        for c in (0, 1):
            for kind in LONG_KINDS:
                pairs.append((p, c, kind))
                p += 1
        sets.append(dict(fs=int(g["long_fs"][i]), srcs=srcs, mix=mix, noisy=None, pairs=pairs))
    assert p == len(g["pair_M"])
    return g, sets


def set_rows(s):
    return stoi_cases.set_rows(s)


def band_magnitudes(x, y, fs, taps, bands):
    """(tob [2, 15, M] float64 or None when M < 30, M) as k_stoi_resample .. k_stoi_spec leave them."""
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
    idx = 128 * np.arange(nF)[:, None] + np.arange(256)[None, :]
    e = np.sum((w * x[idx]) ** 2, axis=1)
    db = 20 * np.log10(np.sqrt(e) + np.finfo(float).eps)
    kept = np.nonzero((db.max() - 40 - db) < 0)[0]
    M = len(kept) - 1
    if M < SEG:
        return None, M
    tob = np.zeros((2, BANDS, M))
    for s, v in enumerate((x, y)):
        fr = w * v[128 * kept[:, None] + np.arange(256)[None, :]]        # windowed kept frames [K, 256]
        c = np.concatenate([fr[:M, :128], fr[1:M + 1, :128]], axis=1)    # first halves of kept frames m, m + 1
        c[1:, :128] += fr[:M - 1, 128:]                                  # second half of kept frame m - 1
        c[:, 128:] += fr[:M, 128:]                                       # second half of kept frame m
        p = np.abs(np.fft.rfft(c * w, 512, axis=1)) ** 2
        tob[s] = np.array([np.sqrt(p[:, lo:hi].sum(axis=1)) for lo, hi in bands])
    return tob, M


TOL2 = 2.0 ** -80  # ST_EX_TOL2: a norm within 2^-40 of the scale it was centred from counts as zero


def row_col_normalize(seg):
    """[J, 15, 30] -> (normalised, zero-norm rows, zero-norm columns). No random term; a zero norm gives zeros, and
    zero includes the rounding remainder of an exact zero (csrc/stoi.hip, st_ex_normalize): a row norm up to
    2^-40 sqrt(30) mean, a column norm up to 2^-40 (the rows have unit norm)."""
    mean = seg.mean(axis=2, keepdims=True)
    r = seg - mean
    ss = np.sum(r * r, axis=2, keepdims=True)
    keep = ss > (TOL2 * SEG) * (mean * mean)
    with np.errstate(divide="ignore"):
        r = r * np.where(keep, 1.0 / np.sqrt(ss), 0.0)
    c = r - r.mean(axis=1, keepdims=True)
    ss2 = np.sum(c * c, axis=1, keepdims=True)
    keep2 = ss2 > TOL2
    with np.errstate(divide="ignore"):
        c = c * np.where(keep2, 1.0 / np.sqrt(ss2), 0.0)
    return c, int((~keep).sum()), int((~keep2).sum())


def estoi_tail(tob):
    """tob [2, 15, M], M >= 30 -> (d, zero-norm rows and columns of both signals)."""
    M = tob.shape[2]
    J = M - SEG + 1
    win = np.arange(J)[:, None] + np.arange(SEG)[None, :]
    xn, xr, xc = row_col_normalize(tob[0][:, win].transpose(1, 0, 2))
    yn, yr, yc = row_col_normalize(tob[1][:, win].transpose(1, 0, 2))
    return float(np.sum(xn * yn) / (SEG * J)), xr + xc + yr + yc


def restate(x, y, fs, taps, bands):
    """(d, M) of the device path: exactly 1e-5 where M < 30."""
    tob, M = band_magnitudes(x, y, fs, taps, bands)
    if tob is None:
        return 1e-5, M
    return estoi_tail(tob)[0], M
