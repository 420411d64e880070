"""Inputs of the STOI golden cases (tests/golden/golden_stoi.npz), shared by the generator
(tests/golden/make_stoi_golden.py) and the tests so that both build the same float32 arrays.

A *set* is one (fs_sig, length) with two clean sources and their mixture from ``synth.make_batch`` (which already
contain pauses), optionally with a stretch of exact zeros inserted into all three. The golden stores the set's
parameters, a sha256 of the rebuilt arrays (checked here) and the one input that is not a function of the package:
the noisy copy of source 0. A *pair* is (set, clean speaker c, estimate kind):

    noisy    0.8 t + 0.05 max|t| noise        (stored; clean speaker 0 only)
    mixture  the set's mixture
    self     the clean signal itself          (STOI 1)
    other    the other speaker                (about 0, can be slightly negative)
    zeros    all zeros                        (a VAD-gated silent output: exactly 0)
"""
import hashlib
import os

import numpy as np

EST_KINDS = ("noisy", "mixture", "self", "other", "zeros")
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_stoi.npz")


def set_inputs(n, seed, zero_at=0, zero_len=0):
    """(srcs [2, n + zero_len] float32, mix [n + zero_len] float32)."""
    from sep_tfanet_vad_amd import synth
    mix, srcs = synth.make_batch(1, int(n), int(seed))
    mix, srcs = mix[0], srcs[0]
    if zero_len:
        z = np.zeros(int(zero_len), np.float32)
        mix = np.concatenate([mix[:zero_at], z, mix[zero_at:]])
        srcs = np.stack([np.concatenate([s[:zero_at], z, s[zero_at:]]) for s in srcs])
    return np.ascontiguousarray(srcs, np.float32), np.ascontiguousarray(mix, np.float32)


def inputs_sha(srcs, mix):
    return hashlib.sha256(srcs.tobytes() + mix.tobytes()).hexdigest()


def estimate(kind, c, srcs, mix, noisy):
    if kind == "noisy":
        assert c == 0
        return noisy
    if kind == "mixture":
        return mix
    if kind == "self":
        return srcs[c]
    if kind == "other":
        return srcs[1 - c]
    return np.zeros_like(mix)


def load_sets(path=GOLDEN_FILE):
    """The golden file and, per set, dict(fs, srcs, mix, noisy, pairs=[(pair index, c, kind)])."""
    g = np.load(path)
    sets = []
    for i in range(len(g["set_fs"])):
        srcs, mix = set_inputs(g["set_n"][i], g["set_seed"][i], int(g["set_zero_at"][i]), int(g["set_zero_len"][i]))
        assert inputs_sha(srcs, mix) == str(g["set_sha"][i]), f"set {i}: synth.make_batch no longer gives the golden inputs"
        pairs = [(int(p), int(g["pair_clean"][p]), EST_KINDS[int(g["pair_est"][p])])
                 for p in np.nonzero(g["pair_set"] == i)[0]]
        sets.append(dict(fs=int(g["set_fs"][i]), srcs=srcs, mix=mix, noisy=g[f"noisy_{i}"], pairs=pairs))
    return g, sets


def set_rows(s):
    """(clean [P, N], estimate [P, N]) float32 rows of the set's pairs, in pair order."""
    clean = np.stack([s["srcs"][c] for _, c, _ in s["pairs"]])
    est = np.stack([estimate(k, c, s["srcs"], s["mix"], s["noisy"]) for _, c, k in s["pairs"]])
    return clean, est
