"""Inputs and float64 numpy expectations of the scene-simulation tests (csrc/sim.hip), shared by the fixture
generator tests/golden/make_sim_golden.py and tests/test_gpu_sim.py. Everything is drawn from fixed PCG64 seeds, so
the fixture stores expectations only (in full where small, every SUB-th sample otherwise: the full arrays would not
fit the size the fixture may have; the tests recompute them with the functions below and compare both)."""
import numpy as np

SUB = 32  # stride of the stored samples of the large expectations

# (Nx, K, L): a plain row, a one-tap filter, K > Nx, and L beyond Nx + K - 1 (exact zeros at the end)
CONV_CASES = [(3000, 257, 3000), (3000, 1, 3000), (100, 700, 500), (1000, 64, 1500)]


def conv_inputs():
    """[(x float32 [Nx], h float64 [K], L)] for CONV_CASES; h decays like a room response."""
    rng = np.random.Generator(np.random.PCG64(501))
    out = []
    for nx, k, L in CONV_CASES:
        x = rng.standard_normal(nx).astype(np.float32)
        h = rng.standard_normal(k) * np.exp(-np.arange(k) / (0.3 * k + 1.0))
        out.append((x, h, L))
    return out


def conv_reference(x, h, L):
    """np.convolve(wave, h)[:cut_length] (create_simulation_data.py:482-500), zero-extended to L."""
    y = np.convolve(x.astype(np.float64), h)[:L]
    return np.concatenate([y, np.zeros(L - len(y))])


def conv_bound(x, h):
    """|y_dev - y_ref| per row: both sides are length-K double sums, error <= K 2^-53 sum|h| max|x| each; x 4."""
    return 4 * len(h) * 2.0 ** -53 * np.abs(h).sum() * float(np.abs(x).max())


MIX_B, MIX_S, MIX_L = 3, 2, 4096
MIX_AB = [(2.0, 1.0), (1.8, 0.9)]  # create_simulation_data.py:585 ; only_inference.py:81


def mix_inputs():
    """rev, dry [B, S, L] float64, noise [B, L] float32 (non-zero mean), snr_db [B] (NaN: scene 1 has no noise)."""
    rng = np.random.Generator(np.random.PCG64(502))
    rev = rng.standard_normal((MIX_B, MIX_S, MIX_L)) * rng.uniform(0.2, 3.0, (MIX_B, MIX_S, 1))
    dry = rev * 0.7 + 0.1 * rng.standard_normal((MIX_B, MIX_S, MIX_L))
    noise = (0.3 + rng.standard_normal((MIX_B, MIX_L))).astype(np.float32)
    snr = np.array([5.0, np.nan, 12.5])
    return rev, dry, noise, snr


def mix_reference(rev, noise, snr, a, b, power_mode=0):
    """The reference's expressions (create_simulation_data.py:558-588, Noise.get_mixed :707-713) in float64.
    Returns (mix float64 [B, L], stats [B, 4] = gain, min, max, a / (max - min))."""
    B = rev.shape[0]
    mix, stats = np.zeros((B, rev.shape[2])), np.zeros((B, 4))
    for i in range(B):
        mixed = rev[i, 0].copy()
        for s in range(1, rev.shape[1]):
            mixed = mixed + rev[i, s]
        gain = 0.0
        if noise is not None and not np.isnan(snr[i]):
            nz = noise[i].astype(np.float64)
            if power_mode == 0:
                mix_std, noise_std = np.std(mixed), np.std(nz)
                gain = np.sqrt(10 ** (-snr[i] / 10) * np.power(mix_std, 2) / np.power(noise_std, 2))
            else:
                gain = np.sqrt(np.mean(mixed ** 2) / (np.mean(nz ** 2) * 10 ** (snr[i] / 10)))
            mixed = mixed + gain * nz
        lo, hi = np.min(mixed), np.max(mixed)
        mix[i] = a * (mixed - lo) / (hi - lo) - b
        stats[i] = gain, lo, hi, a / (hi - lo)
    return mix, stats


def targets_reference(dry, stats, mode, a, b):
    if mode == 1:
        return stats[:, 3][:, None, None] * dry
    lo, hi = dry.min(axis=2, keepdims=True), dry.max(axis=2, keepdims=True)
    return a * (dry - lo) / (hi - lo) - b  # create_simulation_data.py:605-620


def activity_tracks(L):
    """uint8 [5, L]: a frame with exactly 256 ones, one with 257, all ones, a 0..2 sum track, random segments."""
    rng = np.random.Generator(np.random.PCG64(503 + L))
    act = np.zeros((5, L), dtype=np.uint8)
    act[0, 256:512] = 1                       # frames over [0, 512) and [256, 768): 256 ones each -> 0 (tie: lowest)
    act[0, L - 256:L - 128] = 1
    act[1, 255:512] = 1                       # [0, 512): 257 ones -> 1
    act[1, 1024:1100] = 1
    act[2, :] = 1
    for row in (3, 4):
        for _ in range(2 if row == 3 else 1):
            pos = int(rng.integers(0, 300))
            while pos < L:
                on, off = int(rng.integers(100, 900)), int(rng.integers(50, 700))
                act[row, pos:pos + on] += 1
                pos += on + off
    act[3, L - 256:] = 2                      # an edge frame a non-binary track wins under the sum-track rule
    return act
