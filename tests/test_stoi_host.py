"""Host side of the STOI / SNR entries (no GPU): the filter design of sepvad_stoi_filter against the reference's own
taps and OBM band edges (tests/golden/golden_stoi.npz, make_stoi_golden.py), the scratch size query, and the
refusals of the C ABI and of metrics.stoi."""
import ctypes

import numpy as np
import pytest
import torch

from stoi_cases import GOLDEN_FILE

RATES = (16000, 8000, 10000)
E_ARG = -1


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_FILE)


@pytest.mark.parametrize("fs", RATES)
def test_filter_matches_reference(golden, fs):
    from sep_tfanet_vad_amd import metrics
    taps, (up, down), bands = metrics.stoi_filter(fs)
    ref = golden[f"taps_{fs}"]
    assert taps.dtype == np.float32 and taps.shape == ref.shape
    assert len(taps) == {16000: 581, 8000: 365, 10000: 0}[fs]
    assert (up, down) == {16000: (5, 8), 8000: (5, 4), 10000: (1, 1)}[fs]
    if len(ref):
        assert np.abs(taps.astype(np.float64) - ref).max() <= 1e-7
        assert abs(float(taps.astype(np.float64).sum()) - 1.0) <= 1e-6
    assert np.array_equal(bands, golden[f"bands_{fs}"])
    assert bands[0].tolist() == [7, 9] and bands[2].tolist() == [11, 14] and bands[-1].tolist() == [174, 219]
    assert np.array_equal(bands[1:, 0], bands[:-1, 1])  # contiguous bin ranges


def test_golden_holds_the_required_cases(golden):
    """The fixture itself: rebuilt inputs match their checksums, every threshold margin keeps the keep / drop decision
    out of rounding's reach, and the branch cases (M = 30, M = 29, M < 30, zeros, silence joined by compaction) exist."""
    import stoi_cases
    g, sets = stoi_cases.load_sets()
    assert g["pair_margin"].min() >= 0.1
    M, kind, pset = g["pair_M"], g["pair_est"], g["pair_set"]
    assert 30 in M and 29 in M
    first = [(int(g["pair_clean"][p]), int(M[p])) for p in np.nonzero(pset == 0)[0]]
    assert int(g["set_n"][0]) == 9000 and set(first) == {(0, 33), (1, 21)}
    assert set(g["set_n"][g["set_fs"] == 16000]) >= {9000, 12000, 23457, 32000}
    for fs in (8000, 10000):
        n = g["set_n"][g["set_fs"] == fs]
        assert len(n) >= 2 and any(v % 2 for v in n)
    assert (g["set_zero_len"] > 0).sum() >= 2 and 0 in g["set_zero_at"][g["set_zero_len"] > 0]
    zeros = kind == stoi_cases.EST_KINDS.index("zeros")
    assert np.all(g["pair_stoi"][zeros & (M >= 30)] == 0.0) and np.all(g["pair_stoi"][M < 30] == 1e-5)
    assert g["pair_stoi"].min() < 0  # the other speaker can score slightly below zero
    assert sum(len(s["pairs"]) for s in sets) == len(M)


def test_filter_errors():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    info = (ctypes.c_int32 * 34)()
    buf = (ctypes.c_float * 581)()
    assert lib.sepvad_stoi_filter(16000, None, 0, info) == 0 and list(info[:4]) == [5, 8, 581, 15]  # size query
    assert lib.sepvad_stoi_filter(16000, buf, 580, info) == E_ARG
    assert b"capacity" in lib.sepvad_last_error()
    assert lib.sepvad_stoi_filter(16000, buf, 581, info) == 0
    for bad in (44100, 0, -8000, 12000):
        assert lib.sepvad_stoi_filter(bad, buf, 581, info) == E_ARG
    assert lib.sepvad_stoi_filter(16000, buf, 581, None) == E_ARG


def test_scratch_size_query():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    q = lib.sepvad_stoi_scratch_bytes
    n16 = q(1, 32000, 16000)
    # at least the resampled pair (2 x 20000 floats) and, for the 155 frames of 20000 samples, the band magnitudes
    assert n16 >= 2 * 20000 * 4 + 2 * 15 * 155 * 8
    assert n16 % 256 == 0
    assert q(16, 32000, 16000) >= 16 * (2 * 20000 * 4 + 2 * 15 * 155 * 8)
    assert q(16, 32000, 16000) > q(8, 32000, 16000) > n16        # grows with R
    assert q(1, 64000, 16000) > n16                              # and with N
    assert q(1, 20000, 10000) < n16                              # 10 kHz: no resampled copy
    assert q(1, 32000, 44100) == E_ARG                           # unsupported rate
    assert q(0, 32000, 16000) == E_ARG and q(70000, 32000, 16000) == E_ARG
    assert q(1, 256, 10000) == E_ARG                             # range(0, 0, 128): no frame
    assert q(1, 257, 10000) > 0
    assert q(1, 409, 16000) == E_ARG and q(1, 410, 16000) > 0    # ceil(409 * 5 / 8) = 256, ceil(410 * 5 / 8) = 257


def test_stoi_entry_refuses_bad_arguments_without_gpu():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before any launch
    assert lib.sepvad_stoi(one, 1000, one, 1000, 1000, 1, None, None, 44100, one, 1 << 20, one, None, None) == E_ARG
    assert b"fs_sig" in lib.sepvad_last_error()
    assert lib.sepvad_stoi(None, 1000, one, 1000, 1000, 1, None, None, 16000, one, 1 << 20, one, None, None) == E_ARG
    assert lib.sepvad_stoi(one, 999, one, 1000, 1000, 1, None, None, 16000, one, 1 << 20, one, None, None) == E_ARG
    assert lib.sepvad_stoi(one, 1000, one, 1000, 1000, 1, None, None, 16000, None, 1 << 20, one, None, None) == E_ARG
    assert lib.sepvad_snr(None, 10, one, 10, 10, 1, None, None, 1, one, None) == E_ARG
    assert lib.sepvad_snr(one, 9, one, 10, 10, 1, None, None, 1, one, None) == E_ARG


def test_python_layer_refusals():
    from sep_tfanet_vad_amd import metrics
    x = torch.zeros(2, 4000)
    with pytest.raises(NotImplementedError):
        metrics.stoi(x, x, 16000, extended=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.stoi(x, x, 16000)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.Stoi()(x.reshape(1, 2, 4000), x.reshape(1, 2, 4000), None)
    with pytest.raises(RuntimeError, match="same length"):
        metrics.stoi(x, torch.zeros(2, 3000), 16000)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.signal_noise_ratio(x, x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.pit_snr(x.reshape(1, 2, 4000), x.reshape(1, 2, 4000))
    assert metrics.stoi_met.__name__ == "stoi_metric" and metrics.stoi_met.fs_sig == 16000
    assert metrics.Stoi(fs_sig=8000).fs_sig == 8000
    # test.py:149-151 binds config["metrics"]["separation"] by name, calls .to(device) and reads __name__
    for name in ("pit_snr", "pit_si_sdr"):
        met = getattr(metrics, name)
        assert met.to("cuda") is met and met.__name__ == name
