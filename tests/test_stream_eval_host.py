"""Host side of the streaming evaluation with known targets (no GPU): the plain-torch restatement
(tests/stream_eval_cases.py) on the CPU oracle pinned to the reference's own run (tests/golden/golden_stream_eval_*.npz,
make_stream_eval_golden.py), and the refusals of sepvad_stream_eval and its scratch query."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, config_of
from stream_eval_cases import (CASES, MODES, align_hop0, calc_online, case_inputs, check_perms, load_case,
                               stitched_of)

E_ARG = -1


@pytest.fixture(scope="module")
def oracle(state_dicts):
    from oracle.torch_ref import OracleModel
    om = OracleModel(config_of("with_vad"), state_dicts["with_vad"], torch.float32)
    cache = {}

    def forward(x):  # the three modes run the same windows
        key = (tuple(x.shape), hashlib.sha256(x.contiguous().numpy().tobytes()).hexdigest())
        if key not in cache:
            cache[key] = om(x)[0]
        return cache[key]
    return forward


@pytest.mark.parametrize("name,N,save_sec,seed", CASES)
def test_fixture_holds_the_required_cases(name, N, save_sec, seed):
    g = load_case(name)
    assert os.path.getsize(os.path.join(GOLDEN, f"golden_stream_eval_{name}.npz")) <= 1 << 20
    assert int(g["N"]) == N and int(g["seed"]) == seed and float(g["save_sec"]) == save_sec
    K = {"rem": 4, "short": 3, "half": 8}[name]
    H = int(np.floor(16000 * save_sec))
    assert g["raw"].shape == (2, 2, K * H)
    assert float(g["l1_gap_min"]) == 4e-4 and float(g["db_gap_min"]) == 10 * float(g["db_gap_noise"]) > 0
    for mode in MODES:
        assert g[f"{mode}_perm_f32"].shape == (K, 2, 2) and g[f"{mode}_pw_tgt_f32"].shape == (K, 2, 2, 2)
    assert g["l1_pw_sim_f32"].shape == g["sisdr_pw_sim_f32"].shape == (K, 2, 2, 2)
    assert np.array_equal(g["l1_pw_sim_f32"][:, 0], g["l1_pw_sim_f32"][:, 1])   # nn.L1Loss: every batch row alike
    case_inputs(g)


def test_padding_follows_the_reference():
    from stream_eval_cases import pad_signals
    for N, save_sec, total, K in ((70000, 1, 32000 + 70000 + 6000, 4), (30000, 1, 32000 + 48000, 3),
                                  (64000, 0.5, 40000 + 64000, 8)):
        mix, tgt, k, W, H, P = pad_signals(torch.zeros(2, N), torch.zeros(2, 2, N), save_sec)
        assert (mix.shape[-1], tgt.shape[-1], k, W, H, P) == (total, total, K, 48000, int(16000 * save_sec), 48000 - H)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,N,save_sec,seed", CASES)
def test_restatement_matches_reference(oracle, name, N, save_sec, seed, mode):
    g = load_case(name)
    mix, srcs = case_inputs(g)
    r = calc_online(oracle, mix, srcs, save_sec, mode)
    ref = stitched_of(g, mode)
    got, swap = align_hop0(r["online"].numpy(), ref, r["H"], per_batch=(mode == "l1"))
    if mode == "none":
        assert not swap.any()
    d = np.abs(got - ref).max()
    print(name, mode, "stitched max abs vs reference", d, "hop-0 swap", swap)
    assert d <= 1e-6
    check_perms(g, mode, r["perm"], r["perm_tgt"], swap)
    for key in ("online_sisdr", "reference_sisdr"):
        f32, f64 = float(g[f"{mode}_{key}_f32"]), float(g[f"{mode}_{key}_f64"])
        tol = 10 * abs(f32 - f64)
        print(name, mode, key, float(r[key]), "reference", f32, f64, "tolerance", tol)
        assert abs(float(r[key]) - f64) <= tol


def test_scratch_query():
    from sep_tfanet_vad_amd import native
    q = native.load_library().sepvad_stream_eval_scratch_bytes
    assert q(1, 1, 48000, 16000, 0) > 0
    for mode in (0, 1, 2):
        prev = 0
        for n in (1, 2, 7, 357):
            assert q(2, n, 48000, 2560, mode) > prev
            prev = q(2, n, 48000, 2560, mode)
        assert q(3, 4, 48000, 2560, mode) > q(2, 4, 48000, 2560, mode)
    assert q(2, 4, 48000, 2560, 1) > q(2, 4, 48000, 2560, 0)             # the segment sums
    assert q(0, 1, 1000, 250, 0) == E_ARG and q(65536, 1, 1000, 250, 0) == E_ARG and q(1, 0, 1000, 250, 0) == E_ARG
    assert q(1, 1, 1000, 0, 0) == E_ARG and q(1, 1, 1000, 1001, 0) == E_ARG
    assert q(1, 1, 1000, 250, 3) == E_ARG and q(1, 1, 1000, 250, -1) == E_ARG
    assert q(1, 1, 1000, 501, 0) > 0 and q(1, 1, 1000, 501, 1) == E_ARG and q(1, 1, 1000, 501, 2) == E_ARG
    assert q(1, 1, 1000, 500, 1) > 0
    assert q(1, 1, 48000, 1, 0) > 0 and q(1, 1, 48000, 1, 2) == E_ARG    # more than 4096 hops per window
    assert q(65535, 40000, 48000, 2560, 2) == E_ARG                      # more workgroups than one launch takes


def test_stream_eval_refuses_bad_arguments_without_gpu():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before any launch
    K, W, H = 5, 1000, 250
    ok = dict(sep=one, sep_ld=W, n=2, k0=1, K=K, B=3, W=W, H=H, tgt=one, tgt_ld=(K - 1) * H + W, mode=1, sdr_type=0,
              zero_mean=1, take_log=1, eps=1e-8, raw=one, raw_ld=K * H, online=one, online_ld=K * H, perm=one,
              perm_tgt=one, pw_tgt=one, loss_tgt=one, pw_sim=one, scratch=one, scratch_bytes=1 << 24, stream=None)

    def call(**kw):
        return lib.sepvad_stream_eval(*{**ok, **kw}.values())
    for name in ("sep", "tgt", "raw", "online", "perm", "perm_tgt", "pw_tgt", "loss_tgt", "scratch"):
        assert call(**{name: None}) == E_ARG, name
        assert b"null" in lib.sepvad_last_error()
    assert call(B=0) == E_ARG and call(B=65536) == E_ARG and call(n=0) == E_ARG
    assert call(H=0) == E_ARG and call(H=W + 1) == E_ARG
    assert call(H=501, tgt_ld=1 << 20, raw_ld=1 << 20, online_ld=1 << 20) == E_ARG
    assert b"2 H <= W" in lib.sepvad_last_error()
    assert call(k0=-1) == E_ARG and call(k0=4) == E_ARG and call(K=0) == E_ARG
    assert call(sep_ld=W - 1) == E_ARG and call(tgt_ld=(K - 1) * H + W - 1) == E_ARG
    assert call(raw_ld=K * H - 1) == E_ARG and call(online_ld=K * H - 1) == E_ARG
    assert b"stride" in lib.sepvad_last_error()
    assert call(mode=3) == E_ARG and call(sdr_type=3) == E_ARG
    assert call(scratch_bytes=lib.sepvad_stream_eval_scratch_bytes(3, 2, W, H, 1) - 1) == E_ARG
    assert b"scratch" in lib.sepvad_last_error()
    assert call(scratch=ctypes.c_void_p(260)) == E_ARG


def test_python_layer_refusals():
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import metrics, online, online_known, sdr
    assert pkg.OnlineSavingKnownTargets is online_known.OnlineSaving and pkg.OnlineSaving is online.OnlineSaving
    crit = pkg.PITLossWrapper(sdr.pairwise_neg_sisdr, pit_from="pw_mtx")
    ons = pkg.OnlineSavingKnownTargets(crit, None, "unused", "cpu")
    assert (ons.indx, ons.fs, ons.max_len, ons.save_sec, ons.similarity) == (0, 16000, 3, 1, False)
    assert ons.online_sisdr == [] and ons.reference_sisdr == [] and ons.num_save_samples == 2000000
    assert ons._fused_mode() == 0
    l1 = pkg.PITLossWrapper(torch.nn.L1Loss(), pit_from="pw_pt")
    si = pkg.PITLossWrapper(metrics.calc_sisdr_loss, pit_from="pw_pt")
    assert pkg.OnlineSavingKnownTargets(crit, None, "unused", "cpu", l1)._fused_mode() == 1
    assert pkg.OnlineSavingKnownTargets(crit, None, "unused", "cpu", si)._fused_mode() == 2
    mse = pkg.PITLossWrapper(torch.nn.MSELoss(), pit_from="pw_pt")
    assert pkg.OnlineSavingKnownTargets(crit, None, "unused", "cpu", mse)._fused_mode() is None
    with pytest.raises(NotImplementedError, match="sharded"):
        ons.calc_online(torch.zeros(1, 100), torch.zeros(1, 2, 100), "x", 0, process_group=object())
    x = torch.zeros(2, 2, 64)
    with pytest.raises(RuntimeError, match="ROCm"):      # supported, but not on host tensors
        si(x, x)
    with pytest.raises(NotImplementedError, match="calc_sisdr_loss"):
        mse(x, x)
