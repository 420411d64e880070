"""Streaming wrapper on the GPU (reference model/online_class_unknown_targets.py:72-105) through the
C ABI (sepvad_forward_strided, sepvad_pit_l1, sepvad_stream_append) vs the reference's output and
the CPU restatement oracle/stream_ref.py."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEP_TOL = 1e-4


@pytest.fixture(scope="module")
def net(state_dicts):
    import sep_tfanet_vad_amd as pkg
    m = pkg.SeparationModel(**config_of("with_vad"))
    m.load_state_dict(state_dicts["with_vad"], strict=True)
    return m.eval().to(DEV)


def _criterion():
    import sep_tfanet_vad_amd as pkg
    return pkg.PITLossWrapper(loss_func=torch.nn.L1Loss(), pit_from="pw_pt")


def test_online_matches_reference_golden(net, tmp_path):
    import sep_tfanet_vad_amd as pkg
    g = np.load(os.path.join(GOLDEN, "golden_with_vad_stream.npz"))
    ons = pkg.OnlineSaving(net, str(tmp_path), _criterion())
    ons.save_sec = float(g["save_sec"])
    ons.calc_online(torch.from_numpy(g["x"]).to(DEV), "stream", 10 ** 6, dict(pkg.INFERENCE_KW_DEFAULTS))
    online = ons.online_signal.cpu().numpy()
    assert online.shape == g["online"].shape      # 7 windows x 2560 samples
    assert np.abs(online - g["online"]).max() <= SEP_TOL
    assert ons.indx == 0                          # reset() after the loop
    assert not any(tmp_path.iterdir())            # sample_indx >= num_save_samples: no wav writes


def test_online_vs_oracle_other_hops_and_padding(net, state_dicts):
    """save_sec 1 (the reference default) and 0.5; a short input padded to 3 s; B=3."""
    import sep_tfanet_vad_amd as pkg
    from oracle.stream_ref import calc_online
    from oracle.torch_ref import OracleModel
    from sep_tfanet_vad_amd import synth
    om = OracleModel(config_of("with_vad"), state_dicts["with_vad"], torch.float32)
    for n, save_sec in ((56000, 1.0), (40000, 0.5), (30000, 1.0)):
        x = torch.from_numpy(synth.make_batch(3, n, 1234 + n)[0])
        ref = calc_online(om, x, save_sec=save_sec)
        ons = pkg.OnlineSaving(net, "/nonexistent", _criterion())
        ons.save_sec = save_sec
        ons.calc_online(x.to(DEV), "s", 10 ** 6, {})
        got = ons.online_signal.cpu()
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= SEP_TOL


def test_pit_l1_matches_oracle():
    from oracle.stream_ref import pit_l1_pw_pt
    from sep_tfanet_vad_amd import pit
    g = torch.Generator().manual_seed(5)
    for B, L, swap_frac in ((1, 777, 1.0), (4, 5000, 0.0), (3, 500, 0.34), (64, 45440, 0.25)):
        ref = torch.randn(B, 2, L, generator=g)
        est = ref + 0.3 * torch.randn(B, 2, L, generator=g)
        nsw = int(round(swap_frac * B))
        est[:nsw] = est[:nsw].flip(1)
        loss_r, bi_r = pit_l1_pw_pt(est, ref)
        loss, bi, pw = pit.pit_l1(est.to(DEV), ref.to(DEV))
        assert torch.equal(bi.cpu(), bi_r)
        assert abs(loss.item() - loss_r.item()) <= 1e-5 * abs(loss_r.item())


def test_pit_wrapper_api_and_reorder():
    import sep_tfanet_vad_amd as pkg
    crit = _criterion()
    ref = torch.randn(2, 2, 1000, device=DEV)
    est = ref.flip(1).clone()
    loss, bi = crit(est, ref, return_incides=True)
    assert bi.tolist() == [[1, 0], [1, 0]]
    loss2, reordered, bi2 = crit(est, ref, return_est=True, return_incides=True)
    assert torch.equal(reordered, ref) and torch.equal(bi2, bi) and loss2.item() == loss.item() == 0.0
    assert torch.equal(pkg.reorder_source_mse(est, bi), ref)
    with pytest.raises(NotImplementedError):
        pkg.PITLossWrapper(torch.nn.MSELoss(), pit_from="pw_pt")(est, ref)


def test_wav_outputs_written_for_first_samples(net, tmp_path):
    import sep_tfanet_vad_amd as pkg
    from scipy.io import wavfile
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(1, 80000, 77)[0]).to(DEV)
    ons = pkg.OnlineSaving(net, str(tmp_path), _criterion())
    ons.calc_online(x, "utt", 0, {})
    assert (tmp_path / "utt" / "indx_0" / "output_1.wav").exists()
    assert (tmp_path / "utt" / "indx_2" / "mixed.wav").exists()
    sr, on0 = wavfile.read(str(tmp_path / "utt" / "online_signal0.wav"))
    assert sr == 16000 and np.array_equal(on0, ons.online_signal[0, 0].cpu().numpy())


def test_one_forward_equals_window_loop(net, tmp_path):
    """All windows in one forward (sepvad_forward_windows) == the reference's window loop (one forward per
    window), bitwise: kernels are batch-invariant and the PIT chain sees the same inputs."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(5, 64000, 4100)[0]).to(DEV)
    outs = []
    for one in (True, False):
        ons = pkg.OnlineSaving(net, str(tmp_path), _criterion())
        ons.save_sec = 0.16
        ons.one_forward = one
        ons.calc_online(x, "s", 10 ** 6, dict(pkg.INFERENCE_KW_DEFAULTS))
        outs.append(ons.online_signal.clone())
    assert outs[0].shape == (5, 2, 7 * 2560)
    assert torch.equal(outs[0], outs[1])


def test_chunked_windows_equal_one_forward(net, tmp_path):
    """Recordings longer than max_window_utts window-utterances run as several window-major forward_windows calls:
    bitwise equal to one call (bounded workspace)."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(5, 64000, 4101)[0]).to(DEV)
    outs = []
    for cap in (10 ** 6, 10, 5):  # one call; 2 windows per call; 1 window per call
        ons = pkg.OnlineSaving(net, str(tmp_path), _criterion())
        ons.save_sec = 0.16
        ons.max_window_utts = cap
        ons.calc_online(x, "s", 10 ** 6, dict(pkg.INFERENCE_KW_DEFAULTS))
        outs.append(ons.online_signal.clone())
    assert outs[0].shape == (5, 2, 7 * 2560)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_cfg3_full_size_one_forward_equals_window_loop(net, tmp_path):
    """BASELINE cfg 3 at its real size: 256 streams x 64 000 samples (4 s), 160 ms hop = 7 windows of 48 000 samples;
    the one-forward path (1 792 windows of T = 188 in one sepvad_forward_windows) equals the reference's window
    loop (one forward of 256 per window, model/online_class_unknown_targets.py:72-105) bitwise, on the fused TCN."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(256, 64000, 4102)[0]).to(DEV)
    h = net.native_handle(DEV)
    outs = []
    for one in (True, False):
        ons = pkg.OnlineSaving(net, str(tmp_path), _criterion())
        ons.save_sec = 0.16
        ons.one_forward = one
        ons.calc_online(x, "s", 10 ** 6, dict(pkg.INFERENCE_KW_DEFAULTS))
        assert h.fused_status()
        outs.append(ons.online_signal.clone())
    assert outs[0].shape == (256, 2, 7 * 2560)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_pit_sums_decompose_over_shards():
    """What a sharded stream batch does per window (pit_l1_sharded): the 4 pairwise L1 sums of each shard,
    summed (the all-reduce), then the batch-global choice == the unsharded sepvad_pit_l1 (same permutation,
    loss within double-rounding of the shard grouping)."""
    import ctypes
    from sep_tfanet_vad_amd import native, pit
    lib = native.load_library()
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(9, 2, 3000, generator=g)
    est = ref.flip(1) + 0.3 * torch.randn(9, 2, 3000, generator=g)
    est[:4] = ref[:4] + 0.3 * torch.randn(4, 2, 3000, generator=g)   # 4 streams prefer identity, 5 swap
    est, ref = est.to(DEV), ref.to(DEV)
    loss, perm, pw = pit.pit_l1(est, ref)
    sums = torch.zeros(4, dtype=torch.float64, device=DEV)
    for lo, hi in ((0, 4), (4, 9)):
        part = torch.empty(4, dtype=torch.float64, device=DEV)
        e, r = est[lo:hi].contiguous(), ref[lo:hi].contiguous()
        rc = lib.sepvad_pit_l1_sums(native._ptr(e), e.stride(1), native._ptr(r), r.stride(1), hi - lo, 3000,
                                    native._ptr(native.scratch(est.device, pit.PIT_SCRATCH_BYTES)), native._ptr(part),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        native._check(rc, "sepvad_pit_l1_sums")
        sums += part
    perm2 = torch.empty(9, 2, dtype=torch.int64, device=DEV)
    loss2 = torch.empty((), dtype=torch.float32, device=DEV)
    rc = lib.sepvad_pit_l1_choose(native._ptr(sums), 9.0 * 3000, 9, native._ptr(perm2), native._ptr(loss2), None,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    native._check(rc, "sepvad_pit_l1_choose")
    assert torch.equal(perm, perm2)
    assert abs(loss.item() - loss2.item()) <= 1e-6 * abs(loss.item())
