"""Scene simulation on the device (csrc/sim.hip through rirgen.generateRirBatch, simulate.py and
synth.make_reverb_batch_device) against the reference's goldens, the host generator and numpy in float64."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import make_rir_golden as mk  # noqa: E402
import sim_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# max|h_dev - h_ref| / max|h_ref| over the nine jobs of test_rir_matches_goldens_and_host_generator: 16 x the worst
# value measured on one MI355X, rounded up to a power of ten (the measured values: that test's docstring)
RIR_GATE = 1e-11
F32_GATE = 2.4e-7  # two float32 ulps at 1: a double result rounded to float on either side of a tie


def _job(room, src, mics, beta, orient=(0.0, 0.0), hp=1, dim=3, order=-1, n=-1, mtype="o"):
    kw = dict(betaCoeffs=beta) if len(beta) == 6 else dict(reverbTime=beta[0])
    return dict(roomMeasures=room, sourcePosition=src, receiverPositions=mics, orientation=orient,
                isHighPassFilter=bool(hp), nDim=dim, nOrder=order, nSamples=n, micType=mtype, **kw)


# three small jobs compared with the host generator: 3 528 and 5 544 images, and a microphone 0.5 mm from the source
# (floor(dist) = 0, the kernel starts at sample -63 and is clipped at sample 0)
EXTRA = [
    _job([3.2, 2.7, 2.4], [1.1, 0.9, 1.3], [2.2, 1.8, 1.0], [0.3], n=700),
    _job([4.1, 3.3, 2.6], [0.8, 2.5, 1.1], [3.0, 1.2, 1.6], [0.45], n=1100, hp=0),
    _job([5.0, 4.0, 3.0], [2.0, 2.0, 1.5], [2.0005, 2.0, 1.5], [0.25], n=300),
]


def _host_rir(job):
    from sep_tfanet_vad_amd import rirgen
    kw = dict(job)
    return np.array(rirgen.generateRir(kw.pop("roomMeasures"), kw.pop("sourcePosition"), kw.pop("receiverPositions"),
                                       **kw))


@pytest.fixture(scope="module")
def rir_batch():
    """The five golden cases (six rows: case 0 has two microphones) and the three extra jobs in ONE call."""
    from sep_tfanet_vad_amd import rirgen
    jobs = [_job(*c) for c in mk.CASES] + EXTRA
    h, lens = rirgen.generateRirBatch(jobs, device=DEV)
    torch.cuda.synchronize()
    return jobs, h.cpu().numpy(), lens.cpu().numpy()


def test_rir_matches_goldens_and_host_generator(rir_batch):
    """Relative error max|h_dev - h_ref| / max|h_ref| per job against golden_rir.npz (written by the reference's
    generator) and, for the three extra jobs, the bit-exact host generator. Measured on one MI355X, in job order:
    9.6e-15 8.4e-15 1.3e-13 3.1e-15 7.6e-15 4.6e-15 6.5e-14 3.7e-15 4.3e-15 (worst: golden case 1, T60 0.6 s with the
    high-pass; 16 x 1.3e-13 = 2.0e-12 -> gate 1e-11). Golden case 2 holds an image at an exactly integer distance: a contracted distance moves its whole
    128-tap kernel by one sample (an error of order 1, not of order 1e-12)."""
    jobs, h, lens = rir_batch
    g = np.load(os.path.join(GOLDEN, "golden_rir.npz"))
    refs = [row for i in range(len(mk.CASES)) for row in g[f"h{i}"]] + [_host_rir(j) for j in EXTRA]
    assert len(refs) == h.shape[0] == 9 and h.shape[1] == max(lens)
    errs = []
    for j, ref in enumerate(refs):
        assert lens[j] == len(ref)
        errs.append(float(np.abs(h[j, :len(ref)] - ref).max() / np.abs(ref).max()))
        assert not h[j, len(ref):].any(), f"job {j}: the row is not zero beyond its length"
    print("rir relative errors:", " ".join(f"{e:.3e}" for e in errs))
    assert np.abs(refs[8][:64]).max() > 0  # the clipped job does start inside the first taps
    assert max(errs) <= RIR_GATE, errs


def test_rir_deterministic_and_batch_invariant(rir_batch):
    from sep_tfanet_vad_amd import rirgen
    jobs, h, lens = rir_batch
    h2, _ = rirgen.generateRirBatch(jobs, device=DEV)
    assert np.array_equal(h2.cpu().numpy(), h)  # two runs, bitwise
    # one job per row: case 0's two microphones as two jobs
    jobs = [dict(jobs[0], receiverPositions=m) for m in jobs[0]["receiverPositions"]] + jobs[1:]
    # job 6 (n = 700: not a multiple of the 256-sample tile) alone, with a longer row, against itself as job 5 of 8
    # in another order
    alone, l1 = rirgen.generateRirBatch([jobs[6]], device=DEV, ld=1000)
    alone = alone.cpu().numpy()
    assert int(l1[0]) == 700 and alone.shape == (1, 1000) and not alone[0, 700:].any()
    order = [8, 3, 7, 0, 4, 6, 2, 5]
    mixed, l8 = rirgen.generateRirBatch([jobs[i] for i in order], device=DEV)
    mixed = mixed.cpu().numpy()
    assert order[5] == 6 and int(l8[5]) == 700
    assert np.array_equal(mixed[5, :700], alone[0, :700]) and np.array_equal(alone[0, :700], h[6, :700])
    assert not mixed[5, 700:].any()


@pytest.fixture(scope="module")
def conv_batch():
    from sep_tfanet_vad_amd import simulate
    cases = sc.conv_inputs()
    y = []
    for x, h, L in cases:  # one call per shape (Nx, K, L)
        y.append(simulate.fir_convolve(torch.from_numpy(x)[None].to(DEV), torch.from_numpy(h)[None].to(DEV), L))
    torch.cuda.synchronize()
    return cases, [t.cpu().numpy()[0] for t in y]


def test_convolve_matches_numpy(conv_batch):
    """|y_dev - y_ref| <= 4 K 2^-53 sum|h| max|x| per row against np.convolve(x, h)[:L] in float64 (derived: both
    sides are length-K double sums), and the stored golden samples."""
    cases, ys = conv_batch
    g = np.load(os.path.join(GOLDEN, "golden_sim.npz"))
    for i, ((x, h, L), y) in enumerate(zip(cases, ys)):
        ref = sc.conv_reference(x, h, L)
        assert np.array_equal(ref[::sc.SUB], g[f"conv_y{i}"])
        err, bound = float(np.abs(y - ref).max()), sc.conv_bound(x, h)
        print(f"conv case {sc.CONV_CASES[i]}: max err {err:.3e}, bound {bound:.3e}")
        assert y.shape == (L,) and err <= bound
    x, h, L = cases[3]
    assert not ys[3][len(x) + len(h) - 1:].any()  # L beyond Nx + K - 1: exact zeros


def test_convolve_klen_index_arrays_and_invariance(conv_batch):
    from sep_tfanet_vad_amd import simulate
    cases, ys = conv_batch
    rng = np.random.Generator(np.random.PCG64(77))
    X = torch.from_numpy(rng.standard_normal((3, 2500)).astype(np.float32)).to(DEV)
    H = torch.from_numpy(rng.standard_normal((4, 600)) * np.exp(-np.arange(600) / 150.0)).to(DEV)
    klen = torch.tensor([600, 1, 333, 64], dtype=torch.int32, device=DEV)
    xidx = torch.tensor([2, 0, 1, 2, 0], dtype=torch.int32, device=DEV)
    hidx = torch.tensor([1, 3, 0, 2, 2], dtype=torch.int32, device=DEV)
    L = 2700
    y = simulate.fir_convolve(X, H, L, klen=klen, xidx=xidx, hidx=hidx)
    y2 = simulate.fir_convolve(X, H, L, klen=klen, xidx=xidx, hidx=hidx)
    assert torch.equal(y, y2)  # two runs, bitwise
    # gathered rows without index arrays, and every row alone with its filter cut to its length: the same bits
    yg = simulate.fir_convolve(X[xidx.long()].contiguous(), H[hidx.long()].contiguous(), L,
                               klen=klen[hidx.long()].contiguous())
    assert torch.equal(y, yg)
    Xh, Hh = X.cpu().numpy(), H.cpu().numpy()
    for r in range(5):
        k = int(klen[hidx[r]])
        one = simulate.fir_convolve(X[int(xidx[r])][None].contiguous(), H[int(hidx[r]), :k][None].contiguous(), L)
        assert torch.equal(one[0], y[r]), r
        ref = sc.conv_reference(Xh[int(xidx[r])], Hh[int(hidx[r]), :k], L)
        assert float(np.abs(y[r].cpu().numpy() - ref).max()) <= sc.conv_bound(Xh[int(xidx[r])], Hh[int(hidx[r]), :k])
    # a row of the shared cases has the bits it had in its own call when it sits in a batch of other rows
    x0, h0, L0 = cases[0]
    xb = torch.zeros(2, 3000, device=DEV)
    xb[1] = torch.from_numpy(x0).to(DEV)
    xb[0, :2500] = X[0]
    hb = torch.zeros(2, 600, device=DEV, dtype=torch.float64)
    hb[1, :257] = torch.from_numpy(h0).to(DEV)
    hb[0] = H[0]
    yb = simulate.fir_convolve(xb, hb, L0, klen=torch.tensor([600, 257], dtype=torch.int32, device=DEV))
    assert np.array_equal(yb[1].cpu().numpy(), ys[0])


def test_mix_normalise_targets_match_golden():
    """stats within 1e-12 relative, mix and targets within 2.4e-7 of the float64 expectation, minimum exactly -b, a
    scene alone bitwise equal to itself in the batch. B = 3, S = 2, L = 4096; scene 1 has no noise."""
    from sep_tfanet_vad_amd import simulate
    g = np.load(os.path.join(GOLDEN, "golden_sim.npz"))
    rev, dry, noise, snr = sc.mix_inputs()
    trev, tdry, tnoise = (torch.from_numpy(v).to(DEV) for v in (rev, dry, noise))
    tsnr = torch.from_numpy(snr).to(DEV)
    for p, (a, b) in enumerate(sc.MIX_AB):
        mix, stats = simulate.scene_mix(trev, tnoise, tsnr, a, b)
        ref_mix, ref_stats = sc.mix_reference(rev, noise, snr, a, b)
        assert np.array_equal(ref_stats, g[f"mix_stats{p}"]) and np.array_equal(ref_mix[:, ::sc.SUB], g[f"mix{p}"])
        st = stats.cpu().numpy()
        rel = np.abs(st - ref_stats) / np.maximum(np.abs(ref_stats), 1e-300)
        rel[ref_stats == 0] = np.abs(st[ref_stats == 0])
        print(f"(a, b) = {(a, b)}: stats rel err {rel.max():.3e}, mix err "
              f"{np.abs(mix.cpu().numpy() - ref_mix).max():.3e}")
        assert rel.max() <= 1e-12 and st[1, 0] == 0.0
        m = mix.cpu().numpy()
        assert m.dtype == np.float32 and np.abs(m - ref_mix).max() <= F32_GATE
        assert (m.min(axis=1) == np.float32(-b)).all()
        for mode in (0, 1):
            tg = simulate.scene_targets(tdry, stats, mode, a, b).cpu().numpy()
            ref_t = sc.targets_reference(dry, ref_stats, mode, a, b)
            assert np.array_equal(ref_t[:, :, ::sc.SUB], g[f"targets{p}_mode{mode}"])
            assert tg.dtype == np.float32 and np.abs(tg - ref_t).max() <= F32_GATE, (p, mode)
            if mode == 0:
                assert (tg.min(axis=2) == np.float32(-b)).all()
        for i in range(sc.MIX_B):  # the scene alone
            m1, s1 = simulate.scene_mix(trev[i:i + 1], tnoise[i:i + 1], tsnr[i:i + 1], a, b)
            assert torch.equal(m1[0], mix[i]) and torch.equal(s1[0], stats[i])
            t1 = simulate.scene_targets(tdry[i:i + 1], s1, 1, a, b)
            assert torch.equal(t1[0], simulate.scene_targets(tdry, stats, 1, a, b)[i])
    mix, stats = simulate.scene_mix(trev, None, None, 1.8, 0.9)  # no noise at all
    rel = np.abs(stats.cpu().numpy() - g["mix_nonoise_stats"])[:, 1:] / np.abs(g["mix_nonoise_stats"][:, 1:])
    assert rel.max() <= 1e-12 and not stats[:, 0].any()


@pytest.mark.parametrize("L", [2048, 4096])
def test_vad_frame_labels_exact(L):
    from sep_tfanet_vad_amd import metrics, simulate
    g = np.load(os.path.join(GOLDEN, "golden_sim.npz"))
    act = sc.activity_tracks(L)
    assert act[0, 0:512].sum() == 256 and act[1, 0:512].sum() == 257 and act[2].all() and act[3].max() == 2
    tact = torch.from_numpy(act).to(DEV)
    for mode in (0, 1):
        want = g[f"frames_L{L}_edge{mode}"]
        got = simulate.vad_frame_labels(tact, edge_mode=mode)
        assert got.shape == (5, 2 * L // 512 + 1) == want.shape and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), want), mode
    want0, want1 = g[f"frames_L{L}_edge0"], g[f"frames_L{L}_edge1"]
    assert want0[0, 1] == 0 and want0[1, 1] == 1           # 256 ones lose the tie, 257 win
    assert want0[2, 0] == 0 and want1[2, 0] == 1           # all ones: an edge frame only under the sum-track rule
    binary = simulate.vad_frame_labels(tact[[0, 1, 2, 4]].reshape(2, 2, L), edge_mode=1)
    acc = metrics.Accuracy_Vad()(binary.clone(), binary)
    assert binary.shape == (2, 2, 1 + L // 256) and [float(v) for v in acc] == [1.0, 1.0, 1.0]


def test_end_to_end_reverb_batch_device():
    """synth.make_reverb_batch_device against synth.make_reverb_batch (host generator + fftconvolve): mixtures and
    targets within 2.4e-7, then one forward on the device mixture."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    mix, tg = synth.make_reverb_batch_device(2, 16384, 9100, device=DEV, rir_samples=1000)
    ref_mix, ref_tg = synth.make_reverb_batch(2, 16384, 9100, rir_samples=1000)
    assert mix.shape == (2, 16384) and tg.shape == (2, 2, 16384) and mix.dtype == tg.dtype == torch.float32
    em, et = np.abs(mix.cpu().numpy() - ref_mix).max(), np.abs(tg.cpu().numpy() - ref_tg).max()
    print(f"end to end: mix err {em:.3e}, targets err {et:.3e}")
    assert em <= F32_GATE and et <= F32_GATE
    net = pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
    sd = synth.make_state_dict(pkg.CONFIG_WITH_VAD, 1234)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.eval().to(DEV)
    with torch.no_grad():
        sep, vad, est = net(mix)
    assert sep.shape == (2, 2, 16384) and bool(torch.isfinite(sep).all())


def test_simulate_scenes_reference_conventions():
    """simulate_scenes with the reference's conventions, (a, b) = (2, 1), each target's own min-max, no noise,
    frame labels from an activity track, against the host generator + numpy in float64."""
    from sep_tfanet_vad_amd import simulate
    L = 2048
    rng = np.random.Generator(np.random.PCG64(78))
    src = rng.standard_normal((1, 2, L)).astype(np.float32)
    base = dict(roomMeasures=[4.0, 3.5, 2.6], receiverPositions=[2.1, 1.7, 1.3], nSamples=300)
    rir_jobs = [dict(base, sourcePosition=p, reverbTime=0.3) for p in ([1.0, 1.2, 1.1], [3.0, 2.4, 1.5])]
    dry_jobs = [dict(j, reverbTime=0.0) for j in rir_jobs]
    act = torch.from_numpy(sc.activity_tracks(L)[[1, 4]][None]).to(DEV)
    mix, tg, stats, frames = simulate.simulate_scenes(torch.from_numpy(src).to(DEV), rir_jobs, dry_jobs, a=2.0, b=1.0,
                                                      target_mode=0, activity=act)
    rev = np.stack([sc.conv_reference(src[0, s], _host_rir(rir_jobs[s]), L) for s in range(2)])[None]
    dry = np.stack([sc.conv_reference(src[0, s], _host_rir(dry_jobs[s]), L) for s in range(2)])[None]
    ref_mix, ref_stats = sc.mix_reference(rev, None, None, 2.0, 1.0)
    assert np.abs(mix.cpu().numpy() - ref_mix).max() <= F32_GATE
    assert np.abs(tg.cpu().numpy() - sc.targets_reference(dry, ref_stats, 0, 2.0, 1.0)).max() <= F32_GATE
    assert np.allclose(stats.cpu().numpy(), ref_stats, rtol=1e-9, atol=0)
    assert frames.shape == (1, 2, 2 * L // 512 + 1) and torch.equal(frames, simulate.vad_frame_labels(act, 0))
