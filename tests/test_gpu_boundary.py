"""The C-ABI contract of include/sepvad.h beyond parity (reference model/model.py:402-461):

* concurrent forwards on different streams of ONE handle are allowed: each caller stream gets its own
  workspace, hand-off words and give-up words, so two streams running at once give the same bits as a
  serial run;
* a fused-TCN hand-off give-up never passes as success: the forward that gave up writes NaN outputs (stream-
  ordered, no host sync), the next forward on the same stream reports it (or fused_status / SEPVAD_CHECK=1), it
  is not sticky, and the forward after it is valid again;
* side attributes belong to the forward that produced them: reading them after a later forward on the same stream
  raises instead of copying another forward's (differently shaped) workspace; they are safe to read on another
  stream; a stream's context can be released;
* a batch split over several persistent launches (launch salts, epoch counters) is bitwise equal to one;
* the fp16 split of the GEMM operands keeps fp32-equivalent accuracy when weights or inputs are scaled
  by 1e-3 or 1e3 (static power-of-two range scales, pack.h range_exp).
"""
import os

import numpy as np
import pytest
import torch

from conftest import check_vad_labels, config_of, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEP_TOL = 1e-4


def _net(cfg, sd):
    import sep_tfanet_vad_amd as pkg
    net = pkg.SeparationModel(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.eval().to(DEV)


@pytest.fixture(scope="module")
def net(state_dicts):
    return _net(config_of("with_vad"), state_dicts["with_vad"])


def test_two_streams_concurrently_match_serial(net):
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    x1 = torch.from_numpy(synth.make_batch(40, 32000, 11)[0]).to(DEV)
    x2 = torch.from_numpy(synth.make_batch(24, 24000, 12)[0]).to(DEV)
    with torch.no_grad():
        r1 = h.forward(x1)
        r2 = h.forward(x2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):  # several rounds: the two streams' kernels overlap on the device
        with torch.cuda.stream(s1):
            a = h.forward(x1)
        with torch.cuda.stream(s2):
            b = h.forward(x2)
        outs.append((a, b))
    torch.cuda.synchronize()
    assert h.fused_status()
    bad = []
    for i, (a, b) in enumerate(outs):
        for k in ("sep", "vad", "est"):
            for name, got, ref in (("x1", a[k], r1[k]), ("x2", b[k], r2[k])):
                if not torch.equal(got, ref):  # where: utterances, and the first / last differing sample or frame
                    d = (got != ref).reshape(got.shape[0], -1)
                    utts = torch.nonzero(d.any(dim=1)).flatten().tolist()
                    idx = torch.nonzero(d[utts[0]]).flatten()
                    bad.append(f"round {i} {name} {k}: utterances {utts}, utt {utts[0]} positions {idx[0].item()}.."
                               f"{idx[-1].item()} of {d.shape[1]}, max abs {(got - ref).abs().max().item():.3e}")
    assert not bad, "\n".join(bad)


def test_stream_context_eviction_matches_serial(net, monkeypatch):
    """More live streams than the per-handle context cap (SEPVAD_MAX_STREAM_CTX=2): each new stream's context evicts the
    least recently used one while forwards on the other streams are still queued (the eviction drains the device before
    freeing the evicted workspace). Every output equals the serial forward's."""
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    x = torch.from_numpy(synth.make_batch(24, 32000, 31)[0]).to(DEV)
    with torch.no_grad():
        ref = h.forward(x)
    torch.cuda.synchronize()
    monkeypatch.setenv("SEPVAD_MAX_STREAM_CTX", "2")
    streams = [torch.cuda.Stream() for _ in range(5)]
    outs = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                outs.append(h.forward(x))
    torch.cuda.synchronize()
    assert h.fused_status()
    for i, o in enumerate(outs):
        for k in ("sep", "vad", "est"):
            assert torch.equal(o[k], ref[k]), f"forward {i} {k}"


def test_giveup_is_reported_once_and_not_sticky(net):
    g = load_golden("with_vad", "small")
    x = torch.from_numpy(g["x"]).to(DEV)
    h = net.native_handle(DEV)
    os.environ["SEPVAD_TCN_FORCE_GIVEUP"] = "1"
    try:
        h.forward(x)
    finally:
        del os.environ["SEPVAD_TCN_FORCE_GIVEUP"]
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="gave up"):
        h.forward(x)  # the next forward on the same stream reports the earlier give-up
    out = h.forward(x)  # reported once: this one is valid
    assert h.fused_status()
    assert np.abs(out["sep"].cpu().numpy() - g["sep"]).max() <= SEP_TOL
    # and through fused_status (the synchronising check SEPVAD_CHECK=1 runs after every forward)
    os.environ["SEPVAD_TCN_FORCE_GIVEUP"] = "1"
    try:
        h.forward(x)
    finally:
        del os.environ["SEPVAD_TCN_FORCE_GIVEUP"]
    with pytest.raises(RuntimeError, match="gave up"):
        h.fused_status()
    assert h.fused_status()  # not sticky
    out = h.forward(x)
    assert np.abs(out["sep"].cpu().numpy() - g["sep"]).max() <= SEP_TOL


def test_giveup_poisons_the_same_forward(net):
    """The forward whose k_tcn hand-off gave up returns NaN in sep, vad and est (k_istft_pair reads the give-up word,
    stream-ordered): no invalid output passes as a valid one even for a caller's last or only forward."""
    g = load_golden("with_vad", "small")
    x = torch.from_numpy(g["x"]).to(DEV)
    h = net.native_handle(DEV)
    good = h.forward(x)
    assert not torch.isnan(good["sep"]).any()
    os.environ["SEPVAD_TCN_FORCE_GIVEUP"] = "1"
    try:
        bad = h.forward(x)
    finally:
        del os.environ["SEPVAD_TCN_FORCE_GIVEUP"]
    torch.cuda.synchronize()
    assert torch.isnan(bad["sep"]).all()
    assert torch.isnan(bad["vad"]).all()
    assert torch.isnan(torch.view_as_real(bad["est"])).all()
    with pytest.raises(RuntimeError, match="gave up"):
        h.forward(x)
    out = h.forward(x)
    assert h.fused_status()
    assert not torch.isnan(out["sep"]).any()
    assert np.abs(out["sep"].cpu().numpy() - g["sep"]).max() <= SEP_TOL


def test_stale_side_attributes_raise(net):
    """net(xa); a later forward of another shape on the same stream (Handle.forward, or the streaming wrapper's
    window forward); reading net.spectrum must raise, never copy that forward's workspace into xa-sized tensors."""
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    xa = torch.from_numpy(synth.make_batch(3, 20000, 41)[0]).to(DEV)
    xb = torch.from_numpy(synth.make_batch(9, 32000, 42)[0]).to(DEV)
    with torch.no_grad():
        net(xa)
    h.forward(xb)
    with pytest.raises(RuntimeError, match="later forward"):
        _ = net.spectrum
    with pytest.raises(RuntimeError, match="later forward"):
        _ = net.mask_per_speaker
    eager = h.forward(xa, return_aux=True)
    with torch.no_grad():
        net(xa)
    assert torch.equal(net.spectrum, eager["spectrum"])
    assert torch.equal(net.masks_b, eager["masks_b"])


def test_side_attributes_read_on_another_stream(net):
    """A forward on a side stream, its side attributes read on the default stream: the reader's stream waits for
    the copies (wait_stream / record_stream), values equal the eager ones."""
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    x = torch.from_numpy(synth.make_batch(4, 24000, 43)[0]).to(DEV)
    eager = h.forward(x, return_aux=True)
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1), torch.no_grad():
        net(x)
    m = net.mask_per_speaker.clone()  # default stream
    assert torch.equal(m, eager["mask_per_speaker"])
    assert torch.equal(net.spectrum, eager["spectrum"])
    h.release_stream(s1.cuda_stream)  # the side stream's context freed after a sync; a new forward re-creates it
    with torch.cuda.stream(s1), torch.no_grad():
        r = h.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(r["sep"], eager["sep"])


def test_several_launches_per_forward_are_bitwise_identical(net):
    """SEPVAD_TCN_MAX_ITER=1: every group handles one utterance per launch, so B=150 takes 3 launches
    (new salt, offsets of S0 / Xfin / records per launch)."""
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(150, 32000, 4343)[0]).to(DEV)
    h = net.native_handle(DEV)
    a = {k: v.clone() for k, v in h.forward(x).items() if torch.is_tensor(v)}
    os.environ["SEPVAD_TCN_MAX_ITER"] = "1"
    try:
        b = h.forward(x)
        assert h.fused_status()
    finally:
        del os.environ["SEPVAD_TCN_MAX_ITER"]
    for k in ("sep", "vad", "est"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("wscale", [1e-3, 1e3])
def test_scaled_weights_keep_fp32_accuracy(wscale, state_dicts):
    """Every weight except the STFT windows scaled by 1e-3 / 1e3: the fp16 planes would underflow
    (subnormal) or overflow (inf) without the range scales. Gate: HIP (fp16x3) is as close to the fp64
    oracle as the fp32 oracle is (x1e3 makes the problem itself ill-conditioned: the fp32 oracle is
    6.5e-3 from fp64 there), and within 1e-4 where the problem is well conditioned."""
    from oracle.torch_ref import OracleModel
    from sep_tfanet_vad_amd import synth
    cfg = config_of("with_vad")
    sd = {k: (v if k.endswith("window") else v * wscale) for k, v in state_dicts["with_vad"].items()}
    x = torch.from_numpy(synth.make_batch(3, 32000, 77)[0])
    net = _net(cfg, sd)
    net.native_precision = "f16x3"
    with torch.no_grad():
        s, v, _ = net(x.to(DEV))
    assert torch.isfinite(s).all() and torch.isfinite(v).all()
    s32 = OracleModel(cfg, sd, torch.float32)(x)[0].double()
    s64, v64, _ = OracleModel(cfg, sd, torch.float64)(x)
    e32 = (s32 - s64).abs().max().item()
    ehip = (s.cpu().double() - s64).abs().max().item()
    assert ehip <= max(SEP_TOL, 3.0 * e32), (ehip, e32)
    check_vad_labels(v.cpu().numpy(), v64.numpy(), band=1e-3, where=f"weights x{wscale:g}")


@pytest.mark.parametrize("xscale", [1e-3, 1e3])
def test_scaled_inputs(xscale, net, state_dicts):
    from oracle.torch_ref import OracleModel
    from sep_tfanet_vad_amd import synth
    x = torch.from_numpy(synth.make_batch(3, 32000, 78)[0]) * xscale
    with torch.no_grad():
        s, v, _ = net(x.to(DEV))
    s_ref, v_ref, _ = OracleModel(config_of("with_vad"), state_dicts["with_vad"], torch.float32)(x)
    assert np.abs(s.cpu().numpy() - s_ref.numpy()).max() <= SEP_TOL * max(1.0, xscale)
    check_vad_labels(v.cpu().numpy(), v_ref.numpy())


def test_side_attributes_materialised_on_read(net):
    """self.spectrum / masks_b / mask_per_speaker are materialised from the forward's workspace on first
    read (sepvad_side_outputs): bitwise equal to the eagerly written side outputs, and they follow the
    latest forward."""
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    xa = torch.from_numpy(synth.make_batch(5, 20000, 31)[0]).to(DEV)
    xb = torch.from_numpy(synth.make_batch(3, 32000, 32)[0]).to(DEV)
    for x in (xa, xb):
        eager = h.forward(x, return_aux=True)
        with torch.no_grad():
            net(x)
        for k in ("spectrum", "masks_b", "mask_per_speaker"):
            lazy = getattr(net, k)
            assert lazy.shape == eager[k].shape, k
            assert torch.equal(lazy, eager[k]), k
    net.spectrum = "user value"  # plain-attribute assignment keeps working
    assert net.spectrum == "user value"


@pytest.mark.parametrize("N", [32000, 31900, 32002, 20001])
def test_side_outputs_leave_outputs_bitwise(net, N):
    """k_istft_pair writes est in paired 16-byte stores and overlap-adds in float4 when only est is asked for (even T,
    N % 4 == 0) and frame by frame otherwise (side outputs on, odd T, ragged N): the same products in the same order, so
    sep, vad and est are bitwise equal with and without the side outputs."""
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    x = torch.from_numpy(synth.make_batch(6, N, 77 + N)[0]).to(DEV)
    plain = h.forward(x)
    aux = h.forward(x, return_aux=True)
    for k in ("sep", "vad", "est"):
        assert torch.equal(plain[k], aux[k]), k


def test_profiler_range_around_forward():
    """SURVEY §5 tracing: a torch.profiler range around the native forward when a profiler is active."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import synth
    net = pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
    sd = synth.make_state_dict(pkg.CONFIG_WITH_VAD, 1234)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.eval().to("cuda")
    x = torch.from_numpy(synth.make_batch(2, 8000, 5)[0]).to("cuda")
    with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        net(x)
    torch.cuda.synchronize()
    assert any(e.name == "sepvad.forward" for e in prof.events())


def test_shortest_input_and_too_short_input(net, state_dicts):
    """torch.stft(center=True, pad_mode="reflect") of the reference (model/model.py:16-25,408) needs N > n_fft / 2 = 256:
    N = 257 (T = 2) is the shortest forward and matches the oracle; N = 256 raises like the reference's own STFT does
    (sepvad_forward returns SEPVAD_E_SHAPE -> RuntimeError) instead of returning anything."""
    from oracle.torch_ref import OracleModel
    om = OracleModel(config_of("with_vad"), state_dicts["with_vad"], torch.float32)
    x = torch.rand(2, 257, generator=torch.Generator().manual_seed(257)) * 1.8 - 0.9
    with torch.no_grad():
        s, v, _ = net(x.to(DEV))
    s_ref, v_ref, _ = om(x)
    assert s.shape == s_ref.shape and v.shape == v_ref.shape
    assert np.abs(s.cpu().numpy() - s_ref.numpy()).max() <= SEP_TOL
    check_vad_labels(v.cpu().numpy(), v_ref.numpy())
    x = x[:, :256].contiguous()
    with pytest.raises(RuntimeError):
        om(x)
    with pytest.raises(RuntimeError), torch.no_grad():
        net(x.to(DEV))
    with torch.no_grad():  # the handle stays usable after the refused call
        s2, _, _ = net(torch.rand(1, 8000, generator=torch.Generator().manual_seed(1)).to(DEV) * 1.8 - 0.9)
    assert torch.isfinite(s2).all()


@pytest.mark.parametrize("B,N", [(64, 32000), (2, 262144)])
def test_late_member_never_gives_up(net, B, N):
    """Member 0 of every group sleeps after its P1 and P3 publishes (SEPVAD_TCN_DELAY), so the other members run ahead
    into the next epochs while it has not yet polled the earlier ones: no hand-off word a late member still polls may
    be overwritten (tcn_kernel.h GW_* layout). No give-up, bitwise the undelayed outputs; G = 4 and G = 33 (cross-XCD)."""
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    x = torch.from_numpy(synth.make_batch(B, N, 515)[0]).to(DEV)
    ref = {k: v.clone() for k, v in h.forward(x).items() if torch.is_tensor(v)}
    os.environ["SEPVAD_TCN_DELAY"] = "4"
    try:
        out = h.forward(x)
        assert h.fused_status()
    finally:
        del os.environ["SEPVAD_TCN_DELAY"]
    for k in ("sep", "vad", "est"):
        assert torch.equal(out[k], ref[k]), k


def test_salt_wrap_restarts_giveup_words(net):
    """SEPVAD_TCN_SALT_MAX=3: the launch salt wraps every third forward. A give-up's salt reused after the wrap must
    neither poison the later forward (the device give-up word restarts from zero) nor hide a later give-up (the host
    copy and the reported value restart too); a give-up pending when the salt wraps is still reported once."""
    g = load_golden("with_vad", "small")
    x = torch.from_numpy(g["x"]).to(DEV)
    h = net.native_handle(DEV)
    s = torch.cuda.Stream()  # a fresh context: salts start at 1 on it

    def fwd(force=False):
        if force:
            os.environ["SEPVAD_TCN_FORCE_GIVEUP"] = "1"
        try:
            with torch.cuda.stream(s):
                return h.forward(x)
        finally:
            os.environ.pop("SEPVAD_TCN_FORCE_GIVEUP", None)

    os.environ["SEPVAD_TCN_SALT_MAX"] = "3"
    try:
        fwd()                      # salt 1
        bad = fwd(force=True)      # salt 2: gives up
        torch.cuda.synchronize()
        assert torch.isnan(bad["sep"]).all()
        with pytest.raises(RuntimeError, match="gave up"):
            fwd()
        fwd()                      # salt 3
        for _ in range(4):         # wrap; salts 1, 2 (the give-up's), 3, wrap, 1: all valid
            out = fwd()
            torch.cuda.synchronize()
            assert not torch.isnan(out["sep"]).any()
            assert np.abs(out["sep"].cpu().numpy() - g["sep"]).max() <= SEP_TOL
        fwd(force=True)            # a give-up just before the next wrap
        raised = 0
        for _ in range(3):
            try:
                fwd()
            except RuntimeError as e:
                assert "gave up" in str(e)
                raised += 1
        assert raised == 1
        torch.cuda.synchronize()
        assert h.fused_status()
    finally:
        del os.environ["SEPVAD_TCN_SALT_MAX"]
        h.release_stream(s.cuda_stream)


def test_concurrent_long_forwards_make_progress(net):
    """Three streams of one handle forwarding B=2 x 60 s files at once (T = 3751: groups of 118 workgroups, more than
    half the chip each): the big persistent launches are ordered across streams (forward.hip tcn_launch_ordered), so none
    waits on a group that can never become resident. No give-up, every output equal to the serial run, fused."""
    from sep_tfanet_vad_amd import synth
    h = net.native_handle(DEV)
    xs = [torch.from_numpy(synth.make_batch(2, 960000, 600 + k)[0]).to(DEV) for k in range(3)]
    ref = []
    for x in xs:
        r = h.forward(x)
        ref.append({k: r[k].clone() for k in ("sep", "vad", "est")})
    assert h.fused_status()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in xs]
    outs = []
    for x, st in zip(xs, streams):
        with torch.cuda.stream(st):
            outs.append(h.forward(x))
    torch.cuda.synchronize()
    assert h.fused_status()
    for o, r in zip(outs, ref):
        for k in ("sep", "vad", "est"):
            assert torch.equal(o[k], r[k]), k
    for st in streams:
        h.release_stream(st.cuda_stream)


def test_two_handles_concurrent_long_forwards(net, state_dicts):
    """Two handles on one device, each forwarding B=2 x 60 s files (groups of 118 workgroups, more than half the chip)
    from its own host thread on its own stream, at once: the big-launch order (forward.hip tcn_launch_ordered) is one
    process-wide critical section (wait on the previous big launch, launch, record), so the two launches never run side
    by side holding partial groups. No give-up; each output equals its serial run."""
    import threading
    from sep_tfanet_vad_amd import synth
    net2 = _net(config_of("with_vad"), state_dicts["with_vad"])
    hs = [net.native_handle(DEV), net2.native_handle(DEV)]
    xs = [torch.from_numpy(synth.make_batch(2, 960000, 620 + k)[0]).to(DEV) for k in range(2)]
    ref = []
    for h, x in zip(hs, xs):
        r = h.forward(x)
        ref.append({k: r[k].clone() for k in ("sep", "vad", "est")})
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in hs]
    outs = [[], []]
    go = threading.Barrier(2)
    errs = []

    def run(i):
        try:
            go.wait()
            with torch.cuda.stream(streams[i]):
                for _ in range(3):
                    outs[i].append(hs[i].forward(xs[i]))
        except Exception as e:  # surfaced below
            errs.append(e)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for h, o, r in zip(hs, outs, ref):
        assert h.fused_status()
        for oo in o:
            for k in ("sep", "vad", "est"):
                assert torch.equal(oo[k], r[k]), k
    for h, st in zip(hs, streams):
        h.release_stream(st.cuda_stream)
