"""Reverberant scene simulation on the device: the data side of the reference
(``create_data/create_simulation_data.py``) over the C-ABI entries of csrc/sim.hip.

``simulate_scenes`` chains image-method responses (``sepvad_rir_generate_device``), the truncated convolution
(``sepvad_fir_convolve``), mixing at an SNR with min-max normalisation (``sepvad_scene_mix``), the targets
(``sepvad_scene_targets``) and, optionally, frame-level VAD labels (``sepvad_vad_frame_labels``). After the job
table upload nothing returns to the host; every call is ordered on the current stream. There is no fallback: a CPU
tensor or a non-zero status raises."""
from __future__ import annotations

import torch

from . import native as _native
from . import rirgen as _rirgen


def _need(t, dtype, what):
    if t.device.type != "cuda" or t.dtype != dtype:
        raise RuntimeError(f"{what} must be a {dtype} ROCm tensor")
    return t.contiguous()


def fir_convolve(x, h, L, klen=None, xidx=None, hidx=None):
    """``np.convolve(x[xidx[r]], h[hidx[r]][:klen])[:L]`` per row: x [., Nx] float32, h [., K] float64, klen int32
    per h row, index tensors int32 (identity when None). Returns y [R, L] float64."""
    x = _need(x, torch.float32, "fir_convolve: x")
    h = _need(h, torch.float64, "fir_convolve: h")
    R = int(xidx.numel() if xidx is not None else hidx.numel() if hidx is not None else x.shape[0])
    if xidx is None and hidx is None and h.shape[0] != x.shape[0]:
        raise ValueError("fir_convolve: x and h need the same number of rows without index tensors")
    for t, n in ((klen, "klen"), (xidx, "xidx"), (hidx, "hidx")):
        if t is not None:
            _need(t, torch.int32, "fir_convolve: " + n)
    y = torch.empty(R, int(L), device=x.device, dtype=torch.float64)
    lib = _native.load_library()
    _native.check(lib.sepvad_fir_convolve(_native.ptr(x), x.shape[1], x.shape[1], _native.ptr(h), h.shape[1],
                                           h.shape[1], _native.ptr(klen), _native.ptr(xidx), _native.ptr(hidx), R,
                                           int(L), _native.ptr(y), int(L), _native.stream_ptr(x.device)),
                  "sepvad_fir_convolve")
    return y


def scene_mix(rev, noise=None, snr_db=None, a=1.8, b=0.9, power_mode=0):
    """rev [B, S, L] float64 -> (mix [B, L] float32, stats [B, 4] float64 = gain, min, max, a / (max - min))."""
    rev = _need(rev, torch.float64, "scene_mix: rev")
    B, S, L = rev.shape
    if (noise is None) != (snr_db is None):
        raise ValueError("scene_mix: noise and snr_db go together")
    if noise is not None:
        noise = _need(noise, torch.float32, "scene_mix: noise")
        snr_db = _need(torch.as_tensor(snr_db, dtype=torch.float64).to(rev.device), torch.float64, "scene_mix: snr_db")
        if noise.shape != (B, L) or snr_db.shape != (B,):
            raise ValueError("scene_mix: noise must be [B, L] and snr_db [B]")
    mix = torch.empty(B, L, device=rev.device, dtype=torch.float32)
    stats = torch.empty(B, 4, device=rev.device, dtype=torch.float64)
    lib = _native.load_library()
    _native.check(lib.sepvad_scene_mix(_native.ptr(rev), B, S, L, _native.ptr(noise), _native.ptr(snr_db),
                                        int(power_mode), float(a), float(b), _native.ptr(mix), _native.ptr(stats),
                                        _native.stream_ptr(rev.device)), "sepvad_scene_mix")
    return mix, stats


def scene_targets(dry, stats=None, mode=1, a=1.8, b=0.9):
    """dry [B, S, L] float64 -> float32 targets: mode 0 each row's own min-max, mode 1 the mixture's scale."""
    dry = _need(dry, torch.float64, "scene_targets: dry")
    B, S, L = dry.shape
    if stats is not None:
        stats = _need(stats, torch.float64, "scene_targets: stats")
    out = torch.empty(B, S, L, device=dry.device, dtype=torch.float32)
    lib = _native.load_library()
    _native.check(lib.sepvad_scene_targets(_native.ptr(dry), B, S, L, int(mode), float(a), float(b),
                                            _native.ptr(stats), _native.ptr(out), _native.stream_ptr(dry.device)),
                   "sepvad_scene_targets")
    return out


def vad_frame_labels(act, edge_mode=0):
    """act [..., L] uint8 sample-level activity (values 0..8, L a multiple of 512) -> [..., 2 L / 512 + 1] float32."""
    act = _need(act, torch.uint8, "vad_frame_labels: act")
    L = act.shape[-1]
    rows = act.reshape(-1, L)
    T = 2 * L // 512 + 1
    out = torch.empty(rows.shape[0], T, device=act.device, dtype=torch.float32)
    lib = _native.load_library()
    _native.check(lib.sepvad_vad_frame_labels(_native.ptr(rows), L, rows.shape[0], L, int(edge_mode),
                                               _native.ptr(out), _native.stream_ptr(act.device)),
                  "sepvad_vad_frame_labels")
    return out.reshape(*act.shape[:-1], T)


def simulate_scenes(sources, rir_jobs, dry_jobs, noise=None, snr_db=None, a=1.8, b=0.9, target_mode=1, activity=None,
                    power_mode=0, edge_mode=0):
    """B scenes of S sources each. sources [B, S, L] float32 (device); rir_jobs / dry_jobs: B * S ``generateRir``
    keyword dicts each (scene-major, one receiver per job) for the reverberant and the target (direct-path)
    responses; noise [B, L] float32 with snr_db [B] (optional); activity [B, S, L] uint8 (optional).

    Returns (mix [B, L] f32, targets [B, S, L] f32, stats [B, 4] f64, vad_frames [B, S, 2 L / 512 + 1] f32 or None),
    all on the device."""
    sources = _need(sources, torch.float32, "simulate_scenes: sources")
    B, S, L = sources.shape
    if len(rir_jobs) != B * S or len(dry_jobs) != B * S:
        raise ValueError("simulate_scenes: need B * S reverberant and B * S target jobs")
    h, klen = _rirgen.generateRirBatch(list(rir_jobs) + list(dry_jobs), device=sources.device)
    if h.shape[0] != 2 * B * S:
        raise ValueError("simulate_scenes: every job must have one receiver")
    xidx = (torch.arange(2 * B * S, device=sources.device, dtype=torch.int32) % (B * S)).contiguous()
    y = fir_convolve(sources.reshape(B * S, L), h, L, klen=klen, xidx=xidx)
    rev, dry = y[:B * S].view(B, S, L), y[B * S:].view(B, S, L)
    mix, stats = scene_mix(rev, noise, snr_db, a, b, power_mode)
    targets = scene_targets(dry, stats, target_mode, a, b)
    frames = vad_frame_labels(activity, edge_mode) if activity is not None else None
    return mix, targets, stats, frames
