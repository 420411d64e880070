"""ctypes binding of ``libsepvad.so`` (C ABI declared in ``include/sepvad.h``).

This is the reference-side binding a Python caller of the boundary needs; ``model.py`` uses it to
keep the reference's ``SeparationModel`` surface. The library is built in-tree by
``__graft_entry__.build()`` (``make -C sep-tfanet-vad_amd/csrc``). There is no fallback: a missing
library, a CPU tensor or a non-zero status raises.
"""
from __future__ import annotations

import ctypes
import os

import torch

# SEPVAD_LIB: an alternative build of the same library (A/B timing of kernel variants, tools/ab.sh)
LIB_PATH = os.environ.get("SEPVAD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsepvad.so")

SEPVAD_LN_PLAIN, SEPVAD_LN_RECURSIVE, SEPVAD_LN_RESIDUAL = 0, 1, 2
SEPVAD_PREC_FP32, SEPVAD_PREC_F16X3, SEPVAD_PREC_F16, SEPVAD_PREC_BF16 = 0, 1, 2, 3
# fp32 / f16x3: fp32-equivalent (parity path); f16 / bf16: reduced-precision arms (tolerance measured)
PRECISIONS = {"fp32": SEPVAD_PREC_FP32, "f16x3": SEPVAD_PREC_F16X3, "f16": SEPVAD_PREC_F16, "bf16": SEPVAD_PREC_BF16}
# storage of the f16x3 weight lo plane in the fused TCN (include/sepvad.h SEPVAD_WLO_*)
WEIGHT_LO = {"e4m3": 0, "f16": 1, "i8": 2}


def build_id() -> str:
    """Source hash the loaded library was built from (sepvad_build_id, include/sepvad.h)."""
    return load_library().sepvad_build_id().decode()


def tree_build_id() -> str:
    """The same hash computed from this tree's sources (buildid.py)."""
    from . import buildid
    return buildid.source_hash()


class SepVadConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_fft", "bn_dim", "h_dim", "layer", "stack", "num_spk", "tf_attention", "ln_mode",
        "final_vad", "final_vad_masked_speakers", "noisy_phase", "activity_input", "precision")]


class SepVadInferKw(ctypes.Structure):
    _fields_ = [("enabled", ctypes.c_int32), ("filter_signals_by_smo_vad", ctypes.c_int32),
                ("filter_signals_by_unsmo_vad", ctypes.c_int32), ("length_smoothing_filter", ctypes.c_int32),
                ("threshold_activated_vad", ctypes.c_float), ("return_smoothed_vad", ctypes.c_int32)]


class SepVadOutputs(ctypes.Structure):
    _fields_ = [("sep", ctypes.c_void_p), ("vad", ctypes.c_void_p), ("est", ctypes.c_void_p),
                ("spectrum", ctypes.c_void_p), ("masks_b", ctypes.c_void_p), ("mask", ctypes.c_void_p)]


class SepVadRirDesc(ctypes.Structure):
    """One microphone's response as the arguments of sepvad_rir_generate (include/sepvad.h)."""
    _fields_ = [("c", ctypes.c_double), ("fs", ctypes.c_double), ("mic", ctypes.c_double * 3),
                ("src", ctypes.c_double * 3), ("room", ctypes.c_double * 3), ("beta", ctypes.c_double * 6),
                ("orientation", ctypes.c_double * 2), ("n_beta", ctypes.c_int32), ("high_pass", ctypes.c_int32),
                ("n_dim", ctypes.c_int32), ("order", ctypes.c_int32), ("n_samples", ctypes.c_int32),
                ("mic_type", ctypes.c_int32)]


class SepVadRirJob(ctypes.Structure):
    """The resolved job table entry the device generator reads (include/sepvad.h)."""
    _fields_ = [("beta", ctypes.c_double * 6), ("s", ctypes.c_double * 3), ("r", ctypes.c_double * 3),
                ("L", ctypes.c_double * 3), ("cTs", ctypes.c_double), ("angle", ctypes.c_double * 2),
                ("hp", ctypes.c_double * 4), ("n_samples", ctypes.c_int32), ("n1", ctypes.c_int32),
                ("n2", ctypes.c_int32), ("n3", ctypes.c_int32), ("Tw", ctypes.c_int32), ("order", ctypes.c_int32),
                ("high_pass", ctypes.c_int32), ("mic_type", ctypes.c_int32)]


RIR_MAX_IMAGES = 16610600  # SEPVAD_RIR_MAX_IMAGES

# The C ABI of include/sepvad.h, in the header's words: name -> (restype, argtypes). tests/test_host.py parses the
# header and compares every return type, argument and struct field with this table and the classes above.
P, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
_i32p, _i64p, _dblp = ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(dbl)
_outs, _kw = ctypes.POINTER(SepVadOutputs), ctypes.POINTER(SepVadInferKw)
_ABI = {
    "sepvad_create": (P, (ctypes.POINTER(SepVadConfig), ctypes.POINTER(P), ctypes.POINTER(ctypes.c_char_p), _i64p, i32,
                          i32)),
    "sepvad_reserve": (i32, (P, i32, i32)),
    "sepvad_set_precision": (i32, (P, i32)),
    "sepvad_set_weight_lo": (i32, (P, i32)),
    "sepvad_e4m3_encode": (i32, (P, P, i64)),
    "sepvad_forward": (i32, (P, P, i32, i32, _outs, _kw, P)),
    "sepvad_forward_strided": (i32, (P, P, i64, i32, i32, _outs, _kw, P)),
    "sepvad_forward_windows": (i32, (P, P, i64, i32, i32, i64, i32, _outs, _kw, P)),
    "sepvad_set_split": (i32, (P, i32)),
    "sepvad_set_fused": (i32, (P, i32)),
    "sepvad_fused_status": (i32, (P, _i32p)),
    "sepvad_side_outputs": (i32, (P, _outs, P)),
    "sepvad_last_forward": (i32, (P, P, _i64p, _i32p, _i32p)),
    "sepvad_side_outputs_of": (i32, (P, _outs, P, i64, i32, i32)),
    "sepvad_tcn_clock": (i32, (P, P, i32, _i32p)),
    "sepvad_release_stream": (i32, (P, P)),
    "sepvad_stft_gate_test": (i32, (P, P, i32, i32, P, P, P)),
    "sepvad_istft_pair_test": (i32, (P, P, P, i32, i32, P, P, P)),
    "sepvad_set_tcn_dump": (i32, (P, P)),
    "sepvad_pit_l1": (i32, (P, i64, P, i64, i32, i64, P, P, P, P, P)),
    "sepvad_pit_l1_sums": (i32, (P, i64, P, i64, i32, i64, P, P, P)),
    "sepvad_pit_l1_choose": (i32, (P, dbl, i32, P, P, P, P)),
    "sepvad_stream_append": (i32, (P, i64, i64, i32, i64, P, P, i64, i64, P)),
    "sepvad_ring_push": (i32, (P, i64, i32, i64, P, i64, i64, P)),
    "sepvad_pit_l1_rows_scratch_bytes": (i64, (i32, i64)),
    "sepvad_pit_l1_rows": (i32, (P, i64, P, i64, i32, i64, P, i64, P, P, P, P)),
    "sepvad_live_stitch": (i32, (P, i64, i64, i32, i64, P, P, i64, i64, P, i64, i64, P, i32, i32, P, i64, i64, P)),
    "sepvad_si_sdr": (i32, (P, i64, P, i64, i64, i32, P, P, i32, P, P)),
    "sepvad_snr": (i32, (P, i64, P, i64, i64, i32, P, P, i32, P, P)),
    "sepvad_stoi_filter": (i32, (i32, P, i32, P)),
    "sepvad_stoi_scratch_bytes": (i64, (i32, i64, i32)),
    "sepvad_stoi": (i32, (P, i64, P, i64, i64, i32, P, P, i32, P, i64, P, P, P)),
    "sepvad_stoi_ex_scratch_bytes": (i64, (i32, i64, i32, i32)),
    "sepvad_stoi_ex": (i32, (P, i64, P, i64, i64, i32, P, P, i32, P, i64, i32, P, P, P, P)),
    "sepvad_vad_accuracy": (i32, (P, P, i32, i32, i32, i32, P, P)),
    "sepvad_eval_scratch_bytes": (i64, (i32, i64)),
    "sepvad_eval_separation": (i32, (P, i64, P, i64, P, i64, i32, i64, i32, i32, i32, dbl, P, i64, P, P, P, P, P, P)),
    "sepvad_eval_vad": (i32, (P, P, i32, P, P, i32, i32, P, P, P, P, P, P, P)),
    "sepvad_criterion_coef": (i32, (P, i64, P, i64, i32, i64, i32, i32, i32, dbl, P, i64, P, P, P)),
    "sepvad_criterion_backward": (i32, (i32, P, i64, P, i64, i64, P, P, P, i64, P, P, P, i32, P, P, P)),
    "sepvad_tail_scratch_bytes": (i64, (i32, i32)),
    "sepvad_tail_forward": (i32, (P, P, i64, P, i32, i32, P, i64, P, P, P)),
    "sepvad_tail_backward": (i32, (P, P, i64, P, i32, i32, P, i64, i64, i64, P, i64, i64, i64, P, P, i64, P, P, P)),
    "sepvad_head_scratch_bytes": (i64, (i32, i32)),
    "sepvad_head_forward": (i32, (P, i32, i32, P, P, i64, P, P)),
    "sepvad_head_backward": (i32, (P, P, i64, i64, i64, i32, i32, P, P, i64, P, P, P)),
    "sepvad_stream_eval_scratch_bytes": (i64, (i32, i32, i64, i64, i32)),
    "sepvad_stream_eval": (i32, (P, i64, i32, i32, i32, i32, i64, i64, P, i64, i32, i32, i32, i32, dbl, P, i64, P, i64,
                                 P, P, P, P, P, P, i64, P)),
    "sepvad_rir_generate": (i32, (dbl, dbl, _dblp, i32, _dblp, _dblp, _dblp, i32, _dblp, i32, i32, i32, i32,
                                  ctypes.c_char, _dblp, i64)),
    "sepvad_rir_jobs_prepare": (i32, (ctypes.POINTER(SepVadRirDesc), i32, ctypes.POINTER(SepVadRirJob))),
    "sepvad_rir_scratch_bytes": (i64, (i32, i64)),
    "sepvad_rir_generate_device": (i32, (P, i32, P, i64, P, i64, P)),
    "sepvad_fir_convolve": (i32, (P, i64, i64, P, i64, i32, P, P, P, i32, i64, P, i64, P)),
    "sepvad_scene_mix": (i32, (P, i32, i32, i64, P, P, i32, dbl, dbl, P, P, P)),
    "sepvad_scene_targets": (i32, (P, i32, i32, i64, i32, dbl, dbl, P, P, P)),
    "sepvad_vad_frame_labels": (i32, (P, i64, i32, i64, i32, P, P)),
    "sepvad_resample_filter": (i32, (i32, i32, P, i32, P)),
    "sepvad_resample": (i32, (P, i64, P, P, P, i64, P)),
    "sepvad_normalize": (i32, (P, i64, P, P, P)),
    "sepvad_set_timing": (i32, (P, i32)),
    "sepvad_timing": (i32, (P, _dblp, _i32p, _dblp)),
    "sepvad_destroy": (None, (P,)),
    "sepvad_last_error": (ctypes.c_char_p, ()),
    "sepvad_abi_version": (i32, ()),
    "sepvad_build_id": (ctypes.c_char_p, ()),
}
EXPORTED_SYMBOLS = tuple(_ABI)

_lib = None

# SEPVAD_CHECK=1: synchronise after every forward and raise if its fused TCN hand-offs gave up. Without it
# a give-up (which needs the chip to be shared with work that starves the launch's groups for ~1 s) is
# reported by the next forward on the same stream, or by Handle.fused_status().
CHECK_EACH_FORWARD = os.environ.get("SEPVAD_CHECK", "0") not in ("", "0")


def load_library(path: str = LIB_PATH):
    """Load libsepvad.so (after torch, so it binds to torch's HIP runtime) and declare signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"libsepvad.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; "
                           f"g.build()'` or `make -C sep-tfanet-vad_amd/csrc`")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _ABI.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = _lib.sepvad_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


_check, _ptr = check, ptr  # the names older callers use


# ---- glue between torch tensors and the entries: every wrapper module takes these from here ----------------------
def stream_ptr(device):
    """The current stream of `device` as the entries' hipStream_t argument."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_scratch = {}  # (device, stream) -> uint8 scratch, most recently used last


def scratch(device, nbytes):
    """At least nbytes of scratch for the current stream on `device` (one buffer per stream: concurrent streams never
    share it). The entries consume their scratch within their own stream-ordered launches, so PIT, evaluation and STOI
    share it; a caller that reads it across two entries keeps the returned tensor (eval_separation's "scratch")."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _scratch.pop(key, None)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        while len(_scratch) >= 32:  # bounded: drop the least recently used stream's scratch (its blocks return
            _scratch.pop(next(iter(_scratch)))  # to that stream's allocator pool, reused only in its order)
    _scratch[key] = buf
    return buf


def scratch_bytes(query, *args):
    """The answer of the host size query `query` (a sepvad_*_scratch_bytes name of _ABI), or the error of its status."""
    nbytes = getattr(load_library(), query)(*args)
    if nbytes < 0:
        check(nbytes, query)
    return nbytes


def scratch_for(query, device, *args):
    """(the current stream's scratch on `device`, nbytes) for an entry whose size query `query` answers nbytes."""
    nbytes = scratch_bytes(query, *args)
    return scratch(device, nbytes), nbytes


def frame_major_masks(masks_b, device=None):
    """Pre-sigmoid masks [B, 514, T] or [B, 2, 257, T] as the forward keeps them: frame-major, zero-padded [B, Tp, 576]"""
    B, T = masks_b.shape[0], masks_b.shape[-1]
    mf = torch.zeros(B, (T + 63) // 64 * 64, 576, device=device or masks_b.device, dtype=torch.float32)
    mf[:, :T, :514] = masks_b.to(mf.device, torch.float32).reshape(B, 514, T).transpose(1, 2)
    return mf


def rows3(t):
    """[B, 2, N] float32 with unit sample stride, speaker stride ld >= N and batch stride 2 ld -> (tensor, ld).
    One shape and one stride query: this runs for every window of the streaming wrappers."""
    shape = t.shape
    if len(shape) != 3 or shape[1] != 2:
        raise ValueError(f"expected [B, 2, L], got {tuple(shape)}")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    s0, s1, s2 = t.stride()
    if s2 != 1 or s1 < shape[2] or (shape[0] > 1 and s0 != 2 * s1):
        t = t.contiguous()
        s1 = t.stride(1)
    return t, s1


def rows2(t):
    """[B, N] float32 with unit sample stride and row stride ld >= N -> (tensor, ld)."""
    B, N = t.shape
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    s0, s1 = t.stride()
    if s1 != 1 or (B > 1 and s0 < N):
        t = t.contiguous()
        s0 = t.stride(0)
    return t, (s0 if B > 1 else N)


def require_device(what, first, *rest):
    if first.device.type != "cuda":
        raise RuntimeError(f"{what}: inputs must be ROCm device tensors")
    for t in rest:
        if t is not None and t.device != first.device:
            raise RuntimeError(f"{what}: inputs must be on one ROCm device")
    return first.device


def make_config(cfg: dict, precision: str = "f16x3") -> SepVadConfig:
    c = SepVadConfig()
    c.n_fft, c.bn_dim, c.h_dim = cfg["n_fftBins"], cfg["BN_dim"], cfg["H_dim"]
    c.layer, c.stack, c.num_spk = cfg["layer"], cfg["stack"], cfg["num_spk"]
    c.tf_attention = int(bool(cfg["tf_attention"]))
    c.ln_mode = (SEPVAD_LN_RECURSIVE if cfg["apply_recursive_ln"] else
                 SEPVAD_LN_RESIDUAL if cfg["apply_residual_ln"] else SEPVAD_LN_PLAIN)
    c.final_vad = int(bool(cfg["final_vad"]))
    c.final_vad_masked_speakers = int(bool(cfg["final_vad_masked_speakers"]))
    c.noisy_phase = int(bool(cfg["noisy_phase"]))
    c.activity_input = int(bool(cfg["activity_input_bool"]))
    c.precision = PRECISIONS[precision]
    return c


def make_kw(inference_kw) -> SepVadInferKw | None:
    """inference_kw dict -> struct (None or {} == the reference's skipped branch, model/model.py:444)."""
    if not inference_kw:
        return None
    k = SepVadInferKw()
    k.enabled = 1
    # the reference indexes these keys directly (KeyError if absent) — keep that behaviour
    k.filter_signals_by_smo_vad = int(bool(inference_kw["filter_signals_by_smo_vad"]))
    k.filter_signals_by_unsmo_vad = int(bool(inference_kw["filter_signals_by_unsmo_vad"]))
    k.length_smoothing_filter = int(inference_kw["length_smoothing_filter"])
    k.threshold_activated_vad = float(inference_kw["threshold_activated_vad"])
    k.return_smoothed_vad = int(bool(inference_kw["return_smoothed_vad"]))
    return k


class Handle:
    """Owns one ``sepvad_handle`` (device weights + workspace) for one device."""

    def __init__(self, cfg: dict, state_dict: dict, device, precision: str = "f16x3"):
        lib = load_library()
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("libsepvad needs a ROCm device")
        self.device = device
        self.index = device.index if device.index is not None else torch.cuda.current_device()
        self.cfg = dict(cfg)
        host = [(k, v.detach().to("cpu", torch.float32).contiguous()) for k, v in state_dict.items()
                if torch.is_floating_point(v)]
        n = len(host)
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for _, t in host])
        names = (ctypes.c_char_p * n)(*[k.encode() for k, _ in host])
        numels = (ctypes.c_int64 * n)(*[t.numel() for _, t in host])
        self._c = make_config(cfg, precision)
        self.precision = precision
        h = lib.sepvad_create(ctypes.byref(self._c), ptrs, names, numels, n, self.index)
        if not h:
            raise RuntimeError("sepvad_create failed: " + lib.sepvad_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(h)
        self._lib = lib

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.sepvad_destroy(h)
            self._h = None

    @property
    def raw(self):
        return self._h

    def reserve(self, B: int, N: int):
        _check(self._lib.sepvad_reserve(self._h, B, N), "sepvad_reserve")

    def set_precision(self, precision: str):
        _check(self._lib.sepvad_set_precision(self._h, PRECISIONS[precision]), "sepvad_set_precision")
        self.precision = precision

    def set_weight_lo(self, mode: str):
        """Weight lo plane of the fused TCN's f16x3 GEMMs: "i8" (default) / "e4m3" (3 B per weight) or "f16"."""
        if mode not in WEIGHT_LO:
            raise ValueError(f"unknown weight lo-plane format {mode!r} (expected one of {sorted(WEIGHT_LO)})")
        _check(self._lib.sepvad_set_weight_lo(self._h, WEIGHT_LO[mode]), "sepvad_set_weight_lo")
        self.weight_lo = mode

    def set_split(self, nsplit: int):
        """Concurrent utterance chunks per forward (1..4; bitwise-identical results)."""
        _check(self._lib.sepvad_set_split(self._h, int(nsplit)), "sepvad_set_split")

    def set_fused(self, on: bool):
        """TCN schedule of later forwards: one persistent launch (default) or one launch per stage."""
        _check(self._lib.sepvad_set_fused(self._h, int(bool(on))), "sepvad_set_fused")

    def fused_status(self) -> bool:
        """Synchronise; True if the last forward ran the fused TCN. Raises if its hand-offs gave up."""
        used = ctypes.c_int32(0)
        _check(self._lib.sepvad_fused_status(self._h, ctypes.byref(used)), "sepvad_fused_status")
        return bool(used.value)

    def fused_slices(self) -> int:
        """Synchronise; the 32-frame slices per workgroup of the last forward's fused TCN (1 or 2; 0 = not fused).
        Raises if its hand-offs gave up."""
        used = ctypes.c_int32(0)
        _check(self._lib.sepvad_fused_status(self._h, ctypes.byref(used)), "sepvad_fused_status")
        return int(used.value)

    def set_timing(self, on: bool):
        _check(self._lib.sepvad_set_timing(self._h, int(on)), "sepvad_set_timing")

    def timing(self):
        ms = (ctypes.c_double * 2)()
        cnt = (ctypes.c_int32 * 2)()
        tot = ctypes.c_double()
        _check(self._lib.sepvad_timing(self._h, ms, cnt, ctypes.byref(tot)), "sepvad_timing")
        return dict(gemm_ms=ms[0], res_out_ms=ms[1], gemm_launches=cnt[0], res_out_launches=cnt[1], total_ms=tot.value)

    def _stream(self):
        return stream_ptr(self.device)

    @property
    def has_vad(self):
        """Whether the forward produces a VAD track (model/model.py:424-427)."""
        return bool(self.cfg["final_vad"]) and (not self.cfg["final_vad_masked_speakers"] or self.cfg["noisy_phase"])

    def forward(self, x: torch.Tensor, inference_kw=None, return_aux: bool = False, outputs: dict | None = None):
        """One forward. Returns dict(sep, vad, est[, spectrum, masks_b, mask_per_speaker])."""
        if x.device.type != "cuda":
            raise RuntimeError("sepvad forward: input must be a ROCm device tensor")
        x = x.to(self.device, torch.float32)
        if x.stride(-1) != 1 or x.stride(0) < x.shape[-1]:
            x = x.contiguous()
        B, N = x.shape
        ldx = x.stride(0) if B > 1 else N  # strided row views (streaming windows) need no copy
        T = 1 + N // (self.cfg["n_fftBins"] // 2)
        F = self.cfg["n_fftBins"] // 2 + 1
        S = self.cfg["num_spk"]
        dev = self.device
        o = outputs or {}
        sep = o.get("sep") if o.get("sep") is not None else torch.empty(B, S, N, device=dev, dtype=torch.float32)
        vad = (o.get("vad") if o.get("vad") is not None else torch.empty(B, S, T, device=dev, dtype=torch.float32)) \
            if self.has_vad else None
        est = o.get("est") if o.get("est") is not None else torch.empty(B, S, F, T, device=dev, dtype=torch.complex64)
        spectrum = masks_b = mask = None
        if return_aux:
            spectrum = torch.empty(B, F, T, device=dev, dtype=torch.float32)
            masks_b = torch.empty(B, S * F, T, device=dev, dtype=torch.float32)
            mask = torch.empty(B, S, F, T, device=dev, dtype=torch.float32)
        outs = SepVadOutputs(_ptr(sep).value, _ptr(vad).value, _ptr(est).value, _ptr(spectrum).value,
                             _ptr(masks_b).value, _ptr(mask).value)
        kw = make_kw(inference_kw)
        stream = self._stream()
        rc = self._lib.sepvad_forward_strided(self._h, _ptr(x), ldx, B, N, ctypes.byref(outs),
                                              ctypes.byref(kw) if kw is not None else None, stream)
        _check(rc, "sepvad_forward")
        if CHECK_EACH_FORWARD:
            self.fused_status()  # synchronises; raises if this forward's fused TCN gave up
        if vad is None:
            vad_ret = 0  # model/model.py:427
        elif kw is not None and kw.return_smoothed_vad:
            vad_ret = vad.view(B, S, 1, T)  # model/model.py:456-457
        else:
            vad_ret = vad
        seq = ctypes.c_int64()
        lb, ln = ctypes.c_int32(), ctypes.c_int32()
        _check(self._lib.sepvad_last_forward(self._h, stream, ctypes.byref(seq), ctypes.byref(lb), ctypes.byref(ln)),
               "sepvad_last_forward")
        res = dict(sep=sep, vad=vad_ret, est=est, stream=stream.value or 0, B=B, T=T, N=N, seq=seq.value)
        if return_aux:
            res.update(spectrum=spectrum, masks_b=masks_b, mask_per_speaker=mask)
        return res

    def forward_windows(self, x: torch.Tensor, n_win: int, hop: int, N: int, inference_kw=None,
                        return_vad: bool = False):
        """Every streaming window in ONE forward (sepvad_forward_windows): window k of row b of x [B, L]
        starts at sample k * hop; returns sep [n_win, B, num_spk, N] (window-major). No est is produced.
        return_vad: (sep, vad) with vad [n_win, B, num_spk, T] (the smoothed labels with return_smoothed_vad), or
        None when the configuration has no VAD output."""
        if x.device.type != "cuda" or x.dtype != torch.float32 or x.stride(-1) != 1:
            raise RuntimeError("forward_windows: x must be a float32 ROCm tensor with unit sample stride")
        B = x.shape[0]
        S = self.cfg["num_spk"]
        T = 1 + N // (self.cfg["n_fftBins"] // 2)
        sep = torch.empty(n_win, B, S, N, device=self.device, dtype=torch.float32)
        vad = torch.empty(n_win * B, S, T, device=self.device, dtype=torch.float32) if self.has_vad else None
        outs = SepVadOutputs(_ptr(sep).value, _ptr(vad).value, 0, 0, 0, 0)
        kw = make_kw(inference_kw)
        ld = x.stride(0) if B > 1 else x.shape[1]
        _check(self._lib.sepvad_forward_windows(self._h, _ptr(x), ld, B, n_win, hop, N, ctypes.byref(outs),
                                                ctypes.byref(kw) if kw is not None else None, self._stream()),
               "sepvad_forward_windows")
        if CHECK_EACH_FORWARD:
            self.fused_status()
        if return_vad:
            return sep, (vad.view(n_win, B, S, T) if vad is not None else None)
        return sep

    def side_outputs(self, stream: int, B: int, T: int, want=("spectrum", "masks_b", "mask_per_speaker"),
                     seq: int | None = None, N: int | None = None):
        """The side attributes of forward `seq` (shape B x N) on `stream` (sepvad_side_outputs_of), materialised
        now on that stream: dict with the requested subset of spectrum [B,257,T], masks_b [B,514,T] and
        mask_per_speaker [B,2,257,T]. Raises RuntimeError if a later forward on that stream replaced its workspace
        (nothing is written then). Without seq: the last forward on the stream (sepvad_side_outputs).
        The tensors are safe to use on the caller's current stream (it waits for the copies)."""
        F = self.cfg["n_fftBins"] // 2 + 1
        S = self.cfg["num_spk"]
        cur = torch.cuda.current_stream(self.device)
        fwd = torch.cuda.ExternalStream(stream, device=self.device) if cur.cuda_stream != stream else cur
        res = {}
        with torch.cuda.stream(fwd):
            dev = self.device
            if "spectrum" in want:
                res["spectrum"] = torch.empty(B, F, T, device=dev, dtype=torch.float32)
            if "masks_b" in want:
                res["masks_b"] = torch.empty(B, S * F, T, device=dev, dtype=torch.float32)
            if "mask_per_speaker" in want:
                res["mask_per_speaker"] = torch.empty(B, S, F, T, device=dev, dtype=torch.float32)
            outs = SepVadOutputs(0, 0, 0, _ptr(res.get("spectrum")).value, _ptr(res.get("masks_b")).value,
                                 _ptr(res.get("mask_per_speaker")).value)
            if seq is None:
                rc = self._lib.sepvad_side_outputs(self._h, ctypes.byref(outs), ctypes.c_void_p(stream))
            else:
                rc = self._lib.sepvad_side_outputs_of(self._h, ctypes.byref(outs), ctypes.c_void_p(stream), seq, B, N)
            _check(rc, "sepvad_side_outputs")
        if fwd is not cur:  # the caller's stream waits for the copies; the allocator keeps the blocks until then
            cur.wait_stream(fwd)
            for t in res.values():
                t.record_stream(cur)
        return res

    def release_stream(self, stream: int | None = None):
        """Free the per-stream context (workspace, hand-off words) the handle keeps for `stream` (default: the
        current stream) after synchronising it (sepvad_release_stream)."""
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(self._lib.sepvad_release_stream(self._h, ctypes.c_void_p(stream)), "sepvad_release_stream")

    def tcn_clock(self, max_records: int = 4096):
        """Per-launch k_tcn clock records (diagnostics; needs SEPVAD_TCN_CLOCK=1 when the forwards ran):
        numpy [n, 3] of (launch span us, workgroup 0 span us, workgroup 0 shader clock MHz), oldest first."""
        import numpy as np
        buf = (ctypes.c_uint64 * (8 * max_records))()
        n = ctypes.c_int32(0)
        _check(self._lib.sepvad_tcn_clock(self._h, buf, max_records, ctypes.byref(n)), "sepvad_tcn_clock")
        k = min(n.value, max_records)
        u = np.frombuffer(buf, dtype=np.uint64, count=8 * k).reshape(k, 8)
        span = (u[:, 1] - ~u[:, 0]).astype(np.float64) / 100.0  # the min start is stored as a max of complements
        r = u.astype(np.float64)
        w0 = (r[:, 3] - r[:, 2]) / 100.0
        mhz = (r[:, 5] - r[:, 4]) / np.maximum(w0, 1e-9)
        return np.stack([span, w0, mhz], axis=1)

    def tcn_dump(self, x: torch.Tensor):
        """Block-level parity probe (sepvad_set_tcn_dump): one forward of x with the fused TCN, returning
        (tcn_in, blk0_res, blk0_att) as [B, 256, T] like the reference module outputs."""
        B, N = x.shape
        T = 1 + N // 256
        Tp = (T + 63) // 64 * 64
        buf = torch.zeros(3, B, Tp, 256, device=self.device, dtype=torch.float32)
        _check(self._lib.sepvad_set_tcn_dump(self._h, _ptr(buf)), "sepvad_set_tcn_dump")
        try:
            self.forward(x)
            if not self.fused_status():
                raise RuntimeError("tcn_dump: the fused TCN did not run")
        finally:
            _check(self._lib.sepvad_set_tcn_dump(self._h, None), "sepvad_set_tcn_dump")
        v = buf[:, :, :T, :].permute(0, 1, 3, 2)
        return v[0], v[1], v[2]

    def stft_fused(self, x: torch.Tensor):
        """The forward's own front end (k_stft_gate, sepvad_stft_gate_test): (X [B, 257, T] complex64 with DC
        zeroed, its dB spectrum [B, 257, T]) from the frame-major workspace layout."""
        x = x.to(self.device, torch.float32).contiguous()
        B, N = x.shape
        T = 1 + N // 256
        Tp = (T + 63) // 64 * 64
        X = torch.zeros(B, Tp, 257, device=self.device, dtype=torch.complex64)
        db = torch.zeros(B, Tp, 260, device=self.device, dtype=torch.float32)
        _check(self._lib.sepvad_stft_gate_test(self._h, _ptr(x), B, N, _ptr(X), _ptr(db), self._stream()),
               "sepvad_stft_gate_test")
        return X[:, :T].transpose(1, 2), db[:, :T, :257].transpose(1, 2)

    def istft_pair(self, X: torch.Tensor, masks: torch.Tensor, N: int):
        """The forward's own back end (k_istft_pair, sepvad_istft_pair_test): for X [B, 257, T] complex and
        pre-sigmoid masks [B, 2, 257, T], est = X sigmoid(masks) [B, 2, 257, T] and y = istft(est, length=N)
        [B, 2, N]."""
        B, F, T = X.shape
        Tp = (T + 63) // 64 * 64
        Xf = torch.zeros(B, Tp, 257, device=self.device, dtype=torch.complex64)
        Xf[:, :T] = X.to(self.device, torch.complex64).transpose(1, 2)
        mf = frame_major_masks(masks, self.device)
        y = torch.empty(B, 2, N, device=self.device, dtype=torch.float32)
        est = torch.empty(B, 2, 257, T, device=self.device, dtype=torch.complex64)
        _check(self._lib.sepvad_istft_pair_test(self._h, _ptr(Xf), _ptr(mf), B, N, _ptr(y), _ptr(est), self._stream()),
               "sepvad_istft_pair_test")
        return y, est
