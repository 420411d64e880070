"""Live streaming sessions: the algorithm of ``OnlineSaving.calc_online`` (reference
``model/online_class_unknown_targets.py:72-105``) fed a chunk at a time.

``calc_online`` needs the whole recording and emits nothing until every window has run. ``LiveSeparator.push``
takes the next samples of ``n_streams`` live streams and returns what they complete: the separated audio of every
window that became complete (its last hop, reordered to the speakers already emitted), the VAD track of those hops
and the permutations used.

* the input history is a mirrored ring on the device (``sepvad_ring_push``): the windows that are ready are read in
  place by ``sepvad_forward_windows`` (row stride 2R, no gather copy), several in one forward when a push completes
  several;
* the stitched signal is not kept: only its last ``win - hop`` samples are, in a second mirrored ring, which is all
  the next window's PIT reads (``_slice_bounds`` clamping of ``calc_online``, ``online.py``);
* ``per_stream=True`` matches every stream's speakers on its own (``sepvad_pit_l1_rows``): each stream gets what the
  reference computes for a batch of that one stream. ``per_stream=False`` keeps the reference's batch-global choice
  (``sepvad_pit_l1``; ``nn.L1Loss`` reduces over the batch) and reproduces ``calc_online`` of the whole batch bit for
  bit, for any chunking;
* one ``sepvad_live_stitch`` launch per window writes the output chunk, the tail ring and the VAD frames.

Every device buffer that outlives a push (both rings, the PIT scratch, the forward's workspace through
``sepvad_reserve``) is allocated by the constructor; ``push`` is stream-ordered and never synchronises the host.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import native as _native
from . import pit as _pit
from .online import MAX_WINDOW_UTTS, _slice_bounds

VAD_HOP = 256  # samples per VAD frame (n_fftBins / 2, model/model.py:378)
_OFFSET_CHECK_WINDOWS = 1 << 16  # window offsets verified at construction (3 h of 160 ms hops); later ones as they run


def window_offset(fs: int, k: int, save_sec: float) -> int:
    """First sample of window k: the reference's float expression (get_truncated_signal, :39-41)."""
    return int(np.floor(fs * k * save_sec))


def windows_complete(samples_received: int, win: int, hop: int) -> int:
    """Windows [k * hop, k * hop + win) that lie inside the first samples_received samples."""
    return 0 if samples_received < win else (samples_received - win) // hop + 1


def ring_size(win: int, hop: int, max_pending: int) -> int:
    """Input ring length R: max_pending windows hop apart fit in one contiguous span."""
    return win + max_pending * hop


def push_room(samples_received: int, windows_done: int, hop: int, R: int) -> int:
    """Samples the ring can take before it would overwrite the first sample of the next window to run."""
    return R - (samples_received - windows_done * hop)


def ready_windows(samples_received: int, windows_done: int, win: int, hop: int, R: int, cap: int):
    """(m, start): the next m <= cap windows that are complete and not yet run, and the ring index of the first
    one's first sample (the span start .. start + (m - 1) * hop + win is contiguous in the mirrored ring)."""
    m = min(cap, windows_complete(samples_received, win, hop) - windows_done)
    return max(0, m), (windows_done * hop) % R


class LiveSeparator:
    def __init__(self, model, n_streams: int, save_sec: float = 0.16, max_len: int = 3, fs: int = 16000,
                 per_stream: bool = True, inference_kw=None, max_pending: int = 8):
        if not hasattr(model, "native_handle"):
            raise TypeError("LiveSeparator needs the native SeparationModel")
        if n_streams < 1 or max_pending < 1:
            raise ValueError("LiveSeparator: n_streams and max_pending must be >= 1")
        self.model = model
        self.n_streams = int(n_streams)
        self.save_sec, self.max_len, self.fs = save_sec, max_len, fs
        self.per_stream = bool(per_stream)
        self.inference_kw = dict(inference_kw) if inference_kw else None
        self.win = int(fs * max_len)
        self.hop = int(np.floor(fs * save_sec))
        if not 1 <= self.hop < self.win:
            raise ValueError(f"LiveSeparator: save_sec {save_sec} gives a hop of {self.hop} samples; need 1 <= hop < "
                             f"{self.win}")
        k = np.arange(_OFFSET_CHECK_WINDOWS, dtype=np.int64)
        bad = np.nonzero(np.floor(fs * k * save_sec).astype(np.int64) != k * self.hop)[0]
        if bad.size:  # the condition of OnlineSaving._batched_ok: windows hop apart, read in place
            raise ValueError(f"LiveSeparator: save_sec {save_sec}: window {int(bad[0])} starts at sample "
                             f"{window_offset(fs, int(bad[0]), save_sec)}, not at {int(bad[0])} * {self.hop}")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("LiveSeparator: the model must be on a ROCm device")
        self._h = model.native_handle(dev)
        self.device = self._h.device
        self._lib = _native.load_library()
        B = self.n_streams
        # windows per forward: max_pending, and OnlineSaving's bound on the workspace (max_window_utts)
        self.max_pending = max(1, min(int(max_pending), MAX_WINDOW_UTTS // B))
        self.R = ring_size(self.win, self.hop, self.max_pending)
        self.Rt = max(self.win - self.hop, self.hop)  # stitched tail: the PIT reads at most win - hop samples
        cfg = self._h.cfg
        self.T = 1 + self.win // (cfg["n_fftBins"] // 2)
        # window k contributes the frames centred on the multiples of 256 inside its emitted hop: its last hop / 256
        # frames when the hop is a multiple of 256 and the window is not (frame T - 1 = floor(win / 256) is then
        # centred before the window's end; a window of a whole number of frames has that frame centred ON its end,
        # in the next hop, and gets no VAD track)
        tiles = self.hop % VAD_HOP == 0 and self.win % VAD_HOP != 0
        self.vad_frames = self.hop // VAD_HOP if self._h.has_vad and tiles else 0
        self._ring = torch.empty(B, 2 * self.R, dtype=torch.float32, device=self.device)
        self._tail = torch.empty(B, 2, 2 * self.Rt, dtype=torch.float32, device=self.device)
        nbytes = 0
        if self.per_stream:
            nbytes = _native.scratch_bytes("sepvad_pit_l1_rows_scratch_bytes", B, self.win - self.hop)
        self._scratch = torch.empty(max(nbytes, _pit.PIT_SCRATCH_BYTES) // 8, dtype=torch.float64, device=self.device)
        self._h.reserve(B * self.max_pending, self.win)
        self.reset()

    def reset(self):
        """Start a new session (the rings are rewritten before they are read)."""
        self.samples_received = 0
        self.windows_done = 0

    # -- one window of the sequential chain: PIT against the stitched tail, then the stitch -------------------------
    def _match_and_stitch(self, pred, vad, perm, loss, out, vad_out, j, stream):
        B, win, hop, Rt = self.n_streams, self.win, self.hop, self.Rt
        k = self.windows_done
        P = _native.ptr
        filled = k * hop
        n_on = hop if k == 0 else filled                      # calc_online: window 0 meets its own last hop
        pb, pe = _slice_bounds(win, -hop - n_on, -hop)        # reference :87
        ob, oe = _slice_bounds(n_on, -win + hop, None)        # reference :88
        L = pe - pb
        assert L == oe - ob and 1 <= L <= Rt
        est = ctypes.c_void_p(pred.data_ptr() + 4 * pb)
        if k == 0:
            ref, ref_ld = ctypes.c_void_p(pred.data_ptr() + 4 * (win - hop + ob)), win
        else:  # stitched samples [filled - L, filled): contiguous in the mirrored tail
            ref, ref_ld = ctypes.c_void_p(self._tail.data_ptr() + 4 * ((filled - L) % Rt)), 2 * Rt
        if self.per_stream:
            rc = self._lib.sepvad_pit_l1_rows(est, win, ref, ref_ld, B, L, P(self._scratch),
                                              self._scratch.numel() * 8, P(perm), P(loss), None, stream)
            _native.check(rc, "sepvad_pit_l1_rows")
        else:
            rc = self._lib.sepvad_pit_l1(est, win, ref, ref_ld, B, L, P(self._scratch), P(perm), P(loss), None, stream)
            _native.check(rc, "sepvad_pit_l1")
        nf = self.vad_frames
        rc = self._lib.sepvad_live_stitch(P(pred), win, win, B, hop, P(perm), P(out), out.stride(1), j * hop,
                                          P(self._tail), Rt, filled % Rt,
                                          P(vad) if nf else None, self.T, nf,
                                          P(vad_out) if nf else None, vad_out.stride(1) if nf else 0, j * nf, stream)
        _native.check(rc, "sepvad_live_stitch")

    def push(self, chunk: torch.Tensor):
        """chunk [n_streams, n] float32 on the device, any n >= 1 -> (sep [n_streams, 2, m * hop], vad
        [n_streams, 2, m * hop / 256] or None, perm [m, n_streams, 2] int64) for the m >= 0 windows completed."""
        if not isinstance(chunk, torch.Tensor) or chunk.device.type != "cuda":
            raise RuntimeError("LiveSeparator.push: chunk must be on a ROCm device")
        if chunk.dim() != 2 or chunk.shape[0] != self.n_streams:
            raise ValueError(f"LiveSeparator.push: expected [{self.n_streams}, n], got {tuple(chunk.shape)}")
        if chunk.shape[1] < 1:
            raise ValueError("LiveSeparator.push: empty chunk")
        if chunk.device != self.device:
            raise RuntimeError(f"LiveSeparator.push: chunk is on {chunk.device}, the session on {self.device}")
        if chunk.dtype != torch.float32 or chunk.stride(1) != 1 or chunk.stride(0) < chunk.shape[1]:
            chunk = chunk.to(torch.float32).contiguous()
        B, win, hop, R = self.n_streams, self.win, self.hop, self.R
        n = chunk.shape[1]
        m_total = windows_complete(self.samples_received + n, win, hop) - self.windows_done
        dev = self.device
        nf = self.vad_frames
        out = torch.empty(B, 2, m_total * hop, dtype=torch.float32, device=dev)
        vad_out = torch.empty(B, 2, m_total * nf, dtype=torch.float32, device=dev) if nf else None
        perm = torch.empty(m_total, B, 2, dtype=torch.int64, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        stream = _native.stream_ptr(dev)
        ld = chunk.stride(0) if B > 1 else n
        done = j = 0
        while done < n:
            take = min(n - done, push_room(self.samples_received, self.windows_done, hop, R))
            rc = self._lib.sepvad_ring_push(ctypes.c_void_p(chunk.data_ptr() + 4 * done), ld, B, take,
                                            _native.ptr(self._ring), R, self.samples_received % R, stream)
            _native.check(rc, "sepvad_ring_push")
            self.samples_received += take
            done += take
            while True:
                m, start = ready_windows(self.samples_received, self.windows_done, win, hop, R, self.max_pending)
                if m == 0:
                    break
                for q in range(m):  # the reference's float offsets, verified beyond the constructor's range too
                    if window_offset(self.fs, self.windows_done + q, self.save_sec) != (self.windows_done + q) * hop:
                        raise RuntimeError(f"LiveSeparator: window {self.windows_done + q} does not start at a "
                                           f"multiple of the hop for save_sec {self.save_sec}")
                x = self._ring[:, start: start + (m - 1) * hop + win]
                with torch.no_grad():
                    sep_w, vad_w = self._h.forward_windows(x, m, hop, win, self.inference_kw, return_vad=True)
                for q in range(m):
                    self._match_and_stitch(sep_w[q], vad_w[q] if nf else None, perm[j], loss, out, vad_out, j, stream)
                    self.windows_done += 1
                    j += 1
        assert j == m_total
        return out, vad_out, perm
