"""``pyrirgen.generateRir`` mirror (reference ``create_data/pyrirgen.pyx``) over the C-ABI image-method
generator ``sepvad_rir_generate`` (csrc/rir.hip; restates ``create_data/rirgen.cpp:115-351``).

Same keyword surface and errors: exactly one of ``reverbTime`` / ``betaCoeffs``; a single receiver
position (not a list of positions) returns one response; ``soundVelocity`` and ``fs`` pass through a C
``float`` in the reference's Cython signature, which is reproduced (``np.float32`` rounding)."""
from __future__ import annotations

import ctypes
from collections.abc import Iterable

import numpy as np

from . import native as _native


def generateRir(roomMeasures, sourcePosition, receiverPositions, *, reverbTime=None, betaCoeffs=None,  # noqa: N802,N803
                soundVelocity=340, fs=16000, orientation=(0.0, 0.0), isHighPassFilter=True, nDim=3,  # noqa: N803
                nOrder=-1, nSamples=-1, micType="o"):  # noqa: N803
    if not (reverbTime is None) != (betaCoeffs is None):
        raise ValueError("You provide either reverbTime or betaCoeffs.")
    beta = [reverbTime] if betaCoeffs is None else list(betaCoeffs)
    multiple = all(isinstance(e, Iterable) for e in receiverPositions)
    mics = np.ascontiguousarray(receiverPositions if multiple else [receiverPositions], dtype=np.float64)
    src = np.ascontiguousarray(sourcePosition, dtype=np.float64)
    room = np.ascontiguousarray(roomMeasures, dtype=np.float64)
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    orient = np.ascontiguousarray(orientation, dtype=np.float64)
    c, f = float(np.float32(soundVelocity)), float(np.float32(fs))
    lib = _native.load_library()
    dp = ctypes.POINTER(ctypes.c_double)

    def call(out, cap):
        return lib.sepvad_rir_generate(c, f, mics.ctypes.data_as(dp), len(mics), src.ctypes.data_as(dp),
                                       room.ctypes.data_as(dp), beta.ctypes.data_as(dp), len(beta),
                                       orient.ctypes.data_as(dp), int(bool(isHighPassFilter)), int(nDim),
                                       int(nOrder), int(nSamples), micType[0].encode(), out, cap)

    n = call(None, 0)
    if n < 0:
        raise RuntimeError(f"sepvad_rir_generate failed (status {n})")
    h = np.zeros((len(mics), n), dtype=np.float64)
    n2 = call(h.ctypes.data_as(dp), h.size)
    if n2 != n:
        raise RuntimeError(f"sepvad_rir_generate failed (status {n2})")
    return h.tolist() if multiple else h[0].tolist()


def prepare_jobs(jobs):
    """Resolve a list of ``generateRir`` keyword dicts (``roomMeasures``, ``sourcePosition``, ``receiverPositions``
    and its keywords) into the device generator's job table (``sepvad_rir_jobs_prepare``, host): one row per
    receiver. Returns (ctypes array of ``SepVadRirJob``, lengths list)."""
    desc = []
    for kw in jobs:
        kw = dict(kw)
        room, src, recv = kw.pop("roomMeasures"), kw.pop("sourcePosition"), kw.pop("receiverPositions")
        rt, bc = kw.pop("reverbTime", None), kw.pop("betaCoeffs", None)
        if not (rt is None) != (bc is None):
            raise ValueError("You provide either reverbTime or betaCoeffs.")
        beta = [rt] if bc is None else list(bc)
        if len(beta) not in (1, 6):
            raise ValueError("betaCoeffs needs six values")
        c = float(np.float32(kw.pop("soundVelocity", 340)))
        fs = float(np.float32(kw.pop("fs", 16000)))
        orient = kw.pop("orientation", (0.0, 0.0))
        hp, dim = kw.pop("isHighPassFilter", True), kw.pop("nDim", 3)
        order, n, mtype = kw.pop("nOrder", -1), kw.pop("nSamples", -1), kw.pop("micType", "o")
        if kw:
            raise TypeError(f"generateRirBatch: unknown keyword(s) {sorted(kw)}")
        multiple = all(isinstance(e, Iterable) for e in recv)
        for mic in (recv if multiple else [recv]):
            d = _native.SepVadRirDesc()
            d.c, d.fs = c, fs
            d.mic[:], d.src[:], d.room[:] = [float(v) for v in mic], [float(v) for v in src], [float(v) for v in room]
            for i, v in enumerate(beta):
                d.beta[i] = float(v)
            d.orientation[:] = [float(orient[0]), float(orient[1])]
            d.n_beta, d.high_pass, d.n_dim = len(beta), int(bool(hp)), int(dim)
            d.order, d.n_samples, d.mic_type = int(order), int(n), ord(mtype[0])
            desc.append(d)
    if not desc:
        raise ValueError("generateRirBatch: no jobs")
    lib = _native.load_library()
    darr = (_native.SepVadRirDesc * len(desc))(*desc)
    table = (_native.SepVadRirJob * len(desc))()
    rc = lib.sepvad_rir_jobs_prepare(darr, len(desc), table)
    if rc < 0:
        raise RuntimeError(f"sepvad_rir_jobs_prepare failed (status {rc}): bad arguments, or a job above the image "
                           f"cap of {_native.RIR_MAX_IMAGES}")
    return table, [t.n_samples for t in table]


def generateRirBatch(jobs, device="cuda", ld=None):  # noqa: N802
    """``generateRir`` for a batch on the device (``sepvad_rir_generate_device``, csrc/sim.hip): ``jobs`` is a list
    of keyword dicts with ``generateRir``'s arguments by name; a job with several receivers expands to one row per
    receiver. Returns (h [J, max n] float64 device tensor, rows zero beyond their length; lengths int32 device
    tensor [J]). Stream-ordered on the current stream; the only host work is the job table and its upload."""
    import torch
    table, lens = prepare_jobs(jobs)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("generateRirBatch needs a ROCm device")
    J = len(lens)
    ld = max(max(lens), 1) if ld is None else int(ld)
    raw = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8)
    with torch.cuda.device(device):
        tab = raw.to(device)
        h = torch.empty(J, ld, device=device, dtype=torch.float64)
        lib = _native.load_library()
        if lib.sepvad_rir_scratch_bytes(J, ld) < 0:
            raise RuntimeError("sepvad_rir_scratch_bytes failed")
        _native.check(lib.sepvad_rir_generate_device(_native.ptr(tab), J, _native.ptr(h), ld, None, 0,
                                                      _native.stream_ptr(device)),
                       "sepvad_rir_generate_device")
        klen = torch.tensor(lens, dtype=torch.int32).to(device)
    return h, klen
