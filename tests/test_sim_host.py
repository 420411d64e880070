"""Host side of the scene simulation (csrc/rir.hip sepvad_rir_jobs_prepare, csrc/sim.hip size query): the job table
of the device generator against the host generator's own prologue. CPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_rir_golden as mk  # noqa: E402


def _jobs_of(case):
    room, src, mics, beta, orient, hp, dim, order, n, mtype = case
    kw = dict(betaCoeffs=beta) if len(beta) == 6 else dict(reverbTime=beta[0])
    return dict(roomMeasures=room, sourcePosition=src, receiverPositions=mics, orientation=orient,
                isHighPassFilter=bool(hp), nDim=dim, nOrder=order, nSamples=n, micType=mtype, **kw)


def _size_query(case, c=340.0, fs=16000.0, n_beta=None):
    from sep_tfanet_vad_amd import native
    room, src, mics, beta, orient, hp, dim, order, n, mtype = case
    lib = native.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (mics, src, room, beta, orient)]
    return lib.sepvad_rir_generate(c, fs, a[0].ctypes.data_as(dp), len(mics), a[1].ctypes.data_as(dp),
                                   a[2].ctypes.data_as(dp), a[3].ctypes.data_as(dp),
                                   len(beta) if n_beta is None else n_beta, a[4].ctypes.data_as(dp), hp, dim, order, n,
                                   mtype.encode(), None, 0)


def test_jobs_prepare_matches_size_query_on_golden_cases():
    from sep_tfanet_vad_amd import rirgen
    g = np.load(os.path.join(GOLDEN, "golden_rir.npz"))
    table, lens = rirgen.prepare_jobs([_jobs_of(c) for c in mk.CASES])
    want = []
    for i, case in enumerate(mk.CASES):
        want += [_size_query(case)] * len(case[2])
        assert _size_query(case) == g[f"h{i}"].shape[1]
    assert lens == want and len(lens) == 6  # case 0 has two microphones; case 3: n_samples = -1 with six betas
    assert mk.CASES[3][8] == -1 and len(mk.CASES[3][3]) == 6
    for t in table:
        L = np.array(t.L[:])
        assert [t.n1, t.n2, t.n3] == [int(np.ceil(t.n_samples / (2 * v))) for v in L]
        assert t.Tw == 128 and t.cTs == 340.0 / 16000.0
    assert table[5].beta[4] == 0 and table[5].beta[5] == 0  # the 2-D case drops floor and ceiling
    assert [t.high_pass for t in table] == [1, 1, 1, 1, 0, 1] and chr(table[4].mic_type) == "c"


def _desc(**over):
    from sep_tfanet_vad_amd import native
    d = native.SepVadRirDesc()
    d.c, d.fs = 340.0, 16000.0
    d.mic[:], d.src[:], d.room[:] = [2.0, 1.5, 1.2], [1.0, 2.0, 1.5], [5.0, 4.0, 3.0]
    d.beta[0] = 0.3
    d.n_beta, d.high_pass, d.n_dim, d.order, d.n_samples, d.mic_type = 1, 1, 3, -1, 600, ord("o")
    for k, v in over.items():
        if isinstance(v, (list, tuple)):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


def _prepare(d):
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    arr = (native.SepVadRirDesc * 1)(d)
    out = (native.SepVadRirJob * 1)()
    return lib.sepvad_rir_jobs_prepare(arr, 1, out), out[0]


@pytest.mark.parametrize("over", [dict(c=0.0), dict(c=-1.0), dict(fs=0.0), dict(n_beta=2), dict(n_beta=0),
                                  dict(n_samples=-2)])
def test_jobs_prepare_rejects_what_the_host_generator_rejects(over):
    d = _desc(**over)
    case = ([5.0, 4.0, 3.0], [1.0, 2.0, 1.5], [[2.0, 1.5, 1.2]], [0.3] * 6, [0.0, 0.0], 1, 3, -1,
            d.n_samples, "o")
    assert _size_query(case, c=d.c, fs=d.fs, n_beta=d.n_beta) == -1  # SEPVAD_E_ARG from the host generator ...
    assert _prepare(d)[0] == -1                      # ... and from the job table


def test_jobs_prepare_accepts_the_plain_job_and_null_arguments_fail():
    from sep_tfanet_vad_amd import native
    rc, job = _prepare(_desc())
    assert rc == 600 and job.n_samples == 600
    lib = native.load_library()
    out = (native.SepVadRirJob * 1)()
    assert lib.sepvad_rir_jobs_prepare(None, 1, out) == -1
    assert lib.sepvad_rir_jobs_prepare((native.SepVadRirDesc * 1)(_desc()), 0, out) == -1


def test_jobs_prepare_image_cap():
    """The largest legal job is a T60 = 1 s response of a 3 x 3 x 2.2 m room at 16 kHz (n = 57, 57, 78)."""
    from sep_tfanet_vad_amd import native
    small = dict(room=[3.0, 3.0, 2.2], src=[1.0, 1.0, 1.0], mic=[2.0, 2.0, 1.2], n_samples=-1)
    rc, job = _prepare(_desc(beta=[1.0, 0, 0, 0, 0, 0], **small))
    assert rc == 16000 and (job.n1, job.n2, job.n3) == (57, 57, 78)
    assert 8 * (2 * job.n1 + 1) * (2 * job.n2 + 1) * (2 * job.n3 + 1) == native.RIR_MAX_IMAGES
    assert _prepare(_desc(beta=[1.01, 0, 0, 0, 0, 0], **small))[0] == -1   # one more lattice plane
    assert _prepare(_desc(fs=96000.0))[0] == -1                             # Tw = 768 > 512


def test_scratch_size_query():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    assert lib.sepvad_rir_scratch_bytes(0, 100) < 0
    assert lib.sepvad_rir_scratch_bytes(1, 0) < 0
    assert lib.sepvad_rir_scratch_bytes(-3, -3) < 0
    assert lib.sepvad_rir_scratch_bytes(7, 2048) >= 0
