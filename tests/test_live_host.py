"""Live streaming sessions, host side (no GPU): the scratch-size query, the argument checks of the three new C-ABI
entries (each refuses before anything is launched) and the pure-Python window schedule of live.py."""
import ctypes

import numpy as np
import pytest

E_ARG = -1  # SEPVAD_E_ARG
FAKE = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    from sep_tfanet_vad_amd import native
    return native.load_library()


def _refused(lib, rc, text):
    assert rc == E_ARG
    assert text in lib.sepvad_last_error().decode()


def test_pit_rows_scratch_bytes(lib):
    """B rows x the blocks sepvad_pit_l1 gives ONE row (min(512, max(1, ceil(L / 8192)))) x 4 doubles."""
    q = lib.sepvad_pit_l1_rows_scratch_bytes
    for B, L, nblk in ((1, 1, 1), (9, 3000, 1), (9, 8192, 1), (9, 8193, 2), (9, 45440, 6), (256, 45440, 6),
                       (3, 512 * 8192, 512), (3, 10 ** 9, 512)):
        assert q(B, L) == B * nblk * 32
    for B, L in ((0, 100), (-1, 100), (3, 0), (3, -5), (65536, 100)):
        assert q(B, L) < 0
        assert "sepvad_pit_l1_rows_scratch_bytes" in lib.sepvad_last_error().decode()


def test_ring_push_refuses_bad_arguments(lib):
    f = lib.sepvad_ring_push
    _refused(lib, f(None, 10, 3, 10, FAKE, 1000, 0, None), "null")
    _refused(lib, f(FAKE, 10, 3, 10, None, 1000, 0, None), "null")
    _refused(lib, f(FAKE, 10, 0, 10, FAKE, 1000, 0, None), "rows")
    _refused(lib, f(FAKE, 10, 3, 0, FAKE, 1000, 0, None), "n <= R")
    _refused(lib, f(FAKE, 1001, 3, 1001, FAKE, 1000, 0, None), "n <= R")       # n > R
    _refused(lib, f(FAKE, 10, 3, 10, FAKE, 1000, 1000, None), "pos")           # pos >= R
    _refused(lib, f(FAKE, 10, 3, 10, FAKE, 1000, -1, None), "pos")
    _refused(lib, f(FAKE, 9, 3, 10, FAKE, 1000, 0, None), "chunk_ld")


def test_pit_rows_refuses_bad_arguments(lib):
    f = lib.sepvad_pit_l1_rows
    ok = dict(est=FAKE, est_ld=3000, ref=FAKE, ref_ld=3000, B=9, L=3000, scratch=FAKE, nbytes=9 * 32)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["est"], a["est_ld"], a["ref"], a["ref_ld"], a["B"], a["L"], a["scratch"], a["nbytes"],
                 None, None, None, None)
    _refused(lib, call(est=None), "null")
    _refused(lib, call(ref=None), "null")
    _refused(lib, call(scratch=None), "null")
    _refused(lib, call(B=0), "B")
    _refused(lib, call(L=0), "L >= 1")
    _refused(lib, call(est_ld=2999), "row strides")
    _refused(lib, call(nbytes=9 * 32 - 1), "scratch too small")
    _refused(lib, call(L=45440, est_ld=45440, ref_ld=45440, nbytes=9 * 5 * 32), "scratch too small")


def test_live_stitch_refuses_bad_arguments(lib):
    f = lib.sepvad_live_stitch
    ok = dict(win=FAKE, win_ld=48000, N=48000, B=3, H=2560, perm=None, out=FAKE, out_ld=2560, d0=0, tail=FAKE,
              Rt=45440, tpos=0, vad=None, T=188, nf=0, vad_out=None, vad_ld=0, v0=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok], None)
    _refused(lib, call(win=None), "null")
    _refused(lib, call(out=None), "null")
    _refused(lib, call(tail=None), "null")
    _refused(lib, call(H=2560, Rt=2559), "H must be <= Rt")                      # H > Rt
    _refused(lib, call(H=0), "H")
    _refused(lib, call(H=48001, Rt=50000, out_ld=50000), "H <= N")
    _refused(lib, call(tpos=45440), "tpos")
    _refused(lib, call(d0=1), "d0")
    _refused(lib, call(d0=-1), "d0")
    _refused(lib, call(vad=FAKE, nf=10, vad_ld=10), "vad_out")
    _refused(lib, call(vad=FAKE, vad_out=FAKE, nf=189, vad_ld=200), "nf")       # nf > T
    _refused(lib, call(vad=FAKE, vad_out=FAKE, nf=10, vad_ld=10, v0=1), "v0")


@pytest.mark.parametrize("save_sec, n_total", [(0.16, 64000), (0.5, 56000), (1.0, 80000)])
def test_window_schedule(save_sec, n_total):
    """Fed sample counts in irregular steps, the schedule runs every window exactly once, in order, as soon as it is
    complete; each batch of windows is one contiguous span of the mirrored ring that holds exactly the samples
    [k * hop, k * hop + win) (checked on a numpy ring of sample indices); the total equals OnlineSaving.n_windows."""
    from sep_tfanet_vad_amd import live
    from sep_tfanet_vad_amd.online import OnlineSaving
    fs, win = 16000, 48000
    hop = int(np.floor(fs * save_sec))
    ons = OnlineSaving(None, "/nonexistent")
    ons.save_sec = save_sec
    for cap in (1, 3, 8):
        R = live.ring_size(win, hop, cap)
        ring = np.full(2 * R, -1, np.int64)
        S = done = 0
        steps = [1, 999, 2560, 7001, R + 5000, 47999, 160, 2560, 2560, 1]
        while S < n_total:
            n = min(steps[0], n_total - S)
            steps = steps[1:] + steps[:1]
            fed = 0
            while fed < n:
                take = min(n - fed, live.push_room(S, done, hop, R))
                assert 1 <= take <= R
                idx = (S + np.arange(take)) % R
                ring[idx] = ring[idx + R] = S + np.arange(take)
                S += take
                fed += take
                while True:
                    m, start = live.ready_windows(S, done, win, hop, R, cap)
                    if m == 0:
                        break
                    assert 1 <= m <= cap and 0 <= start < R and start + (m - 1) * hop + win <= 2 * R
                    for q in range(m):
                        k = done + q
                        assert live.window_offset(fs, k, save_sec) == k * hop
                        assert k * hop + win <= S                      # complete ...
                        span = ring[start + q * hop: start + q * hop + win]
                        assert np.array_equal(span, k * hop + np.arange(win))
                    done += m
                assert done == live.windows_complete(S, win, hop)      # ... and run as soon as it is
            if S >= win:
                assert done == ons.n_windows(S)
        assert done == ons.n_windows(n_total) == {0.16: 7, 0.5: 2, 1.0: 3}[save_sec]


def test_offsets_that_are_not_multiples_of_the_hop():
    """The condition LiveSeparator's constructor refuses: floor(fs * k * save_sec) != k * hop for some k."""
    from sep_tfanet_vad_amd import live
    hop = int(np.floor(16000 * 0.16001))
    assert hop == 2560 and live.window_offset(16000, 7, 0.16001) == 17921 != 7 * hop
