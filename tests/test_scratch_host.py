"""The scratch of every entry that takes one (no GPU): the value of every size query on a table of shapes, the
workspace's size through the stand-alone program tools/scratch_check.cpp, and the full text of both scratch refusals
of each entry.

Every expected number was recorded from the library of the commit before csrc/scratch_plan.h existed, when each family
still wrote its own offsets; the workspace's from that commit's ws_reserve with its size pass lifted out unchanged. They
pin the layouts: a change of any of them changes what callers must allocate. The refusal texts are that commit's too.
sepvad_tail_forward and sepvad_tail_backward read their handle before they look at the scratch, and a handle needs a
device: their refusals are in tests/test_gpu_tail_grad.py."""
import ctypes
import os
import subprocess

import pytest
import torch

import stream_eval_cases as sc
from conftest import REPO

E_ARG = -1

HEAD = {(1, 2): 1072384, (1, 64): 1262848, (3, 65): 3795456, (1, 127): 1456384, (1, 128): 1459456, (1, 129): 2515456,
        (16, 126): 23237888, (3, 300): 12291072, (32767, 2): 35099224064, (1, 1 << 20): 11863859968}
TAIL = {(1, 257): 266240, (1, 3840): 266240, (3, 4096): 797696, (1, 8191): 266240, (1, 8193): 266240,
        (2, 32000): 1063424, (32767, 257): 8711303680}
# (R, N, fs_sig): classic, then modes 1, 2, 3 of the extended query; at 10 kHz the resampled-signal array is empty
STOI = {(1, 1000, 16000): (6656, 6656, 6912, 6912), (3, 30000, 8000): (1120768, 1120768, 1121024, 1121024),
        (2, 30000, 10000): (118016, 118016, 118272, 118272)}
# the cases of stream_eval_cases.CASES as one chunk of all K windows, B = 2: name -> (K, W, H, bytes per mode)
STREAM_EVAL = {"rem": (4, 48000, 16000, (12544, 30784, 14080)), "short": (3, 48000, 16000, (9408, 27200, 10560)),
               "half": (8, 48000, 8000, (25088, 50496, 32768))}
EVAL = {(2, 100): 320, (1, 4096): 160, (1, 4097): 288}
PIT_ROWS = {(9, 45440): 1728}
WS = {(1, 257): 822528, (3, 8292): 2465536, (64, 32000): 105104640, (1, 2100000): 105860352}   # (B, N)


@pytest.fixture(scope="module")
def lib():
    from sep_tfanet_vad_amd import native
    return native.load_library()


def test_size_queries(lib):
    for (B, T), want in HEAD.items():
        assert lib.sepvad_head_scratch_bytes(B, T) == want, ("head", B, T)
    for (B, N), want in TAIL.items():
        assert lib.sepvad_tail_scratch_bytes(B, N) == want, ("tail", B, N)
    for (R, N, fs), (classic, *ex) in STOI.items():
        assert lib.sepvad_stoi_scratch_bytes(R, N, fs) == classic, ("stoi", R, N, fs)
        assert [lib.sepvad_stoi_ex_scratch_bytes(R, N, fs, m) for m in (1, 2, 3)] == ex, ("stoi_ex", R, N, fs)
    for (B, N), want in EVAL.items():
        assert lib.sepvad_eval_scratch_bytes(B, N) == want, ("eval", B, N)
    for (B, L), want in PIT_ROWS.items():
        assert lib.sepvad_pit_l1_rows_scratch_bytes(B, L) == want, ("pit rows", B, L)


def test_stream_eval_size_query(lib):
    assert {c[0] for c in sc.CASES} == set(STREAM_EVAL)
    for name, N, save_sec, _seed in sc.CASES:
        K, W, H, want = STREAM_EVAL[name]
        assert sc.pad_signals(torch.zeros(2, N), torch.zeros(2, 2, N), save_sec)[2:5] == (K, W, H)
        got = tuple(lib.sepvad_stream_eval_scratch_bytes(2, K, W, H, sc.MODE_ID[m]) for m in sc.MODES)
        assert got == want, name


def test_workspace_bytes_and_the_planner():
    """tools/scratch_check.cpp: ws_bytes on the pinned shapes, the planner's rules, and the smallest workspace bound
    into a host block and written end to end."""
    csrc = os.path.join(REPO, "sep-tfanet-vad_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "ARCH=gfx950", "scratch_check"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "\nok\n" in r.stdout  # (after the sizes: every check passed)
    got = {(int(b), int(n)): int(v) for _, b, n, v in
           (ln.split() for ln in r.stdout.splitlines() if ln.startswith("ws_bytes "))}
    assert got == WS


# ---- the two scratch refusals of each entry: one byte too small, then 8 bytes off the alignment ----------------------
ONE = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before any device call


def refused(lib, rc, text):
    assert rc == E_ARG and lib.sepvad_last_error().decode() == text


def both(lib, entry, query, need, align, call):
    """call(scratch, nbytes) -> status; scratch aligned to 4096 unless the case moves it."""
    assert need > 0
    refused(lib, call(ONE, need - 1), f"{entry}: scratch too small ({query})")
    refused(lib, call(ctypes.c_void_p(4096 + 8), need), f"{entry}: scratch must be {align}-byte aligned")


def test_head_refusals(lib):
    need = lib.sepvad_head_scratch_bytes(3, 65)
    both(lib, "sepvad_head_forward", "sepvad_head_scratch_bytes", need, 256,
         lambda s, n: lib.sepvad_head_forward(ONE, 3, 65, ONE, s, n, ONE, None))
    both(lib, "sepvad_head_backward", "sepvad_head_scratch_bytes", need, 256,
         lambda s, n: lib.sepvad_head_backward(ONE, ONE, 0, 0, 0, 3, 65, ONE, s, n, ONE, ONE, None))
    refused(lib, lib.sepvad_head_forward(ONE, 3, 65, ONE, None, 1 << 40, ONE, None),
            "sepvad_head_forward: scratch too small (sepvad_head_scratch_bytes)")


@pytest.mark.parametrize("fs", (16000, 10000))
def test_stoi_refusals(lib, fs):
    R, N = 2, 30000
    need = lib.sepvad_stoi_scratch_bytes(R, N, fs)
    both(lib, "sepvad_stoi", "sepvad_stoi_scratch_bytes", need, 256,
         lambda s, n: lib.sepvad_stoi(ONE, N, ONE, N, N, R, None, None, fs, s, n, ONE, None, None))
    for modes in (1, 2, 3):
        need = lib.sepvad_stoi_ex_scratch_bytes(R, N, fs, modes)
        both(lib, "sepvad_stoi_ex", "sepvad_stoi_ex_scratch_bytes", need, 256,
             lambda s, n: lib.sepvad_stoi_ex(ONE, N, ONE, N, N, R, None, None, fs, s, n, modes, ONE, ONE, None, None))


def test_stoi_refuses_before_any_device_call(lib):
    """sepvad_stoi's other refusals, in its words and its order: every one comes before the design is uploaded."""
    def call(X=ONE, x_ld=1000, Y=ONE, y_ld=1000, N=1000, R=1, fs=16000, scratch=ONE, nbytes=1 << 24, out=ONE):
        return lib.sepvad_stoi(X, x_ld, Y, y_ld, N, R, None, None, fs, scratch, nbytes, out, None, None)

    for bad in (dict(X=None), dict(Y=None), dict(out=None), dict(scratch=None), dict(N=0), dict(x_ld=999), dict(y_ld=999),
                dict(out=None, fs=44100), dict(scratch=None, R=0)):
        refused(lib, call(**bad), "sepvad_stoi: bad arguments")
    refused(lib, call(fs=44100, R=0, nbytes=0), "sepvad_stoi: fs_sig must be 8000, 10000 or 16000")
    for bad in (dict(R=0), dict(R=65536), dict(N=409, x_ld=409, y_ld=409), dict(R=0, nbytes=0)):
        refused(lib, call(**bad), "sepvad_stoi: need 1 <= R <= 65535 and more than 256 samples at 10 kHz")
    refused(lib, call(nbytes=0, scratch=ctypes.c_void_p(4104)), "sepvad_stoi: scratch too small (sepvad_stoi_scratch_bytes)")


def both8(lib, entry, query, need, call):
    """As `both` for the entries that ask for 8-byte alignment: 8 bytes off is still aligned, 4 bytes off is not."""
    refused(lib, call(ONE, need - 1), f"{entry}: scratch too small ({query})")
    assert call(ctypes.c_void_p(4096 + 8), need - 1) == E_ARG  # (refused for its size first)
    refused(lib, call(ctypes.c_void_p(4096 + 4), need), f"{entry}: scratch must be 8-byte aligned")


def test_eval_family_refusals(lib):
    B, N = 2, 4097
    need = lib.sepvad_eval_scratch_bytes(B, N)
    both8(lib, "sepvad_eval_separation", "sepvad_eval_scratch_bytes", need,
          lambda s, n: lib.sepvad_eval_separation(ONE, N, ONE, N, ONE, N, B, N, 0, 1, 1, 1e-8, s, n, ONE, ONE, ONE, ONE, ONE,
                                                  None))
    both8(lib, "sepvad_criterion_coef", "sepvad_eval_scratch_bytes", need,
          lambda s, n: lib.sepvad_criterion_coef(ONE, N, ONE, N, B, N, 0, 1, 1, 1e-8, s, n, ONE, ONE, None))


@pytest.mark.parametrize("mode", sc.MODES)
def test_stream_eval_refusals(lib, mode):
    B, K, W, H = 3, 5, 1000, 250
    m = sc.MODE_ID[mode]
    need = lib.sepvad_stream_eval_scratch_bytes(B, 2, W, H, m)
    both8(lib, "sepvad_stream_eval", "sepvad_stream_eval_scratch_bytes", need,
          lambda s, n: lib.sepvad_stream_eval(ONE, W, 2, 0, K, B, W, H, ONE, (K - 1) * H + W, m, 0, 1, 1, 1e-8, ONE, K * H,
                                              ONE, K * H, ONE, ONE, ONE, ONE, ONE, s, n, None))


def test_pit_rows_refusal(lib):
    B, L = 9, 45440
    need = lib.sepvad_pit_l1_rows_scratch_bytes(B, L)
    refused(lib, lib.sepvad_pit_l1_rows(ONE, L, ONE, L, B, L, ONE, need - 1, ONE, ONE, None, None),
            "sepvad_pit_l1_rows: scratch too small (sepvad_pit_l1_rows_scratch_bytes)")  # (it asks for no alignment)
