"""The scoring kernels outside the 7 dB, unit-scale regime of the other tests: k_si_sdr / k_snr (csrc/metrics.hip) and
k_eval_moments / k_eval_finish (csrc/eval.hip) on the regime grid of score_cases.py (DC of 0 .. 1000 standard
deviations, residuals of 8 .. 78 dB, N = 32 000 and 2 000 000, amplitudes 1e-4 .. 3000, identical and all-zero rows,
one to five samples), every number against the float64 two-pass truth at TOL_DB = 1e-3 dB, no cell looser.

Both kernels evaluate closed forms of double moments; on raw rows that loses (mean^2 / variance) (signal / residual)
of the moments' precision. They now take the moments of the rows less their first sample (and k_si_sdr adds 16
samples' terms on their own before they join a thread's running sum). Worst |device - truth| in dB on an MI355X,
before (the raw-moment kernels under these tests) and after; "metric" is calc_sisdr and signal_noise_ratio with both
zero_mean values, "pairwise" PairwiseNegSDR of the three kinds with both, "sheet" score_batch's sheet, min_loss and
means. Cells not listed are below 1e-4 dB before and 2e-5 dB after (float32 rounding of the stored result: 7.6e-6 dB
above 64 dB):

    cell                       SI-SDR   before: metric pairwise    sheet   after: metric pairwise    sheet
    N32000-dc100-nl0.001        57.9 dB          1.4e-04  1.7e-05  1.8e-05         1.4e-06  1.9e-06  3.0e-06
    N32000-dc100-nl0.0001       71.4 dB          3.1e-03  1.4e-03  1.1e-03         2.8e-06  3.8e-06  3.7e-06
    N32000-dc1000-nl0.01        38.1 dB          1.6e-04  2.3e-05  2.1e-05         1.8e-06  3.6e-06  2.5e-06
    N32000-dc1000-nl0.001       57.8 dB          1.7e-02  1.1e-03  1.1e-03         1.8e-06  3.2e-06  5.5e-06
    N32000-dc1000-nl0.0001      71.3 dB          3.5e-01  1.2e-01  7.8e-02         1.9e-06  1.9e-06  3.8e-06
    N2000000-dc10-nl0.0001      77.8 dB          1.5e-03  1.1e-04  9.9e-05         1.8e-06  3.0e-06  1.8e-06
    N2000000-dc100-nl0.001      58.1 dB          1.5e-03  1.5e-04  1.5e-04         1.8e-06  3.8e-06  1.5e-06
    N2000000-dc100-nl0.0001     77.8 dB          1.4e-01  1.1e-02  1.1e-02         2.9e-06  1.7e-06  2.9e-06
    N2000000-dc1000-nl0.01      38.1 dB          1.5e-03  5.2e-05  5.1e-05         2.1e-06  3.7e-06  1.9e-06
    N2000000-dc1000-nl0.001     58.1 dB          1.5e-01  8.2e-04  8.2e-04         1.9e-06  3.3e-06  1.9e-06
    N2000000-dc1000-nl0.0001    77.3 dB          5.8e+00  1.1e+00  1.1e+00         3.3e-06  3.4e-06  3.9e-06

The sheet's SI-SDR / SNR columns and the separate sepvad_si_sdr / sepvad_snr calls add the same terms in different
orders (one workgroup per row against one per 4096 samples), so they are held to 1e-5 dB, not to the bit. Measured:
the float32 values were the same in every cell after the change (up to 6.9 dB apart before). sepvad_si_sdr / sepvad_snr give the same bits for rows 1, 2 and 3 floats past 16-byte alignment,
for gathered rows and for aligned contiguous copies (the scalar path now gives each thread the float4 path's samples).
"""
import ctypes

import pytest
import torch

import score_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_DB = sc.TOL_DB          # the project's gate (test_gpu_metrics.py, test_gpu_eval.py)
CROSS_DB = 1e-5             # the sheet against the separate metric entries


def dev(a):
    return torch.tensor(a, device=DEV)


def err(got, ref):
    return float((got.double().cpu() - torch.as_tensor(ref).double().cpu()).abs().max())


def device_numbers(est, tgt, mix, zm_false=True):
    """Every number of score_cases.truth from the device, under the same keys (float32 device tensors)."""
    from sep_tfanet_vad_amd import evaluate, metrics, sdr
    out = {}
    for zm in (True, False) if zm_false else (True,):
        out["si", zm] = metrics.calc_sisdr(est, tgt, zero_mean=zm)
        out["snr", zm] = metrics.signal_noise_ratio(est, tgt, zero_mean=zm)
        for ty in sc.SDR_TYPES:
            out["pw", ty, zm] = sdr.PairwiseNegSDR(ty, zero_mean=zm)(est, tgt)
    r = evaluate.score_batch(est, tgt, mix)
    out.update(sheet=r["sheet"], min_loss=r["min_loss"], perm=r["perm"], means=r["means"], score=r)
    return out


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if k != "score")


def pit_max(m):
    """ev_pit_max / permutation_invariant_si_sdr for two speakers on a float32 matrix m[b, t, p]."""
    return torch.maximum((m[:, 0, 0] + m[:, 1, 1]) * 0.5, (m[:, 0, 1] + m[:, 1, 0]) * 0.5)


def separate_entries(est, tgt, mix, perm):
    """The sheet's eight columns from sepvad_si_sdr / sepvad_snr calls, [B, 8] float32."""
    from sep_tfanet_vad_amd import metrics
    B = est.shape[0]
    reordered = torch.stack([est[b][perm[b]] for b in range(B)])
    mix2 = mix.unsqueeze(1).repeat(1, 2, 1)
    own, start = metrics.calc_sisdr(reordered, tgt), metrics.calc_sisdr(mix2, tgt)

    def matrix(fn, preds):  # m[b, t, p]
        return torch.stack([torch.stack([fn(preds[:, p], tgt[:, t]) for p in range(2)], -1) for t in range(2)], 1)
    return torch.stack([own[:, 0], own[:, 1], start[:, 0], start[:, 1],
                        pit_max(matrix(metrics.calc_sisdr, est)), pit_max(matrix(metrics.signal_noise_ratio, est)),
                        pit_max(matrix(metrics.calc_sisdr, mix2)), pit_max(matrix(metrics.signal_noise_ratio, mix2))], 1)


@pytest.mark.parametrize("cell", sc.CELLS, ids=lambda c: c.name)
def test_cell_against_float64_truth(cell):
    tr = sc.truth(cell)
    est, tgt, mix = (dev(a) for a in sc.make(cell))
    got = device_numbers(est, tgt, mix, cell.zm_false)
    zms = (True, False) if cell.zm_false else (True,)
    e_metric = max(err(got[k, zm], tr[k, zm]) for k in ("si", "snr") for zm in zms)
    e_pw = max(err(got["pw", ty, zm], tr["pw", ty, zm]) for ty in sc.SDR_TYPES for zm in zms)
    e_sheet = max(err(got[k], tr[k]) for k in ("sheet", "min_loss", "means"))
    cross = separate_entries(est, tgt, mix, got["perm"])
    e_cross = err(got["sheet"], cross)
    print(f"CELL {cell.name:28s} si {float(tr['si', True][0, 0]):8.3f} dB  metric {e_metric:8.1e}  pairwise {e_pw:8.1e}  "
          f"sheet {e_sheet:8.1e}  sheet-vs-entries {e_cross:8.1e}")
    for k in ("si", "snr"):
        for zm in zms:
            assert got[k, zm].dtype == torch.float32 and err(got[k, zm], tr[k, zm]) <= TOL_DB, (k, zm)
    for ty in sc.SDR_TYPES:
        for zm in zms:
            assert err(got["pw", ty, zm], tr["pw", ty, zm]) <= TOL_DB, (ty, zm)
    for k, name in (("sheet", sc.SHEET_COLUMNS), ("min_loss", None), ("means", ("loss", "pit_si_sdr", "pit_snr", "si_sdri"))):
        d = (got[k].double().cpu() - tr[k]).abs()
        assert bool((d <= TOL_DB).all()), (k, name, d.tolist())
    # permutations: everywhere the truth decides them (>= 1 dB apart, or an exact tie, which keeps the identity)
    gap, perm = tr["gap"], got["perm"].cpu()
    assert not cell.perm_gap or bool((gap >= 1.0).all())
    for b in range(cell.B):
        if gap[b] >= 1.0 or gap[b] == 0:
            assert perm[b].tolist() == tr["perm"][b].tolist(), b
    # the sheet against the separate entries
    assert e_cross <= CROSS_DB, (got["sheet"] - cross).abs().max(0).values.tolist()
    # two calls give the same bits
    assert same_bits(got, device_numbers(est, tgt, mix, cell.zm_false))
    # a row alone has the bits it has inside a batch (a one-utterance cell is batched with itself)
    if cell.B == 1:
        est, tgt, mix = est.repeat(2, 1, 1), tgt.repeat(2, 1, 1), mix.repeat(2, 1)
        both = device_numbers(est, tgt, mix, cell.zm_false)
        assert all(torch.equal(both[k][0], got[k][0]) and torch.equal(both[k][1], got[k][0])
                   for k in got if k not in ("score", "means"))
    else:
        for b in range(cell.B):
            one = device_numbers(est[b:b + 1], tgt[b:b + 1], mix[b:b + 1], cell.zm_false)
            assert all(torch.equal(one[k][0], got[k][b]) for k in got if k not in ("score", "means")), b


def test_all_zero_rows_have_the_reference_s_exact_values():
    """All-zero rows: PairwiseNegSDR is exactly 80 = -10 log10(1e-8) (test_silence_gives_80_db_and_the_identity, here
    with the shifted moments and both zero_mean values); calc_sisdr and signal_noise_ratio are exactly 0 dB for an
    all-zero estimate (alpha t against itself; the noise is the target) and for two all-zero rows (eps / eps)."""
    for zero in ("est", "tgt", "both"):
        cell = sc.BY_NAME[f"zero-{zero}"]
        est, tgt, mix = (dev(a) for a in sc.make(cell))
        got = device_numbers(est, tgt, mix)
        for zm in (True, False):
            for ty in sc.SDR_TYPES:
                if zero == "est" and ty == "snr":   # the projection is the target itself: about 0 dB, not 80
                    continue
                assert torch.equal(got["pw", ty, zm], torch.full((2, 2, 2), 80.0, device=DEV)), (zero, ty, zm)
            if zero in ("est", "both"):
                assert torch.equal(got["si", zm], torch.zeros(2, 2, device=DEV)), (zero, zm)
                assert torch.equal(got["snr", zm], torch.zeros(2, 2, device=DEV)), (zero, zm)
        assert got["perm"].tolist() == [[0, 1], [0, 1]]
        assert torch.equal(got["min_loss"], torch.full((2,), 80.0, device=DEV))


def test_one_sample_with_zero_mean_is_finite():
    """N = 1: the centred rows are empty of energy; calc_sisdr and signal_noise_ratio are 10 log10(eps / eps) = 0 and
    PairwiseNegSDR is 80, exactly, as in the truth."""
    cell = sc.BY_NAME["tiny-N1"]
    tr = sc.truth(cell)
    est, tgt, mix = (dev(a) for a in sc.make(cell))
    got = device_numbers(est, tgt, mix)
    for k in (("si", True), ("snr", True), ("pw", "sisdr", True), ("pw", "sdsdr", True), ("pw", "snr", True), "sheet"):
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k].double().cpu(), tr[k]), k


@pytest.mark.parametrize("N,name", [(4097, "tiny-N4097"), (32000, "N32000-dc100-nl0.0001")])
def test_unaligned_and_gathered_rows_have_the_bits_of_aligned_copies(N, name):
    """The C ABI on rows that start 1, 2 and 3 floats past 16-byte alignment with row strides above N (so the rows of one
    call sit at different offsets, some of them aligned), and on gathered rows (pidx / tidx): sepvad_si_sdr and
    sepvad_snr return the bits they return for aligned contiguous copies of the same rows."""
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    est, tgt, _ = sc.make(sc.BY_NAME[name])
    P, T = dev(est.reshape(-1, N)), dev(tgt.reshape(-1, N))
    R = P.shape[0]
    stream = torch.cuda.current_stream().cuda_stream

    def call(entry, p, p_off, p_ld, t, t_off, t_ld, zm, pidx=None, tidx=None, rows=R):
        n = len(pidx) if pidx is not None else rows
        out = torch.full((n,), float("nan"), device=DEV)
        pi = torch.tensor(pidx, dtype=torch.int32, device=DEV) if pidx is not None else None
        ti = torch.tensor(tidx, dtype=torch.int32, device=DEV) if tidx is not None else None
        rc = getattr(lib, entry)(ctypes.c_void_p(p.data_ptr() + 4 * p_off), p_ld, ctypes.c_void_p(t.data_ptr() + 4 * t_off),
                                 t_ld, N, n, native._ptr(pi), native._ptr(ti), int(zm), native._ptr(out), stream)
        native._check(rc, entry)
        return out

    def placed(rows, off, ld):
        buf = torch.zeros(R * ld + 8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[off:off + R * ld].view(R, ld)[:, :N] = rows
        return buf

    ld_al = (N + 3) // 4 * 4                      # aligned copies: every row on the 16-byte grid
    Pa, Ta = placed(P, 0, ld_al), placed(T, 0, ld_al)
    pidx, tidx = [3, 1, 0, 2, 1], [0, 1, 3, 2, 2]
    for entry in ("sepvad_si_sdr", "sepvad_snr"):
        for zm in (True, False):
            ref = call(entry, Pa, 0, ld_al, Ta, 0, ld_al, zm)
            ref_g = call(entry, Pa, 0, ld_al, Ta, 0, ld_al, zm, pidx, tidx)
            assert bool(torch.isfinite(ref).all()) and torch.equal(ref_g, torch.stack([call(
                entry, Pa, p * ld_al, ld_al, Ta, t * ld_al, ld_al, zm, rows=1)[0] for p, t in zip(pidx, tidx)]))
            for off in (1, 2, 3):
                p_ld, t_ld = N + 5, N + 7 + off   # > N, and the rows' offsets from the grid differ within a call
                Pu, Tu = placed(P, off, p_ld), placed(T, (off + 1) % 4, t_ld)
                assert torch.equal(call(entry, Pu, off, p_ld, Tu, (off + 1) % 4, t_ld, zm), ref), (entry, zm, off)
                assert torch.equal(call(entry, Pu, off, p_ld, Tu, (off + 1) % 4, t_ld, zm, pidx, tidx), ref_g), (entry, zm, off)
