"""The training criterion on the device (train_criterion.CombinedLoss; csrc/criterion.hip: sepvad_criterion_coef,
sepvad_criterion_backward) against

* the reference's own autograd (tests/golden/golden_train_criterion.npz, make_train_criterion_golden.py): losses and
  permutations gated as test_gpu_eval.py gates them, gradients against the float64 run within grad_cases' gate;
* float64 autograd of grad_cases' restatement, for every PairwiseNegSDR setting and over the SDR x DC regime grid;
* itself: the forward-only criterion's bits, reproducibility, independence of alignment, strides and batch size, and a
  backward that needs nothing of the shared scratch.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import grad_cases as gc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_DB = 1e-3   # the project's gate for dB values (test_gpu_eval.py)
WEIGHTS = dict(weight_separation_loss=0.99, weight_vad_loss=0.01, learn_weight_bool=False)
NOVAD = dict(WEIGHTS, weight_vad_loss=0)
CASES = ("n3", "n257", "n4096", "n4101", "sil", "one")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_train_criterion.npz"))


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def signals(g, tag):
    if tag == "n4096":
        return t_(g["n4101_est"][:, :, :4096]), t_(g["n4101_tgt"][:, :, :4096])
    return t_(g[f"{tag}_est"]), t_(g[f"{tag}_tgt"])


def make_crit(weights=WEIGHTS, sdr_type="sisdr", zero_mean=True, take_log=True, module=None):
    from sep_tfanet_vad_amd import combined_loss, pit, sdr, train_criterion
    sep = pit.PITLossWrapper(sdr.PairwiseNegSDR(sdr_type, zero_mean=zero_mean, take_log=take_log), pit_from="pw_mtx")
    vad = pit.PITLossWrapper(combined_loss.BinaryCrossEntropyLoss_Mean(), pit_from="pw_pt")
    return (module or train_criterion).CombinedLoss(sep, vad, dict(weights))


def run_sep(est, tgt, **pw):
    """-> (separation_loss, perm, grad_est) of the native criterion without a VAD track, upstream gradient 1."""
    e = est.to(DEV).requires_grad_(True)
    sep, vad_loss, idx_vad, idx = make_crit(NOVAD, **pw)(e, tgt.to(DEV), None, None)
    assert vad_loss.dim() == 0 and vad_loss.item() == 0 and idx_vad.item() == 0 and not idx.requires_grad
    sep.backward()
    return sep.detach(), idx, e.grad


def run_both(est, tgt, vad, lab, crit=None):
    """-> (sep, vad_loss, perm, grad_est, grad_vad, labels on the device) with both upstream gradients 1."""
    e, v = est.to(DEV).requires_grad_(True), vad.to(DEV).requires_grad_(True)
    lab = lab.to(DEV)
    sep, vad_loss, idx_vad, idx = (crit or make_crit())(e, tgt.to(DEV), v, lab)
    assert idx_vad is idx and sep.is_cuda and vad_loss.is_cuda and sep.dim() == 0 and vad_loss.dim() == 0
    assert sep.requires_grad and vad_loss.requires_grad and not idx.requires_grad and idx.dtype == torch.int64
    (sep + vad_loss).backward()
    return sep.detach(), vad_loss.detach(), idx, e.grad, v.grad, lab


def check_est(grad, grad64, sdr_db, where):
    assert grad.dtype == torch.float32 and bool(torch.isfinite(grad).all())
    worst, ulps = gc.est_error_in_gates(grad.cpu(), grad64, sdr_db)
    print(where, "grad_est error / gate:", worst, "worst row error in 2^-24 rowmax:", float(ulps.max()))
    assert worst <= 1.0, where


# ---- 1. the reference's goldens ----------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", CASES)
def test_fixture_case(g, tag):
    est, tgt = signals(g, tag)
    sep, vad_loss, idx, ge, gv, lab = run_both(est, tgt, t_(g[f"{tag}_vad"]), t_(g[f"{tag}_labels"]))
    s32, s64 = float(g[f"{tag}_sep_f32"]), float(g[f"{tag}_sep_f64"])
    assert abs(sep.item() - s64) <= max(TOL_DB, 2 * abs(s32 - s64))
    v32, v64 = float(g[f"{tag}_vadloss_f32"]), float(g[f"{tag}_vadloss_f64"])
    assert abs(vad_loss.item() - v64) <= max(2 * abs(v32 - v64), 1e-6 * abs(v64))
    assert np.array_equal(idx.cpu().numpy(), g[f"{tag}_idx"])
    assert np.array_equal(lab.cpu().numpy(), g[f"{tag}_labels_after"])  # combined_loss.py:130-131, in place
    truth, _, _ = gc.autograd_truth(est, tgt)
    check_est(ge, t_(g[f"{tag}_grad_est_f64"]), truth["sdr_db"], tag)
    ok, rel = gc.vad_within_gate(gv.cpu(), t_(g[f"{tag}_grad_vad_f64"]))
    print(tag, "grad_vad worst relative error:", rel)
    assert ok and bool(torch.isfinite(gv).all())
    if tag == "sil":    # all-zero estimates, all-zero targets: the reference's finite zero
        assert not bool(ge[:2].any()) and bool(ge[2].any())
    if tag == "one":
        assert not bool(ge.any())


# ---- 2. every pairwise loss, and the regimes, against float64 autograd -------------------------------------------

@pytest.mark.parametrize("case", gc.PW_CASES, ids=lambda c: gc.pw_key(*c))
def test_every_pairwise_loss(g, case):
    key = gc.pw_key(*case)
    kw = dict(sdr_type=case[0], zero_mean=case[1], take_log=case[2])
    est, tgt = signals(g, "n257")
    sep, idx, ge = run_sep(est, tgt, **kw)
    truth, g64, _ = gc.autograd_truth(est, tgt, **kw)
    assert torch.equal(idx.cpu(), truth["perm"]) and np.array_equal(idx.cpu().numpy(), g[f"n257_{key}_idx"])
    ref = float(g[f"n257_{key}_loss_f64"])
    assert abs(sep.item() - ref) <= max(TOL_DB, 2 * abs(float(g[f"n257_{key}_loss_f32"]) - ref))
    check_est(ge, g64, truth["sdr_db"], key)
    check_est(ge, t_(g[f"n257_{key}_grad_est_f64"]), truth["sdr_db"], key + " (golden)")


@pytest.mark.parametrize("sdr_db,dc", gc.regime_grid())
def test_regime(sdr_db, dc):
    est, tgt = gc.regime_case(sdr_db, dc)
    truth, g64, _ = gc.autograd_truth(est, tgt)
    sep, idx, ge = run_sep(est, tgt)
    assert torch.equal(idx.cpu(), truth["perm"]) and idx.tolist() == [[0, 1], [1, 0]]
    check_est(ge, g64, truth["sdr_db"], f"SDR {sdr_db} dB, DC {dc} sigma:")


# ---- 3. the forward is the forward-only criterion's ---------------------------------------------------------------

def test_no_grad_forward_has_the_forward_only_bits(g):
    from sep_tfanet_vad_amd import combined_loss
    est, tgt = (a.to(DEV) for a in signals(g, "n4101"))
    vad = t_(g["n4101_vad"]).to(DEV)
    for weights in (WEIGHTS, NOVAD, dict(WEIGHTS, learn_weight_bool=True)):
        new, old = make_crit(weights).to(DEV), make_crit(weights, module=combined_loss).to(DEV)
        with torch.no_grad():
            a = new(est, tgt, vad, t_(g["n4101_labels"]).to(DEV))
            b = old(est, tgt, vad, t_(g["n4101_labels"]).to(DEV))
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y)
    # and under grad mode the same numbers
    c = make_crit()(est.clone().requires_grad_(True), tgt, vad, t_(g["n4101_labels"]).to(DEV))
    d = make_crit(module=combined_loss)(est, tgt, vad, t_(g["n4101_labels"]).to(DEV))
    assert c[0].requires_grad and all(torch.equal(x.detach(), y) for x, y in zip(c, d))


# ---- 4. bits -----------------------------------------------------------------------------------------------------

def test_two_backwards_give_the_same_bits(g):
    est, tgt = signals(g, "n4101")
    vad, lab = t_(g["n4101_vad"]), t_(g["n4101_labels"])
    a, b = run_both(est, tgt, vad, lab), run_both(est, tgt, vad, lab)
    assert all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))


def strided_leaf(x, width, offset):
    """A leaf [B, 2, width] holding x at [..., offset : offset + N]; the view is what the criterion is given."""
    wide = torch.zeros(x.shape[0], 2, width, device=DEV)
    wide[:, :, offset:offset + x.shape[2]] = x.to(DEV)
    wide.requires_grad_(True)
    return wide, wide[:, :, offset:offset + x.shape[2]]


@pytest.mark.parametrize("N", [4101, 5000])
def test_alignment_and_strides_do_not_change_the_bits(N):
    """Contiguous rows (aligned to 16 bytes when N is a multiple of 4: the float4 path), a one-float offset (the
    scalar path) and a row stride above N, for est and for tgt: the same losses and gradient bits."""
    est, tgt = gc.regime_case(20, 0, seed=7, N=N)
    sep0, idx0, g0 = run_sep(est, tgt)
    wide_t = torch.zeros(2, 2, N + 7, device=DEV)
    wide_t[:, :, 1:1 + N] = tgt.to(DEV)
    for width, off in ((N + 4, 1), (N + 8, 0), (N + 7, 4)):
        leaf, view = strided_leaf(est, width, off)
        assert not view.is_contiguous()
        for tg in (tgt.to(DEV), wide_t[:, :, 1:1 + N]):
            leaf.grad = None
            sep, _, _, idx = make_crit(NOVAD)(view, tg, None, None)
            sep.backward()
            assert torch.equal(sep.detach(), sep0) and torch.equal(idx, idx0)
            assert torch.equal(leaf.grad[:, :, off:off + N], g0)
            assert not bool(leaf.grad[:, :, :off].any()) and not bool(leaf.grad[:, :, off + N:].any())


def test_c_abi_strided_gradient_rows_have_the_same_bits():
    """sepvad_criterion_backward with est_ld, tgt_ld and grad_ld above N such that every row is 16-byte aligned while
    N is odd: the float4 path with its scalar tail, against the bits of the contiguous call (the scalar path)."""
    from sep_tfanet_vad_amd import evaluate, native, train_criterion
    N, ld = 2051, 2052
    est, tgt = gc.regime_case(20, 0, seed=9, N=N)
    _, idx0, g0 = run_sep(est, tgt)
    lib = native.load_library()
    e, t = torch.zeros(2, 2, ld, device=DEV), torch.zeros(2, 2, ld, device=DEV)
    e[:, :, :N], t[:, :, :N] = est.to(DEV), tgt.to(DEV)
    r = evaluate.eval_separation(e[:, :, :N], t[:, :, :N], sheet=False)
    assert torch.equal(r["perm"], idx0)
    scratch = r["scratch"]
    coef = torch.empty(2, 2, train_criterion.CRIT_COEF, dtype=torch.float64, device=DEV)
    stream = native.stream_ptr(e.device)
    P = native._ptr
    native._check(lib.sepvad_criterion_coef(P(e), ld, P(t), ld, 2, N, 0, 1, 1, 1e-8, P(scratch), scratch.numel(),
                                            P(r["perm"]), P(coef), stream), "sepvad_criterion_coef")
    one = torch.ones((), device=DEV)
    grad = torch.full((2, 2, ld), 7.0, device=DEV)
    assert e.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0 and grad.data_ptr() % 16 == 0
    native._check(lib.sepvad_criterion_backward(2, P(e), ld, P(t), ld, N, P(coef), P(one), P(grad), ld, None, None, None,
                                                0, None, None, stream), "sepvad_criterion_backward")
    assert torch.equal(grad[:, :, :N], g0) and bool((grad[:, :, N:] == 7.0).all())  # nothing written past a row's N
    assert coef[:, :, 5].tolist() == [[0.0, 1.0], [1.0, 0.0]]
    # argument errors launch nothing
    for args in ((0, P(e), ld, P(t), ld, N, P(coef), P(one), P(grad), ld, None, None, None, 0, None, None),
                 (2, None, ld, P(t), ld, N, P(coef), P(one), P(grad), ld, None, None, None, 0, None, None),
                 (2, P(e), ld, P(t), ld, N, P(coef), P(one), P(grad), N - 1, None, None, None, 0, None, None),
                 (2, P(e), ld, P(t), ld, N, P(coef), None, P(grad), ld, None, None, None, 0, None, None),
                 (2, None, ld, None, ld, N, None, None, None, ld, P(e), None, None, 5, P(one), P(grad))):
        assert lib.sepvad_criterion_backward(*args, stream) != 0
    assert bool((grad[:, :, N:] == 7.0).all())


def test_an_utterance_does_not_depend_on_its_batch(g):
    """B times the gradient of an utterance, alone, in a batch of 2 and in a batch of 4: the same bits (the scalings are
    powers of two)."""
    est, tgt = gc.regime_case(20, 0, seed=3, N=4101)
    e4, t4 = torch.cat([est, est.flip(0)]), torch.cat([tgt, tgt.flip(0)])
    gen = torch.Generator().manual_seed(5)
    vad = torch.rand(4, 2, 9, generator=gen)
    lab = torch.randint(0, 3, (4, 2, 9), generator=gen).float()
    full = run_both(e4, t4, vad, lab)
    for B in (1, 2):
        for b0 in range(0, 4, B):
            part = run_both(e4[b0:b0 + B], t4[b0:b0 + B], vad[b0:b0 + B], lab[b0:b0 + B])
            assert torch.equal(part[2], full[2][b0:b0 + B])
            assert torch.equal(part[3] * B, full[3][b0:b0 + B] * 4), (B, b0)
            assert torch.equal(part[4] * B, full[4][b0:b0 + B] * 4), (B, b0)


# ---- 5. the backward keeps its own state -------------------------------------------------------------------------

def test_backward_after_an_unrelated_forward(g):
    est, tgt = signals(g, "n4101")
    vad, lab = t_(g["n4101_vad"]), t_(g["n4101_labels"])
    clean = run_both(est, tgt, vad, lab)
    e, v = est.to(DEV).requires_grad_(True), vad.to(DEV).requires_grad_(True)
    crit = make_crit()
    sep, vad_loss, _, _ = crit(e, tgt.to(DEV), v, lab.to(DEV))
    other_e, other_t = gc.regime_case(40, 100, seed=1, N=9000)
    with torch.no_grad():
        crit(other_e.to(DEV), other_t.to(DEV), torch.rand(2, 2, 33, device=DEV), torch.ones(2, 2, 33, device=DEV))
    oe = other_e.to(DEV).requires_grad_(True)
    crit(oe, other_t.to(DEV), torch.rand(2, 2, 33, device=DEV), torch.zeros(2, 2, 33, device=DEV))  # graph left alone
    (sep + vad_loss).backward()
    assert torch.equal(e.grad, clean[3]) and torch.equal(v.grad, clean[4])


# ---- 6. upstream gradients ---------------------------------------------------------------------------------------

def test_upstream_gradients_accumulation_and_zero(g):
    est, tgt = signals(g, "n257")
    vad, lab = t_(g["n257_vad"]), t_(g["n257_labels"])
    unit = run_both(est, tgt, vad, lab)
    truth, _, _ = gc.autograd_truth(est, tgt)
    e, v = est.to(DEV).requires_grad_(True), vad.to(DEV).requires_grad_(True)
    crit = make_crit()
    accum = 4

    def step():
        sep, vad_loss, _, _ = crit(e, tgt.to(DEV), v, lab.to(DEV))
        ((sep * WEIGHTS["weight_separation_loss"] + vad_loss * WEIGHTS["weight_vad_loss"]) / accum).backward()
    step()
    once_e, once_v = e.grad.clone(), v.grad.clone()
    check_est(once_e, t_(g["n257_grad_est_f64"]) * (0.99 / accum), truth["sdr_db"], "trainer's weighting")
    assert gc.vad_within_gate(once_v.cpu(), t_(g["n257_grad_vad_f64"]) * (0.01 / accum))[0]
    step()
    assert torch.equal(e.grad, once_e + once_e) and torch.equal(v.grad, once_v + once_v)
    # a zero upstream gradient gives exact zeros (the VAD track holds p = 0 against label 1: a finite 3.6e11)
    e.grad = v.grad = None
    sep, vad_loss, _, _ = crit(e, tgt.to(DEV), v, lab.to(DEV))
    (sep * 0 + vad_loss * 0).backward()
    assert not bool(e.grad.any()) and not bool(v.grad.any())
    # one loss alone leaves the other input's gradient zero
    e.grad = v.grad = None
    sep, vad_loss, _, _ = crit(e, tgt.to(DEV), v, lab.to(DEV))
    vad_loss.backward()
    assert torch.equal(v.grad, unit[4]) and (e.grad is None or not bool(e.grad.any()))


def test_learned_weights_get_their_gradients(g):
    """learn_weight_bool: loss / (2 w^2) + log(1 + w^2) (combined_loss.py:101-103,111-112) through ordinary torch ops:
    d / dw = -loss / w^3 + 2 w / (1 + w^2) = -8 loss + 0.8 at w = 0.5, so the parameters' gradients carry eight times
    the losses' own tolerances; the inputs' gradients are those of the plain criterion times 1 / (2 w^2) = 2."""
    est, tgt = signals(g, "n257")
    vad, lab = t_(g["n257_vad"]), t_(g["n257_labels"])
    unit = run_both(est, tgt, vad, lab)
    crit = make_crit(dict(WEIGHTS, learn_weight_bool=True)).to(DEV)
    out = run_both(est, tgt, vad, lab, crit)
    s64, v64 = float(g["n257_sep_f64"]), float(g["n257_vadloss_f64"])
    gs, gv = crit.learn_weight_separationLoss.grad.item(), crit.learn_weight_vadLoss.grad.item()
    assert abs(gs - (-8 * s64 + 0.8)) <= 8 * TOL_DB + 1e-6 * abs(gs)
    assert abs(gv - (-8 * v64 + 0.8)) <= 8 * 1e-6 * abs(v64) + 1e-6 * abs(gv)
    assert torch.equal(out[3], unit[3] * 2) and torch.equal(out[4], unit[4] * 2)


# ---- 7. chained autograd -----------------------------------------------------------------------------------------

class Toy(torch.nn.Module):
    """est = Conv1d(1, 2, 5)(mix); vad = sigmoid(Linear(1, 2)(frame energies of mix))."""
    FRAME = 128

    def __init__(self, kernels):
        super().__init__()
        self.conv = torch.nn.Conv1d(1, 2, 5, padding=2)
        self.lin = torch.nn.Linear(1, 2)
        with torch.no_grad():
            self.conv.weight.copy_(kernels)

    def energies(self, mix):
        T = mix.shape[-1] // self.FRAME
        return mix[:, :T * self.FRAME].reshape(mix.shape[0], T, self.FRAME).square().mean(-1, keepdim=True)

    def forward(self, mix):
        return self.conv(mix.unsqueeze(1)), torch.sigmoid(self.lin(self.energies(mix))).transpose(1, 2)


def test_chained_autograd_through_a_toy_module():
    """Parameter gradients through the native criterion (float32, device) against the same module and the restatement
    in float64 on the host. Propagated gate of a parameter whose gradient is sum_k g[k] J[k]: the criterion's gate
    on every g[k] times |J[k]|, plus 2^-20 sum_k |g[k] J[k]| for the float32 forward and the float32 accumulation of
    the module's own backward (16 float32 roundings of the sum of magnitudes; a worst-case bound of a float32 dot
    product of this length is above 1000 roundings)."""
    gen = torch.Generator().manual_seed(21)
    B, N = 2, 1027
    mix = torch.randn(B, N, generator=gen)
    true_k = torch.randn(2, 1, 5, generator=gen)
    tgt = torch.nn.functional.conv1d(mix.unsqueeze(1), true_k, padding=2) + 0.1 * torch.randn(B, 2, N, generator=gen)
    tgt[1] = tgt[1].flip(0)
    lab = torch.randint(0, 3, (B, 2, N // Toy.FRAME), generator=gen).float()
    toy = Toy(true_k + 0.2 * torch.randn(2, 1, 5, generator=gen))
    ref = Toy(true_k).double()
    ref.load_state_dict({k: v.double() for k, v in toy.state_dict().items()})
    # float64 on the host
    e64, v64 = ref(mix.double())
    e64.retain_grad(), v64.retain_grad()
    r = gc.restated_criterion(e64, tgt.double(), v64, lab.double())
    (r["sep"] + r["vad"]).backward()
    # float32 on the device
    toy = toy.to(DEV)
    est, vad = toy(mix.to(DEV))
    sep, vad_loss, _, idx = make_crit()(est, tgt.to(DEV), vad, lab.to(DEV))
    assert torch.equal(idx.cpu(), r["perm"])
    (sep + vad_loss).backward()
    ge = e64.grad.detach()
    gate_e = gc.est_gate(ge, r["sdr_db"]).expand_as(ge)
    pad = torch.nn.functional.pad(mix.double(), (2, 2))
    taps = torch.stack([pad[:, k:k + N] for k in range(5)], 0)           # [5, B, N]: d est[b, i, n] / d weight[i, 0, k]
    for i in range(2):
        for k in range(5):
            tol = float((gate_e[:, i] * taps[k].abs()).sum() + 2.0 ** -20 * (ge[:, i] * taps[k]).abs().sum())
            d = abs(toy.conv.weight.grad[i, 0, k].item() - ref.conv.weight.grad[i, 0, k].item())
            print(f"conv.weight[{i}, 0, {k}]: |d| {d:.3e}, tolerance {tol:.3e}")
            assert d <= tol
        tol = float(gate_e[:, i].sum() + 2.0 ** -20 * ge[:, i].abs().sum())
        assert abs(toy.conv.bias.grad[i].item() - ref.conv.bias.grad[i].item()) <= tol
    gv = v64.grad.detach()                                                # [B, 2, T]
    p = v64.detach()
    en = ref.energies(mix.double()).transpose(1, 2)                       # [B, 1, T]
    for i in range(2):
        for name, J in (("weight", p[:, i] * (1 - p[:, i]) * en[:, 0]), ("bias", p[:, i] * (1 - p[:, i]))):
            tol = float((gc.VAD_GATE + 2.0 ** -20) * (gv[:, i] * J).abs().sum())
            got = getattr(toy.lin, name).grad.reshape(-1)[i].item()
            want = getattr(ref.lin, name).grad.reshape(-1)[i].item()
            print(f"lin.{name}[{i}]: |d| {abs(got - want):.3e}, tolerance {tol:.3e}")
            assert abs(got - want) <= tol


# ---- 8. the forward-only classes stay forward-only ----------------------------------------------------------------

def test_forward_only_classes_still_refuse_grad():
    from sep_tfanet_vad_amd import combined_loss, evaluate
    x = torch.randn(2, 2, 500, device=DEV)
    w = x.clone().requires_grad_(True)
    p = torch.rand(2, 2, 4, device=DEV)
    old = make_crit(module=combined_loss)
    for fn in (lambda: old(w, x, p, torch.ones_like(p)), lambda: old.criterion_separation(w, x),
               lambda: old.criterion_separation.loss_func(w, x), lambda: evaluate.score_batch(w, x),
               lambda: combined_loss.BinaryCrossEntropyLoss_Mean()(p.clone().requires_grad_(True), torch.ones_like(p))):
        with pytest.raises(RuntimeError, match="requires grad"):
            fn()
    with pytest.raises(RuntimeError, match="target requires grad"):
        make_crit()(x, w, p, torch.ones_like(p))
