"""The evaluation criterion on the device (csrc/eval.hip: sepvad_eval_separation, sepvad_eval_vad) against

* the reference's own outputs (tests/golden/golden_eval.npz, make_eval_golden.py): PairwiseNegSDR, PITLossWrapper over
  it, BinaryCrossEntropyLoss_Mean, pit_CE_vad, CombinedLoss and calc_vad. dB values are gated at
  max(TOL_DB, 2 |ref32 - ref64|) against the float64 run of the reference, BCE sums at
  max(2 |ref32 - ref64|, 1e-6 |ref64|); permutations, counts, calc_vad and the mutated labels are exact;
* a float64 restatement of the reference's formulas written here (element-wise, not the closed form the kernel
  evaluates), at the shapes where the kernel changes path: fewer samples than one float4, less than one chunk, an
  exact chunk, a ragged last chunk, strided and unaligned rows, no mixture;
* the existing metric entries (calc_sisdr, pit_si_sdr, pit_snr, si_sdri, Accuracy_Vad) on the same tensors.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_DB = 1e-3           # the project's gate for dB values (test_gpu_metrics.py)
EV_CHUNK = 4096         # csrc/sepvad_internal.h
EPS32 = float(torch.finfo(torch.float32).eps)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_eval.npz"))


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ---- float64 restatement of the reference (CPU) ----------------------------------------------------------------

def ref_pw(est, tgt, sdr_type="sisdr", zero_mean=True, take_log=True, eps=1e-8):
    """model/sdr.py:48-86 on float64 tensors: [B, 2, N] -> [B, 2, 2]."""
    est, tgt = est.double(), tgt.double()
    if zero_mean:
        est, tgt = est - est.mean(2, keepdim=True), tgt - tgt.mean(2, keepdim=True)
    s_t, s_e = tgt.unsqueeze(1), est.unsqueeze(2)
    if sdr_type in ("sisdr", "sdsdr"):
        proj = (s_e * s_t).sum(3, keepdim=True) * s_t / ((s_t ** 2).sum(3, keepdim=True) + eps)
    else:
        proj = s_t.repeat(1, 2, 1, 1)
    noise = s_e - s_t if sdr_type in ("sdsdr", "snr") else s_e - proj
    val = (proj ** 2).sum(3) / ((noise ** 2).sum(3) + eps)
    return -(10 * torch.log10(val + eps)) if take_log else -val


def ref_perm(pw):
    """find_best_perm_factorial on the float32-rounded matrix: (min_loss float32 [B], batch_indices [B, 2], gap)."""
    pw = pw.float()
    loss_id, loss_sw = (pw[:, 0, 0] + pw[:, 1, 1]) / 2, (pw[:, 1, 0] + pw[:, 0, 1]) / 2
    swap = loss_sw < loss_id
    idx = torch.where(swap[:, None], torch.tensor([[1, 0]]), torch.tensor([[0, 1]]))
    return torch.minimum(loss_id, loss_sw), idx, (loss_id - loss_sw).abs()


def ref_si_sdr(p, t):
    p, t = p.double(), t.double()
    p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    alpha = ((p * t).sum(-1, keepdim=True) + EPS32) / ((t ** 2).sum(-1, keepdim=True) + EPS32)
    ts = alpha * t
    return 10 * torch.log10(((ts ** 2).sum(-1) + EPS32) / (((ts - p) ** 2).sum(-1) + EPS32))


def ref_snr(p, t):
    p, t = p.double(), t.double()
    p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    return 10 * torch.log10(((t ** 2).sum(-1) + EPS32) / (((t - p) ** 2).sum(-1) + EPS32))


def ref_pit_max(metric, preds, tgt):
    """metrics.permutation_invariant_si_sdr for two speakers: the best mean over the targets, per utterance."""
    m = torch.stack([torch.stack([metric(preds[:, p], tgt[:, t]) for p in range(2)], -1) for t in range(2)], 1)
    return torch.maximum((m[:, 0, 0] + m[:, 1, 1]) / 2, (m[:, 0, 1] + m[:, 1, 0]) / 2)


def ref_sheet(est, tgt, mix, idx):
    """[B, 8] in the order of evaluate.SHEET_COLUMNS, and the four means."""
    B = est.shape[0]
    reordered = torch.stack([est[b][idx[b]] for b in range(B)])
    mix2 = (mix if mix is not None else torch.zeros(B, est.shape[2])).unsqueeze(1).repeat(1, 2, 1)
    own, start = ref_si_sdr(reordered, tgt), ref_si_sdr(mix2, tgt)
    cols = [own[:, 0], own[:, 1], start[:, 0], start[:, 1], ref_pit_max(ref_si_sdr, est, tgt),
            ref_pit_max(ref_snr, est, tgt), ref_pit_max(ref_si_sdr, mix2, tgt), ref_pit_max(ref_snr, mix2, tgt)]
    sheet = torch.stack(cols, 1)
    return sheet, sheet[:, 4].mean(), sheet[:, 5].mean(), sheet[:, 4].mean() - start.mean()


def ref_bce_cells(vad, labels):
    """combined_loss.py:130-137 per utterance for vad[:, i] against labels[:, j]: [B, 2, 2] float64."""
    y = torch.where(labels == 2, torch.ones_like(labels), labels).double()
    p = vad.double()
    lp, lq = torch.log(p).clamp(min=-100), torch.log(1 - p).clamp(min=-100)
    w = y * 0.36 + 0.64 * (1 - y)
    return torch.stack([torch.stack([(-(y[:, j] * lp[:, i] + (1 - y[:, j]) * lq[:, i]) * w[:, j]).sum(-1)
                                     for j in range(2)], -1) for i in range(2)], 1)


def ref_conf(pred01, labels):
    """confusion_matrix(labels=[0., 1.]).ravel() per (b, s): [B, 2, 4] (tn, fp, fn, tp)."""
    y = torch.where(labels == 2, torch.ones_like(labels), labels)
    out = [((y == a) & (pred01 == b)).sum(-1) for a in (0, 1) for b in (0, 1)]
    return torch.stack(out, -1).to(torch.int32)


def ref_vad(vad, labels, idx, masks=None):
    B = vad.shape[0]
    cells = ref_bce_cells(vad, labels)
    rows = torch.stack([cells[b, idx[b, 0], 0] + cells[b, idx[b, 1], 1] for b in range(B)])
    pred = torch.stack([vad[b][idx[b]] for b in range(B)])
    out = dict(bce_rows=rows, bce_mean=rows.float().double().mean(), pw_ce=cells.sum(0),
               conf=ref_conf((pred > 0.5).long(), labels))
    if masks is not None:
        m = torch.stack([masks[b][idx[b]] for b in range(B)])
        out["simple_vad"] = ((m >= 0.5).sum(2) >= 257 * 0.25).long()
        out["conf_simple"] = ref_conf(out["simple_vad"], labels)
    return out


def close_db(got, ref, tol=TOL_DB):
    d = (got.double().cpu() - ref.double()).abs()
    print("max |d| dB:", float(d.max()), "tol:", float(torch.as_tensor(tol).max()))
    return bool((d <= torch.as_tensor(tol)).all())


def gaussian_case(B, N, seed):
    """Gaussian rows (as test_si_sdr_vs_oracle), a non-zero mean, alternate utterances with their speakers swapped."""
    gen = torch.Generator().manual_seed(seed)
    tgt = torch.randn(B, 2, N, generator=gen)
    est = 0.7 * tgt + 0.3 * torch.randn(B, 2, N, generator=gen) + 0.1
    est[1::2] = est[1::2].flip(1)
    mix = tgt.sum(1) + 0.2 * torch.randn(B, N, generator=gen)
    return est, tgt, mix


# ---- the reference's goldens -----------------------------------------------------------------------------------

def golden_tol(g, key, floor=TOL_DB):
    r32, r64 = g[key + "_f32"].astype(np.float64), g[key + "_f64"]
    return torch.as_tensor(np.asarray(r64)), torch.as_tensor(np.asarray(np.maximum(floor, 2 * np.abs(r32 - r64))))


def bce_tol(g, key):
    r32, r64 = g[key + "_f32"].astype(np.float64), g[key + "_f64"]
    return torch.as_tensor(np.asarray(r64)), torch.as_tensor(np.asarray(np.maximum(2 * np.abs(r32 - r64), 1e-6 * np.abs(r64))))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_pairwise_neg_sdr_matches_reference(g, tag):
    from sep_tfanet_vad_amd import sdr
    est, tgt = dev(g[f"{tag}_est"]), dev(g[f"{tag}_tgt"])
    for sdr_type in ("sisdr", "sdsdr", "snr"):
        for zm in (True, False):
            ref, tol = golden_tol(g, f"{tag}_pw_{sdr_type}_zm{int(zm)}")
            got = sdr.PairwiseNegSDR(sdr_type, zero_mean=zm)(est, tgt)
            assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_cuda
            assert close_db(got, ref, tol), (sdr_type, zm)
    ref, tol = golden_tol(g, f"{tag}_pw_sisdr_zm1_nolog")
    assert close_db(sdr.PairwiseNegSDR("sisdr", take_log=False)(est, tgt), ref, tol)
    for alias, key in ((sdr.pairwise_neg_sisdr, "sisdr"), (sdr.pairwise_neg_sdsdr, "sdsdr"), (sdr.pairwise_neg_snr, "snr")):
        assert torch.equal(alias(est, tgt), sdr.PairwiseNegSDR(key)(est, tgt))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_pit_wrapper_over_pairwise_sisdr_matches_reference(g, tag):
    """PITLossWrapper(pairwise_neg_sisdr, "pw_mtx") in each return form; every utterance's permutation is compared
    (the generator asserts the two permutation losses of every row differ by >= 1 dB)."""
    from sep_tfanet_vad_amd import evaluate, pit, sdr
    est, tgt = dev(g[f"{tag}_est"]), dev(g[f"{tag}_tgt"])
    idx = torch.from_numpy(g[f"{tag}_pit_idx"])
    ref_loss, tol = golden_tol(g, f"{tag}_pit_loss")
    reordered = torch.stack([est[b][idx[b].to(DEV)] for b in range(est.shape[0])])
    for perm_reduce in (None, False):
        crit = pit.PITLossWrapper(sdr.pairwise_neg_sisdr, pit_from="pw_mtx", perm_reduce=perm_reduce)
        loss = crit(est, tgt)
        assert loss.is_cuda and loss.dim() == 0 and close_db(loss, ref_loss, tol)
        loss_i, bi = crit(est, tgt, return_incides=True)
        assert torch.equal(bi.cpu(), idx) and bi.dtype == torch.int64 and bi.is_cuda and torch.equal(loss_i, loss)
        loss_e, out = crit(est, tgt, return_est=True)
        assert torch.equal(out, reordered) and torch.equal(loss_e, loss)
        loss_b, out_b, bi_b = crit(est, tgt, return_est=True, return_incides=True)
        assert torch.equal(out_b, reordered) and torch.equal(bi_b.cpu(), idx) and torch.equal(loss_b, loss)
    ref_min, tol_min = golden_tol(g, f"{tag}_pit_min_loss")
    assert close_db(evaluate.eval_separation(est, tgt)["min_loss"], ref_min, tol_min)


def test_vad_criterion_matches_reference(g):
    """BinaryCrossEntropyLoss_Mean (labels changed in place as the reference changes them), pit_CE_vad and calc_vad."""
    from sep_tfanet_vad_amd import combined_loss, evaluate, metrics, pit
    vad = dev(g["vad"])
    lab = dev(g["vad_labels"])
    ref, tol = bce_tol(g, "bce")
    got = combined_loss.BinaryCrossEntropyLoss_Mean()(vad, lab)
    assert got.is_cuda and got.dim() == 0 and close_db(got, ref, tol)
    assert np.array_equal(lab.cpu().numpy(), g["vad_labels_after"])
    # labels of another dtype are converted, as .to(float32) copies them in the reference: the argument stays
    lab64 = dev(g["vad_labels"], torch.float64)
    assert torch.equal(combined_loss.BinaryCrossEntropyLoss_Mean()(vad, lab64), got)
    assert np.array_equal(lab64.cpu().numpy(), g["vad_labels"].astype(np.float64))
    idx = torch.from_numpy(g["ce_idx"])
    ref_loss, tol_loss = bce_tol(g, "ce_loss")
    ref_pw, tol_pw = bce_tol(g, "ce_pw")
    reordered = torch.stack([vad[b][idx[b].to(DEV)] for b in range(3)])
    for crit in (metrics.pit_CE_vad, pit.PITLossWrapper(combined_loss.BinaryCrossEntropyLoss_Mean(), pit_from="pw_pt")):
        lab = dev(g["vad_labels"])
        loss, out, bi = crit(vad, lab, return_est=True, return_incides=True)
        assert close_db(loss, ref_loss, tol_loss) and torch.equal(bi.cpu(), idx) and torch.equal(out, reordered)
        assert np.array_equal(lab.cpu().numpy(), g["vad_labels_after"])
        assert torch.equal(crit(vad, dev(g["vad_labels"])), loss)
        loss_i, bi_i = crit(vad, dev(g["vad_labels"]), return_incides=True)
        assert torch.equal(loss_i, loss) and torch.equal(bi_i, bi)
        loss_e, out_e = crit(vad, dev(g["vad_labels"]), return_est=True)
        assert torch.equal(loss_e, loss) and torch.equal(out_e, reordered)
    assert close_db(evaluate.eval_vad(vad, dev(g["vad_labels"]))["pw_ce"], ref_pw, tol_pw)
    simple = metrics.calc_vad(dev(g["masks"]))
    assert simple.dtype == torch.int64 and simple.is_cuda and np.array_equal(simple.cpu().numpy(), g["simple_vad"])


def criterion_from_config(cfg):
    """test.py:49-64 on the config's dicts, with module_loss / module_func_loss / combined_loss pointed at the
    package (ConfigParser.init_obj(name, module, **kw) is getattr(module, cfg[name]["type"])(**cfg[name]["args"], **kw))."""
    from sep_tfanet_vad_amd import combined_loss, pit as module_loss, sdr as module_func_loss

    def init_obj(name, module, **kw):
        return getattr(module, cfg[name]["type"])(**cfg[name]["args"], **kw)
    func_loss_separation = getattr(module_func_loss, cfg["loss_separation"]["loss_func"])
    if cfg["loss_separation"]["perm_reduce"] is not False:
        reduce = getattr(module_loss, cfg["loss_separation"]["perm_reduce"])
    else:
        reduce = None
    criterion_separation = init_obj("loss_separation", module_loss, loss_func=func_loss_separation, perm_reduce=reduce)
    func_loss_vad = getattr(combined_loss, cfg["loss_vad"]["loss_func"])()
    criterion_vad = init_obj("loss_vad", module_loss, loss_func=func_loss_vad)
    return combined_loss.CombinedLoss(criterion_separation, criterion_vad, **cfg["combined_loss"])


def test_combined_loss_matches_reference(g):
    from sep_tfanet_vad_amd import combined_loss
    cfg = json.loads(str(g["criterion_config_json"]))
    est, tgt, vad = dev(g["a_est"]), dev(g["a_tgt"]), dev(g["vad"])
    idx = torch.from_numpy(g["comb_shipped_idx_sep"])
    crit = criterion_from_config(cfg)
    lab = dev(g["vad_labels"])
    sep_loss, vad_loss, bi_vad, bi_sep = crit(est, tgt, vad, lab)
    assert all(t.is_cuda for t in (sep_loss, vad_loss, bi_vad, bi_sep))
    assert close_db(sep_loss, *golden_tol(g, "comb_shipped_sep")) and close_db(vad_loss, *bce_tol(g, "comb_shipped_vad"))
    assert torch.equal(bi_sep.cpu(), idx) and bi_vad is bi_sep
    assert np.array_equal(lab.cpu().numpy(), g["vad_labels_after"])
    novad = combined_loss.CombinedLoss(crit.criterion_separation, crit.criterion_vad,
                                       dict(cfg["combined_loss"], weight_vad_loss=0))
    sep_loss, vad_loss, bi_vad, bi_sep = novad(est, tgt, vad, dev(g["vad_labels"]))
    assert close_db(sep_loss, *golden_tol(g, "comb_novad_sep")) and torch.equal(bi_sep.cpu(), idx)
    assert vad_loss.dim() == 0 and vad_loss.item() == 0 and bi_vad.dim() == 0 and bi_vad.item() == 0
    # learn_weight_bool: loss / (2 w^2) + log(1 + w^2) with w = 0.5 (combined_loss.py:101-103,111-112)
    learn = combined_loss.CombinedLoss(crit.criterion_separation, crit.criterion_vad,
                                       dict(cfg["combined_loss"], learn_weight_bool=True)).to(DEV)
    s2, v2, _, _ = learn(est, tgt, vad, dev(g["vad_labels"]))
    s1, v1, _, _ = crit(est, tgt, vad, dev(g["vad_labels"]))
    assert s2.is_cuda and abs(s2.item() - (2 * s1.item() + np.log(1.25))) <= 1e-5 * abs(s2.item())
    assert abs(v2.item() - (2 * v1.item() + np.log(1.25))) <= 1e-5 * abs(v2.item())


# ---- shapes where the kernel changes path, against the float64 restatement -------------------------------------

def check_against_restatement(r, est, tgt, mix, sdr_type="sisdr"):
    from sep_tfanet_vad_amd import evaluate
    pw = ref_pw(est, tgt, sdr_type)
    assert close_db(r["pw"], pw)
    min_loss, idx, gap = ref_perm(pw)
    print("permutation gaps (dB):", gap.tolist())
    # every row is compared: the cases are built so that no permutation is decided by the tolerance of pw
    assert bool((gap > 2 * TOL_DB).all()), "a case whose permutation losses agree to the tolerance checks nothing"
    assert torch.equal(r["perm"].cpu(), idx) and close_db(r["min_loss"], min_loss)
    sheet, pit_si, pit_snr, si_sdri = ref_sheet(est, tgt, mix, r["perm"].cpu())
    if mix is None:  # the mixture columns are those of a silent mixture; nothing reads them
        keep = [0, 1, 4, 5]
        assert close_db(r["sheet"][:, keep], sheet[:, keep]) and "si_sdri" not in r
    else:
        assert close_db(r["sheet"], sheet) and close_db(r["si_sdri"], si_sdri)
    assert close_db(r["loss"], r["min_loss"].double().mean().cpu()) and close_db(r["pit_si_sdr"], pit_si)
    assert close_db(r["pit_snr"], pit_snr)
    assert tuple(r["sheet"].shape) == (est.shape[0], len(evaluate.SHEET_COLUMNS))
    assert torch.equal(r["sep_reordered"].cpu(), torch.stack([est[b][r["perm"][b].cpu()] for b in range(est.shape[0])]))


def same_bits(a, b, keys=("pw", "min_loss", "perm", "sheet")):
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("N", [7, 1027, EV_CHUNK, EV_CHUNK + 1, 12345])
@pytest.mark.parametrize("B", [1, 3])
def test_score_batch_shapes_determinism_and_batch_invariance(B, N):
    """The float4 tail, fewer samples than a chunk, an exact chunk, a ragged last chunk; two calls give the same bits;
    row b of the batch has the bits of a call on that row alone (whose rows are aligned differently when N is odd)."""
    from sep_tfanet_vad_amd import evaluate
    est, tgt, mix = gaussian_case(B, N, 100 * N + B)
    e, t, m = est.to(DEV), tgt.to(DEV), mix.to(DEV)
    r = evaluate.score_batch(e, t, m)
    check_against_restatement(r, est, tgt, mix)
    again = evaluate.score_batch(e, t, m)
    assert same_bits(r, again) and torch.equal(r["means"], again["means"])
    for b in range(B):
        one = evaluate.score_batch(e[b:b + 1], t[b:b + 1], m[b:b + 1])
        assert all(torch.equal(one[k][0], r[k][b]) for k in ("pw", "min_loss", "perm", "sheet")), b


@pytest.mark.parametrize("sdr_type", ["sdsdr", "snr"])
def test_score_batch_other_sdr_types(sdr_type):
    from sep_tfanet_vad_amd import evaluate
    est, tgt, mix = gaussian_case(3, 5000, 77)
    check_against_restatement(evaluate.score_batch(est.to(DEV), tgt.to(DEV), mix.to(DEV), sdr_type=sdr_type),
                              est, tgt, mix, sdr_type)


def test_strided_unaligned_rows_and_no_mixture():
    """est as a speaker-strided view of a wider buffer with an odd row stride (rows off the 16-byte grid: the scalar
    path), tgt contiguous; the result has the bits of the contiguous call (both paths give each thread the same
    samples in the same order). Then the same without a mixture."""
    from sep_tfanet_vad_amd import evaluate
    B, N = 3, 5003
    est, tgt, mix = gaussian_case(B, N, 5)
    wide = torch.zeros(B, 2, N + 6, device=DEV)
    view = wide[:, :, 3:3 + N]
    view.copy_(est)
    assert not view.is_contiguous() and view.stride(1) % 4 != 0 and view.data_ptr() % 16 != 0
    r = evaluate.score_batch(view, tgt.to(DEV), mix.to(DEV))
    check_against_restatement(r, est, tgt, mix)
    assert same_bits(r, evaluate.score_batch(est.to(DEV), tgt.to(DEV), mix.to(DEV)))
    wide_mix = torch.zeros(B, N + 1, device=DEV)
    wide_mix[:, :N] = mix.to(DEV)
    assert same_bits(r, evaluate.score_batch(view, tgt.to(DEV), wide_mix[:, :N]))
    nomix = evaluate.score_batch(view, tgt.to(DEV))
    check_against_restatement(nomix, est, tgt, None)
    assert all(torch.equal(nomix[k], r[k]) for k in ("pw", "min_loss", "perm", "sep_reordered"))
    # an expanded (stride 0) mixture-as-estimate, as test.py:139-140 builds it, is copied, not misread
    rep = evaluate.eval_separation(mix.to(DEV).unsqueeze(1).expand(B, 2, N), tgt.to(DEV))
    mix2 = mix.unsqueeze(1).repeat(1, 2, 1)
    assert close_db(rep["pw"], ref_pw(mix2, tgt))


@pytest.mark.parametrize("T", [1, 32, 126])
@pytest.mark.parametrize("B", [1, 3, 19])
def test_vad_track_against_restatement(B, T):
    """BCE rows / mean / pairwise table, confusion counts and calc_vad under a permutation, for one frame, the model's
    T of 8000 samples and a T that is no multiple of the wave; B = 19 makes waves take a second utterance."""
    from sep_tfanet_vad_amd import evaluate
    gen = torch.Generator().manual_seed(1000 * B + T)
    labels = torch.randint(0, 3, (B, 2, T), generator=gen).float()
    vad = torch.rand(B, 2, T, generator=gen)
    vad[0, 0, 0], vad[-1, 1, -1] = 0.5, 1.0
    if T > 2:
        vad[0, 1, 1], labels[0, 0, 2] = 0.0, 0.3   # a label that is neither 0 nor 1: left out of the counts
    counts = torch.randint(0, 4, (B, 2, T), generator=gen)
    masks = torch.rand(B, 2, 257, T, generator=gen) * 0.49
    for b, s, t in np.ndindex(B, 2, T):
        n = (0, 64, 65, 257)[int(counts[b, s, t])]
        masks[b, s, torch.randperm(257, generator=gen)[:n], t] = 0.5
    idx = torch.tensor([[0, 1], [1, 0]])[torch.randint(0, 2, (B,), generator=gen)]
    ref = ref_vad(vad, labels, idx, masks)
    lab = labels.to(DEV)
    r = evaluate.eval_vad(vad.to(DEV), lab, idx.to(DEV), masks.to(DEV))
    for k in ("bce_rows", "bce_mean", "pw_ce"):
        d = (r[k].double().cpu() - ref[k]).abs()
        assert bool((d <= 1e-6 * ref[k].abs()).all()), (k, float(d.max()))
    for k in ("conf", "simple_vad", "conf_simple"):
        assert torch.equal(r[k].cpu(), ref[k]), k
    assert r["labels"] is lab and torch.equal(lab.cpu(), torch.where(labels == 2, torch.ones(()), labels))
    # fix_labels=False leaves the labels; no permutation is the identity; two calls give the same bits
    lab = labels.to(DEV)
    r0 = evaluate.eval_vad(vad.to(DEV), lab, None, None, fix_labels=False)
    assert torch.equal(lab.cpu(), labels) and "simple_vad" not in r0
    ref0 = ref_vad(vad, labels, torch.tensor([[0, 1]]).repeat(B, 1))
    assert torch.equal(r0["conf"].cpu(), ref0["conf"]) and torch.equal(r0["pw_ce"], r["pw_ce"])
    again = evaluate.eval_vad(vad.to(DEV), labels.to(DEV), idx.to(DEV), masks.to(DEV))
    assert all(torch.equal(again[k], r[k]) for k in ("bce_rows", "bce_mean", "pw_ce", "conf", "simple_vad", "conf_simple"))
    # row b does not depend on the batch
    one = evaluate.eval_vad(vad[:1].to(DEV), labels[:1].to(DEV), idx[:1].to(DEV), masks[:1].to(DEV))
    assert torch.equal(one["bce_rows"][0], r["bce_rows"][0]) and torch.equal(one["conf"][0], r["conf"][0])


# ---- the score sheet against the existing entries --------------------------------------------------------------

def test_sheet_matches_existing_metric_entries(g):
    from sep_tfanet_vad_amd import evaluate, metrics
    est, tgt, mix = dev(g["a_est"]), dev(g["a_tgt"]), dev(g["a_mix"])
    r = evaluate.score_batch(est, tgt, mix)
    col = {name: r["sheet"][:, i] for i, name in enumerate(evaluate.SHEET_COLUMNS)}
    mix2 = mix.unsqueeze(1).repeat(1, 2, 1)
    own, start = metrics.calc_sisdr(r["sep_reordered"], tgt), metrics.calc_sisdr(mix2, tgt)
    assert close_db(torch.stack([col["si_sdr_speaker0"], col["si_sdr_speaker1"]], 1), own.cpu())
    assert close_db(torch.stack([col["si_sdr_start_speaker0"], col["si_sdr_start_speaker1"]], 1), start.cpu())
    assert close_db(col["pit_si_sdr"], metrics.permutation_invariant_si_sdr(est, tgt)[0].cpu())
    assert close_db(col["pit_snr"], metrics.permutation_invariant_snr(est, tgt)[0].cpu())
    assert close_db(col["pit_si_sdr_start"], metrics.permutation_invariant_si_sdr(mix2, tgt)[0].cpu())
    assert close_db(col["pit_snr_start"], metrics.permutation_invariant_snr(mix2, tgt)[0].cpu())
    assert close_db(r["pit_si_sdr"], metrics.pit_si_sdr(est, tgt).cpu()) and close_db(r["pit_snr"], metrics.pit_snr(est, tgt).cpu())
    assert close_db(r["si_sdri"], metrics.si_sdri(est, tgt, mix).cpu())


def test_vad_confusion_reproduces_accuracy_vad(g):
    """The counts of vad_confusion give Accuracy_Vad's three numbers exactly (labels without 2s, as Accuracy_Vad
    compares values)."""
    from sep_tfanet_vad_amd import metrics
    vad, lab = dev(g["vad"]), dev(g["vad_labels_after"])
    conf = metrics.vad_confusion(vad, lab)
    assert conf.dtype == torch.int32 and tuple(conf.shape) == (3, 2, 4) and torch.equal(lab.cpu(), torch.from_numpy(g["vad_labels_after"]))
    assert int(conf.sum()) == vad.numel()
    acc, acc0, acc1 = metrics.Accuracy_Vad()(vad.clone(), lab)
    hits = (conf[:, :, 0] + conf[:, :, 3]).sum(0).cpu()
    n = vad.shape[0] * vad.shape[2]
    assert acc.item() == (hits.sum().float() / (2 * n)).item()
    assert acc0.item() == (hits[0].float() / n).item() and acc1.item() == (hits[1].float() / n).item()
    # thresholded predictions (what test.py:164 passes after Accuracy_Vad) count the same; a permutation swaps speakers
    hard = (vad > 0.5).float()
    assert torch.equal(metrics.vad_confusion(hard, lab), conf)
    swap = torch.tensor([[1, 0]] * 3, device=DEV)
    assert torch.equal(metrics.vad_confusion(vad.flip(1), lab, swap), conf)
    assert torch.equal(conf.cpu(), ref_conf((g_t(g["vad"]) > 0.5).long(), g_t(g["vad_labels_after"])))


def g_t(a):
    return torch.from_numpy(np.asarray(a))


def test_nan_prediction_counts_as_prediction_zero():
    """`pred > 0.5` is false for a NaN, so the pair is counted with prediction 0 (include/sepvad.h), not left out."""
    from sep_tfanet_vad_amd import metrics
    vad = torch.tensor([[[0.9, float("nan"), 0.2, float("nan")], [float("nan"), 0.7, 0.6, 0.1]]])
    lab = torch.tensor([[[1.0, 1.0, 0.0, 0.0], [0.0, 1.0, 2.0, 0.3]]])
    conf = metrics.vad_confusion(vad.to(DEV), lab.to(DEV)).cpu()
    assert conf.tolist() == [[[2, 0, 1, 1], [1, 0, 0, 2]]]     # (tn, fp, fn, tp); the 0.3 label is left out
    assert torch.equal(conf, ref_conf((vad > 0.5).long(), lab))


# ---- end to end ------------------------------------------------------------------------------------------------

def test_criterion_on_a_model_forward(g, state_dicts):
    """A B = 3, N = 8000 forward of the with_vad model scored by the criterion test.py builds from config_with_vad's
    dicts: four outputs on the device, the permutations of the float64 restatement, and score_batch on the same
    tensors (masks included) agreeing with it."""
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import evaluate, synth
    cfg = json.loads(str(g["criterion_config_json"]))
    net = pkg.SeparationModel(**config_of("with_vad"))
    net.load_state_dict(state_dicts["with_vad"], strict=True)
    net = net.eval().to(DEV)
    mixes, srcs = synth.make_batch(3, 8000, 31)
    x, tgt = torch.from_numpy(mixes).to(DEV), torch.from_numpy(srcs)
    tgt[1] = tgt[1].flip(0)
    gen = torch.Generator().manual_seed(3)
    labels = torch.randint(0, 3, (3, 2, 32), generator=gen).float()
    with torch.no_grad():
        sep, vad, _ = net(x)
        masks = net.mask_per_speaker
        crit = criterion_from_config(cfg)
        lab = labels.to(DEV)
        sep_loss, vad_loss, bi_vad, bi_sep = crit(sep, tgt.to(DEV), vad, lab)
    assert all(t.is_cuda for t in (sep_loss, vad_loss, bi_vad, bi_sep)) and bi_vad is bi_sep
    pw = ref_pw(sep.cpu(), tgt)
    min_loss, idx, gap = ref_perm(pw)
    print("permutation gaps (dB):", gap.tolist())
    assert bool((gap > 2 * TOL_DB).all()) and torch.equal(bi_sep.cpu(), idx)  # no row is left out
    assert close_db(sep_loss, min_loss.double().mean())
    ref = ref_vad(vad.cpu(), labels, bi_sep.cpu(), masks.cpu())
    assert abs(vad_loss.item() - ref["bce_mean"].item()) <= 1e-6 * abs(ref["bce_mean"].item())
    assert torch.equal(lab.cpu(), torch.where(labels == 2, torch.ones(()), labels))
    r = evaluate.score_batch(sep, tgt.to(DEV), x, vad, labels.to(DEV), masks)
    assert torch.equal(r["perm"], bi_sep) and torch.equal(r["loss"], sep_loss) and torch.equal(r["bce_mean"], vad_loss)
    assert torch.equal(r["simple_vad"].cpu(), ref["simple_vad"]) and torch.equal(r["conf_simple"].cpu(), ref["conf_simple"])
    assert torch.equal(r["conf"].cpu(), ref["conf"])
    check_against_restatement(r, sep.cpu(), tgt, mixes if torch.is_tensor(mixes) else torch.from_numpy(mixes))


# ---- edge cases ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sdr_type", ["sisdr", "sdsdr", "snr"])
def test_silence_gives_80_db_and_the_identity(sdr_type):
    """An all-zero target gives exactly 80.0 = -10 log10(1e-8) in every cell of every sdr_type, and so does an all-zero
    estimate for sisdr and sdsdr (for snr the projection is the target itself, model/sdr.py:73, and the reference
    returns -10 log10(<t,t> / (<t,t> + EPS) + EPS) there, about 0 dB); the tie keeps the identity."""
    from sep_tfanet_vad_amd import pit, sdr
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 2, 1027, generator=gen).to(DEV)
    zero = torch.zeros_like(x)
    loss = sdr.PairwiseNegSDR(sdr_type)
    crit = pit.PITLossWrapper(loss, pit_from="pw_mtx")
    cases = [(x, zero), (zero, zero)] + ([(zero, x)] if sdr_type != "snr" else [])
    for est, tgt in cases:
        assert torch.equal(loss(est, tgt), torch.full((2, 2, 2), 80.0, device=DEV))
        mean_loss, bi = crit(est, tgt, return_incides=True)
        assert mean_loss.item() == 80.0 and bi.tolist() == [[0, 1], [0, 1]]
    if sdr_type == "snr":
        assert close_db(loss(zero, x), ref_pw(zero.cpu(), x.cpu(), "snr"))


def test_host_tensors_and_grad_inputs_are_refused():
    from sep_tfanet_vad_amd import combined_loss, evaluate, metrics, pit, sdr
    x = torch.randn(2, 2, 500)
    with pytest.raises(RuntimeError, match="ROCm"):
        sdr.pairwise_neg_sisdr(x, x)
    with pytest.raises(RuntimeError, match="ROCm"):
        evaluate.score_batch(x.to(DEV), x)
    with pytest.raises(RuntimeError, match="ROCm"):
        metrics.pit_CE_vad(x.sigmoid(), x.sigmoid().to(DEV))
    w = x.to(DEV).requires_grad_(True)
    crit = pit.PITLossWrapper(sdr.pairwise_neg_sisdr, pit_from="pw_mtx")
    for fn in (lambda: sdr.pairwise_neg_sisdr(w, x.to(DEV)), lambda: crit(x.to(DEV), w),
               lambda: combined_loss.BinaryCrossEntropyLoss_Mean()(w.sigmoid(), x.to(DEV)),
               lambda: evaluate.score_batch(w, x.to(DEV))):
        with pytest.raises(RuntimeError, match="requires grad"):
            fn()
    with torch.no_grad():
        assert crit(w, x.to(DEV)).is_cuda
