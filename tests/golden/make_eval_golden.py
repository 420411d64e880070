"""Golden vectors of the reference's evaluation criterion (run where the reference tree is, never on the GPU box).

    python tests/golden/make_eval_golden.py

Imports the reference's ``model/sdr.py`` (``PairwiseNegSDR``, :7-86), ``model/pit_wrapper.py`` (``PITLossWrapper``),
``model/combined_loss.py`` (``BinaryCrossEntropyLoss_Mean``, ``CombinedLoss``), ``model/metric.py`` (``pit_CE_vad``,
:264) and ``Our_utils/utils_test.py`` (``calc_vad``, :67-73) through the offline stand-ins of make_golden.py and the
``torchmetrics`` stand-in of make_metric_golden.py. Inputs are seeded; only inputs, the reference's outputs and the
criterion dicts of ``config_with_vad.json`` (settings) are written (golden_eval.npz).

Every floating-point output is stored twice: ``<name>_f32`` as the reference computes it, and ``<name>_f64`` from the
same reference code on float64 inputs (for ``BinaryCrossEntropyLoss_Mean``, whose ``.to(torch.float32)`` is spelled
out in its body, with that name bound to float64 for the call). Their difference is the reference's own rounding
noise, which the GPU tests use as the tolerance floor.
"""
from __future__ import annotations

import json
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from make_golden import REF, import_reference  # noqa: E402
from sep_tfanet_vad_amd import synth  # noqa: E402

PW_CASES = [("sisdr", True, True), ("sisdr", False, True), ("sdsdr", True, True), ("sdsdr", False, True),
            ("snr", True, True), ("snr", False, True), ("sisdr", True, False)]


def pw_key(sdr_type, zero_mean, take_log):
    return f"pw_{sdr_type}_zm{int(zero_mean)}" + ("" if take_log else "_nolog")


def as64(fn):
    """Run fn with torch.float32 bound to float64 (the reference's BCE casts its labels by that name)."""
    with mock.patch.object(torch, "float32", torch.float64):
        return fn()


def separation_case(tag, est, tgt, ref_sdr, ref_pit, out):
    out[f"{tag}_est"], out[f"{tag}_tgt"] = est, tgt
    for dt, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
        e, t = torch.from_numpy(est).to(dt), torch.from_numpy(tgt).to(dt)
        for sdr_type, zm, tl in PW_CASES:
            out[f"{tag}_{pw_key(sdr_type, zm, tl)}_{suffix}"] = ref_sdr.PairwiseNegSDR(sdr_type, zm, tl)(e, t).numpy()
        crit = ref_pit.PITLossWrapper(ref_sdr.pairwise_neg_sisdr, pit_from="pw_mtx")
        loss = crit(e, t)
        loss_i, idx = crit(e, t, return_incides=True)
        loss_e, reordered = crit(e, t, return_est=True)
        loss_b, reordered_b, idx_b = crit(e, t, return_est=True, return_incides=True)
        assert loss == loss_i == loss_e == loss_b and torch.equal(idx, idx_b) and torch.equal(reordered, reordered_b)
        # the reordered estimates are a gather by the indices (exact): the tests rebuild them from est and pit_idx
        assert torch.equal(reordered, torch.stack([e[b][idx[b]] for b in range(e.shape[0])]))
        pw = out[f"{tag}_{pw_key('sisdr', True, True)}_{suffix}"]
        gap = np.abs((pw[:, 0, 0] + pw[:, 1, 1]) / 2 - (pw[:, 1, 0] + pw[:, 0, 1]) / 2)
        assert gap.min() >= 1.0, f"{tag}: permutation losses within {gap.min()} dB"
        out[f"{tag}_pit_loss_{suffix}"] = loss.numpy()
        min_loss, _ = ref_pit.PITLossWrapper.find_best_perm(torch.from_numpy(pw))
        out[f"{tag}_pit_min_loss_{suffix}"] = min_loss.numpy()
        if suffix == "f32":
            out[f"{tag}_pit_idx"] = idx.numpy()
        else:
            assert np.array_equal(out[f"{tag}_pit_idx"], idx.numpy())


def main():
    import_reference()  # shims on sys.path, turtle stub, reference root importable

    class _PitStandIn:  # metric.py:255-258 instantiate PIT(...) at import; never called here
        def __init__(self, *args, **kwargs):
            pass
    sys.modules.setdefault("torchmetrics", types.SimpleNamespace(PIT=_PitStandIn, PermutationInvariantTraining=_PitStandIn))
    import model.combined_loss as ref_loss  # noqa: E402
    import model.metric as ref_metric  # noqa: E402
    import model.pit_wrapper as ref_pit  # noqa: E402
    import model.sdr as ref_sdr  # noqa: E402
    try:
        from Our_utils.utils_test import calc_vad as ref_calc_vad  # pulls plotting modules in
    except ImportError:
        # utils_test.py imports matplotlib / soundfile at the top; run its calc_vad (:67-73) alone
        src = open(os.path.join(REF, "Our_utils", "utils_test.py")).read()
        start = src.index("def calc_vad(")
        scope = {"torch": torch}
        exec(compile(src[start:], "utils_test.py", "exec"), scope)
        ref_calc_vad = scope["calc_vad"]

    rng = np.random.Generator(np.random.PCG64(4242))
    out = {}
    # ---- separation: B = 3, N = 8000 (T = 32), the middle row's speakers swapped
    mixes, srcs = synth.make_batch(3, 8000, 900)
    tgt = srcs.astype(np.float32)
    noise = rng.standard_normal(tgt.shape).astype(np.float32)
    est = (0.8 * tgt + 0.05 * noise + 0.01).astype(np.float32)
    est[1] = est[1, ::-1].copy()
    out["a_mix"] = mixes.astype(np.float32)
    separation_case("a", est, tgt, ref_sdr, ref_pit, out)
    assert out["a_pit_idx"].tolist() == [[0, 1], [1, 0], [0, 1]]
    # ---- B = 1, N = 1027 from an active region (the first ~1000 samples of a synth source are silent)
    _, long_src = synth.make_batch(1, 8000, 911)
    tgt_b = long_src[:, :, 3000:4027].astype(np.float32)
    assert np.abs(tgt_b).max(axis=-1).min() > 1e-3
    est_b = (0.7 * tgt_b[:, ::-1] + 0.1 * rng.standard_normal(tgt_b.shape) - 0.02).astype(np.float32)
    separation_case("b", est_b, tgt_b, ref_sdr, ref_pit, out)
    assert out["b_pit_idx"].tolist() == [[1, 0]]

    # ---- the VAD track: B = 3, T = 32; labels with 2s, one all-silent speaker, probabilities exactly 0, 1 and 0.5
    B, T = 3, 32
    labels = (rng.random((B, 2, T)) > 0.45).astype(np.float32)
    labels[rng.random((B, 2, T)) > 0.85] = 2.0
    labels[2, 1] = 0.0
    vad = np.where(labels > 0, 0.55 + 0.44 * rng.random((B, 2, T)), 0.45 * rng.random((B, 2, T))).astype(np.float32)
    flip = rng.random((B, 2, T)) > 0.8
    vad[flip] = 1.0 - vad[flip]
    vad[0, 0, :3] = [0.0, 1.0, 0.5]
    vad[1, 1, 4:7] = [0.5, 0.0, 1.0]
    vad = vad[:, ::-1].copy()  # the VAD tracks come out swapped: pit_CE_vad (one permutation per batch) picks (1, 0)
    assert (labels == 2).sum() >= 10 and set(np.unique(labels)) == {0.0, 1.0, 2.0}
    out["vad"], out["vad_labels"] = vad, labels
    for dt, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
        run = as64 if dt == torch.float64 else (lambda fn: fn())
        v = torch.from_numpy(vad).to(dt)

        def fresh():
            return torch.from_numpy(labels.copy()).to(dt)
        lab = fresh()
        out[f"bce_{suffix}"] = run(lambda: ref_loss.BinaryCrossEntropyLoss_Mean()(v, lab)).numpy()
        if suffix == "f32":
            out["vad_labels_after"] = lab.numpy()  # mutated in place: 2 -> 1 (combined_loss.py:130-131)
            assert (out["vad_labels_after"] == 2).sum() == 0 and not np.array_equal(out["vad_labels_after"], labels)
        # pit_CE_vad (metric.py:264): PITLossWrapper(BinaryCrossEntropyLoss_Mean(), "pw_pt")
        crit = ref_pit.PITLossWrapper(loss_func=ref_loss.BinaryCrossEntropyLoss_Mean(), pit_from="pw_pt")
        assert isinstance(ref_metric.pit_CE_vad, ref_pit.PITLossWrapper) and ref_metric.pit_CE_vad.pit_from == "pw_pt"
        pw = run(lambda: ref_pit.PITLossWrapper.get_pw_losses(ref_loss.BinaryCrossEntropyLoss_Mean(), v, fresh()))
        assert torch.equal(pw[0], pw[1]) and torch.equal(pw[0], pw[2])  # a scalar loss: every batch row alike
        gap = abs(float((pw[0, 0, 0] + pw[0, 1, 1]) / 2 - (pw[0, 1, 0] + pw[0, 0, 1]) / 2))
        assert gap >= 0.05 * float(pw[0].abs().max()), "pit_CE_vad: the two permutations are too close"
        out[f"ce_pw_{suffix}"] = pw[0].numpy()
        lab = fresh()
        loss, reordered, idx = run(lambda: crit(v, lab, return_est=True, return_incides=True))
        assert torch.equal(reordered, torch.stack([v[b][idx[b]] for b in range(B)]))
        assert float(run(lambda: crit(v, fresh()))) == float(loss)
        out[f"ce_loss_{suffix}"] = loss.numpy()
        if suffix == "f32":
            out["ce_idx"] = idx.numpy()
            assert out["ce_idx"].tolist() == [[1, 0]] * B
            assert np.array_equal(lab.numpy(), out["vad_labels_after"])  # pit_CE_vad mutates its labels as well
        else:
            assert np.array_equal(out["ce_idx"], idx.numpy())
        # CombinedLoss (combined_loss.py:80-118) built as test.py:49-64 builds it
        e, t = torch.from_numpy(est).to(dt), torch.from_numpy(tgt).to(dt)
        for name, weights in (("shipped", dict(weight_separation_loss=0.99, weight_vad_loss=0.01, learn_weight_bool=False)),
                              ("novad", dict(weight_separation_loss=1.0, weight_vad_loss=0, learn_weight_bool=False))):
            crit_sep = ref_pit.PITLossWrapper(loss_func=ref_sdr.pairwise_neg_sisdr, pit_from="pw_mtx", perm_reduce=None)
            comb = ref_loss.CombinedLoss(crit_sep, crit, weights)
            sep_loss, vad_loss, idx_vad, idx_sep = run(lambda: comb(e, t, v, fresh()))
            out[f"comb_{name}_sep_{suffix}"] = sep_loss.numpy()
            out[f"comb_{name}_vad_{suffix}"] = np.asarray(vad_loss.numpy(), dtype=np.float64 if name == "novad" else None)
            if suffix == "f32":
                out[f"comb_{name}_idx_sep"] = idx_sep.numpy()
                out[f"comb_{name}_idx_vad"] = idx_vad.numpy()
            if name == "novad":
                assert vad_loss.item() == 0 and idx_vad.item() == 0 and vad_loss.dim() == 0
            else:
                assert idx_vad is idx_sep
    # ---- calc_vad: masks [3, 2, 257, 32] with per-frame counts on both sides of 257 * 0.25 = 64.25
    masks = (0.49 * rng.random((B, 2, 257, T))).astype(np.float32)
    counts = rng.choice([0, 30, 64, 65, 66, 128, 257], size=(B, 2, T))
    counts[0, 0, :2] = [64, 65]
    for b in range(B):
        for s in range(2):
            for t in range(T):
                bins = rng.permutation(257)[:counts[b, s, t]]
                masks[b, s, bins, t] = (0.5 + 0.5 * rng.random(len(bins))).astype(np.float32)
                if len(bins):
                    masks[b, s, bins[0], t] = 0.5  # the threshold itself counts (>=)
    simple = ref_calc_vad(torch.from_numpy(masks)).numpy()
    assert np.array_equal(simple, (counts >= 65).astype(np.int64)) and 0 < simple.mean() < 1
    out.update(masks=masks, masks_counts=counts.astype(np.int32), simple_vad=simple)
    # ---- the criterion's settings as the shipped config spells them (test.py:49-71 reads these dicts)
    cfg = json.load(open(os.path.join(REF, "config_with_vad.json")))
    out["criterion_config_json"] = np.array(json.dumps({k: cfg[k] for k in
                                                        ("loss_separation", "loss_vad", "combined_loss", "metrics")}))
    fn = os.path.join(HERE, "golden_eval.npz")
    np.savez_compressed(fn, **out)
    print(sorted(out), os.path.getsize(fn))
    for k in sorted(out):
        if k.endswith("_f32") and out[k].size <= 12:
            print(k, out[k].ravel(), np.abs(out[k].astype(np.float64) - out[k[:-3] + "f64"]).max())


if __name__ == "__main__":
    main()
