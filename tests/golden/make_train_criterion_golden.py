"""Golden vectors of the reference's training criterion and its autograd gradients (run where the reference tree is,
never on the GPU box).

    python tests/golden/make_train_criterion_golden.py

Imports the reference as make_eval_golden.py does and runs ``CombinedLoss`` (``model/combined_loss.py:80-118``) over
``PITLossWrapper(pairwise_neg_sisdr, "pw_mtx")`` (``model/pit_wrapper.py``, ``model/sdr.py:48-86``) with autograd, in
float32 as the trainer runs it (``trainer/trainer.py:57-63``) and on float64 inputs (``torch.float32`` bound to float64
for the call, as make_eval_golden.as64). Only seeded inputs and the reference's outputs are written
(golden_train_criterion.npz): both losses, the permutation, d separation_loss / d pred_separation and
d vad_loss / d pred_vad in both precisions, and for one small case the separation gradient of every PW_CASES loss.

Cases (B = 3, the middle utterance's speakers swapped; the permutation gap is >= 1 dB, asserted):
  n3, n257, n4096, n4101  N below a float4, odd, one exact EV_CHUNK, a ragged second chunk; T = 1, 7, 130, 7.
                          n4096's signals are the first 4096 samples of n4101's (stored once).
  sil                     N = 257: utterance 0 with all-zero estimates, utterance 1 with all-zero targets
  one                     N = 1
Every VAD track has labels equal to 2 and probabilities exactly 0 and exactly 1 (where T allows). The reference's
gradient on silence and at N = 1 is a finite zero; asserted here.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from make_eval_golden import PW_CASES, as64, pw_key  # noqa: E402
from make_golden import import_reference  # noqa: E402

WEIGHTS = dict(weight_separation_loss=0.99, weight_vad_loss=0.01, learn_weight_bool=False)
CASES = (("n3", 3, 1), ("n257", 257, 7), ("n4096", 4096, 130), ("n4101", 4101, 7), ("sil", 257, 7), ("one", 1, 1))


def signals(rng, N):
    tgt = (0.1 * rng.standard_normal((3, 2, N))).astype(np.float32)
    est = (0.8 * tgt + 0.01 * rng.standard_normal(tgt.shape) + 0.01).astype(np.float32)
    est[1] = est[1, ::-1].copy()
    return est, tgt


def vad_track(rng, T):
    labels = (rng.random((3, 2, T)) > 0.45).astype(np.float32)
    labels[rng.random((3, 2, T)) > 0.8] = 2.0
    labels[0, 0, 0] = 2.0
    vad = np.where(labels > 0, 0.55 + 0.44 * rng.random((3, 2, T)), 0.45 * rng.random((3, 2, T))).astype(np.float32)
    # exact 0 and 1, each against a label it agrees with and one it contradicts
    vad[1, 0, 0], labels[1, 0, 0] = 0.0, 0.0
    vad[1, 1, 0], labels[1, 1, 0] = 1.0, 2.0
    vad[2, 0, 0], labels[2, 0, 0] = 0.0, 1.0
    vad[2, 1, 0], labels[2, 1, 0] = 1.0, 0.0
    return vad, labels


def main():
    import_reference()

    class _PitStandIn:
        def __init__(self, *args, **kwargs):
            pass
    sys.modules.setdefault("torchmetrics", types.SimpleNamespace(PIT=_PitStandIn, PermutationInvariantTraining=_PitStandIn))
    import model.combined_loss as ref_loss  # noqa: E402
    import model.pit_wrapper as ref_pit  # noqa: E402
    import model.sdr as ref_sdr  # noqa: E402

    rng = np.random.Generator(np.random.PCG64(5151))
    out = {}
    est_long, tgt_long = signals(rng, 4101)
    for tag, N, T in CASES:
        if tag == "n4101":
            est, tgt = est_long, tgt_long
        elif tag == "n4096":
            est, tgt = est_long[:, :, :4096].copy(), tgt_long[:, :, :4096].copy()
        else:
            est, tgt = signals(rng, N)
        if tag == "sil":
            est[0] = 0.0
            tgt[1] = 0.0
        vad, labels = vad_track(rng, T)
        if tag != "n4096":  # the tests slice n4101's
            out[f"{tag}_est"], out[f"{tag}_tgt"] = est, tgt
        out[f"{tag}_vad"], out[f"{tag}_labels"] = vad, labels
        for dt, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
            run = as64 if dt == torch.float64 else (lambda fn: fn())
            e = torch.from_numpy(est).to(dt).requires_grad_(True)
            v = torch.from_numpy(vad).to(dt).requires_grad_(True)
            t = torch.from_numpy(tgt).to(dt)
            lab = torch.from_numpy(labels.copy()).to(dt)
            crit_sep = ref_pit.PITLossWrapper(loss_func=ref_sdr.pairwise_neg_sisdr, pit_from="pw_mtx", perm_reduce=None)
            crit_vad = ref_pit.PITLossWrapper(loss_func=ref_loss.BinaryCrossEntropyLoss_Mean(), pit_from="pw_pt")
            comb = ref_loss.CombinedLoss(crit_sep, crit_vad, dict(WEIGHTS))

            def step():
                sep_loss, vad_loss, idx_vad, idx_sep = comb(e, t, v, lab)
                assert idx_vad is idx_sep
                sep_loss.backward()
                vad_loss.backward()
                return sep_loss, vad_loss, idx_sep
            sep_loss, vad_loss, idx = run(step)
            assert e.grad.dtype == dt and v.grad.dtype == dt
            assert bool(torch.isfinite(e.grad).all()) and bool(torch.isfinite(v.grad).all())
            out[f"{tag}_sep_{suffix}"] = sep_loss.detach().numpy()
            out[f"{tag}_vadloss_{suffix}"] = vad_loss.detach().numpy()
            out[f"{tag}_grad_est_{suffix}"] = e.grad.numpy()
            out[f"{tag}_grad_vad_{suffix}"] = v.grad.numpy()
            if suffix == "f32":
                out[f"{tag}_idx"] = idx.numpy()
                out[f"{tag}_labels_after"] = lab.numpy()
                assert (lab == 2).sum() == 0 and (labels == 2).sum() >= 2
            else:
                assert np.array_equal(out[f"{tag}_idx"], idx.numpy())
            pw = ref_sdr.pairwise_neg_sisdr(e.detach(), t).numpy()
            gap = np.abs((pw[:, 0, 0] + pw[:, 1, 1]) / 2 - (pw[:, 1, 0] + pw[:, 0, 1]) / 2)
            if tag == "sil":  # silence ties at 80 dB and keeps the identity; the reference's gradient is a finite zero
                assert gap[2] >= 1.0 and not e.grad[:2].any() and e.grad[2].any()
            elif tag == "one":
                assert not e.grad.any()
            else:
                assert gap.min() >= 1.0, f"{tag}: permutation losses within {gap.min()} dB"
                assert idx.tolist() == [[0, 1], [1, 0], [0, 1]]
                assert e.grad.abs().amax(-1).min() > 0
    # ---- every PW_CASES loss on the small odd case: the separation gradient alone
    est, tgt = out["n257_est"], out["n257_tgt"]
    for dt, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
        for sdr_type, zm, tl in PW_CASES:
            key = pw_key(sdr_type, zm, tl)
            e = torch.from_numpy(est).to(dt).requires_grad_(True)
            crit = ref_pit.PITLossWrapper(ref_sdr.PairwiseNegSDR(sdr_type, zm, tl), pit_from="pw_mtx")
            loss, idx = crit(e, torch.from_numpy(tgt).to(dt), return_incides=True)
            loss.backward()
            assert bool(torch.isfinite(e.grad).all())
            out[f"n257_{key}_loss_{suffix}"] = loss.detach().numpy()
            out[f"n257_{key}_grad_est_{suffix}"] = e.grad.numpy()
            if suffix == "f32":
                out[f"n257_{key}_idx"] = idx.numpy()
            else:
                assert np.array_equal(out[f"n257_{key}_idx"], idx.numpy())
    fn = os.path.join(HERE, "golden_train_criterion.npz")
    np.savez_compressed(fn, **out)
    size = os.path.getsize(fn)
    print(sorted(out), size)
    assert size <= 1 << 20, size
    for tag, _, _ in CASES:
        g32, g64 = out[f"{tag}_grad_est_f32"].astype(np.float64), out[f"{tag}_grad_est_f64"]
        rowmax = np.maximum(np.abs(g64).max(-1, keepdims=True), 1e-300)
        print(tag, "reference float32 autograd, worst |g32 - g64| / rowmax:", float((np.abs(g32 - g64) / rowmax).max()))


if __name__ == "__main__":
    main()
