"""Golden vectors of the reference's streaming evaluation with known targets (run where the reference tree is,
never on the GPU box).

    python tests/golden/make_stream_eval_golden.py

Runs the reference's own ``model/online_class_known_targets.OnlineSaving.calc_online`` (:85-154) on the shimmed
reference model of make_golden.py (recipe weights), wrapped so that forward returns the six values the class unpacks
(:105,126), with the reference's ``PITLossWrapper(pairwise_neg_sisdr, "pw_mtx")`` as the separation criterion and each
similarity mode of ``test.py:96-106``: none, ``PITLossWrapper(nn.L1Loss(), "pw_pt")`` and
``PITLossWrapper(calc_sisdr_loss, "pw_pt")``. Every PIT decision of the run is recorded through the wrapper's
``find_best_perm`` (pairwise table and chosen indices), in a float32 and in a float64 run.

One file per case (tests/stream_eval_cases.CASES), data only: the per-window permutations and pairwise tables of both
runs, both scores, and the stitched signals. The three modes stitch the same hops under different permutations, so
the hops are stored once, un-permuted (``raw``), after checking that each mode's stitched signal is exactly ``raw``
under its recorded permutations. Inputs are ``synth.make_batch(2, N, seed)``; their SHA-256 is stored and the tests
regenerate them.

Which decisions count (asserted here, read by the tests): a decision is decided when the reference's gap between the
two permutations is at least ``l1_gap_min`` = 4e-4 for L1 (both sides may move by the 1e-4 waveform tolerance, so each
loss by at most 2e-4), or at least ``db_gap_min`` = 10 x the largest float32-vs-float64 difference of a dB gap in the
fixture (the GPU forward is allowed 1e-4 where the reference's own float32 noise is 2.7e-5, a factor 3.7; the rest is
margin). Window 0's similarity decision is never decided (the left pad leaves the window silent before its last hop:
the reference itself sits on a near-tie). No other decision of a case may be undecided.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import sep_tfanet_vad_amd as pkg  # noqa: E402
from make_golden import build, import_reference  # noqa: E402
from sep_tfanet_vad_amd import synth  # noqa: E402
from stream_eval_cases import CASES, MODES  # noqa: E402

L1_GAP_MIN = 4e-4


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class SixTuple:
    """The reference model behind the 6-tuple calc_online unpacks; forwards are cached by input (the three modes
    run the same windows)."""

    def __init__(self, net):
        self.net, self.cache = net, {}

    def __call__(self, x):
        key = (x.shape, sha(x.numpy()))
        if key not in self.cache:
            with torch.no_grad():
                self.cache[key] = self.net(x)[0]
        return self.cache[key].clone(), None, None, None, None, None


def recording(crit, log):
    orig = crit.find_best_perm

    def find_best_perm(pw_losses, perm_reduce=None, **kw):
        min_loss, idx = orig(pw_losses, perm_reduce=perm_reduce, **kw)
        log.append((pw_losses.detach().clone().numpy(), idx.clone().numpy()))
        return min_loss, idx
    crit.find_best_perm = find_best_perm
    return crit


def gap_of(pw):
    return (pw[..., 0, 0] + pw[..., 1, 1]) / 2 - (pw[..., 1, 0] + pw[..., 0, 1]) / 2


def run_reference(ref_known, ref_pit, ref_sdr, ref_loss, model, mix, tgt, save_sec, mode):
    log_t, log_s = [], []
    crit = recording(ref_pit.PITLossWrapper(loss_func=ref_sdr.pairwise_neg_sisdr, pit_from="pw_mtx"), log_t)
    sim = None
    if mode == "l1":
        sim = recording(ref_pit.PITLossWrapper(loss_func=torch.nn.L1Loss(), pit_from="pw_pt"), log_s)
    elif mode == "sisdr":
        sim = recording(ref_pit.PITLossWrapper(loss_func=ref_loss.calc_sisdr_loss, pit_from="pw_pt"), log_s)
    ons = ref_known.OnlineSaving(crit, model, "/nonexistent", "cpu", sim)
    ons.save_sec = save_sec
    stitched = []
    update = ons.update_online_signal

    def update_and_keep(est):  # the stitched signal before :143 reorders it against the targets
        update(est)
        stitched[:] = [ons.online_signal.clone()]
    ons.update_online_signal = update_and_keep
    ons.calc_online(mix, tgt, "golden", 0)
    assert ons.indx == 0 and len(ons.online_sisdr) == len(ons.reference_sisdr) == 1
    K = len(log_t) - 2  # the windows, then the whole-file PIT and the stitched signal's PIT
    assert not log_s or len(log_s) == K
    out = dict(K=K, pw_tgt=np.stack([p for p, _ in log_t[:K]]), perm_tgt=np.stack([i for _, i in log_t[:K]]),
               ref_perm=log_t[K][1], online_perm=log_t[K + 1][1], stitched=stitched[0].numpy(),
               online_final=ons.online_signal.numpy(), online_sisdr=ons.online_sisdr[0],
               reference_sisdr=ons.reference_sisdr[0])
    if log_s:
        out["pw_sim"] = np.stack([p for p, _ in log_s])
        out["perm_sim"] = np.stack([i for _, i in log_s])
    out["perm"] = out["perm_sim"] if log_s else out["perm_tgt"]
    return out


def main():
    ref_model, _, ref_pit = import_reference()
    import model.combined_loss as ref_loss
    import model.online_class_known_targets as ref_known
    import model.sdr as ref_sdr
    torch.set_num_threads(8)
    net, sd = build(ref_model, pkg.CONFIG_WITH_VAD)
    net64 = ref_model.SeparationModel(**pkg.CONFIG_WITH_VAD).double()
    net64.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=True)
    net64.eval()
    models = {"f32": (SixTuple(net), torch.float32), "f64": (SixTuple(net64), torch.float64)}
    runs, db_noise = {}, 0.0
    for name, N, save_sec, seed in CASES:
        mix, srcs = synth.make_batch(2, N, seed)
        for mode in MODES:
            for suffix, (model, dt) in models.items():
                r = run_reference(ref_known, ref_pit, ref_sdr, ref_loss, model, torch.from_numpy(mix).to(dt),
                                  torch.from_numpy(srcs).to(dt), save_sec, mode)
                runs[name, mode, suffix] = r
                print(name, mode, suffix, "K", r["K"], "online", r["online_sisdr"], "reference", r["reference_sisdr"])
            a, b = runs[name, mode, "f32"], runs[name, mode, "f64"]
            d = np.abs(gap_of(a["pw_tgt"]) - gap_of(b["pw_tgt"])).max()
            if mode == "sisdr":  # |gap|: window 0 may fall either way in the two runs, which exchanges the columns
                d = max(d, np.abs(np.abs(gap_of(a["pw_sim"]))[1:] - np.abs(gap_of(b["pw_sim"]))[1:]).max())
            print(name, mode, "float32-vs-float64 difference of the dB gaps:", d)
            db_noise = max(db_noise, d)
    db_gap_min = 10.0 * float(db_noise)
    print("largest float32-vs-float64 difference of a dB gap:", db_noise, "-> db_gap_min", db_gap_min)
    for name, N, save_sec, seed in CASES:
        mix, srcs = synth.make_batch(2, N, seed)
        out = dict(N=np.array(N), save_sec=np.array(float(save_sec)), seed=np.array(seed),
                   mix_sha256=np.array(sha(mix.astype(np.float32))), sources_sha256=np.array(sha(srcs.astype(np.float32))),
                   weights_seed=np.array(1234), l1_gap_min=np.array(L1_GAP_MIN), db_gap_min=np.array(db_gap_min),
                   db_gap_noise=np.array(float(db_noise)))
        raw = None
        for mode in MODES:
            a, b = runs[name, mode, "f32"], runs[name, mode, "f64"]
            K = a["K"]
            H = a["stitched"].shape[-1] // K
            # the decisions: every target PIT, and the similarity PIT of windows 1 .. K - 1
            g = np.abs(gap_of(a["pw_tgt"]))
            assert g.min() >= db_gap_min, f"{name} {mode}: target-PIT gap {g.min()} dB"
            if mode != "none":
                g = np.abs(gap_of(a["pw_sim"]))[1:]
                lim = L1_GAP_MIN if mode == "l1" else db_gap_min
                assert g.min() >= lim, f"{name} {mode}: similarity gap {g.min()} at window {1 + int(g.min(axis=1).argmin())}"
                print(name, mode, "similarity gaps: window 0", np.abs(gap_of(a["pw_sim"]))[0], "others >=", g.min())
                # window 0 may fall either way in the two runs; every later window follows it
                flip = (a["perm_sim"][0] != b["perm_sim"][0])[None, :, :]
                assert np.array_equal(a["perm_sim"][1:], np.where(flip, 1 - b["perm_sim"], b["perm_sim"])[1:])
            assert np.array_equal(a["perm_tgt"], b["perm_tgt"])
            assert np.array_equal(a["ref_perm"], b["ref_perm"])
            # the stitched signal is the un-permuted hops under the recorded permutations, to the bit
            hops = a["stitched"].reshape(2, 2, K, H)
            undo = np.empty_like(hops)
            for k in range(K):
                for bb in range(2):
                    undo[bb, a["perm"][k, bb], k] = hops[bb, :, k]
            if raw is None:
                raw = undo
            assert np.array_equal(raw, undo), f"{name} {mode}: the modes do not stitch the same hops"
            assert np.array_equal(a["online_final"], np.stack([a["stitched"][bb][a["online_perm"][bb]] for bb in range(2)]))
            out[f"{mode}_stitched_f64_maxdiff"] = np.array(np.abs(a["stitched"] - b["stitched"]).max()
                                                           if np.array_equal(a["perm"], b["perm"]) else np.nan)
            for key in ("pw_tgt", "perm_tgt", "pw_sim", "perm_sim", "perm", "ref_perm", "online_perm"):
                if key in a:
                    out[f"{mode}_{key}_f32"] = a[key]
                    out[f"{mode}_{key}_f64"] = b[key]
            for key in ("online_sisdr", "reference_sisdr"):
                out[f"{mode}_{key}_f32"] = np.array(a[key], np.float64)
                out[f"{mode}_{key}_f64"] = np.array(b[key], np.float64)
        out["raw"] = raw.reshape(2, 2, -1)
        fn = os.path.join(HERE, f"golden_stream_eval_{name}.npz")
        np.savez_compressed(fn, **out)
        size = os.path.getsize(fn)
        print(fn, size)
        assert size <= 1 << 20, "fixture above 1 MiB"


if __name__ == "__main__":
    main()
