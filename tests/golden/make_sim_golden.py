"""Expectations of the scene-simulation entries (csrc/sim.hip) -> tests/golden/golden_sim.npz (data only).

Convolution, mixing and normalisation: numpy in float64 on the inputs of tests/sim_cases.py (np.convolve(...)[:L],
np.std, np.min / np.max and the reference's expressions). Frame labels: the reference's own
convert_samples2frames_vad, taken from the reference tree when this script runs (the one function is extracted
from create_data/vad_labels2stft_labels.py with ast, the rest of that script writes files); the two edge rules of
its lines 52-56 and 62-66 are applied here. RIR expectations need no fixture of their own: golden_rir.npz.

    python tests/golden/make_sim_golden.py [reference root]
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sim_cases as sc  # noqa: E402


def reference_frames_fn(ref_root):
    path = os.path.join(ref_root, "create_data", "vad_labels2stft_labels.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "convert_samples2frames_vad"]
    ns = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["convert_samples2frames_vad"]


def frame_labels(fn, act, edge_mode):
    out = np.zeros((act.shape[0], 2 * act.shape[1] // 512 + 1))
    for r, row in enumerate(act.astype(np.int64)):
        out[r, 1:-1] = fn(row)
        zeros = np.zeros(256, dtype=np.int64)
        first = np.concatenate((zeros, row[:256])) if edge_mode == 0 else row[:256]
        last = np.concatenate((row[-256:], zeros)) if edge_mode == 0 else row[-256:]
        out[r, 0] = np.argmax(np.bincount(first))
        out[r, -1] = np.argmax(np.bincount(last))
    return out.astype(np.float32)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    d = {}
    for i, (x, h, L) in enumerate(sc.conv_inputs()):
        d[f"conv_y{i}"] = sc.conv_reference(x, h, L)[::sc.SUB]
    rev, dry, noise, snr = sc.mix_inputs()
    for p, (a, b) in enumerate(sc.MIX_AB):
        mix, stats = sc.mix_reference(rev, noise, snr, a, b)
        d[f"mix_stats{p}"] = stats
        d[f"mix{p}"] = mix[:, ::sc.SUB]
        for mode in (0, 1):
            d[f"targets{p}_mode{mode}"] = sc.targets_reference(dry, stats, mode, a, b)[:, :, ::sc.SUB]
    mix, stats = sc.mix_reference(rev, None, None, 1.8, 0.9)
    d["mix_nonoise_stats"] = stats
    fn = reference_frames_fn(ref_root)
    for L in (2048, 4096):
        act = sc.activity_tracks(L)
        for mode in (0, 1):
            d[f"frames_L{L}_edge{mode}"] = frame_labels(fn, act, mode)
    out = os.path.join(HERE, "golden_sim.npz")
    np.savez_compressed(out, **d)
    print({k: v.shape for k, v in d.items()}, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
