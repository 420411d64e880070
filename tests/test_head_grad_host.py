"""head_grad_cases' restatement and closed form against the reference's own float64 autograd, the new ABI rows against the
header, and train_head's refusals (no GPU).

tests/golden/golden_head_grad.npz holds the float64 masks_b, the gradient at the trunk output and the six parameter
gradients of the real reference ``net.TCN.output`` (golden/make_head_grad_golden.py). The restatement's float64 results
must equal them to 1e-9 of each tensor's maximum, and so must the closed form of DESIGN.md section 16; pinned this way, the
restatement is the truth for the shapes too large to commit (test_gpu_head_grad.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import head_grad_cases as hc
from conftest import GOLDEN, REPO, config_of

TAGS = ("t2", "t3", "t11")
TOL = 1e-9


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_head_grad.npz"))


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close(a, ref, where):
    ref = t_(ref).double()
    err = float((a.double().reshape(ref.shape) - ref).abs().max())
    scale = float(ref.abs().max())
    print(where, "max error / tensor max:", err / scale if scale else err)
    assert err <= TOL * scale, where


def golden_rows(k, a):
    return a[list(hc.GOLDEN_ROWS)] if k == hc.P_V else a


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference(g, state_dicts, tag):
    assert tuple(g[f"{tag}_y"].shape[1:]) == (hc.CH, int(tag[1:]))
    r = hc.autograd_grads(t_(g[f"{tag}_y"]), hc.head_params(state_dicts["with_vad"]), t_(g[f"{tag}_G"]), torch.float64)
    close(r["masks"], g[f"{tag}_masks_f64"], f"{tag} masks")
    for k in ("y",) + hc.HEAD_PARAMS:
        close(golden_rows(k, r[k]), g[f"{tag}_{k}_f64"], f"{tag} {k}")


@pytest.mark.parametrize("tag", TAGS)
def test_closed_form_equals_the_reference(g, state_dicts, tag):
    cf = hc.closed_form(t_(g[f"{tag}_y"]), hc.head_params(state_dicts["with_vad"]), t_(g[f"{tag}_G"]))
    for k in ("y",) + hc.HEAD_PARAMS:
        close(golden_rows(k, cf[k]), g[f"{tag}_{k}_f64"], f"{tag} closed form {k}")


@pytest.mark.parametrize("kind", ("seeded", "zeros", "constant", "negative_alpha"))
def test_closed_form_equals_float64_autograd(state_dicts, kind):
    """The same on the edge values the device tests use: exact zeros in y (torch's convention: the slope alpha and no
    contribution to alpha's gradient), a constant utterance (var = 0) and a negative slope."""
    y, G = hc.seeded_case(3, 5, seed=40)
    p = {k: v.clone() for k, v in hc.head_params(state_dicts["with_vad"]).items()}
    if kind == "zeros":
        y[:, ::3] = 0.0
    elif kind == "constant":
        y[1] = 0.75
    elif kind == "negative_alpha":
        p[hc.P_ALPHA] = torch.tensor([-0.3])
    r = hc.autograd_grads(y, p, G, torch.float64)
    cf = hc.closed_form(y, p, G)
    for k in ("y",) + hc.HEAD_PARAMS:
        assert bool(torch.isfinite(cf[k]).all()), k
        close(cf[k], r[k].numpy(), f"{kind} {k}")


def test_new_abi_rows_match_the_header():
    from sep_tfanet_vad_amd import native, train_head
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(REPO, "include", "sepvad.h")).read(), flags=re.S)
    protos = {name: (" ".join(ret.split()), [" ".join(a.split()) for a in args.split(",")]) for ret, name, args in
              re.findall(r"^([\w \*]+?)\s*\b(sepvad_head_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    assert set(protos) == {"sepvad_head_scratch_bytes", "sepvad_head_forward", "sepvad_head_backward"}
    scalars = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name, (ret, args) in protos.items():
        restype, argtypes = native._ABI[name]
        assert restype is scalars[ret] and len(args) == len(argtypes), name
        for decl, t in zip(args, argtypes):
            assert (t is ctypes.c_void_p) if "*" in decl else (t is scalars[decl.split()[0]]), (name, decl)
    assert int(re.search(r"SEPVAD_HEAD_NPAR\s*=\s*(\d+)", src).group(1)) == train_head.HEAD_NPAR == 132611
    assert re.search(r"#define\s+SEPVAD_ABI_VERSION\s+2\b", src)
    assert train_head.HEAD_PARAMS == hc.HEAD_PARAMS
    lib = native.load_library()
    assert lib.sepvad_abi_version() == 2
    # the size query and the argument checks run without a device: nothing is launched for a bad argument
    assert lib.sepvad_head_scratch_bytes(0, 8) < 0 and lib.sepvad_head_scratch_bytes(1, 1) < 0
    assert lib.sepvad_head_scratch_bytes(32768, 8) < 0 and lib.sepvad_head_scratch_bytes(1, (1 << 20) + 1) < 0
    small, big = lib.sepvad_head_scratch_bytes(1, 2), lib.sepvad_head_scratch_bytes(64, 126)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    assert lib.sepvad_head_forward(None, 1, 2, None, None, 0, None, None) != 0
    assert b"sepvad_head_forward" in lib.sepvad_last_error()
    assert lib.sepvad_head_backward(None, None, 0, 0, 0, 1, 2, None, None, 0, None, None, None) != 0
    assert b"sepvad_head_backward" in lib.sepvad_last_error()


def test_train_head_refuses_before_any_library_call(monkeypatch):
    import sep_tfanet_vad_amd as pkg
    from sep_tfanet_vad_amd import native, train_head

    def no_library(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(native, "load_library", no_library)
    net = pkg.SeparationModel(**config_of("with_vad"))
    head = train_head.TrainableHead(net)
    y, _ = hc.seeded_case(2, 4, seed=41)
    with pytest.raises(RuntimeError, match="ROCm device"):
        head.from_trunk(y)
    for bad in (y[:, :255], y[:, :, :1], y[0], y.unsqueeze(0)):
        with pytest.raises(ValueError, match="expected y"):
            head.from_trunk(bad)
    three = pkg.SeparationModel(**config_of("with_vad"))
    three.num_spk = 3
    with pytest.raises(NotImplementedError, match="two speakers"):
        train_head.TrainableHead(three)
