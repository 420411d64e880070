"""Host-side contract of the drop-in (no GPU): kwargs, state_dict keys, errors, C-ABI exports."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import CONFIGS, GOLDEN, REPO, config_of


@pytest.mark.parametrize("cname", CONFIGS)
def test_state_dict_keys_match_reference(cname):
    import sep_tfanet_vad_amd as pkg
    ref = json.load(open(os.path.join(GOLDEN, f"state_dict_keys_{cname}.json")))
    net = pkg.SeparationModel(**config_of(cname))
    mine = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert mine == {k: s for k, s in ref}
    assert len(mine) == (719 if cname == "with_vad" else 671)


@pytest.mark.parametrize("cname", CONFIGS)
def test_load_state_dict_strict(cname, state_dicts):
    import sep_tfanet_vad_amd as pkg
    net = pkg.SeparationModel(**config_of(cname))
    net.load_state_dict(state_dicts[cname], strict=True)
    net.eval()
    assert net.casual is False and net.n_fftBins_h == 257  # attributes set from kwargs


def test_param_spec_matches_module():
    import sep_tfanet_vad_amd as pkg
    for cname in CONFIGS:
        cfg = config_of(cname)
        net = pkg.SeparationModel(**cfg)
        spec = {n: tuple(s) for n, s, _ in pkg.param_spec(cfg)}
        assert spec == {k: tuple(v.shape) for k, v in net.state_dict().items()}


def test_forward_contract_errors():
    import sep_tfanet_vad_amd as pkg
    net = pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
    with pytest.raises(AssertionError):
        net(torch.zeros(1, 2, 8000))  # model/model.py:406
    with pytest.raises(RuntimeError, match="ROCm device"):
        net(torch.zeros(1, 8000))     # no CPU fallback


@pytest.mark.parametrize("bad", [dict(casual=True), dict(skip=True), dict(weight_norm=False),
                                 dict(num_spk=3), dict(n_fftBins=256, BN_dim=128, H_dim=256)])
def test_unsupported_configs_fail_loudly(bad):
    import sep_tfanet_vad_amd as pkg
    with pytest.raises(NotImplementedError):
        pkg.SeparationModel(**dict(pkg.CONFIG_WITH_VAD, **bad))


def _header(comments=False):
    src = open(os.path.join(REPO, "include", "sepvad.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)


_C_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float,
              "char": ctypes.c_char, "sepvad_handle": ctypes.c_void_p}


def _is_pointer_like(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _header_prototypes():
    """name -> (return type text, [argument declaration text]) of every `ret sepvad_xxx(args);` of the header."""
    protos = {}
    for ret, name, args in re.findall(r"^([\w \*]+?)\s*\b(sepvad_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header(), flags=re.M):
        args = [" ".join(a.split()) for a in args.split(",")]
        protos[name] = (" ".join(ret.split()), [] if args == ["void"] else args)
    return protos


def _header_constants():
    """Every `#define NAME integer` and enumerator of the header."""
    src = _header()
    consts = {k: int(v, 0) for k, v in re.findall(r"^#define[ \t]+(SEPVAD_\w+)[ \t]+(-?\w+)[ \t]*$", src, flags=re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", src, flags=re.S):
        nxt = 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, val = (p.strip() for p in item.partition("="))
            consts[name] = nxt = int(val, 0) if val else nxt
            nxt += 1
    return consts


def test_ctypes_signatures_match_the_header():
    """Every prototype of include/sepvad.h against native's ABI table: the names (both ways, and in the library),
    the return type, the argument count and every argument's class."""
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    protos = _header_prototypes()
    mentioned = set(re.findall(r"\b(sepvad_[a-z0-9_]+)\s*\(", _header(comments=True)))
    assert {"sepvad_criterion_coef", "sepvad_criterion_backward"} <= mentioned
    assert mentioned == set(native.EXPORTED_SYMBOLS) == set(protos)
    assert len(protos) == len(native.EXPORTED_SYMBOLS)  # a prototype the pattern misses fails here
    for s in native.EXPORTED_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.sepvad_abi_version() == 2 == _header_constants()["SEPVAD_ABI_VERSION"]
    for name, (ret, args) in protos.items():
        restype, argtypes = native._ABI[name]
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name  # load_library applied the table
        want = None if ret == "void" else ctypes.c_char_p if ret == "const char*" else _C_SCALARS[ret]
        assert restype is want, (name, ret, restype)
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            if "*" in decl:
                assert _is_pointer_like(t), (name, i, decl, t)
            else:
                assert t is _C_SCALARS[decl.replace("const ", "").split()[0]], (name, i, decl, t)


def test_ctypes_structs_match_the_header():
    """Field names in order, element type and array length of the header's structs against the ctypes mirrors."""
    from sep_tfanet_vad_amd import native
    structs = dict(re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", _header(), flags=re.S))
    assert set(structs) == {"SepVadConfig", "SepVadInferKw", "SepVadOutputs", "SepVadRirDesc", "SepVadRirJob"}
    for sname, body in structs.items():
        want = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            ctype, _, names = decl.partition(" ")  # `int32_t a`, `float* sep`, `double s[3], r[3], L[3]`
            base = ctypes.c_void_p if "*" in ctype else _C_SCALARS[ctype]
            for item in names.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", item.strip())
                want.append((m.group(1), base, int(m.group(2)) if m.group(2) else None))
        got = [(n, getattr(t, "_type_", t) if hasattr(t, "_length_") else t, getattr(t, "_length_", None))
               for n, t in getattr(native, sname)._fields_]
        assert got == want, sname


def test_python_constants_match_the_header():
    """The header constants that the Python side restates."""
    from sep_tfanet_vad_amd import evaluate, inference, native, online_known, pit, train_criterion
    c = _header_constants()

    def by_name(prefix):  # SEPVAD_SDR_SISDR -> "sisdr"
        return {k[len(prefix):].lower(): v for k, v in c.items() if k.startswith(prefix)}

    assert pit.PIT_SCRATCH_BYTES == c["SEPVAD_PIT_SCRATCH_BYTES"]
    assert inference.NORM_SCRATCH_BYTES == c["SEPVAD_NORM_SCRATCH_BYTES"]
    assert native.RIR_MAX_IMAGES == c["SEPVAD_RIR_MAX_IMAGES"]
    assert (online_known.SE_NONE, online_known.SE_L1, online_known.SE_SISDR) == \
        (c["SEPVAD_SE_NONE"], c["SEPVAD_SE_L1"], c["SEPVAD_SE_SISDR"])
    assert evaluate.SDR_TYPES == by_name("SEPVAD_SDR_")
    for prefix in ("SEPVAD_LN_", "SEPVAD_PREC_"):
        names = [k for k in c if k.startswith(prefix)]
        assert len(names) >= 3 and all(getattr(native, k) == c[k] for k in names), prefix
    assert native.PRECISIONS == by_name("SEPVAD_PREC_") and native.WEIGHT_LO == by_name("SEPVAD_WLO_")
    assert len(evaluate.SHEET_COLUMNS) == c["SEPVAD_EV_COLS"]
    assert len(evaluate.MEANS) == 1 + max(v for k, v in c.items() if k.startswith("SEPVAD_EV_MEAN_"))
    assert train_criterion.CRIT_COEF == c["SEPVAD_CRIT_COEF"]


def test_library_is_built_from_this_tree():
    """The loaded library's source hash (sepvad_build_id) equals the hash of this tree's sources (buildid.py)."""
    from sep_tfanet_vad_amd import native
    if os.environ.get("SEPVAD_LIB"):
        pytest.skip("SEPVAD_LIB: an alternative build on purpose")
    assert native.build_id() == native.tree_build_id()


def test_library_rejects_bad_config_without_gpu():
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    c = native.make_config(dict(config_of("with_vad"), n_fftBins=1024, BN_dim=512, H_dim=1024))
    h = lib.sepvad_create(ctypes.byref(c), None, None, None, 0, 0)
    assert not h
    assert b"" != lib.sepvad_last_error()


def test_inference_kw_struct():
    from sep_tfanet_vad_amd import native
    assert native.make_kw({}) is None and native.make_kw(None) is None
    k = native.make_kw(dict(filter_signals_by_smo_vad=True, filter_signals_by_unsmo_vad=False,
                            length_smoothing_filter=5, threshold_activated_vad=0.3, return_smoothed_vad=True))
    assert k.enabled == 1 and k.filter_signals_by_smo_vad == 1 and abs(k.threshold_activated_vad - 0.3) < 1e-7
    with pytest.raises(KeyError):  # the reference indexes the keys directly
        native.make_kw({"threshold_activated_vad": 0.5})


def test_resample_filter_matches_restatement():
    """Host filter of sepvad_resample_filter vs the float64 restatement of torchaudio's kernel (no GPU)."""
    import numpy as np
    from oracle.prep_ref import sinc_kernel
    from sep_tfanet_vad_amd.inference import resample_filter
    for o, n in ((8000, 16000), (44100, 16000), (22050, 16000), (48000, 16000), (16000, 8000)):
        taps, info = resample_filter(o, n)
        k, width, oo, nn = sinc_kernel(o, n)
        assert info == (nn, 2 * width + oo, oo, width)
        assert np.abs(taps - k[:, 0, :].numpy()).max() <= 1e-7


def test_e4m3_encoder_matches_torch():
    """The packer's e4m3 encoder (weight lo plane of the fused TCN, include/sepvad.h SEPVAD_WLO_E4M3) vs torch's
    float8_e4m3fn cast (OCP, round to nearest even): every finite magnitude class, ties, subnormals, saturation."""
    import numpy as np
    import torch
    from sep_tfanet_vad_amd import native
    lib = native.load_library()
    rng = np.random.default_rng(7)
    x = np.concatenate([
        rng.standard_normal(20000) * np.exp2(rng.uniform(-12, 9, 20000)),      # every binade of the range
        # all 256 codes' values and the midpoints between neighbouring codes (ties to even)
        torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy(),
        np.array([0.0, -0.0, 2.0 ** -10, 3 * 2.0 ** -11, 2.0 ** -9 * 1.5, 440.0, 448.0, 449.0, 1e4, -1e4]),
    ]).astype(np.float32)
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    fin = np.sort(np.unique(codes[np.isfinite(codes)]))
    x = np.concatenate([x, ((fin[1:] + fin[:-1]) / 2).astype(np.float32)])
    x = x[np.isfinite(x)]
    out = np.zeros(x.size, np.uint8)
    assert lib.sepvad_e4m3_encode(x.ctypes.data, out.ctypes.data, x.size) == 0
    got = torch.from_numpy(out).view(torch.float8_e4m3fn).float().numpy()
    want = torch.from_numpy(np.clip(x, -448, 448)).to(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(got, want)
    # the lo plane's range: |lo| <= 2^-12 of a row-scaled weight, stored * 2^19 -> <= 128, 4 significant bits
    lo = (rng.uniform(-1, 1, 4096) * 2.0 ** -12).astype(np.float32)
    assert lib.sepvad_e4m3_encode((lo * 2 ** 19).ctypes.data, out.ctypes.data, 4096) == 0
    back = torch.from_numpy(out[:4096].copy()).view(torch.float8_e4m3fn).float().numpy() / 2 ** 19
    assert np.all(np.abs(back - lo) <= np.abs(lo) * 2.0 ** -4 + 2.0 ** -29)


def test_packer_host_check():
    """tools/pack_check.cpp, the stand-alone check of csrc/pack.h (no GPU): the fp16 split error, the int8 lo plane, the
    fused TCN's blobs against the planes and parameters they are assembled from, and the packer's two errors."""
    import subprocess
    csrc = os.path.join(REPO, "sep-tfanet-vad_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "ARCH=gfx950", "pack_check"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "\nok\n" in r.stdout  # (after the digests: every case passed)


def test_unknown_weight_lo_is_rejected(monkeypatch):
    """SEPVAD_WLO is validated in both layers (the C library refuses the same values at sepvad_create)."""
    import sep_tfanet_vad_amd as pkg
    monkeypatch.setenv("SEPVAD_WLO", "int8")
    with pytest.raises(ValueError, match="SEPVAD_WLO"):
        pkg.SeparationModel(**pkg.CONFIG_WITH_VAD)
    monkeypatch.setenv("SEPVAD_WLO", "e4m3")
    assert pkg.SeparationModel(**pkg.CONFIG_WITH_VAD).native_weight_lo == "e4m3"


def test_dump_outputs_samples_above_its_budget(tmp_path):
    """dump_outputs on host tensors: float64 kept, complex as (re, im) pairs, and above the budget a fixed sample whose
    size keeps all files together within it: the same elements for the same shapes."""
    import numpy as np
    import bench
    a = torch.arange(5 * 10 ** 6, dtype=torch.float32).reshape(5, -1)          # 20 MB
    c = torch.complex(torch.arange(7 * 10 ** 6, dtype=torch.float32), torch.ones(7 * 10 ** 6))  # 56 MB
    e = torch.arange(10, dtype=torch.float64)
    for sub in ("r1", "r2"):
        bench.dump_outputs(str(tmp_path / sub), {"a": a, "c": c, "e": e, "none": 0})
    out = {n: np.load(str(tmp_path / "r1" / f"{n}.npy")) for n in ("a", "c", "e")}
    assert sorted(f.name for f in (tmp_path / "r1").iterdir()) == ["a.npy", "c.npy", "e.npy"]
    assert out["a"].dtype == np.float32 and out["c"].dtype == np.float32 and out["e"].dtype == np.float64
    total = sum(v.nbytes for v in out.values())
    assert 0.99 * bench.DUMP_BUDGET <= total <= bench.DUMP_BUDGET
    assert out["a"].ndim == 1 and np.all(np.diff(out["a"]) > 0) and 0 < out["a"].size < a.numel()
    for n in out:
        assert np.array_equal(out[n], np.load(str(tmp_path / "r2" / f"{n}.npy")))
    bench.dump_outputs(str(tmp_path / "small"), {"c": c[:3], "e": e})
    assert np.array_equal(np.load(str(tmp_path / "small" / "c.npy")), [[0, 1], [1, 1], [2, 1]])
    assert np.array_equal(np.load(str(tmp_path / "small" / "e.npy")), e.numpy())
