"""``forward_lowrate`` of ``BiGRU`` and ``Transformer`` (the reference's egs/ema/voc1/local/predict_ema.py:83-101 on the device) on a MI355X:
against golden vectors of the REAL reference classes (tools/make_golden_predict_ema.py), against the existing forward on a materialised
``F.interpolate``, and against the float64 restatement (tests/predict_ema_oracle.py).  ``pytest -m gpu``.

Bars, none of them new: 2e-5 of max|y| in exact fp32 (tests/test_gpu_bigru.py, tests/test_gpu_transformer.py), 2e-4 on a bf16x3 / bf16x3a
handle (tests/test_gpu_transformer_bf16x3*.py).  The comparison with the materialised path takes twice the bar: both sides are within one
bar of float64.
"""

import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import predict_ema_oracle as P
from bigru_oracle import BiGRUOracle
from conftest import GOLDEN, rel_err
from transformer_oracle import TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin import predict_ema as PE
from articulatory_amd.models import BiGRU, Transformer
from articulatory_amd.utils.synth import synth_bigru_state_dict, synth_transformer_state_dict, uniform

pytestmark = pytest.mark.gpu
TOL = 2e-5
TOL_X3 = 2e-4
# (model, tag, interp_factor, zscore, low-rate frames): the cases of tools/make_golden_predict_ema.py
CASES = [("bigru", "small", 4, False, 1), ("bigru", "small", 4, False, 2), ("bigru", "small", 4, False, 33), ("bigru", "small", 4, False, 75),
         ("bigru", "small", 2, False, 50), ("bigru", "small", 3, False, 11), ("bigru", "mfcc", 1, True, 130),
         ("xfmr", "small", 4, False, 1), ("xfmr", "small", 4, False, 33), ("xfmr", "small", 1, True, 100)]
RAGGED = (75, 1, 34, 0)
# models without a golden case: (kind, constructor keywords, seed)
EXTRA = {
    "bigru13": ("bigru", dict(in_channels=13, hidden_size=64, out_channels=12, use_tanh=True), 7102),  # (= the golden mfcc model)
    "bigru128": ("bigru", dict(in_channels=80, hidden_size=128, out_channels=12, use_tanh=False), 7111),
    "xfmr13": ("xfmr", dict(in_channels=13, out_channels=18, elayers=2, hidden_dim=128), 7112),
    "xfmr128": ("xfmr", dict(in_channels=128, out_channels=18, elayers=1, hidden_dim=128), 7113),  # in_channels == hidden_dim: no residual_path
}


def case_name(model, tag, f, z, Tl):
    return f"{model}_{tag}_f{f}{'_z' if z else ''}_Tl{Tl}"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gold_predict_ema.npz"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


_MODELS = {}


def model_of(gold, key, precision="f32"):
    """(device model, float64 restatement, constructor keywords, seed) of "bigru_small", "bigru_mfcc", "xfmr_small" (the golden models) or
    a key of EXTRA, built once per module and arithmetic."""
    if (key, precision) not in _MODELS:
        if key in EXTRA:
            kind, params, seed = EXTRA[key]
        else:
            kind = key.split("_")[0]
            v = [int(x) for x in gold[key + "_params"]]
            params = (dict(in_channels=v[0], hidden_size=v[1], out_channels=v[2], use_tanh=bool(v[3])) if kind == "bigru" else
                      dict(in_channels=v[0], out_channels=v[1], elayers=v[2], hidden_dim=v[3]))
            seed = v[4]
        assert torch.cuda.is_available()
        if kind == "bigru":
            sd = synth_bigru_state_dict(params, seed=seed)
            m = BiGRU(**params)
            o = BiGRUOracle(sd, use_tanh=params["use_tanh"], dtype=torch.float64)
        else:
            sd = synth_transformer_state_dict(params, seed=seed)
            m = Transformer(**params, precision=precision)
            o = TransformerOracle(sd)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        _MODELS[key, precision] = (m.eval().to("cuda:0"), o, params, seed)
    return _MODELS[key, precision]


def features(seed, name, Tl, C, z=False):
    lo, hi = (-1.0, 3.0) if z else (-1.0, 1.0)
    return uniform(seed, f"feat.{name}", (Tl, C), lo, hi)


# ---------------------------------------------------------------------------------------------- golden cases
@pytest.mark.parametrize("case", CASES, ids=lambda c: case_name(*c))
def test_golden_cases(gold, case):
    model, tag, f, z, Tl = case
    name = case_name(*case)
    for precision, tol in ((("f32", TOL),) if model == "bigru" else (("f32", TOL), ("bf16x3", TOL_X3), ("bf16x3a", TOL_X3))):
        m, _, params, seed = model_of(gold, f"{model}_{tag}", precision)
        x = dev(features(seed, name, Tl, params["in_channels"], z).T[None])
        y = m.forward_lowrate(x, interp_factor=f, zscore=z)
        assert y.shape == (1, params["out_channels"], f * Tl) and y.dtype == torch.float32
        err = rel_err(y[0].t().cpu().numpy(), gold[name + "_y"])
        print(f"{name} [{precision}]: {err:.3g}")
        assert err < tol, (name, precision)
    assert "libhificar.so" in open("/proc/self/maps").read()


def test_golden_ragged_batch(gold):
    m, _, params, seed = model_of(gold, "bigru_small")
    x = uniform(seed, "ragged.feat", (len(RAGGED), max(RAGGED), params["in_channels"]), -1.0, 1.0).transpose(0, 2, 1).copy()
    for b, n in enumerate(RAGGED):
        x[b, :, n:] = np.nan  # padded frames are never read
    y = m.forward_lowrate(dev(x), lengths=RAGGED, interp_factor=4)
    err = rel_err(y.permute(0, 2, 1).cpu().numpy(), gold["bigru_small_ragged_y"])
    print(f"ragged: {err:.3g}")
    assert err < TOL
    for b, n in enumerate(RAGGED):
        assert not y[b, :, 4 * n:].any(), b


# ---------------------------------------------------------------------------------------------- against the materialised path
def materialised(m, x, lens, f):
    """What a user does without the front end: stock F.interpolate on the device, then the existing forward, per utterance."""
    out = torch.zeros((x.shape[0], m._params["out_channels"], f * x.shape[2]), device=x.device)
    for b, l in enumerate(lens):
        if l:
            out[b, :, :f * l] = m(F.interpolate(x[b:b + 1, :, :l], size=f * l, mode="linear", align_corners=False))[0]
    return out


def sweep_against_materialised(gold, key, f, precision="f32", tol=2 * TOL, frames=(1, 2, 7, 8, 9, 31, 32, 33)):
    m, _, params, seed = model_of(gold, key, precision)
    for Tl in frames:
        x = dev(uniform(seed, f"mat.{f}.{Tl}", (3, params["in_channels"], Tl), -1.0, 1.0))
        for lens in ((Tl, 1, 0), (Tl - 1, Tl, min(2, Tl))):
            y = m.forward_lowrate(x, lengths=lens, interp_factor=f)
            want = materialised(m, x, lens, f)
            assert y.shape == want.shape
            if not any(lens):
                assert not y.any()
                continue
            err = rel_err(y.cpu().numpy(), want.cpu().numpy())
            print(f"{key} [{precision}] f={f} Tl={Tl} lengths={lens}: {err:.3g}")
            assert err < tol, (key, f, Tl, lens)
            for b, l in enumerate(lens):
                assert not y[b, :, f * l:].any(), (key, f, Tl, lens, b)


@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("key", ["bigru13", "bigru_small", "xfmr13", "xfmr_small"])
def test_against_materialised_interpolation(gold, key, f):
    """Output lengths on, before and past the 32-frame rows tile and the BiGRU head's 64-frame tile; C = 13 (padded to 32) and 80 (no
    multiple of 32); B = 3 with low-rate lengths (Tl, 1, 0) and (Tl - 1, Tl, 2)."""
    sweep_against_materialised(gold, key, f)


def test_against_materialised_bigru_h128_two_sequences_per_workgroup(gold, monkeypatch):
    monkeypatch.setenv("HIFICAR_BIGRU_NS", "2")
    sweep_against_materialised(gold, "bigru128", 4, frames=(1, 9, 33))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16x3a"])
@pytest.mark.parametrize("key", ["xfmr_small", "xfmr128"])
def test_against_materialised_bf16x3(gold, key, precision):
    """The split rows of a bf16x3 handle, with (xfmr128: in_channels == hidden_dim) and without the fp32 residual copy.  Twice the bf16x3 bar."""
    sweep_against_materialised(gold, key, 4, precision, 2 * TOL_X3, frames=(1, 9, 33))


# ---------------------------------------------------------------------------------------------- identity, independence, scratch
@pytest.mark.parametrize("key,precision", [("bigru_small", "f32"), ("xfmr_small", "f32"), ("xfmr_small", "bf16x3")])
def test_factor_one_is_the_existing_forward(gold, key, precision):
    m, _, params, seed = model_of(gold, key, precision)
    x = dev(uniform(seed, "ident", (3, params["in_channels"], 70), -1.0, 1.0))
    lens = [70, 33, 1]
    assert torch.equal(m.forward_lowrate(x, lengths=lens, interp_factor=1, zscore=False), m(x, lengths=lens))
    assert torch.equal(m.forward_lowrate(x), m(x))


def run_c_entry(m, x, lens, f, z, poison):
    """hificar_*_forward_lowrate on caller-owned buffers; ``poison``: the whole workspace (and the output) filled with NaN on entry."""
    kind = "bigru" if isinstance(m, BiGRU) else "xfmr"
    handle, lib = m._native_handle(), m._lib
    B, _, Tl = x.shape
    n = getattr(lib, f"hificar_{kind}_workspace_bytes_lowrate")(handle, B, Tl, f)
    assert n > 0
    ws = torch.empty(n // 4 + 64, dtype=torch.float32, device=x.device)
    ws.fill_(float("nan") if poison else 0.0)
    off = (-ws.data_ptr()) % 256
    out = torch.full((B, m._params["out_channels"], f * Tl), float("nan") if poison else 0.0, device=x.device)
    host = torch.tensor(lens, dtype=torch.int32)
    devl = host.to(x.device)
    rc = getattr(lib, f"hificar_{kind}_forward_lowrate")(handle, x.data_ptr(), devl.data_ptr(), host.data_ptr(), out.data_ptr(), B, Tl, f, int(z),
                                                         ws.data_ptr() + off, n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, f"hificar_{kind}_forward_lowrate")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("key,precision,z", [("bigru_small", "f32", False), ("bigru13", "f32", True), ("xfmr_small", "f32", False),
                                             ("xfmr13", "f32", True), ("xfmr_small", "bf16x3a", False)])
def test_batch_independence_and_dirty_scratch(gold, key, precision, z):
    m, _, params, seed = model_of(gold, key, precision)
    lens = [33, 1, 0, 20, 32]
    f = 4
    x = dev(uniform(seed, "indep", (len(lens), params["in_channels"], 33), -1.0, 3.0 if z else 1.0))
    y = m.forward_lowrate(x, lengths=lens, interp_factor=f, zscore=z)
    assert torch.equal(m.forward_lowrate(x, lengths=lens, interp_factor=f, zscore=z), y)  # two runs, the same bits
    for b, l in enumerate(lens):
        assert not y[b, :, f * l:].any(), b
        if l:
            alone = m.forward_lowrate(x[b:b + 1, :, :l].contiguous(), interp_factor=f, zscore=z)
            assert torch.equal(alone[0], y[b, :, :f * l]), (b, l)
    # NaN in every padded low-rate frame, in the whole workspace and in the output buffer, through the C entry point
    xn = x.clone()
    for b, l in enumerate(lens):
        xn[b, :, l:] = float("nan")
    assert torch.equal(run_c_entry(m, x, lens, f, z, poison=False), y)
    assert torch.equal(run_c_entry(m, xn, lens, f, z, poison=True), y)


# ---------------------------------------------------------------------------------------------- zscore
@pytest.mark.parametrize("key", ["bigru13", "bigru_small", "xfmr13", "xfmr_small"])
def test_zscore_against_restatement(gold, key):
    """C x l in (13 x 1, 13 x 130, 80 x 33), among them an input with mean 1e3 and standard deviation 1, which a one-pass fp32 variance gets
    wrong."""
    m, o, params, seed = model_of(gold, key)
    C = params["in_channels"]
    rng = np.random.default_rng(seed)
    for l in ((1, 130) if C == 13 else (33,)):
        for mean in (0.0, 1e3):
            x = (rng.standard_normal((2, C, l)) + mean).astype(np.float32)
            x[1] = x[1] * 3 - 1  # every utterance by its own statistics
            y = m.forward_lowrate(dev(x), zscore=True)
            want = P.forward_lowrate(o, x, None, 1, True).numpy()
            err = rel_err(y.cpu().numpy(), want)
            print(f"{key} {C} x {l} mean {mean:g}: {err:.3g}")
            assert err < TOL, (key, l, mean)
    # with interpolation: normalisation first, every utterance over its own valid frames
    lens = [20, 7]
    x = (rng.standard_normal((2, C, 20)) * 2 + 5).astype(np.float32)
    y = m.forward_lowrate(dev(x), lengths=lens, interp_factor=4, zscore=True)
    assert rel_err(y.cpu().numpy(), P.forward_lowrate(o, x, lens, 4, True).numpy()) < TOL


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_end_to_end(gold, tmp_path):
    """predict_ema on the device: best_mel_ckpt.pkl + config.yml in a directory whose name selects interpolation by 4, three utterances;
    the files written at --batch-size 1 and 2 are equal."""
    _, o, params, seed = model_of(gold, "bigru_small")
    d = tmp_path / "mngu0_h2"
    d.mkdir()
    sd = synth_bigru_state_dict(params, seed=seed)
    torch.save({"model": {"generator": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, d / "best_mel_ckpt.pkl")
    (d / "config.yml").write_text(yaml.safe_dump(dict(generator_type="BiGRU", generator_params=params, format="npy")))
    feats = tmp_path / "feats"
    feats.mkdir()
    name = case_name("bigru", "small", 4, False, 33)
    c = features(seed, name, 33, params["in_channels"])
    utts = {"uttA": c, "uttB": c[:7].copy(), "uttC": c[20:21].copy()}
    for u, f in utts.items():
        np.save(feats / f"{u}.npy", f)
    for bs in (1, 2):
        PE.main([str(d), str(feats), str(tmp_path / f"out{bs}"), "--batch-size", str(bs), "--verbose", "0"])
    y = np.load(tmp_path / "out1" / "uttA.npy")
    assert y.shape == (132, 12) and y.dtype == np.float32 and rel_err(y, gold[name + "_y"]) < TOL
    for u, f in utts.items():
        a, b = np.load(tmp_path / "out1" / f"{u}.npy"), np.load(tmp_path / "out2" / f"{u}.npy")
        assert a.shape == (4 * len(f), 12) and np.array_equal(a, b), u
