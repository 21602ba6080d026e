"""Every weight-gradient kernel form of the generator's backward, by name and against the float64 oracle.  ``pytest -m gpu``.

The weight gradient of a conv layer runs as one of 22 instantiations (wgrad_taps_kernel<NT, EXACT, R>, wgrad_gemm_kernel<2,64> / <4,32>, the
per-tap wgrad_kernel), further varied by row_split, g_per_tile and one or two layers per launch; which one depends on the layer's width, tap
count, halo and the rows per sequence (launch_wgrad_n, csrc/hificar_train.hip.inc).  tests/wgrad_forms.py restates that rule and lists
thirteen small generators (CASES) chosen from it; tests/test_wgrad_forms_host.py proves from the rule that they reach every instantiation and
every condition of its table.  Here each case, in train() mode, exact fp32, LeakyReLU slope 1, B = 3:
  (a) by name, both ways: the weight-gradient rows of the profile (HIFICAR_PROFILE_DETAIL=1: "kernel<instantiation> shape sS rR nN") are
      exactly the launches the rule predicts, each with the predicted instantiation, row_split and layer count; the split count S is read,
      not predicted (it depends on the CU count).  The generator's backward defers every reduction: one reduce_multi_kernel row, which says
      how many weight and bias reductions it ran (a layer without bias has none); wreduce_kernel / breduce_kernel launches of their own are
      not reachable through the generator and must not appear.
  (b) every element of every parameter gradient and of c / ar against O.gradients(..., dtype=float64): 2e-4 of each tensor's scale (TOL of
      test_gpu_train.py, GRAD_TOL of test_gpu_conv_tiles.py), the waveform within 2e-5.  No allowance for the one-element tensors (the fuzz holds
      output_conv.1.weight_g to 25 x the bar): the oracle's own fp32 run is within 5.3e-6 of its float64 run on output_conv.1.weight_g in every
      case here (worst: case gemm_wide) and within 3.2e-5 on output_conv.1.bias (case r128_single), far inside the bar.
  (c) a second forward + backward on the same inputs gives bit-identical gradients (fixed-order reductions, no atomics).

With slope 1 the generator has no kinks but the output conv's LeakyReLU(0.01) and the PastFCEncoder's (0.1); as in test_gpu_train_fuzz.py the
input seed of a case is the first whose float64 forward keeps every such pre-activation further than 2e-6 of its tensor's scale from zero
(``case_inputs``; no case needs more than its first few seeds, and a case without such a seed fails)."""

import numpy as np
import pytest
import torch

import wgrad_forms as W
from conftest import rel_err
from articulatory_amd import _native
from articulatory_amd.models import HiFiGANGenerator
from articulatory_amd.utils.synth import synth_features, synth_state_dict, uniform
from oracle import hificar_oracle as O
from test_gpu_train_fuzz import kink_margin

pytestmark = pytest.mark.gpu
GRAD_TOL = 2e-4
OUT_TOL = 2e-5
SEEDS_TRIED = 6


def case_seed(name):
    return 4100 + 10 * list(W.CASES).index(name)


def case_inputs(name):
    """(state dict, c, ar or None, cotangent) of a case: numpy, deterministic; the first input seed clear of the two remaining kinks."""
    params, T = W.CASES[name]
    seed = case_seed(name)
    sd = synth_state_dict(params, seed=seed)
    cf = params["in_channels"] - (params["ar_output"] if params["use_ar"] else 0)
    hop = int(np.prod(params["upsample_scales"]))
    for attempt in range(SEEDS_TRIED):
        c = synth_features(W.B, T, cf, seed=seed + 1 + 1000 * attempt).transpose(0, 2, 1).copy()
        ar = ((synth_features(W.B, 512, 1, seed=seed + 2 + 1000 * attempt)[:, :, 0] * 0.4).reshape(W.B, 1, 512).astype(np.float32)
              if params["use_ar"] else None)
        if kink_margin(sd, params, c, ar) > 2e-6:
            return sd, c, ar, uniform(seed + 3, "cot", (W.B, 1, hop * T), -1.0, 1.0)
    pytest.fail("%s: no input clear of the output conv's / PastFCEncoder's kinks in %d seeds" % (name, SEEDS_TRIED))


@pytest.fixture(scope="module")
def detail_env():
    """HIFICAR_PROFILE_DETAIL=1: profile rows carry the instantiation and the layer's shape.  Read when a native handle is built, so it is set
    before any model of this module exists."""
    mp = pytest.MonkeyPatch()
    mp.setenv("HIFICAR_PROFILE_DETAIL", "1")
    yield mp
    mp.undo()


def profile_rows(lib, eng):
    """{row: launches} since hificar_profile_begin."""
    rows, n = _native.profile_rows(lib, eng, 512)
    assert n <= 512
    return {r["name"]: r["launches"] for r in rows}


def step(g, c_np, ar_np, cot, profile=False):
    """One forward and backward of (y * cot).sum(): CPU gradients of every parameter, of c and ar, the waveform; the profile's rows."""
    handle = g._native_handle()  # (builds the handle and loads the library on first use)
    lib = g._lib
    eng = lib.hificar_engine_of(handle)
    c = torch.from_numpy(c_np).cuda().requires_grad_(True)
    ar = torch.from_numpy(ar_np).cuda().requires_grad_(True) if ar_np is not None else None
    g.zero_grad(set_to_none=True)
    rows = None
    if profile:
        _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    try:
        y = g(c, ar=ar)
        (y * torch.from_numpy(cot).cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        if profile:
            rows = profile_rows(lib, eng)
    got = {k: p.grad.detach().cpu().clone() for k, p in g.named_parameters()}
    got["c"] = c.grad.cpu()
    if ar is not None:
        got["ar"] = ar.grad.cpu()
    return got, y.detach().cpu(), rows


def check_rows(name, rows):
    """(a): the weight-gradient and reduction rows of one backward against the rule's launches, both ways."""
    launches = W.case_launches(name)
    got = {}
    for row, count in rows.items():
        if row.startswith("wgrad_"):
            key, split = W.strip_split(row)
            assert split >= 1, row
            got[key] = got.get(key, 0) + count
    want = dict(W.expected_rows(launches))
    assert got == want, (name, sorted(set(got) - set(want)), sorted(set(want) - set(got)), {k: (got[k], want[k]) for k in set(got) & set(want) if got[k] != want[k]})
    assert not [r for r in rows if r.startswith(("wreduce", "breduce"))], sorted(rows)  # every reduction of the pass is deferred
    multi = {r: n for r, n in rows.items() if r.startswith("reduce_multi_kernel")}
    assert multi and all(n == 1 for n in multi.values()), multi
    nw = nb = 0
    for r in multi:
        _, w, b = r.split(" ")
        nw, nb = nw + int(w[1:]), nb + int(b[1:])
    assert (nw, nb) == (len(launches), sum(l.bias for l in launches)), (name, multi, len(launches), sum(l.bias for l in launches))
    return sorted(r for r in rows if r.startswith("wgrad_"))


@pytest.mark.parametrize("name", list(W.CASES))
def test_wgrad_forms_case(detail_env, name):
    assert torch.cuda.is_available()
    params, T = W.CASES[name]
    sd, c_np, ar_np, cot = case_inputs(name)
    g = HiFiGANGenerator(**params, precision="f32")
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g = g.train().cuda()
    got, y, rows = step(g, c_np, ar_np, cot, profile=True)
    ran = check_rows(name, rows)
    out64, ref64 = O.gradients(sd, params, c_np, ar_np, cot, dtype=torch.float64)
    err_y = rel_err(y.numpy(), out64.numpy())
    assert sorted(got) == sorted(ref64), name
    errs = {}
    for k in ref64:
        assert tuple(got[k].shape) == tuple(ref64[k].shape) and bool(torch.isfinite(got[k]).all()), (name, k)
        errs[k] = rel_err(got[k].numpy(), ref64[k].numpy())
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print(name, "waveform %.3g, worst gradients %s" % (err_y, ", ".join("%s %.3g" % kv for kv in worst)))
    print("   ", "\n    ".join(ran))
    assert err_y < OUT_TOL, (name, err_y)
    assert worst[0][1] < GRAD_TOL, (name, worst)
    again, y2, _ = step(g, c_np, ar_np, cot)
    assert torch.equal(y, y2)
    for k in got:
        assert torch.equal(got[k], again[k]), (name, k)
