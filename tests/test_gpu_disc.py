"""Native discriminators on a MI355X against golden vectors of the REAL reference
(tests/golden/gold_disc_*.npz, oracle/make_golden_disc.py) and against the CPU oracle.  ``pytest -m gpu``."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from articulatory_amd import losses as NL
from articulatory_amd.models import HiFiGANMultiScaleMultiPeriodDiscriminator
from articulatory_amd.utils.synth import synth_disc_state_dict, uniform
from oracle import disc_oracle as DO
from oracle import hificar_oracle as O
from test_disc_oracle import case_params

pytestmark = pytest.mark.gpu
TOL = 2e-4


def build(params, seed):
    assert torch.cuda.is_available()
    sd = synth_disc_state_dict(params, seed=seed)
    d = HiFiGANMultiScaleMultiPeriodDiscriminator(**params)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return d.to("cuda:0"), sd


def load(tag):
    gold = np.load(os.path.join(GOLDEN, f"gold_disc_{tag}.npz"))
    params = case_params(tag)
    seed, B, T = int(gold["seed"]), int(gold["B"]), int(gold["T"])
    return gold, params, seed, uniform(seed, "x", (B, 1, T), -0.6, 0.6), uniform(seed, "x_hat", (B, 1, T), -0.6, 0.6)


@pytest.mark.parametrize("tag", ["small", "default"])
def test_outputs_and_gradients_vs_reference_golden(tag):
    """Every layer output of every sub-discriminator, and d(sum(out * cot)) / d(every raw parameter, x), against the real reference."""
    gold, params, seed, x_np, _ = load(tag)
    d, sd = build(params, seed)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    outs = d(x)
    assert "libhificar.so" in open("/proc/self/maps").read()
    n_layers = [int(n) for n in gold["n_layers"]]
    assert [len(o) for o in outs] == n_layers
    loss = 0.0
    worst = 0.0
    for i, o in enumerate(outs):
        for l, t in enumerate(o):
            assert tuple(t.shape) == tuple(gold[f"shape::{i}.{l}"]), (i, l, tuple(t.shape))
            e = O.check_packed(gold, f"out::{i}.{l}", t, 2e-5)
            worst = max(worst, e)
            assert e < 2e-5, (i, l, e)
            cot = uniform(seed, f"cot.{i}.{l}", tuple(t.shape), -1.0, 1.0) / np.sqrt(np.prod(t.shape[1:]))
            loss = loss + (t * torch.from_numpy(cot.astype(np.float32)).cuda()).sum()
    loss.backward()
    bad = {}
    for k, p in list(d.named_parameters()) + [("x", x)]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        e = O.check_packed(gold, "grad::" + k, p.grad, TOL)
        if e >= TOL:
            bad[k] = e
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:10]


@pytest.mark.parametrize("tag", ["small", "default"])
def test_vectorised_layer_gradient_gather_is_bit_identical(monkeypatch, tag):
    """col2im_mask4_kernel / im2col4_kernel (four channels per thread, 16-byte accesses, one group per blockIdx.y; taken where the layer's
    widths and strides are multiples of 4) copy / sum every element in the scalar kernels' order: every layer output, parameter gradient
    and the input gradient are bit-identical with HIFICAR_COL2IM_VEC4=0."""
    _, params, seed, x_np, _ = load(tag)
    grads = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("HIFICAR_COL2IM_VEC4", flag)  # read when the engine is created
        d, _ = build(params, seed)
        x = torch.from_numpy(x_np).cuda().requires_grad_(True)
        loss = 0.0
        outs = d(x)
        grads["out" + flag] = [t.detach().cpu().clone() for o in outs for t in o]
        for i, o in enumerate(outs):
            for l, t in enumerate(o):
                cot = uniform(seed, f"cot.{i}.{l}", tuple(t.shape), -1.0, 1.0) / np.sqrt(np.prod(t.shape[1:]))
                loss = loss + (t * torch.from_numpy(cot.astype(np.float32)).cuda()).sum()
        loss.backward()
        grads[flag] = {k: p.grad.detach().cpu().clone() for k, p in list(d.named_parameters()) + [("x", x)]}
    for k in grads["1"]:
        assert torch.equal(grads["1"][k], grads["0"][k]), k
    for a, b in zip(grads["out1"], grads["out0"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tag", ["small", "default"])
def test_losses_vs_reference_golden(tag):
    """The reference's loss modules' values (adversarial mse / hinge, feature matching) from the engine's own buffers."""
    gold, params, seed, x_np, xh_np = load(tag)
    d, _ = build(params, seed)
    with torch.no_grad():
        real = d(torch.from_numpy(x_np).cuda(), native=True)
        fake = d(torch.from_numpy(xh_np).cuda(), native=True)

    def close(a, key):
        ref = float(gold[key])
        assert abs(float(a) - ref) <= 5e-5 * max(abs(ref), 1e-3), (key, float(a), ref)

    for avg in (False, True):
        for lt in ("mse", "hinge"):
            close(NL.generator_adversarial_loss(fake, avg, lt), f"loss::gen_adv::{lt}::{int(avg)}")
            r, f = NL.discriminator_adversarial_loss(fake, real, avg, lt)
            close(r, f"loss::dis_real::{lt}::{int(avg)}")
            close(f, f"loss::dis_fake::{lt}::{int(avg)}")
        for inc in (False, True):
            close(NL.feature_match_loss(fake, real, avg, avg, inc), f"loss::feat_match::{int(avg)}::{int(inc)}")


def test_generator_side_gradient_through_native_losses_vs_oracle():
    """The generator step's use (train.py:341-362): adversarial + feature-matching loss on D(fake), gradient with respect to the
    waveform only, through the native-layout losses — against the CPU oracle's autograd."""
    params = case_params("small")
    d, sd = build(params, 77)
    B, T = 2, 700
    w = DO.fold_disc_weight_norm(sd)
    x_np = uniform(5, "real", (B, 1, T), -0.5, 0.5)
    xh_np = uniform(5, "fake", (B, 1, T), -0.5, 0.5)
    xr = torch.from_numpy(xh_np).requires_grad_(True)
    f_ref = DO.disc_forward(w, params, xr)
    with torch.no_grad():
        r_ref = DO.disc_forward(w, params, torch.from_numpy(x_np))
    loss_ref = DO.gen_adv_loss(f_ref, False) + 2.0 * DO.feat_match_loss(f_ref, r_ref, False, False, False)
    loss_ref.backward()
    for p in d.parameters():
        p.requires_grad_(False)
    xh = torch.from_numpy(xh_np).cuda().requires_grad_(True)
    fake = d(xh, native=True)
    with torch.no_grad():
        real = d(torch.from_numpy(x_np).cuda(), native=True)
    loss = NL.generator_adversarial_loss(fake, False) + 2.0 * NL.feature_match_loss(fake, real, False, False, False)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 2e-5 * abs(float(loss_ref.detach()))
    # |a - b| (and LeakyReLU) are kinked, and with 10^5 feature elements some pair always sits within rounding distance of its kink
    # (min |a - b| ~ 1e-8 for every input seed): such an element's sign is a coin flip between two correct fp32 implementations and
    # moves the gradient of the ~100 samples in its receptive field by O(1 / numel).  Flip-robust check: all but a few % of the samples
    # agree to the exact-fp32 tolerance, and the whole gradient to 1e-4 in direction.
    g, gr = xh.grad.cpu().numpy().reshape(-1).astype(np.float64), xr.grad.numpy().reshape(-1).astype(np.float64)
    err = np.abs(g - gr) / np.abs(gr).max()
    assert (err < TOL).mean() > 0.9, (err < TOL).mean()
    assert 1.0 - float(g @ gr) / float(np.linalg.norm(g) * np.linalg.norm(gr)) < 1e-4
    assert err.max() < 5e-2


@pytest.mark.parametrize("tag", ["small", "default"])
@pytest.mark.parametrize("loss_type", ["mse", "hinge"])
def test_fused_criterion_vs_reference_values_and_unfused_gradients(tag, loss_type):
    """generator_loss / discriminator_loss (one autograd node each: both passes, the loss kernels, the native backward) against the
    reference's loss values (golden) and against the gradients of the same losses taken through the unfused path (native forward +
    torch reductions on the engine's buffers) — identical forward outputs, so kinks fall on the same side and the gradients agree to
    rounding."""
    gold, params, seed, x_np, xh_np = load(tag)
    d, _ = build(params, seed)
    real = torch.from_numpy(x_np).cuda()

    def close(a, key, tol=5e-5):
        ref = float(gold[key])
        assert abs(float(a) - ref) <= tol * max(abs(ref), 1e-3), (key, float(a), ref)

    for avg in (False, True):
        # ---- generator side
        fake = torch.from_numpy(xh_np).cuda().requires_grad_(True)
        total, adv, fm = d.generator_loss(fake, real, loss_type=loss_type, average_by_discriminators=avg, lambda_adv=1.5, lambda_feat_match=2.0,
                                          fm_average_by_layers=avg, fm_average_by_discriminators=avg, fm_include_final_outputs=avg)
        close(adv, f"loss::gen_adv::{loss_type}::{int(avg)}")
        close(fm, f"loss::feat_match::{int(avg)}::{int(avg)}")
        assert abs(float(total) - 1.5 * (float(adv) + 2.0 * float(fm))) < 1e-5 * abs(float(total))
        (3.0 * total).backward()
        fake2 = torch.from_numpy(xh_np).cuda().requires_grad_(True)
        p_ = d(fake2, native=True)
        with torch.no_grad():
            p = d(real, native=True)
        ref = 1.5 * (NL.generator_adversarial_loss(p_, avg, loss_type) + 2.0 * NL.feature_match_loss(p_, p, avg, avg, avg))
        (gx,) = torch.autograd.grad(3.0 * ref, fake2)
        assert rel_err_t(fake.grad, gx) < 2e-5, (avg, rel_err_t(fake.grad, gx))
        assert all(q.grad is None for q in d.parameters())
        # ---- discriminator side
        tot, r, f = d.discriminator_loss(torch.from_numpy(xh_np).cuda(), real, loss_type=loss_type, average_by_discriminators=avg)
        close(r, f"loss::dis_real::{loss_type}::{int(avg)}")
        close(f, f"loss::dis_fake::{loss_type}::{int(avg)}")
        d.zero_grad(set_to_none=True)
        (0.75 * tot).backward()  # (an upstream gradient other than 1: applied inside the weight-norm chain rule, hificar_disc_set_grad_scale)
        got = {k: q.grad.clone() for k, q in d.named_parameters()}
        d.zero_grad(set_to_none=True)
        p = d(real, native=True)
        p_ = d(torch.from_numpy(xh_np).cuda(), native=True)
        rr, ff = NL.discriminator_adversarial_loss(p_, p, avg, loss_type)
        (0.75 * (rr + ff)).backward()
        bad = {k: rel_err_t(got[k], q.grad) for k, q in d.named_parameters()}
        bad = {k: v for k, v in bad.items() if not v < 5e-5}
        assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:5]
        d.zero_grad(set_to_none=True)


def test_feature_matching_with_zero_lambda_still_logs_and_backpropagates():
    """use_feat_match_loss with lambda_feat_match = 0 (or lambda_adv = 0): the reference still computes and logs the feature-matching
    value (train.py:349-357) and the generator gets the adversarial gradient alone.  (Round-2 defect: the feature layers were skipped,
    the logged value was 0 and their gradient buffers stayed uninitialised.)"""
    gold, params, seed, x_np, xh_np = load("small")
    d, _ = build(params, seed)
    real = torch.from_numpy(x_np).cuda()
    torch.empty(1 << 24, device="cuda").fill_(float("nan"))  # poison the allocator's free blocks: stale memory must not pass as zeros
    fake = torch.from_numpy(xh_np).cuda().requires_grad_(True)
    total, adv, fm = d.generator_loss(fake, real, lambda_adv=1.5, lambda_feat_match=0.0, average_by_discriminators=False, fm_average_by_layers=False,
                                      fm_average_by_discriminators=False)
    ref_fm = float(gold["loss::feat_match::0::0"])
    assert abs(float(fm) - ref_fm) < 5e-5 * ref_fm and abs(float(total) - 1.5 * float(adv)) < 1e-6 * abs(float(total))
    total.backward()
    fake2 = torch.from_numpy(xh_np).cuda().requires_grad_(True)
    t2, _, fm2 = d.generator_loss(fake2, None, lambda_adv=1.5, average_by_discriminators=False)
    t2.backward()
    assert float(fm2) == 0.0 and torch.isfinite(fake.grad).all() and rel_err_t(fake.grad, fake2.grad) < 1e-6
    fake3 = torch.from_numpy(xh_np).cuda().requires_grad_(True)
    t3, adv3, fm3 = d.generator_loss(fake3, real, lambda_adv=0.0, lambda_feat_match=2.0, average_by_discriminators=False, fm_average_by_layers=False,
                                     fm_average_by_discriminators=False)
    t3.backward()
    assert float(t3) == 0.0 and abs(float(fm3) - ref_fm) < 5e-5 * ref_fm and float(fake3.grad.abs().max()) == 0.0


def rel_err_t(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("log_base,T", [(None, 2000), (10.0, 2000), (None, 1791)])
def test_mel_loss_vs_oracle(log_base, T):
    """MelSpectrogramLoss (e2w_hifigan_car.yaml:100-111 parameters) value and gradient against the oracle (torch.stft on the CPU).
    librosa is absent, so the filterbank is the restated one on both sides (parity unpinned for that matrix, oracle/disc_oracle.py)."""
    from articulatory_amd.losses import MelSpectrogramLoss
    from articulatory_amd.utils.mel import mel_filterbank

    kw = dict(fs=16000, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=0, fmax=11025, log_base=log_base)
    assert np.array_equal(mel_filterbank(16000, 1024, 80, 0, 11025), DO.mel_filterbank(16000, 1024, 80, 0, 11025))
    B = 3
    rng = np.random.default_rng(11)
    y = (rng.standard_normal((B, 1, T)) * 0.2).astype(np.float32)
    yh = (y + rng.standard_normal((B, 1, T)) * 0.05).astype(np.float32)
    crit = MelSpectrogramLoss(**kw)
    a = torch.from_numpy(yh).cuda().requires_grad_(True)
    loss = crit(a, torch.from_numpy(y).cuda())
    (2.0 * loss).backward()
    ar = torch.from_numpy(yh).requires_grad_(True)
    ref = DO.mel_loss(ar, torch.from_numpy(y), **kw)
    (2.0 * ref).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-4 * abs(float(ref.detach())), (float(loss), float(ref))
    g, gr = a.grad.cpu().numpy().reshape(-1).astype(np.float64), ar.grad.numpy().reshape(-1).astype(np.float64)
    # |.| of log-mel differences is kinked (sign flips where the two log-mels agree to rounding): direction + most elements
    assert 1.0 - float(g @ gr) / float(np.linalg.norm(g) * np.linalg.norm(gr)) < 1e-5
    assert (np.abs(g - gr) < 1e-3 * np.abs(gr).max()).mean() > 0.98


@pytest.mark.parametrize("T", [2000, 2483])
def test_multi_resolution_stft_loss_vs_oracle(T):
    """MultiResolutionSTFTLoss with the reference's default resolutions (fft 1024 / 2048 / 512, windows shorter than the frames):
    both values and the gradient of a weighted sum against torch.stft on the CPU."""
    from articulatory_amd.losses import MultiResolutionSTFTLoss

    B = 3
    rng = np.random.default_rng(13)
    y = (rng.standard_normal((B, 1, T)) * 0.2).astype(np.float32)
    yh = (y + rng.standard_normal((B, 1, T)) * 0.05).astype(np.float32)
    crit = MultiResolutionSTFTLoss()
    a = torch.from_numpy(yh).cuda().requires_grad_(True)
    sc, mag = crit(a, torch.from_numpy(y).cuda())
    (0.7 * sc + 1.3 * mag).backward()
    ar = torch.from_numpy(yh).requires_grad_(True)
    sc_r, mag_r = DO.multi_resolution_stft_loss(ar, torch.from_numpy(y))
    (0.7 * sc_r + 1.3 * mag_r).backward()
    assert abs(float(sc.detach()) - float(sc_r.detach())) < 1e-4 * float(sc_r.detach())
    assert abs(float(mag.detach()) - float(mag_r.detach())) < 1e-4 * float(mag_r.detach())
    g, gr = a.grad.cpu().numpy().reshape(-1).astype(np.float64), ar.grad.numpy().reshape(-1).astype(np.float64)
    assert 1.0 - float(g @ gr) / float(np.linalg.norm(g) * np.linalg.norm(gr)) < 1e-5
    assert (np.abs(g - gr) < 1e-3 * np.abs(gr).max()).mean() > 0.98


@pytest.mark.parametrize("tag", ["recipe", "odd", "silence"])
@pytest.mark.parametrize("sname", ["default", "alt"])
def test_multi_resolution_stft_loss_vs_reference_golden(tag, sname):
    """hificar_stft_loss_forward / _backward against the REAL reference module (articulatory/losses/stft_loss.py:128-170 run by
    oracle/make_golden_loss.py behind a torch.stft return_complex shim): both values to 2e-5, the spectral-convergence gradient
    element-wise, the log-magnitude gradient (an L1 of differences: kinked) by direction and 98 % of the elements."""
    from articulatory_amd.losses import MultiResolutionSTFTLoss
    from test_disc_oracle import STFT_SETS, kinked_gradient_close

    gold = np.load(os.path.join(GOLDEN, "gold_loss_aux.npz"))
    yh_np, y_np = DO.loss_test_signals(int(gold[f"{tag}::seed"]), int(gold[f"{tag}::B"]), int(gold[f"{tag}::T"]))
    crit = MultiResolutionSTFTLoss(**STFT_SETS[sname])
    for which in ("sc", "mag"):
        a = torch.from_numpy(yh_np).cuda().requires_grad_(True)
        sc, mag = crit(a, torch.from_numpy(y_np).cuda())
        val = sc if which == "sc" else mag
        val.backward()
        ref = float(gold[f"{tag}::stft::{sname}::{which}::f32"])
        assert abs(float(val.detach()) - ref) < 2e-5 * abs(ref), (which, float(val), ref)
        g, gr = a.grad.cpu().numpy(), gold[f"{tag}::stft::{sname}::d{which}::f32"]
        if which == "sc":
            assert np.abs(g - gr).max() < 2e-4 * np.abs(gr).max()
        else:
            assert kinked_gradient_close(g, gr)
    assert "libhificar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("tag", ["recipe", "odd", "silence"])
@pytest.mark.parametrize("mname", ["recipe", "default"])
def test_mel_loss_vs_reference_golden(tag, mname):
    """hificar_mel_loss against the REAL reference module (articulatory/losses/mel_loss.py:114-166; librosa's filterbank is the restated
    one on both sides, its checksum is in the fixture)."""
    from articulatory_amd.losses import MelSpectrogramLoss
    from articulatory_amd.utils.mel import mel_filterbank
    from test_disc_oracle import MEL_SETS, kinked_gradient_close

    gold = np.load(os.path.join(GOLDEN, "gold_loss_aux.npz"))
    yh_np, y_np = DO.loss_test_signals(int(gold[f"{tag}::seed"]), int(gold[f"{tag}::B"]), int(gold[f"{tag}::T"]))
    kw = MEL_SETS[mname]
    fb = mel_filterbank(kw.get("fs", 22050), kw.get("fft_size", 1024), kw.get("num_mels", 80), kw.get("fmin", 80), kw.get("fmax", 7600))
    assert abs(float(fb.astype(np.float64).sum()) - float(gold[f"melmat::{mname}::sum"])) < 1e-9
    crit = MelSpectrogramLoss(**kw)
    a = torch.from_numpy(yh_np).cuda().requires_grad_(True)
    loss = crit(a, torch.from_numpy(y_np).cuda())
    loss.backward()
    ref = float(gold[f"{tag}::mel::{mname}::loss::f32"])
    assert abs(float(loss.detach()) - ref) < 2e-5 * abs(ref), (float(loss), ref)
    assert kinked_gradient_close(a.grad.cpu().numpy(), gold[f"{tag}::mel::{mname}::dloss::f32"])


@pytest.mark.parametrize("which", ["msd", "mpd"])
def test_stand_alone_multi_scale_and_multi_period_classes(which):
    """HiFiGANMultiScaleDiscriminator / HiFiGANMultiPeriodDiscriminator (hifigan.py:666-738, 451-500) on the same engine: the reference's
    state_dict keys ("discriminators.<i>. ...", the combined class's keys without the msd. / mpd. prefix), outputs and gradients against
    the oracle."""
    from articulatory_amd.models import HiFiGANMultiPeriodDiscriminator, HiFiGANMultiScaleDiscriminator

    if which == "msd":
        d = HiFiGANMultiScaleDiscriminator(scales=2, discriminator_params=SMALL_SCALE)
        params = dict(scales=2, scale_discriminator_params=SMALL_SCALE, periods=[])
    else:
        d = HiFiGANMultiPeriodDiscriminator(periods=[3, 5], discriminator_params=SMALL_PERIOD)
        params = dict(scales=0, periods=[3, 5], period_discriminator_params=SMALL_PERIOD)
    sd = synth_disc_state_dict(params, seed=61)
    assert list(d.state_dict()) == [k[len(which) + 1:] for k in sd]
    d.load_state_dict({k[len(which) + 1:]: torch.from_numpy(v) for k, v in sd.items()})
    d = d.cuda()
    x_np = uniform(3, "x", (2, 1, 613), -0.6, 0.6)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    outs = d(x)
    cots = [[uniform(3, f"cot.{i}.{l}", tuple(t.shape), -1.0, 1.0) / np.sqrt(np.prod(t.shape[1:])) for l, t in enumerate(o)] for i, o in enumerate(outs)]
    ref_outs, ref = DO.disc_gradients(sd, params, x_np, cots)
    loss = 0.0
    for o, r, c in zip(outs, ref_outs, cots):
        for t, tr, ct in zip(o, r, c):
            assert float((t.detach().cpu() - tr).abs().max()) < 2e-5 * float(tr.abs().max())
            loss = loss + (t * torch.from_numpy(ct).cuda()).sum()
    loss.backward()
    for k, p in d.named_parameters():
        a, b = p.grad.cpu().double().reshape(-1), ref[which + "." + k].double().reshape(-1)
        err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        cos = 1.0 - float(a @ b / (a.norm() * b.norm()).clamp_min(1e-30))
        assert err < 2e-4 or cos < 1e-5, (k, err, cos)


def test_spectral_norm_period_discriminators_vs_reference_golden():
    """HiFiGANMultiPeriodDiscriminator with use_spectral_norm (hifigan.py:390-399, 440-448): the reference's state_dict layout (bias,
    weight_orig, weight_u, weight_v), two training-mode forwards (one power iteration each), the second one's gradients with respect to
    weight_orig / bias / the input, and the advanced u / v buffers, against the real reference (oracle/make_golden_disc_sn.py)."""
    from articulatory_amd.models import HiFiGANMultiPeriodDiscriminator
    from oracle.make_golden_disc_sn import PERIODS, SN_PERIOD

    gold = np.load(os.path.join(GOLDEN, "gold_disc_sn.npz"))
    params = dict(scales=0, periods=PERIODS, period_discriminator_params=SN_PERIOD)
    seed, B, T = int(gold["seed"]), int(gold["B"]), int(gold["T"])
    sd = {k[4:]: v for k, v in synth_disc_state_dict(params, seed=seed).items()}
    d = HiFiGANMultiPeriodDiscriminator(periods=PERIODS, discriminator_params=SN_PERIOD)
    assert list(d.state_dict()) == [str(k) for k in gold["keys"]]
    d.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    d = d.cuda().train()
    x = torch.from_numpy(uniform(seed, "x", (B, 1, T), -0.6, 0.6)).cuda().requires_grad_(True)
    for tag in ("1", "2"):
        outs = d(x)
        for i, o in enumerate(outs):
            for l, t in enumerate(o):
                ref = gold[f"out{tag}::{i}.{l}"]
                assert tuple(t.shape) == ref.shape and np.abs(t.detach().cpu().numpy() - ref).max() < 2e-5 * max(np.abs(ref).max(), 1e-3), (tag, i, l)
        for k, v in d.state_dict().items():
            if k.endswith(("weight_u", "weight_v")):
                assert np.abs(v.cpu().numpy() - gold[f"state{tag}::{k}"]).max() < 2e-6, (tag, k)
    loss = 0.0
    for i, o in enumerate(outs):
        for l, t in enumerate(o):
            loss = loss + (t * torch.from_numpy(uniform(seed, f"cot.{i}.{l}", tuple(t.shape), -1.0, 1.0) / np.sqrt(t[0].numel())).cuda()).sum()
    loss.backward()
    for k, p in list(d.named_parameters()) + [("x", x)]:
        ref = gold["grad::" + k]
        assert np.abs(p.grad.cpu().numpy() - ref).max() < TOL * np.abs(ref).max(), k
    d.eval()  # eval mode: no power iteration, the buffers stay
    before = {k: v.clone() for k, v in d.state_dict().items() if k.endswith("weight_u")}
    with torch.no_grad():
        d(x)
    assert all(torch.equal(v, d.state_dict()[k]) for k, v in before.items())
    with pytest.raises(NotImplementedError, match="spectral norm"):
        d.discriminator_loss(x.detach(), x.detach())


SMALL_SCALE = {"in_channels": 1, "out_channels": 1, "kernel_sizes": [15, 41, 5, 3], "channels": 16, "max_downsample_channels": 64, "max_groups": 4,
               "bias": True, "downsample_scales": [4, 4, 1], "nonlinear_activation": "LeakyReLU", "nonlinear_activation_params": {"negative_slope": 0.1}}
SMALL_PERIOD = {"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3], "channels": 8, "downsample_scales": [3, 3, 1], "max_downsample_channels": 64,
                "bias": True, "nonlinear_activation": "LeakyReLU", "nonlinear_activation_params": {"negative_slope": 0.1}, "use_weight_norm": True,
                "use_spectral_norm": False}


@pytest.mark.parametrize("which", ["scale", "period"])
def test_single_scale_and_period_discriminator_classes(which):
    """HiFiGANScaleDiscriminator / HiFiGANPeriodDiscriminator (one sub-discriminator, forward returns its list of layer outputs)."""
    from articulatory_amd.models import HiFiGANPeriodDiscriminator, HiFiGANScaleDiscriminator

    if which == "scale":
        d = HiFiGANScaleDiscriminator(**SMALL_SCALE)
        params, prefix = dict(scales=1, scale_discriminator_params=SMALL_SCALE, periods=[]), "msd.discriminators.0."
    else:
        d = HiFiGANPeriodDiscriminator(period=5, **SMALL_PERIOD)
        params, prefix = dict(scales=0, periods=[5], period_discriminator_params=SMALL_PERIOD), "mpd.discriminators.0."
    sd = synth_disc_state_dict(params, seed=62)
    assert list(d.state_dict()) == [k[len(prefix):] for k in sd]
    d.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items()})
    d = d.cuda()
    x_np = uniform(4, "x", (2, 1, 517), -0.6, 0.6)
    outs = d(torch.from_numpy(x_np).cuda())
    with torch.no_grad():
        ref = DO.disc_forward(DO.fold_disc_weight_norm(sd), params, torch.from_numpy(x_np))[0]
    assert len(outs) == len(ref)
    for t, tr in zip(outs, ref):
        assert tuple(t.shape) == tuple(tr.shape) and float((t.detach().cpu() - tr).abs().max()) < 2e-5 * float(tr.abs().max())


@pytest.mark.parametrize("kind", ["generator", "discriminator", "bigru"])
def test_profiling_through_an_engine_of_every_kind(kind):
    """hificar_profile_begin / hificar_profile_end take the conv engine of any model: the generator's own (hificar_engine_of), the
    discriminators' and the BiGRU's.  One forward at B = 1 and the shortest length each model's tests use: every launch is a row with a
    count and a device time, and the shared conv kernels are among them."""

    from conftest import E2W_PARAMS
    from articulatory_amd import _native
    from articulatory_amd.models import BiGRU, HiFiGANGenerator
    from articulatory_amd.utils.synth import synth_bigru_state_dict, synth_features, synth_state_dict

    assert torch.cuda.is_available()
    with torch.no_grad():
        if kind == "generator":
            m = HiFiGANGenerator(**E2W_PARAMS)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(dict(E2W_PARAMS), seed=1234).items()})
            m.remove_weight_norm()
            m = m.eval().to("cuda:0")
            c = torch.from_numpy(synth_features(1, 10, 13, seed=5)).permute(0, 2, 1).contiguous().cuda()
            m.profile_begin()
            m(c, ar=torch.zeros(1, 1, 512, device="cuda:0"))
            rows = m.profile_end()
        elif kind == "discriminator":
            m, _ = build(case_params("small"), 77)
            m.profile_begin()
            m(torch.from_numpy(uniform(5, "fake", (1, 1, 700), -0.5, 0.5)).cuda())
            torch.cuda.synchronize()  # (the sub-discriminators run on side streams; profile_end waits for the last one used only)
            rows = m.profile_end()
        else:
            params = dict(in_channels=80, hidden_size=64, out_channels=12, use_tanh=False)
            m = BiGRU(**params)
            m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_bigru_state_dict(params, seed=3).items()}, strict=True)
            m = m.eval().to("cuda:0")
            x = torch.from_numpy(uniform(3, "x", (1, 80, 1), -1.0, 1.0)).cuda()
            lib, eng = _native.load_library(), m.engine()
            _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
            m(x)
            rows, _ = _native.profile_rows(lib, eng, 32)
    print(kind, [(r["name"], r["launches"], round(r["total_ms"], 4)) for r in rows])
    assert len(rows) >= 1
    assert all(r["launches"] >= 1 and r["total_ms"] > 0 for r in rows), rows
    assert any(r["name"].startswith("conv_") for r in rows), rows
