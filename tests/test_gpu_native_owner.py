"""``articulatory_amd._owner`` on a MI355X: copies and pickles of owners that have run give the original's bits from handles of their
own, deleting them leaves the original's handle alone, and the generator's grow-only workspace lives in ``_workspace_buf``.
``pytest -m gpu``."""

import copy
import gc
import pickle

import numpy as np
import pytest
import torch

from articulatory_amd.features import MFCC, LinearHead
from articulatory_amd.losses import MelSpectrogramLoss, MultiResolutionSTFTLoss
from articulatory_amd.models import HiFiGANGenerator

pytestmark = pytest.mark.gpu
DEV = "cuda"


def check_clones(owner, run):
    """``run(module)`` -> tensors.  Forward (and backward) on ``owner``, then on a deep copy and on a pickle round trip: the same bits, from
    handles of their own; with the clones deleted the original gives the same bits again (no handle was shared, none destroyed under it)."""
    first = run(owner)
    handle = owner._handle
    assert handle is not None
    clones = [copy.deepcopy(owner), pickle.loads(pickle.dumps(owner))]
    for clone in clones:
        assert clone._handle is None and clone._lib is None
        got = run(clone)
        assert len(got) == len(first) and all(torch.equal(a, b) for a, b in zip(got, first))
        assert clone._handle is not None and clone._handle.value != handle.value
    del clone, clones
    gc.collect()
    assert owner._handle is handle
    again = run(owner)
    assert all(torch.equal(a, b) for a, b in zip(again, first))


def loss_case(T=1791):
    rng = np.random.default_rng(11)
    y = (rng.standard_normal((1, 1, T)) * 0.2).astype(np.float32)
    yh = (y + rng.standard_normal((1, 1, T)) * 0.05).astype(np.float32)
    return torch.from_numpy(yh).to(DEV), torch.from_numpy(y).to(DEV)


def run_loss(crit, yh, y):
    a = yh.clone().requires_grad_(True)
    values = crit(a, y)
    values = values if isinstance(values, tuple) else (values,)
    sum(values).backward()
    return [v.detach().clone() for v in values] + [a.grad]


def test_mel_loss_copies_after_use():
    """tests/test_gpu_disc.py's arguments at B = 1 and its odd length.  (Before ``NativeOwner``, copying a used criterion raised.)"""
    crit = MelSpectrogramLoss(fs=16000, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=0, fmax=11025, log_base=None)
    yh, y = loss_case()
    check_clones(crit, lambda m: run_loss(m, yh, y))


def test_multi_resolution_stft_loss_copies_after_use():
    crit = MultiResolutionSTFTLoss()
    yh, y = loss_case()
    first = run_loss(crit, yh, y)
    handles = [f._handle for f in crit.stft_losses]
    assert all(h is not None for h in handles)
    clones = [copy.deepcopy(crit), pickle.loads(pickle.dumps(crit))]
    for clone in clones:
        assert all(f._handle is None and f._lib is None for f in clone.stft_losses)
        assert all(torch.equal(a, b) for a, b in zip(run_loss(clone, yh, y), first))
        assert all(f._handle.value != h.value for f, h in zip(clone.stft_losses, handles))
    del clone, clones
    gc.collect()
    assert all(f._handle is h for f, h in zip(crit.stft_losses, handles))
    assert all(torch.equal(a, b) for a, b in zip(run_loss(crit, yh, y), first))


def test_mfcc_copies_after_use():
    wav = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 1600)).astype(np.float32) * 0.1).to(DEV)  # more than n_fft / 2 samples
    check_clones(MFCC(), lambda m: list(m(wav)))


def test_linear_head_copies_after_use():
    rng = np.random.default_rng(7)
    head = LinearHead(rng.standard_normal((3, 16)), rng.standard_normal(3)).to(DEV)
    feats = torch.from_numpy(rng.standard_normal((2, 16, 5)).astype(np.float32)).to(DEV)
    check_clones(head, lambda m: [m(feats, [5, 2])])


def test_generator_workspace_grows_only_and_lives_in_workspace_buf():
    torch.manual_seed(3)
    g = HiFiGANGenerator(in_channels=13, channels=64, use_ar=False).to(DEV).eval()
    small, large = torch.randn(1, 13, 8, device=DEV), torch.randn(2, 13, 40, device=DEV)
    with torch.no_grad():
        first = g(small)
        ws_small = g._workspace_buf
        assert ws_small.dtype == torch.uint8 and ws_small.is_cuda
        g(large)
        ws_large = g._workspace_buf
        assert ws_large is not ws_small and ws_large.numel() > ws_small.numel()
        again = g(small)
    assert g._workspace_buf is ws_large and torch.equal(again, first)
    assert "_workspaces" not in g.__dict__
