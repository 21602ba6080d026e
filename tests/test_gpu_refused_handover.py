"""A refused parameter hand-over leaves a feature model's handle exactly as it was (MI355X; ``pytest -m gpu``).

``hificar_bigru_set_parameters_device`` and ``hificar_xfmr_set_parameters_device`` check every name of the list before they copy a byte
(DESIGN.md 3.9): a list whose LAST name is a repeat or unknown, behind valid tensors of other values, returns HIFICAR_E_INVALID, and the
training forward before and after it — same seed, same offset, no tape — gives the same output and batch statistics bit for bit.  Each model
at the smallest configuration and shape of its own training tests: ``b3`` of tests/test_gpu_bigru_train.py, ``t2`` of
tests/transformer_train_oracle.py.
"""

import ctypes

import numpy as np
import pytest
import torch

import transformer_train_oracle as XO
from articulatory_amd import _native
from articulatory_amd.models import BiGRU, Transformer
from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform

pytestmark = pytest.mark.gpu
HIFICAR_E_INVALID = -1  # include/hificar.h
SEED, OFFSET = 777, 3


def bigru_b3():
    cin, H, out, B, T, p = 8, 64, 12, 3, 4, 0.3
    params = dict(in_channels=cin, hidden_size=H, out_channels=out, use_tanh=False, dropout=p)
    return BiGRU(**params), synth_bigru_state_dict(params, seed=1), uniform(1, "x", (B, cin, T), -1.0, 1.0)


def transformer_t2():
    params, sd, x, _ = XO.case("t2")
    return Transformer(**params), sd, x


def forward(m, x):
    """The tape-less training forward at (SEED, OFFSET): (out, batch statistics).  It moves no parameter, buffer or counter of ``m``."""
    out, stats, tape, _ = m._run_forward_train(x, m._params["dropout"], SEED, OFFSET, keep_tape=False)
    torch.cuda.synchronize()
    assert tape is None and torch.isfinite(out).all() and torch.isfinite(stats).all()
    return out.clone(), stats.clone()


@pytest.mark.parametrize("last", ["repeat", "unknown"])
@pytest.mark.parametrize("make", [bigru_b3, transformer_t2], ids=["BiGRU", "Transformer"])
def test_refused_hand_over_leaves_the_handle_as_it_was(make, last):
    m, sd, x = make()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to("cuda:0").train()
    x = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    handle = m._native_handle(train=True)
    before = forward(m, x)

    # the list _send_parameters hands over, as tensors of other values, with its last name spoilt
    names = [k for k in m.state_dict() if k not in ("mean", "scale") and not k.endswith("num_batches_tracked")]
    other = [m.state_dict()[k].detach().to(torch.float32).clone().mul_(0.5).add_(1.0).contiguous() for k in names]
    assert len(names) > 2 and all(t.is_cuda for t in other)
    names[-1] = names[0] if last == "repeat" else "no.such.tensor"
    arr = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
    ptrs = (ctypes.c_void_p * len(other))(*[t.data_ptr() for t in other])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hand_over = m._lib.hificar_bigru_set_parameters_device if isinstance(m, BiGRU) else m._lib.hificar_xfmr_set_parameters_device
    rc = hand_over(handle, arr, ptrs, len(other), stream)
    assert rc == HIFICAR_E_INVALID
    msg = _native.load_library().hificar_last_error().decode()
    assert ("given twice" if last == "repeat" else "unexpected tensor name") in msg, msg
    torch.cuda.synchronize()

    after = forward(m, x)
    assert torch.equal(after[0], before[0])
    assert torch.equal(after[1], before[1])
    assert "libhificar.so" in open("/proc/self/maps").read()
