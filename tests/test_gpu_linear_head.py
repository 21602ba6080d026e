"""``features.LinearHead`` and ``bin/linear_inference`` on a MI355X: the head against sklearn's ``predict`` on the same device features
fetched to the CPU (2e-5 of max|y|, the project's exact-fp32 bar), zeros behind each length, and the command line against the API.
``pytest -m gpu``."""

import json

import numpy as np
import pytest
import torch

import wavlm_oracle as W
from conftest import rel_err
from articulatory_amd.bin import linear_inference as LI
from articulatory_amd.bin.predict_ema import read_wav
from articulatory_amd.features import LinearHead, WavLM
from articulatory_amd.utils.synth import synth_wavlm_state_dict
from test_gpu_hubert import DEV, dev, samples, write_wav
from test_gpu_wavlm import TINY, model_of, ragged_batch
from test_hubert_host import SEED
from test_linear_head_host import _fit

pytestmark = pytest.mark.gpu
TOL = 2e-5


def test_head_is_sklearns_predict_on_the_device_features():
    pytest.importorskip("sklearn")
    reg = _fit()
    head = LinearHead(reg.coef_, reg.intercept_).to(DEV)
    m, _ = model_of("f32")
    lens, wavs, padded = ragged_batch()
    lens, padded = lens[:3], padded[:3]  # 129, 65 and 1 frames
    feats, frames = m(dev(padded), lengths=lens, layer=1)
    out = head(feats, frames)
    assert out.shape == (3, 12, 129) and out.dtype == torch.float32
    host = feats.cpu().numpy().astype(np.float64)
    for i, n in enumerate(frames.tolist()):
        want = reg.predict(host[i, :, :n].T)
        err = rel_err(out[i, :, :n].cpu().numpy().T, want)
        print(f"utterance {i}: rel_err {err:.3e}")
        assert err < TOL, (i, err)
        assert not out[i, :, n:].any(), i
        alone = head(feats[i:i + 1, :, :n].contiguous())
        assert torch.equal(alone[0], out[i, :, :n]), i
    head._workspace_buf.fill_(255)
    assert torch.equal(head(feats, frames.tolist()), out)
    full = head(feats)  # (no lengths: every row is computed, the zero rows give the intercept)
    assert torch.equal(full[0], out[0]) and rel_err(full[2, :, 5].cpu().numpy(), reg.intercept_) < TOL
    # an input width that is no multiple of 32 and one output
    one = _fit(n_out=1, n_in=70, seed=3)
    h1 = LinearHead(one.coef_, one.intercept_).to(DEV)
    x = torch.randn(2, 70, 33, device=DEV)
    y = h1(x, [33, 7])
    assert y.shape == (2, 1, 33) and not y[1, :, 7:].any()
    assert rel_err(y[0, 0].cpu().numpy(), one.predict(x[0].cpu().numpy().astype(np.float64).T)) < TOL


def test_linear_inference_writes_what_the_api_gives(tmp_path):
    pytest.importorskip("sklearn")
    joblib = pytest.importorskip("joblib")
    reg = _fit()
    joblib.dump(reg, tmp_path / "linear.joblib")
    wl = tmp_path / "wavlm"
    wl.mkdir()
    (wl / "config.json").write_text(json.dumps(dict(TINY, model_type="wavlm")))
    torch.save({k: torch.from_numpy(v) for k, v in synth_wavlm_state_dict(TINY, seed=SEED).items()}, wl / "pytorch_model.bin")
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    lens = {"uttA": 12000, "uttB": 8117, "uttC": 400}
    for i, (u, l) in enumerate(lens.items()):
        write_wav(wavs / f"{u}.wav", W.synth_wav(SEED + 11 * i, l, amplitude=0.3))
    for bs in (1, 3):
        LI.main([str(wavs), str(tmp_path / "linear.joblib"), str(tmp_path / f"out{bs}"), "--ssl-model", str(wl), "--layer", "1", "--batch-size", str(bs),
                 "--verbose", "0"])
    wavlm = WavLM.from_pretrained(str(wl)).to(DEV)
    head = LinearHead.load(str(tmp_path / "linear.joblib")).to(DEV)
    for u, l in lens.items():
        y, _ = read_wav(str(wavs / f"{u}.wav"))
        feats, frames = wavlm(dev(y)[None], layer=1)
        want = head(feats, frames)[0].T.cpu().numpy()
        a = np.load(tmp_path / "out1" / f"{u}.npy")
        assert a.shape == (W.frames(l), 12) and a.dtype == np.float32 and np.array_equal(a, want), u
        assert (tmp_path / "out1" / f"{u}.npy").read_bytes() == (tmp_path / "out3" / f"{u}.npy").read_bytes(), u
