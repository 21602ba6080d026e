"""``features.LinearHead`` and ``bin/linear_inference``, host side (no GPU): reading a fitted regression back from ``.joblib`` and ``.npz``,
the refusals, and the command line's plan."""

import json

import numpy as np
import pytest
import torch

from articulatory_amd.bin import linear_inference as LI
from articulatory_amd.features import LinearHead
from tests.test_hubert_host import TINY as HUBERT_TINY, _write_wav
from tests.test_wavlm_host import TINY


def _fit(n_out=12, n_in=128, ridge=False, seed=0):
    from sklearn.linear_model import LinearRegression, Ridge

    rng = np.random.default_rng(seed)
    X = rng.standard_normal((400, n_in))
    Y = X @ rng.standard_normal((n_in, n_out)) + rng.standard_normal(n_out) + 0.1 * rng.standard_normal((400, n_out))
    return (Ridge(alpha=1.0) if ridge else LinearRegression()).fit(X, Y if n_out > 1 else Y[:, 0])


@pytest.mark.parametrize("ridge", [False, True])
def test_load_reads_a_fitted_regression_back(tmp_path, ridge):
    pytest.importorskip("sklearn")
    joblib = pytest.importorskip("joblib")
    reg = _fit(ridge=ridge)
    joblib.dump(reg, tmp_path / "linear.joblib")
    np.savez(tmp_path / "linear.npz", coef=reg.coef_, intercept=reg.intercept_)
    a, b = LinearHead.load(str(tmp_path / "linear.joblib")), LinearHead.load(str(tmp_path / "linear.npz"))
    for h in (a, b):
        assert (h.in_features, h.out_features) == (128, 12) and h.coef.dtype == torch.float32
        assert np.array_equal(h.coef.numpy(), reg.coef_.astype(np.float32)) and np.array_equal(h.intercept.numpy(), reg.intercept_.astype(np.float32))
    one = _fit(n_out=1)  # (a 1-D coef_ and a scalar intercept_: one output)
    joblib.dump(one, tmp_path / "one.joblib")
    h = LinearHead.load(str(tmp_path / "one.joblib"))
    assert h.coef.shape == (1, 128) and h.intercept.shape == (1,) and float(h.intercept[0]) == np.float32(one.intercept_)


def test_refusals(tmp_path):
    joblib = pytest.importorskip("joblib")
    with pytest.raises(ValueError, match=r"\.joblib .* or an \.npz"):
        LinearHead.load(str(tmp_path / "linear.pkl"))
    np.savez(tmp_path / "bad.npz", weights=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="holds 'coef' and 'intercept'"):
        LinearHead.load(str(tmp_path / "bad.npz"))
    joblib.dump({"coef": 1}, tmp_path / "dict.joblib")
    with pytest.raises(ValueError, match="dict has no coef_"):
        LinearHead.load(str(tmp_path / "dict.joblib"))
    with pytest.raises(ValueError, match="do not make"):
        LinearHead(np.zeros((3, 8)), np.zeros(2))
    with pytest.raises(ValueError, match="out of range"):
        LinearHead(np.zeros((2000, 8)), np.zeros(2000))
    h = LinearHead(np.zeros((3, 8)), np.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h(torch.zeros(1, 8, 4))


def test_linear_inference_plan_and_errors(tmp_path, capsys):
    wl = tmp_path / "wavlm"
    wl.mkdir()
    (wl / "config.json").write_text(json.dumps(dict(TINY, model_type="wavlm")))  # (no weights: the plan reads the configuration alone)
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    _write_wav(wavs / "a.wav", 16000)
    _write_wav(wavs / "b.wav", 719)

    def plan(*extra, src=wavs, model=wl):
        LI.main([str(src), str(tmp_path / "linear.npz"), str(tmp_path / "never"), "--ssl-model", str(model), "--dry-run", "--verbose", "0", *extra])
        return json.loads(capsys.readouterr().out)

    p = plan("--layer", "1", "--batch-size", "3")
    assert (p["encoder"], p["layer"], p["layers_run"], p["frames"], p["samples"], p["frame_rate"]) == ("wavlm", 1, 1, 49 + 1, 16719, 50)
    assert (p["utterances"], p["batch_size"], p["ssl_precision"], p["hidden_size"]) == (["a", "b"], 3, "f32", 128)
    assert plan("--layer", "-1")["layers_run"] == 2
    assert plan("--layer", "0", src=wavs / "a.wav")["utterances"] == ["a"]  # one wav file
    (tmp_path / "wav.scp").write_text(f"x {wavs / 'a.wav'}\ny {wavs / 'b.wav'}\n")
    assert plan("--layer", "0", src=tmp_path / "wav.scp")["utterances"] == ["x", "y"]
    assert not (tmp_path / "never").exists()
    with pytest.raises(ValueError, match="--layer 9 outside -1 .. 1"):
        plan()  # (the reference's default, on a two-layer model)
    with pytest.raises(ValueError, match="WavLM: precision='bf16x3a' is not built"):
        plan("--layer", "1", "--ssl-precision", "bf16x3a")
    hub = tmp_path / "hub"
    hub.mkdir()
    (hub / "config.json").write_text(json.dumps(HUBERT_TINY))
    assert plan("--layer", "1", "--ssl-precision", "bf16x3a", model=hub)["encoder"] == "hubert"
    _write_wav(wavs / "c.wav", 399)
    with pytest.raises(ValueError, match=r"c\.wav: 399 samples"):
        plan("--layer", "1")
    (wavs / "c.wav").unlink()
    _write_wav(wavs / "d.wav", 8000, rate=8000)
    with pytest.raises(ValueError, match=r"d\.wav: sampling rate 8000"):
        plan("--layer", "1")
