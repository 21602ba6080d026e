"""CPU restatement of the BiGRU inversion model for the tests, from a reference-layout state_dict with torch's own operators
(torch.nn.GRU, F.linear, F.batch_norm on the running statistics) — the reference's forward, pytorch_models.py:45-72, in eval mode.

Test infrastructure only: no file of the package imports it.  ``forward`` takes (B, C, T) and returns (B, out, T); ``lengths`` runs every
utterance of a padded batch ALONE with its own length (rows past it come back as zeros), which is what the native ``lengths=`` promises;
``inference`` is pytorch_models.py:86-105.
"""

import numpy as np
import torch
import torch.nn.functional as F


class BiGRUOracle:
    def __init__(self, state_dict, use_tanh=False, dtype=torch.float32):
        sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()}
        self.dtype = dtype
        self.use_tanh = use_tanh
        H = sd["gru1.weight_hh_l0"].shape[1]
        self.grus = []
        for name in ("gru1", "gru2"):
            g = torch.nn.GRU(input_size=sd[name + ".weight_ih_l0"].shape[1], hidden_size=H, num_layers=1, batch_first=True, bidirectional=True)
            g.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}, strict=True)
            self.grus.append(g.to(dtype).eval())
        f = lambda k: sd[k].to(dtype)  # noqa: E731
        self.fc1 = (f("fc1.0.weight"), f("fc1.0.bias"))
        self.bn = (f("bn.running_mean"), f("bn.running_var"), f("bn.weight"), f("bn.bias"))
        fc2 = "fc2.0" if use_tanh else "fc2"
        self.fc2 = (f(fc2 + ".weight"), f(fc2 + ".bias"))
        self.mean = self.scale = None

    def register_stats(self, mean, scale):
        self.mean = torch.as_tensor(np.asarray(mean)).to(self.dtype)
        self.scale = torch.as_tensor(np.asarray(scale)).to(self.dtype)

    @torch.no_grad()
    def forward(self, x, lengths=None):
        x = torch.as_tensor(np.asarray(x)).to(self.dtype)
        if lengths is not None:
            out = torch.zeros((x.shape[0], self.fc2[0].shape[0], x.shape[2]), dtype=self.dtype)
            for b, n in enumerate(lengths):
                if n > 0:
                    out[b, :, :n] = self.forward(x[b:b + 1, :, :n])[0]
            return out
        y = x.transpose(1, 2)
        for g in self.grus:
            y, _ = g(y)
        y = F.linear(y, *self.fc1).transpose(1, 2)
        y = F.batch_norm(y, self.bn[0], self.bn[1], self.bn[2], self.bn[3], training=False, eps=1e-5).transpose(1, 2)
        y = F.linear(y, *self.fc2)
        if self.use_tanh:
            y = torch.tanh(y)
        return y.transpose(1, 2)

    def inference(self, c, normalize_before=True):
        c = torch.as_tensor(np.asarray(c)).to(self.dtype)
        if normalize_before:
            c = (c - self.mean) / self.scale
        return self.forward(c.unsqueeze(0).transpose(1, 2)).transpose(1, 2).squeeze(0)
