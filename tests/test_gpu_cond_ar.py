"""Autoregressive synthesis of speaker- / phoneme-conditioned models on a MI355X, through every loop the package has (C ABI
hificar_ar_loop_cond, hificar_ar_loop_packed_cond, hificar_ar_step_cond).  The definition every test is held to: one utterance's
result is the reference's chunking and feedback (decode.py:54-83) with every chunk's forward the reference's
``forward(c, spk_id=, ar=prev, ph=)`` (hifigan.py:212-220) on the utterance's speaker and the chunk's slice of its phoneme row; in a
batch, a packed list or a set of streaming sessions every utterance gets that result as if it were alone.
``pytest -m gpu``; both conv arithmetics, as tests/test_gpu_stream.py."""

import ast
import os

import numpy as np
import pytest
import torch

from conftest import E2W_PARAMS, GOLDEN, rel_err, same_across_shapes
from articulatory_amd.bin import decode
from articulatory_amd.models import GBlockGenerator, HiFiGANGenerator
from articulatory_amd.streaming import StreamingSynthesizer
from articulatory_amd.utils.synth import synth_features, synth_gblock_state_dict, synth_state_dict

pytestmark = pytest.mark.gpu

PRECISIONS = [os.environ["HIFICAR_PRECISION"]] if os.environ.get("HIFICAR_PRECISION") else ["f32", "bf16x3"]
TOLS = {"f32": 2e-5, "bf16x3": 2e-4}
XSHAPE_TOL = {"f32": 5e-6, "bf16x3": 2e-4}
LENGTHS = [260, 131, 130, 99, 64, 26, 25, 7, 0]
ABANDONED = 2
CHUNK = 25
SPK_PARAMS = dict(E2W_PARAMS, channels=128, use_spk_id=True, num_spk=5, spk_emb_size=32)
PH_PARAMS = dict(E2W_PARAMS, channels=128, in_channels=13 + 128 + 8, use_ph=True, num_ph=11, ph_emb_size=8)
CASES = {"spk": (SPK_PARAMS, 4321), "ph": (PH_PARAMS, 4323)}


def make(prec, tag):
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' on CPU boxes"
    params, seed = CASES[tag]
    sd = synth_state_dict(params, seed=seed)
    g = HiFiGANGenerator(**params, precision=prec)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g.remove_weight_norm()
    return g.eval().to("cuda:0")


@pytest.fixture(params=PRECISIONS, scope="module")
def prec(request):
    return request.param


@pytest.fixture(params=sorted(CASES), scope="module")
def tag(request):
    return request.param


@pytest.fixture(scope="module")
def model(prec, tag):
    return make(prec, tag)


def utterances(g, seed=2024, lengths=LENGTHS):
    """Device utterances (T_i, 13) with a speaker each (use_spk_id) or a phoneme row each (use_ph): neighbours never share a speaker."""
    rng = np.random.default_rng(seed)
    feats = synth_features(len(lengths), max(max(lengths), 1), 13, seed=seed)
    utts = [torch.from_numpy(feats[u, :n]).cuda() for u, n in enumerate(lengths)]
    spks = [int((3 * u + 1) % g._params["num_spk"]) for u in range(len(lengths))] if g.use_spk_id else None
    phs = [torch.from_numpy(rng.integers(0, g._params["num_ph"], size=n)).cuda() for n in lengths] if g.use_ph else None
    return utts, spks, phs


def cond_of(spks, phs, u):
    return dict(spk_id=None if spks is None else torch.tensor([spks[u]]), ph=None if phs is None else phs[u][None])


def alone(g, x, chunk=CHUNK, spk_id=None, ph=None):
    return g.ar_synthesis(x.t()[None].contiguous(), chunk, spk_id=spk_id, ph=ph)[0]


def python_loop(g, x, chunk, spk_id=None, ph=None):
    """The definition through the pinned forward: one g(c_chunk, spk_id=, ar=prev, ph=) call per chunk."""
    prev = torch.zeros((1, 1, g._params["ar_input"]), device=x.device)
    outs = []
    for i in range(0, len(x), chunk):
        kw = {}
        if spk_id is not None:
            kw["spk_id"] = spk_id.to(x.device)
        if ph is not None:
            kw["ph"] = ph[:, i:i + chunk]
        y = g(x[i:i + chunk].t()[None].contiguous(), ar=prev, **kw)
        y = y[0] if isinstance(y, tuple) else y
        outs.append(y[0, 0])
        prev = y[:, :, -g._params["ar_input"]:]
    return torch.cat(outs)


# ---- against the reference -----------------------------------------------------------------------------------------------------------
def test_reference_golden(model, tag):
    g = model
    gold = np.load(os.path.join(GOLDEN, "gold_arloop_cond.npz"))
    for T in (60, 260):
        x = torch.from_numpy(gold[f"{tag}_x{T}"]).cuda()
        spk = torch.from_numpy(gold[f"spk_spk{T}"]).reshape(1) if tag == "spk" else None
        ph = torch.from_numpy(gold[f"ph_ph{T}"])[None].cuda() if tag == "ph" else None
        with torch.no_grad():
            y = alone(g, x, int(gold["chunk_frames"]), spk, ph)
            if tag == "spk":
                other = alone(g, x, CHUNK, (spk + 1) % 5, None)
            else:
                other = alone(g, x, CHUNK, None, torch.roll(ph, 1, dims=1))
        assert y.shape == (80 * T,)
        err, diff = rel_err(y.cpu().numpy(), gold[f"{tag}_out{T}"]), rel_err(other.cpu().numpy(), gold[f"{tag}_out{T}"])
        print(f"{tag} {g.precision} T={T}: vs reference {err:.3e}; other speaker / shifted phonemes differ by {diff:.3e}")
        assert err < TOLS[g.precision], (tag, T)
        assert diff > 1e-2, (tag, T)  # the conditioning matters


# ---- against the pinned forward ------------------------------------------------------------------------------------------------------
def _loop_equals_per_chunk_forward(g):
    utts, spks, phs = utterances(g, seed=31, lengths=[60, 260])
    with torch.no_grad():
        for u, x in enumerate(utts):
            kw = cond_of(spks, phs, u)
            assert same_across_shapes(alone(g, x, CHUNK, **kw), python_loop(g, x, CHUNK, **kw), XSHAPE_TOL[g.precision]), u


def test_loop_equals_per_chunk_forward(model):
    _loop_equals_per_chunk_forward(model)


def test_loop_equals_per_chunk_forward_bit_for_bit_without_split_k(monkeypatch, prec, tag):
    monkeypatch.setenv("HIFICAR_KSPLIT", "0")  # read when the handle is created: a fresh model
    _loop_equals_per_chunk_forward(make(prec, tag))  # same_across_shapes is torch.equal in this mode


# ---- batches -------------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_ragged_and_packed(model):
    """Mixed speakers / phoneme rows and mixed lengths, the empty utterance included: ragged, and packed with fewer slots than
    utterances (a slot is taken over by an utterance of another speaker)."""
    g = model
    utts, spks, phs = utterances(g)
    padded, lens = decode.pad_utterances(utts)
    c = padded.permute(0, 2, 1).contiguous()
    spk = None if spks is None else torch.tensor(spks)
    ph = None if phs is None else decode._ph_tensor(phs, lens, "cuda:0")
    with torch.no_grad():
        ragged = g.ar_synthesis(c, CHUNK, lengths=lens, spk_id=spk, ph=ph)
        packed = g.ar_synthesis_packed(c, CHUNK, lens, batch=4, spk_id=spk, ph=ph)
        listed = decode.ar_loop_ragged(g, utts, {"batch_max_steps": 80 * CHUNK, "hop_size": 80, "generator_params": g._params}, batch=3,
                                       spk_id=spks, ph=phs)
        for u, n in enumerate(LENGTHS):
            assert float(ragged[u, 80 * n:].abs().sum()) == 0.0 and float(packed[u, 80 * n:].abs().sum()) == 0.0
            assert listed[u].shape == (80 * n,)
            if n:
                ref = alone(g, utts[u], CHUNK, **cond_of(spks, phs, u))
                for name, y in (("ragged", ragged[u, :80 * n]), ("packed", packed[u, :80 * n]), ("decode.ar_loop_ragged", listed[u])):
                    assert same_across_shapes(y, ref, XSHAPE_TOL[g.precision]), (name, u, n)


def test_two_stream_window_gives_the_second_half_its_own_conditioning(model):
    g = model
    B, T = 20, 60  # inside the default two-stream window (HIFICAR_AR_DUAL_MIN.._MAX = 17..62): halves of 10
    utts, spks, phs = utterances(g, seed=77, lengths=[T] * B)
    if spks is not None:
        spks = [int(v) for v in np.random.default_rng(77).integers(0, 5, size=B)]
        assert len(set(spks[10:])) > 1 and spks[:10] != spks[10:]
    c = torch.stack(utts).permute(0, 2, 1).contiguous()
    with torch.no_grad():
        y = g.ar_synthesis(c, CHUNK, spk_id=None if spks is None else torch.tensor(spks), ph=None if phs is None else torch.stack(phs))
        z = decode.ar_loop_batch(g, torch.stack(utts), {"batch_max_steps": 80 * CHUNK, "hop_size": 80, "generator_params": g._params},
                                 spk_id=None if spks is None else torch.tensor(spks), ph=None if phs is None else torch.stack(phs))
        assert torch.equal(y, z)
        for u in range(B):
            assert same_across_shapes(y[u], alone(g, utts[u], CHUNK, **cond_of(spks, phs, u)), XSHAPE_TOL[g.precision]), u


# ---- streaming -----------------------------------------------------------------------------------------------------------------------
def drive(st, utts, spks, phs, seed, max_packet=40, abandon=None, abandon_after=50):
    """tests/test_gpu_stream.py's drive with a speaker per session / phoneme indices per packet: sessions opened in order as rows
    free up, fed in seeded random packets, flushed after their last frame, one step() per round."""
    rng = np.random.default_rng(seed)
    pending = list(range(len(utts)))
    live = {}
    outs = {u: [] for u in range(len(utts))}
    rows = {}
    while pending or live:
        while pending and len(st.sched.sessions()) < st.sched.max_sessions:
            u = pending.pop(0)
            sid = st.open(**({} if spks is None else {"spk_id": spks[u]}))
            live[sid] = [u, 0]
            rows[u] = st.sched.row(sid)
            if len(utts[u]) == 0:
                st.flush(sid)
        for sid, (u, done) in list(live.items()):
            if not st.sched.is_open(sid) or done == len(utts[u]) and done > 0:
                continue
            if u == abandon and done >= abandon_after:
                st.close(sid)
                outs[u] = None
                continue
            room = st.sched.ring_frames - st.sched.buffered(sid)
            n = min(int(rng.integers(1, max_packet + 1)), len(utts[u]) - done, room)
            if n > 0:
                ph = None if phs is None else phs[u][done:done + n]
                if ph is not None and rng.integers(0, 2):
                    ph = ph.cpu().numpy()  # host and device packets alike
                st.push(sid, utts[u][done:done + n], **({} if ph is None else {"ph": ph}))
                live[sid][1] += n
            if live[sid][1] == len(utts[u]):
                st.flush(sid)
        for sid, y in st.step().items():
            outs[live[sid][0]].append(y)
        live = {sid: v for sid, v in live.items() if st.sched.is_open(sid)}
    cat = {u: (torch.cat(o) if o else torch.zeros(0, device="cuda:0")) if o is not None else None for u, o in outs.items()}
    return [cat[u] for u in range(len(utts))], rows


def _sessions_reproduce_the_offline_loop(g):
    utts, spks, phs = utterances(g)
    st = StreamingSynthesizer(g, CHUNK, max_sessions=4, conditioned=True)  # ring of 100 frames: the 260-frame session wraps twice
    with torch.no_grad():
        ys, rows = drive(st, utts, spks, phs, seed=7, abandon=ABANDONED)
        assert ys[ABANDONED] is None
        taken = [u for u in range(ABANDONED + 1, len(LENGTHS)) if rows[u] == rows[ABANDONED]]
        assert taken, rows  # a later session reused the abandoned row ...
        assert spks is None or any(spks[u] != spks[ABANDONED] for u in taken)  # ... with another speaker
        for u, n in enumerate(LENGTHS):
            if u == ABANDONED:
                continue
            assert ys[u].shape == (80 * n,), u
            if n:
                assert same_across_shapes(ys[u], alone(g, utts[u], CHUNK, **cond_of(spks, phs, u)), XSHAPE_TOL[g.precision]), (u, n)


def test_sessions_reproduce_the_offline_loop(model):
    _sessions_reproduce_the_offline_loop(model)


def test_sessions_bit_for_bit_without_split_k(monkeypatch, prec, tag):
    monkeypatch.setenv("HIFICAR_KSPLIT", "0")
    _sessions_reproduce_the_offline_loop(make(prec, tag))


def test_a_step_launches_the_kernels_of_one_ar_synthesis_step(model):
    g = model
    n = 3
    utts, spks, phs = utterances(g, seed=11, lengths=[CHUNK] * n)
    st = StreamingSynthesizer(g, CHUNK, max_sessions=8, conditioned=True)
    sids = [st.open(**({} if spks is None else {"spk_id": spks[b]})) for b in range(n)]
    c = torch.stack(utts).permute(0, 2, 1).contiguous()
    kw = dict(spk_id=None if spks is None else torch.tensor(spks).cuda(), ph=None if phs is None else torch.stack(phs))
    with torch.no_grad():
        for k in range(2):  # the first round builds the launch shapes' schedules
            for b, sid in enumerate(sids):
                st.push(sid, utts[b], **({} if phs is None else {"ph": phs[b].cpu()}))
            if k:
                g.profile_begin()
            st.step()
            if k:
                streamed = sorted((s["name"], s["launches"]) for s in g.profile_end())
            g.ar_synthesis(c, CHUNK, **kw)
        g.profile_begin()
        g.ar_synthesis(c, CHUNK, **kw)
        offline = sorted((s["name"], s["launches"]) for s in g.profile_end())
    assert streamed == offline
    assert any(name == "front_kernel" for name, _ in streamed) and any(name == "output_conv_kernel" for name, _ in streamed)


def test_step_does_not_wait_for_the_device(model):
    g = model
    n = 3
    utts, spks, phs = utterances(g, seed=12, lengths=[75] * n)
    st = StreamingSynthesizer(g, CHUNK, max_sessions=4, conditioned=True)
    outs = {}
    with torch.no_grad():
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        sids = []
        for b in range(n):
            sids.append(st.open(**({} if spks is None else {"spk_id": spks[b]})))
            outs[sids[b]] = []
            st.push(sids[b], utts[b][:CHUNK], **({} if phs is None else {"ph": phs[b][:CHUNK].cpu()}))
        for sid, y in st.step().items():  # warm-up: this launch shape's schedules exist afterwards
            outs[sid].append(y)
        for b, sid in enumerate(sids):
            st.push(sid, utts[b][CHUNK:], **({} if phs is None else {"ph": phs[b][CHUNK:].cpu()}))
        torch.cuda.synchronize()
        torch.cuda._sleep(100_000_000)  # tens of ms of device work ahead of the steps
        extra = st.open(**({} if spks is None else {"spk_id": 0}))  # a session joining meanwhile: its speaker is written in stream order
        r1 = st.step()
        r2 = st.step()
        busy = not stream.query()
        torch.cuda.synchronize()
        assert busy, "open() / step() waited for the device"
        st.close(extra)
        for r in (r1, r2):
            for sid, y in r.items():
                outs[sid].append(y)
        for b, sid in enumerate(sids):
            ref = alone(g, utts[b], CHUNK, **cond_of(spks, phs, b))
            assert same_across_shapes(torch.cat(outs[sid]), ref, XSHAPE_TOL[g.precision]), b


# ---- refusals: each raises and enqueues nothing ------------------------------------------------------------------------------------------
def test_refusals(model, tag):
    g = model
    x = torch.zeros(2, 13, 50, device="cuda:0")
    ok_spk, ok_ph = torch.zeros(2, dtype=torch.int64), torch.zeros(2, 50, dtype=torch.int64)
    g.profile_begin()
    try:
        with pytest.raises(ValueError, match="hificar_forward_cond"):  # no conditioning: exactly as before
            g.ar_synthesis(x, CHUNK)
        with pytest.raises(ValueError, match="hificar_forward_cond"):
            g.ar_synthesis_packed(x, CHUNK, [50, 20])
        with pytest.raises(ValueError, match="conditioned"):
            StreamingSynthesizer(g, CHUNK)
        st = StreamingSynthesizer(g, CHUNK, max_sessions=2, conditioned=True)
        if tag == "spk":
            with pytest.raises(RuntimeError, match="3 entries for a batch of 2"):
                g.ar_synthesis(x, CHUNK, spk_id=torch.zeros(3, dtype=torch.int64))
            for bad in (torch.tensor([0, 5]), torch.tensor([-1, 0])):
                with pytest.raises(IndexError, match="index out of range in self"):
                    g.ar_synthesis(x, CHUNK, spk_id=bad)
                with pytest.raises(IndexError, match="index out of range in self"):
                    g.ar_synthesis_packed(x, CHUNK, [50, 20], spk_id=bad)
            with pytest.raises(ValueError, match="use_ph=false"):
                g.ar_synthesis(x, CHUNK, spk_id=ok_spk, ph=ok_ph)
            with pytest.raises(ValueError, match="needs the session's spk_id"):
                st.open()
            for bad in (5, -1):
                with pytest.raises(IndexError, match="index out of range in self"):
                    st.open(spk_id=bad)
            assert st.sched.sessions() == []  # a refused open() takes no row
            sid = st.open(spk_id=4)
            with pytest.raises(ValueError, match="use_ph=False"):
                st.push(sid, torch.zeros(5, 13), ph=torch.zeros(5, dtype=torch.int64))
        else:
            with pytest.raises(RuntimeError, match=r"ph=\(B, T\)=\(2, 50\)"):
                g.ar_synthesis(x, CHUNK, ph=ok_ph[:, :49])
            bad = ok_ph.clone()
            bad[1, 49] = 11
            for b in (bad, bad.cuda(), -ok_ph - 1):
                with pytest.raises(IndexError, match="index out of range in self"):
                    g.ar_synthesis(x, CHUNK, ph=b)
            with pytest.raises(ValueError, match="use_spk_id=false"):
                g.ar_synthesis(x, CHUNK, spk_id=ok_spk, ph=ok_ph)
            with pytest.raises(ValueError, match="use_spk_id=False"):
                st.open(spk_id=0)
            sid = st.open()
            with pytest.raises(ValueError, match="needs ph"):
                st.push(sid, torch.zeros(5, 13))
            with pytest.raises(ValueError, match=r"ph must be \(5,\)"):
                st.push(sid, torch.zeros(5, 13), ph=torch.zeros(4, dtype=torch.int64))
            for b in (torch.tensor([0, 1, 2, 3, 11]), torch.tensor([0, 1, 2, 3, 11]).cuda(), np.array([0, -1, 2, 3, 4])):
                with pytest.raises(IndexError, match="index out of range in self"):
                    st.push(sid, torch.zeros(5, 13), ph=b)
            assert st.sched.buffered(sid) == 0  # a refused push buffers nothing
        assert st.step() == {}
    finally:
        launched = g.profile_end()
    assert launched == [], launched


# ---- GBlockGenerator (speaker conditioning is the only conditioning it has) ------------------------------------------------------------
def test_gblock_speaker_conditioned_loop_and_sessions():
    p = dict(ast.literal_eval(str(np.load(os.path.join(GOLDEN, "gold_gblock_small.npz"))["params"])))
    assert p["use_ar"]
    p.update(use_spk_id=True, num_spk=5, spk_emb_size=8)
    sd = synth_gblock_state_dict(p, seed=1234)
    g = GBlockGenerator(**p)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g.remove_weight_norm()
    g = g.eval().to("cuda:0")
    cf = p["in_channels"] - p["ar_output"]
    lengths = [60, 33, 25, 7]
    feats = synth_features(len(lengths), max(lengths), cf, seed=5)
    utts = [torch.from_numpy(feats[u, :n]).cuda() for u, n in enumerate(lengths)]
    spks = [4, 0, 2, 3]
    hop = g.hop
    with torch.no_grad():
        refs = [python_loop(g, x, CHUNK, spk_id=torch.tensor([s])) for x, s in zip(utts, spks)]
        padded, lens = decode.pad_utterances(utts)
        packed = g.ar_synthesis_packed(padded.permute(0, 2, 1).contiguous(), CHUNK, lens, batch=2, spk_id=torch.tensor(spks))
        st = StreamingSynthesizer(g, CHUNK, max_sessions=2, ring_chunks=2, conditioned=True)
        ys, _ = drive(st, utts, spks, None, seed=3, max_packet=17)
        for u, n in enumerate(lengths):
            assert refs[u].shape == (hop * n,)
            assert same_across_shapes(alone(g, utts[u], CHUNK, spk_id=torch.tensor([spks[u]])), refs[u]), u
            assert same_across_shapes(packed[u, :hop * n], refs[u]), u
            assert same_across_shapes(ys[u], refs[u]), u
        other = alone(g, utts[0], CHUNK, spk_id=torch.tensor([1]))
        assert rel_err(other.cpu().numpy(), refs[0].cpu().numpy()) > 1e-2
