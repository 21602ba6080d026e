"""Streaming synthesis: many live sessions of the reference's chunked AR loop on one GPU (C ABI: ``hificar_ar_step``, and
``hificar_ar_step_cond`` for speaker- / phoneme-conditioned models: one model, each session its own voice).

The reference's ``ar_loop`` (articulatory/bin/decode.py:54-83) conditions each chunk on one thing only, the last ``ar_input``
output samples of the chunk before it.  :class:`StreamingSynthesizer` keeps that context on the device between calls, one row of a
context arena per session, and feeds every session's EMA frames through a device feature ring as they arrive.  Each
:meth:`StreamingSynthesizer.step` is one native call that advances every session with a full chunk buffered (or flushed with frames
left) by one chunk: the kernels of one ``ar_synthesis`` step of that batch, no gather / copy launches, no host wait.

Per session the concatenated output equals ``ar_loop`` on the concatenation of its pushed frames, whatever the packet sizes and the
other sessions in flight: bit for bit with ``HIFICAR_KSPLIT=0``, to fp32 rounding otherwise (the launch shapes differ).

The host bookkeeping (which sessions advance, ring offsets, first-chunk flags, row reuse) is :class:`StreamSchedule`, which knows
nothing of the device.
"""

import ctypes

import numpy as np
import torch

from . import _native
from ._owner import current_stream


class _Session:
    __slots__ = ("row", "pushed", "consumed", "flushed")

    def __init__(self, row):
        self.row = row
        self.pushed = 0      # frames pushed so far; frame f lives in ring column f % ring_frames
        self.consumed = 0    # frames already synthesised (a multiple of chunk_frames until the final chunk)
        self.flushed = False


class StreamSchedule:
    """Host bookkeeping of the sessions: rows, ring placement, which sessions a step advances.

    A session's frame f lives in column ``f % ring_frames`` of its row of the feature ring.  Chunks start at multiples of
    ``chunk_frames`` and ``ring_frames`` is a multiple of it, so a chunk never wraps; a push may."""

    def __init__(self, max_sessions, chunk_frames, ring_chunks):
        if max_sessions < 1 or chunk_frames < 1 or ring_chunks < 1:
            raise ValueError(f"max_sessions={max_sessions}, chunk_frames={chunk_frames}, ring_chunks={ring_chunks} must be positive")
        self.max_sessions = int(max_sessions)
        self.chunk_frames = int(chunk_frames)
        self.ring_frames = int(ring_chunks) * self.chunk_frames
        self._sessions = {}  # id -> _Session, in opening order
        self._rows = [None] * self.max_sessions  # row -> id
        self._next_id = 0

    def open(self):
        """A new session on the lowest free row; its id (ids are never reused)."""
        try:
            row = self._rows.index(None)
        except ValueError:
            raise RuntimeError(f"all {self.max_sessions} sessions are in use: close or flush one first") from None
        sid = self._next_id
        self._next_id += 1
        self._rows[row] = sid
        self._sessions[sid] = _Session(row)
        return sid

    def _get(self, sid):
        s = self._sessions.get(sid)
        if s is None:
            raise KeyError(f"session {sid} is not open (unknown, closed, or finished after its flush)")
        return s

    def row(self, sid):
        return self._get(sid).row

    def is_open(self, sid):
        return sid in self._sessions

    def sessions(self):
        return list(self._sessions)

    def buffered(self, sid):
        s = self._get(sid)
        return s.pushed - s.consumed

    def push(self, sid, t):
        """Reserve ring room for t more frames of a session: [(ring column, source offset, frames)] (two pieces when the push wraps)."""
        s = self._get(sid)
        if s.flushed:
            raise RuntimeError(f"session {sid} was flushed: no more frames can be pushed")
        t = int(t)
        if t < 0:
            raise ValueError("a push cannot have a negative number of frames")
        if s.pushed + t - s.consumed > self.ring_frames:
            raise RuntimeError(f"session {sid}: {s.pushed - s.consumed} frames buffered + {t} pushed exceed the ring's {self.ring_frames}; "
                               "call step() first")
        pieces = []
        done = 0
        while done < t:
            col = (s.pushed + done) % self.ring_frames
            n = min(t - done, self.ring_frames - col)
            pieces.append((col, done, n))
            done += n
        s.pushed += t
        return pieces

    def flush(self, sid):
        """No more frames will come: what is buffered becomes the final (possibly shorter) chunk.  A session with nothing left is
        closed at once."""
        s = self._get(sid)
        s.flushed = True
        if s.pushed == s.consumed:
            self.close(sid)

    def close(self, sid):
        """Abandon a session: its buffered frames are dropped and its row is free."""
        s = self._get(sid)
        self._rows[s.row] = None
        del self._sessions[sid]

    def plan(self):
        """The next step: [(id, (row, ring column, valid frames, first))] for every session with a full chunk buffered, or flushed
        with frames left, in opening order.  Nothing changes until :meth:`advance`."""
        out = []
        for sid, s in self._sessions.items():
            left = s.pushed - s.consumed
            if left >= self.chunk_frames or (s.flushed and left > 0):
                valid = min(left, self.chunk_frames)
                out.append((sid, (s.row, s.consumed % self.ring_frames, valid, int(s.consumed == 0))))
        return out

    def advance(self, plan):
        """Commit a step of :meth:`plan`: its sessions consumed their chunk; flushed sessions with nothing left close."""
        for sid, (_, _, valid, _) in plan:
            s = self._sessions[sid]
            s.consumed += valid
            if s.flushed and s.consumed == s.pushed:
                self.close(sid)

    def step(self, native, hop):
        """One step: ``native((n, 4) int32 table)`` returns the (n, hop * chunk_frames) output of its n sequences; it is called only
        when a session is ready.  Returns {id: its hop * valid new samples}."""
        plan = self.plan()
        if not plan:
            return {}
        table = np.array([e for _, e in plan], dtype=np.int32).reshape(len(plan), 4)
        out = native(table)
        self.advance(plan)
        return {sid: out[b, :hop * e[2]] for b, (sid, e) in enumerate(plan)}


class StreamingSynthesizer:
    """Live AR synthesis of up to ``max_sessions`` sessions on one generator (HiFiGANGenerator or GBlockGenerator, use_ar, on the
    GPU), ``chunk_frames`` frames per chunk (``batch_max_steps // hop_size``, decode.py:50).  Inference only, at the model's
    precision.

    A speaker- or phoneme-conditioned model needs ``conditioned=True``: the reference's loop calls ``model(c, ar=prev)`` only
    (decode.py:72) and cannot run one, so leaving it is explicit.  Every chunk's forward is then the reference's
    ``forward(c, spk_id=, ar=prev, ph=)`` (hifigan.py:212-220): ``open(spk_id=)`` gives a use_spk_id session its speaker,
    ``push(sid, frames, ph=)`` a use_ph session the phoneme index of each frame.

    ``push(sid, frames)`` buffers ``(t, C)`` frames (host or device) in the session's device feature ring of ``ring_chunks``
    chunks; ``step()`` advances every ready session by one chunk and returns ``{id: 1-D device tensor of hop * frames samples}``.
    Nothing synchronises the device: the returned tensors are ready in stream order on the current stream."""

    def __init__(self, model, chunk_frames, max_sessions=64, ring_chunks=4, conditioned=False):
        if not getattr(model, "use_ar", False):
            raise ValueError("streaming synthesis needs a use_ar=True generator")
        self.use_spk_id = bool(getattr(model, "use_spk_id", False))
        self.use_ph = bool(getattr(model, "use_ph", False))
        if (self.use_spk_id or self.use_ph) and not conditioned:
            raise ValueError("streaming synthesis of a speaker- or phoneme-conditioned model leaves the reference's ar_loop (it calls "
                             "model(c, ar=prev) only): pass conditioned=True")
        if conditioned and not (self.use_spk_id or self.use_ph):
            raise ValueError("conditioned=True needs a use_spk_id or use_ph generator: this model takes neither")
        p = model._params
        self.model = model
        self.chunk_frames = int(chunk_frames)
        self.hop = int(model.hop)
        self.ar_input = int(p["ar_input"])
        if self.ar_input > self.hop * self.chunk_frames:
            raise ValueError(f"ar_input ({self.ar_input}) > chunk audio length ({self.hop * self.chunk_frames}): the reference loop "
                             "(decode.py:79-81) is ill-formed there")
        self.channels = int(p["in_channels"]) - int(p["ar_output"]) - (int(p["ph_emb_size"]) if self.use_ph else 0)
        self._handle = model._native_handle()  # raises for a model that is not on the GPU
        self.device = model._device()
        self.sched = StreamSchedule(max_sessions, chunk_frames, ring_chunks)
        S, R = self.sched.max_sessions, self.sched.ring_frames
        self._feat = torch.zeros((S, self.channels, R), dtype=torch.float32, device=self.device)
        self._ctx = torch.empty((S, self.ar_input), dtype=torch.float32, device=self.device)  # first-chunk flags: never read unwritten
        # conditioning, addressed by session row like the two above and written in stream order like them (steps may be queued): one
        # speaker per row; a phoneme ring laid out as the feature ring.  Zeros are valid indices: a row never holds anything else
        self._spk = torch.zeros((S,), dtype=torch.int32, device=self.device) if self.use_spk_id else None
        self._ph = torch.zeros((S, R), dtype=torch.int32, device=self.device) if self.use_ph else None

    # -- sessions -----------------------------------------------------------------------------------------------------------------
    def open(self, spk_id=None):
        """A new session (the lowest free row); raises when all max_sessions rows are in use.  ``spk_id``: the session's speaker
        index (a host integer; required for a use_spk_id model, refused otherwise), range-checked here and written into the
        session's row in stream order, without waiting for the device."""
        if self.use_spk_id:
            if spk_id is None:
                raise ValueError("use_spk_id model: open() needs the session's spk_id")
            spk_id = int(spk_id)
            if not 0 <= spk_id < int(self.model._params["num_spk"]):
                raise IndexError("index out of range in self")  # torch.nn.Embedding's message
        elif spk_id is not None:
            raise ValueError("open(spk_id=) on a model built with use_spk_id=False")
        sid = self.sched.open()
        if self.use_spk_id:
            self._spk[self.sched.row(sid)].fill_(spk_id)
        return sid

    def push(self, sid, frames, ph=None):
        """Buffer (t, C) frames of a session (t >= 0; host or device).  Raises when the session's ring would overflow (step()
        first), or for a flushed / unknown session.  Pushes are ordered on the current stream, as steps are.

        ``ph``: the (t,) phoneme indices of these frames (required for a use_ph model, refused otherwise).  Given on the host they
        are range-checked for free; a device tensor is checked as ``forward()`` checks it, with one reduction and a wait for it."""
        frames = torch.as_tensor(frames)
        if frames.dim() != 2 or frames.shape[1] != self.channels:
            raise ValueError(f"frames must be (t, {self.channels}), got {tuple(frames.shape)}")
        if self.use_ph:
            if ph is None:
                raise ValueError("use_ph model: push() needs ph, the (t,) phoneme indices of the frames")
            ph = torch.as_tensor(ph)
            if ph.dim() != 1 or ph.shape[0] != frames.shape[0]:
                raise ValueError(f"ph must be ({frames.shape[0]},), one index per frame, got {tuple(ph.shape)}")
            if ph.numel() and (int(ph.min()) < 0 or int(ph.max()) >= int(self.model._params["num_ph"])):
                raise IndexError("index out of range in self")
        elif ph is not None:
            raise ValueError("push(ph=) on a model built with use_ph=False")
        pieces = self.sched.push(sid, frames.shape[0])
        if not pieces:
            return
        src = frames.to(device=self.device, dtype=torch.float32, non_blocking=True)
        row = self.sched.row(sid)
        for col, off, n in pieces:
            self._feat[row, :, col:col + n].copy_(src[off:off + n].t())
        if self.use_ph:
            psrc = ph.to(device=self.device, dtype=torch.int32, non_blocking=True)
            for col, off, n in pieces:
                self._ph[row, col:col + n].copy_(psrc[off:off + n])

    def flush(self, sid):
        """No more frames: the remainder becomes the session's final, shorter chunk (decode.py:56); the session closes after it."""
        self.sched.flush(sid)

    def close(self, sid):
        """Abandon a session and drop its buffered frames."""
        self.sched.close(sid)

    # -- steps --------------------------------------------------------------------------------------------------------------------
    def step(self):
        """Advance every ready session by one chunk (one native call; none when nothing is ready): {id: new samples}."""
        return self.sched.step(self._step_native, self.hop)

    def _step_native(self, table):
        """One hificar_ar_step[_cond] over the (n, 4) host table {row, ring column, valid, first}: (n, hop * chunk_frames) device output."""
        n = table.shape[0]
        m = self.model
        handle = m._native_handle()
        out = torch.empty((n, self.hop * self.chunk_frames), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws_ptr, ws_bytes = m._workspace(n, self.chunk_frames)
            stream = current_stream()
            if self.use_spk_id or self.use_ph:
                rc = m._lib.hificar_ar_step_cond(handle, self._feat.data_ptr(), self._feat.stride(0), self._feat.stride(1),
                                                 self._spk.data_ptr() if self.use_spk_id else None,
                                                 self._ph.data_ptr() if self.use_ph else None, self._ph.stride(0) if self.use_ph else 0,
                                                 table.ctypes.data_as(ctypes.c_void_p), n, self.chunk_frames, self._ctx.data_ptr(),
                                                 self.sched.max_sessions, out.data_ptr(), ws_ptr, ws_bytes, stream)
            else:
                rc = m._lib.hificar_ar_step(handle, self._feat.data_ptr(), self._feat.stride(0), self._feat.stride(1),
                                            table.ctypes.data_as(ctypes.c_void_p), n, self.chunk_frames, self._ctx.data_ptr(),
                                            self.sched.max_sessions, out.data_ptr(), ws_ptr, ws_bytes, stream)
        _native.check(rc, "hificar_ar_step")
        return out
