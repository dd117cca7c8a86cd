"""Stateful streaming inference for the causal SuDoRM-RF (v3): ``CausalSuDORMRF.stream()`` returns a ``CausalStream``,
``CausalSuDORMRF.stream_pool()`` a ``CausalStreamPool`` whose streams open, push and close independently of each other.

A session owns three device buffers (prepared weights, state, workspace) and a small remainder of samples that do not
fill a granule yet.  ``push`` takes any number of new samples per stream and returns every separated sample that
became final; ``finish`` pads to the reference's length rule and returns the rest, so that the concatenation is the full
forward's output.  All arithmetic is the srf_stream_* entry points of libsudormrf_hip.so (include/sudormrf_hip.h); torch
is used for memory, slicing and concatenation only, and nothing here synchronises with the host.
"""
import ctypes as C

import torch

from . import _lib
from .dnn.models._base import _refuse_autograd
from .engine import _checked_params, _config_struct, _weights


def _pyramid_lds_bytes(depth, frames):
    """LDS of srf_stream_pyramid_kernel for a chunk of `frames` frames (stream_pyr_lds of csrc/srf_causal_stream.hip): four rows per
    wavefront, per row [10 of state | input] of every level and the last level's output."""
    per_row = sum(10 + (frames if k == 0 else frames >> (k - 1)) for k in range(depth)) + (frames >> (depth - 1))
    return 4 * 4 * per_row


def default_max_chunk(enc_kernel_size, upsampling_depth):
    """max_chunk_samples of a session opened without one: 16 granules where the streaming pyramid holds such a chunk in its
    64 KiB of LDS (every depth up to 7), else the most granules that fit (10 at depth 8, where 16 granules are 2048 frames
    and srf_stream_create refuses them)."""
    h, depth = enc_kernel_size // 2, max(upsampling_depth, 1)
    unit = 1 << (depth - 1)
    n = 16
    while n > 1 and _pyramid_lds_bytes(depth, n * unit) > 64 * 1024:
        n -= 1
    return n * h * unit


class _Session:
    """The srf_stream handle and its geometry (needs no GPU)."""

    def __init__(self, cfg_tuple, batch, max_chunk=None):
        lib = _lib.load()
        cfg = _config_struct(*cfg_tuple[:10])
        if max_chunk is None:
            # 16 granules, or as many as the streaming pyramid's LDS takes (10 at depth 8), from the config alone (the
            # library checks the same arithmetic)
            max_chunk = default_max_chunk(cfg.enc_kernel_size, cfg.upsampling_depth)
        handle = C.c_void_p()
        _lib.check(lib.srf_stream_create(C.byref(cfg), int(batch), int(max_chunk), C.byref(handle)), "srf_stream_create")
        self.handle = handle
        if len(cfg_tuple) > 10:
            scales = cfg_tuple[10]
            alpha = (C.c_float * len(scales))(*[a for a, _ in scales])
            beta = (C.c_float * len(scales))(*[b for _, b in scales])
            _lib.check(lib.srf_stream_set_block_scales(handle, alpha, beta, len(scales)), "srf_stream_set_block_scales")
        self.batch, self.max_chunk = int(batch), int(max_chunk)
        self.granule = lib.srf_stream_granule(handle)
        self.delay = lib.srf_stream_delay(handle)
        self.state_bytes = lib.srf_stream_state_bytes(handle)
        self.weights_bytes = lib.srf_stream_weights_bytes(handle)
        self.workspace_bytes = lib.srf_stream_workspace_bytes(handle)
        self.num_launches = lib.srf_stream_num_launches(handle)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().srf_stream_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def _buffer(nbytes, device):
    t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    if t.data_ptr() % 256:
        raise _lib.SrfError("torch returned a buffer that is not 256-byte aligned")
    return t


def _prepare_weights(owner, who):
    """srf_stream_prepare of owner._module's parameters into owner._weights (CausalStream and CausalStreamPool)."""
    if owner._module._config_tuple() != owner._cfg_tuple:
        raise _lib.SrfError("%s: the module's configuration or block scales changed; open a new stream" % who)
    params = _checked_params(_weights(owner._module), owner.device, detach=True)
    arr = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
    with torch.cuda.device(owner.device):
        rc = _lib.load().srf_stream_prepare(owner._s.handle, arr, len(params), _lib.ptr(owner._weights), owner._stream())
    _lib.check(rc, "srf_stream_prepare")


class CausalStream:
    """One streaming session over ``batch`` independent streams of a CausalSuDORMRF.

    The weights are snapshot at construction (and by ``refresh_weights()``): later in-place changes of the module's
    parameters do not reach a running session until it is refreshed."""

    def __init__(self, module, batch=1, max_chunk=None, device=None):
        self._module = module
        _refuse_autograd("CausalSuDORMRF.stream", list(module.parameters()))
        weights = _weights(module)
        device = torch.device(device) if device is not None else weights[0].device
        if device.type != "cuda":
            raise _lib.SrfError("sudo_rm_rf_amd runs on an MI355X only: the module is on %s.  There is deliberately no CPU "
                                "fallback (use the reference implementation for CPU inference)." % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self._cfg_tuple = module._config_tuple()
        self._s = _Session(self._cfg_tuple, batch, max_chunk)
        self._A = module.in_audio_channels
        self._SA = module.num_sources * module.in_audio_channels
        # the reference pads a signal to a multiple of this many samples (n_least_samples_req)
        self._pad_unit = module.n_least_samples_req
        with torch.cuda.device(device):
            self._weights = _buffer(self._s.weights_bytes, device)
            self._state = _buffer(self._s.state_bytes, device)
            self._workspace = _buffer(self._s.workspace_bytes, device)
        self._rem = torch.empty((self._s.batch, self._A, 0), dtype=torch.float32, device=device)
        self._pos = 0              # samples pushed through the kernels since the last reset
        self._emitted = 0          # samples returned since the last reset
        self._head_pending = True  # the next output still starts with `delay` negative-time samples
        self.refresh_weights()
        self.reset()

    # -- geometry ----------------------------------------------------------------------------
    granule = property(lambda self: self._s.granule, doc="samples per granule g = h * 2^(D-1): pushes are cut at multiples of it")
    delay = property(lambda self: self._s.delay, doc="output delay h = enc_kernel_size // 2 samples")
    state_bytes = property(lambda self: self._s.state_bytes, doc="device bytes of state carried between pushes")
    batch = property(lambda self: self._s.batch)
    max_chunk = property(lambda self: self._s.max_chunk)
    num_launches = property(lambda self: self._s.num_launches, doc="kernel launches per srf_stream_push")

    def _stream(self):
        return _lib.current_stream(self.device)

    # -- weights and state -------------------------------------------------------------------
    def refresh_weights(self):
        """Snapshot the module's parameters again (srf_stream_prepare): skipinit_gain is read on the device."""
        _prepare_weights(self, "CausalStream")

    def reset(self, rows=None):
        """Start new streams.  rows=None: every stream, position and remainder included.  rows=[...]: only those streams'
        state, on a granule boundary (no remainder pending); the batch position carries on, so the first `delay` samples
        the next push returns for those rows lie before their new start and are the caller's to drop."""
        lib = _lib.load()
        with torch.cuda.device(self.device):
            if rows is None:
                _lib.check(lib.srf_stream_reset(self._s.handle, _lib.ptr(self._state), -1, self._stream()), "srf_stream_reset")
                self._rem = self._rem[..., :0]
                self._pos = 0
                self._emitted = 0
                self._head_pending = True
                return
            if self._rem.shape[-1]:
                raise _lib.SrfError("CausalStream.reset(rows): %d samples are pending below a granule; single streams restart "
                                    "on a granule boundary" % self._rem.shape[-1])
            for r in rows:
                _lib.check(lib.srf_stream_reset(self._s.handle, _lib.ptr(self._state), int(r), self._stream()), "srf_stream_reset")

    # -- data path ---------------------------------------------------------------------------
    def _check_input(self, x):
        if not isinstance(x, torch.Tensor):
            raise TypeError("input must be a torch.Tensor")
        _refuse_autograd("CausalStream.push", [x])
        if x.device.type != "cuda":
            raise _lib.SrfError("sudo_rm_rf_amd runs on an MI355X only: input is on %s.  There is deliberately no CPU "
                                "fallback (use the reference implementation for CPU inference)." % x.device)
        if x.dim() != 3 or x.shape[0] != self._s.batch or x.shape[1] != self._A:
            raise RuntimeError("expected input of shape [%d, %d, n], got %s" % (self._s.batch, self._A, tuple(x.shape)))
        if x.device != self.device:
            raise _lib.SrfError("input is on %s, the stream on %s" % (x.device, self.device))
        return x.detach().to(torch.float32)

    def _push_whole(self, x):
        """x: [batch, A, n], n a positive multiple of the granule -> the n delayed samples minus the negative-time head
        after a reset; run in pieces of at most max_chunk."""
        lib = _lib.load()
        n = x.shape[-1]
        pieces = []
        for lo in range(0, n, self._s.max_chunk):
            m = min(self._s.max_chunk, n - lo)
            xi = x[..., lo:lo + m].contiguous()
            oi = torch.empty((self._s.batch, self._SA, m), dtype=torch.float32, device=self.device)
            rc = lib.srf_stream_push(self._s.handle, _lib.ptr(self._weights), _lib.ptr(self._state), _lib.ptr(xi), m,
                                     _lib.ptr(oi), _lib.ptr(self._workspace), self._s.workspace_bytes, self._stream())
            _lib.check(rc, "srf_stream_push")
            pieces.append(oi)
        self._pos += n
        y = pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=-1)
        if self._head_pending:
            y = y[..., self._s.delay:]
            self._head_pending = False
        return y

    def push(self, x):
        """x: [batch, A, n] on the device, any n >= 0 -> [batch, S*A, m]: every sample that became final (m may be 0)."""
        x = self._check_input(x)
        with torch.cuda.device(self.device):
            if self._rem.shape[-1]:
                x = torch.cat([self._rem, x], dim=-1)
            n = x.shape[-1] // self._s.granule * self._s.granule
            self._rem = x[..., n:].clone()
            if n == 0:
                return torch.empty((self._s.batch, self._SA, 0), dtype=torch.float32, device=self.device)
            y = self._push_whole(x[..., :n]).contiguous()
            self._emitted += y.shape[-1]
            return y

    def finish(self):
        """End of every stream: zero-pad to the reference's padded length T', return the samples still owed so that
        cat(pushes + [finish()]) is the full forward's [batch, S*A, T]; the session is reset afterwards."""
        with torch.cuda.device(self.device):
            T = self._pos + self._rem.shape[-1]
            if T == 0:
                self.reset()
                return torch.empty((self._s.batch, self._SA, 0), dtype=torch.float32, device=self.device)
            u = self._pad_unit
            Tp = u if T < u else -(-T // u) * u
            outs = []
            if Tp > self._pos:
                pad = torch.zeros((self._s.batch, self._A, Tp - self._pos), dtype=torch.float32, device=self.device)
                pad[..., :self._rem.shape[-1]] = self._rem
                outs.append(self._push_whole(pad))
            tail = torch.empty((self._s.batch, self._SA, self._s.delay), dtype=torch.float32, device=self.device)
            _lib.check(_lib.load().srf_stream_flush(self._s.handle, _lib.ptr(self._state), _lib.ptr(tail), self._stream()),
                       "srf_stream_flush")
            outs.append(tail)
            y = torch.cat(outs, dim=-1)[..., :T - self._emitted].contiguous()
            self.reset()
            return y


class _PoolStream:
    """What CausalStream keeps per session, per stream of a pool."""

    def __init__(self, slot, rem):
        self.slot = slot
        self.rem = rem             # [A, r] on the device: samples that do not fill a granule yet
        self.pos = 0               # samples pushed through the kernels since open()
        self.emitted = 0           # samples returned since open()
        self.head_pending = True   # the next output still starts with `delay` negative-time samples


class CausalStreamPool:
    """Up to ``capacity`` streams of one CausalSuDORMRF that open, push and close independently: one ``push`` serves any
    subset of them, each with its own number of samples, in ONE pass of the kernels (srf_stream_push_rows), and every stream
    gets bit for bit what a ``CausalStream(batch=1)`` of its own would have returned.

    The weights are snapshot at construction (and by ``refresh_weights()``), as for ``CausalStream``."""

    def __init__(self, module, capacity, max_chunk=None, device=None):
        self._module = module
        _refuse_autograd("CausalSuDORMRF.stream_pool", list(module.parameters()))
        weights = _weights(module)
        device = torch.device(device) if device is not None else weights[0].device
        if device.type != "cuda":
            raise _lib.SrfError("sudo_rm_rf_amd runs on an MI355X only: the module is on %s.  There is deliberately no CPU "
                                "fallback (use the reference implementation for CPU inference)." % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self._cfg_tuple = module._config_tuple()
        self._s = _Session(self._cfg_tuple, capacity, max_chunk)
        self._A = module.in_audio_channels
        self._SA = module.num_sources * module.in_audio_channels
        self._pad_unit = module.n_least_samples_req
        # the documented state layout (include/sudormrf_hip.h): three sections, each padded to 64 floats
        h, Bt = self._s.delay, self._s.batch
        self._UD, self._C = module.num_blocks * module.upsampling_depth, module.in_channels
        a64 = lambda n: -(-n // 64) * 64
        self._off_dw = a64(Bt * self._A * 2 * h)
        self._off_tail = self._off_dw + a64(self._UD * Bt * self._C * 10)
        with torch.cuda.device(device):
            self._weights = _buffer(self._s.weights_bytes, device)
            self._state = _buffer(self._s.state_bytes, device)
            self._workspace = _buffer(self._s.workspace_bytes, device)
        self._streams = {}         # sid -> _PoolStream
        self._next_sid = 0
        self.refresh_weights()

    # -- geometry ----------------------------------------------------------------------------
    granule = property(lambda self: self._s.granule, doc="samples per granule g = h * 2^(D-1): pushes are cut at multiples of it")
    delay = property(lambda self: self._s.delay, doc="output delay h = enc_kernel_size // 2 samples")
    state_bytes = property(lambda self: self._s.state_bytes, doc="device bytes of state of all `capacity` streams")
    capacity = property(lambda self: self._s.batch, doc="the most streams that can be open at once")
    max_chunk = property(lambda self: self._s.max_chunk)
    active = property(lambda self: sorted(self._streams), doc="the open stream ids")

    def num_launches(self, m):
        """Kernel launches of one pass over m streams (srf_stream_push_rows_num_launches)."""
        return _lib.load().srf_stream_push_rows_num_launches(self._s.handle, int(m))

    def slot_of(self, sid):
        """The state slot (0 .. capacity - 1) stream `sid` occupies."""
        return self._get(sid).slot

    def _stream(self):
        return _lib.current_stream(self.device)

    def _get(self, sid):
        st = self._streams.get(sid)
        if st is None:
            raise _lib.SrfError("CausalStreamPool: stream %r is not open" % (sid,))
        return st

    def refresh_weights(self):
        """Snapshot the module's parameters again (srf_stream_prepare): skipinit_gain is read on the device."""
        _prepare_weights(self, "CausalStreamPool")

    def _sections(self, slot):
        """Views of one slot's encoder history [A, 2h], depthwise state [U*D, C, 10] and decoder tail [S*A, h+1]."""
        f = self._state.view(torch.float32)
        h, Bt, A, SA = self._s.delay, self._s.batch, self._A, self._SA
        hist = f[:Bt * A * 2 * h].view(Bt, A, 2 * h)[slot]
        dw = f[self._off_dw:self._off_dw + self._UD * Bt * self._C * 10].view(self._UD, Bt, self._C, 10)[:, slot]
        tail = f[self._off_tail:self._off_tail + Bt * SA * (h + 1)].view(Bt, SA, h + 1)[slot]
        return {"hist": hist, "dw": dw, "tail": tail}

    # -- life of a stream --------------------------------------------------------------------
    def open(self):
        """Start a stream in the lowest free slot (its state zeroed) and return its id.  No other stream is touched and no
        granule boundary is needed: nothing is shared between streams."""
        used = {st.slot for st in self._streams.values()}
        slot = next((i for i in range(self._s.batch) if i not in used), None)
        if slot is None:
            raise _lib.SrfError("CausalStreamPool: all %d streams are open" % self._s.batch)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().srf_stream_reset(self._s.handle, _lib.ptr(self._state), slot, self._stream()), "srf_stream_reset")
            rem = torch.empty((self._A, 0), dtype=torch.float32, device=self.device)
        sid = self._next_sid
        self._next_sid += 1
        self._streams[sid] = _PoolStream(slot, rem)
        return sid

    def _check_input(self, sid, x):
        if not isinstance(x, torch.Tensor):
            raise TypeError("input must be a torch.Tensor")
        _refuse_autograd("CausalStreamPool.push", [x])
        if x.device.type != "cuda":
            raise _lib.SrfError("sudo_rm_rf_amd runs on an MI355X only: input is on %s.  There is deliberately no CPU "
                                "fallback (use the reference implementation for CPU inference)." % x.device)
        if x.dim() != 2 or x.shape[0] != self._A:
            raise RuntimeError("stream %r: expected input of shape [%d, n], got %s" % (sid, self._A, tuple(x.shape)))
        if x.device != self.device:
            raise _lib.SrfError("input is on %s, the stream on %s" % (x.device, self.device))
        return x.detach().to(torch.float32)

    def _run(self, work):
        """work: [(_PoolStream, x [A, n])], n a positive multiple of the granule, distinct streams -> [y [S*A, n'] per
        entry]: the n delayed samples minus the negative-time head after open().  One srf_stream_push_rows per round of at
        most max_chunk samples per stream."""
        lib = _lib.load()
        mc, h, SA = self._s.max_chunk, self._s.delay, self._SA
        pieces = [[] for _ in work]
        lo = 0
        while True:
            todo = [(i, st, x[:, lo:lo + mc]) for i, (st, x) in enumerate(work) if x.shape[-1] > lo]
            if not todo:
                break
            rows = (_lib.srf_stream_row * len(todo))(*[(st.slot, xi.shape[-1]) for _, st, xi in todo])
            wav = torch.cat([xi.reshape(-1) for _, _, xi in todo])           # row j: a contiguous [A, n_j] block
            out = torch.empty(SA * (wav.numel() // self._A), dtype=torch.float32, device=self.device)
            rc = lib.srf_stream_push_rows(self._s.handle, _lib.ptr(self._weights), _lib.ptr(self._state), rows, len(todo),
                                          _lib.ptr(wav), _lib.ptr(out), _lib.ptr(self._workspace), self._s.workspace_bytes,
                                          self._stream())
            _lib.check(rc, "srf_stream_push_rows")
            o = 0
            for i, _, xi in todo:                                            # row j: a contiguous [S*A, n_j] block
                n = xi.shape[-1]
                pieces[i].append(out[o:o + SA * n].view(SA, n))
                o += SA * n
            lo += mc
        ys = []
        for (st, x), p in zip(work, pieces):
            st.pos += x.shape[-1]
            y = p[0] if len(p) == 1 else torch.cat(p, dim=-1)
            if st.head_pending:
                y = y[:, h:]
                st.head_pending = False
            ys.append(y)
        return ys

    def push(self, chunks):
        """chunks: {sid: x [A, n]} on the device, any n >= 0 per stream, any subset of the open streams -> {sid: y [S*A, m]}:
        every sample of that stream that became final (m may be 0: a stream without a whole granule is left out of the
        launch).  Streams that are not listed are not touched."""
        g = self._s.granule
        checked = [(sid, self._get(sid), self._check_input(sid, x)) for sid, x in chunks.items()]
        with torch.cuda.device(self.device):
            res, work, sids = {}, [], []
            for sid, st, x in checked:
                if st.rem.shape[-1]:
                    x = torch.cat([st.rem, x], dim=-1)
                n = x.shape[-1] // g * g
                st.rem = x[:, n:].clone()
                if n == 0:
                    res[sid] = torch.empty((self._SA, 0), dtype=torch.float32, device=self.device)
                else:
                    work.append((st, x[:, :n]))
                    sids.append(sid)
            for sid, (st, _), y in zip(sids, work, self._run(work) if work else []):
                res[sid] = y.contiguous()
                st.emitted += y.shape[-1]
            return {sid: res[sid] for sid in chunks}

    def close(self, sid):
        """End of stream `sid`: zero-pad it to the reference's padded length T', return the samples still owed so that
        cat(its pushes + [close(sid)]) is the full forward's [S*A, T] of its samples, and free its slot."""
        st = self._get(sid)
        with torch.cuda.device(self.device):
            T = st.pos + st.rem.shape[-1]
            if T == 0:
                del self._streams[sid]
                return torch.empty((self._SA, 0), dtype=torch.float32, device=self.device)
            u = self._pad_unit
            Tp = u if T < u else -(-T // u) * u
            outs = []
            if Tp > st.pos:
                pad = torch.zeros((self._A, Tp - st.pos), dtype=torch.float32, device=self.device)
                pad[:, :st.rem.shape[-1]] = st.rem
                outs += self._run([(st, pad)])
            tail = torch.empty((1, self._SA, self._s.delay), dtype=torch.float32, device=self.device)
            slots = (C.c_int * 1)(st.slot)
            _lib.check(_lib.load().srf_stream_flush_rows(self._s.handle, _lib.ptr(self._state), slots, 1, _lib.ptr(tail),
                                                         self._stream()), "srf_stream_flush_rows")
            outs.append(tail[0])
            y = torch.cat(outs, dim=-1)[:, :T - st.emitted].contiguous()
            del self._streams[sid]
            return y

    # -- moving a stream ---------------------------------------------------------------------
    def export_state(self, sid):
        """Everything stream `sid` is: clones of its three state sections, its remainder and its host-side counters.
        import_state() of it into an open stream of a pool of the same configuration continues the stream there."""
        st = self._get(sid)
        with torch.cuda.device(self.device):
            out = {k: v.clone() for k, v in self._sections(st.slot).items()}
            out.update(rem=st.rem.clone(), pos=st.pos, emitted=st.emitted, head_pending=st.head_pending, granule=self._s.granule)
        return out

    def import_state(self, sid, state):
        """Make the open stream `sid` the continuation of an exported one (its slot stays its own)."""
        st = self._get(sid)
        with torch.cuda.device(self.device):
            mine = self._sections(st.slot)
            for k, v in mine.items():
                if k not in state or tuple(state[k].shape) != tuple(v.shape):
                    raise _lib.SrfError("CausalStreamPool.import_state: section '%s' of shape %s does not fit this pool's %s (another "
                                        "model geometry)" % (k, tuple(state[k].shape) if k in state else None, tuple(v.shape)))
            if state["granule"] != self._s.granule or state["rem"].dim() != 2 or state["rem"].shape[0] != self._A or \
                    state["rem"].shape[1] >= self._s.granule or state["pos"] % self._s.granule:
                raise _lib.SrfError("CausalStreamPool.import_state: remainder / position do not fit this pool's granule %d"
                                    % self._s.granule)
            for k, v in mine.items():
                v.copy_(state[k])
            st.rem = state["rem"].to(self.device, torch.float32).clone()
            st.pos, st.emitted, st.head_pending = int(state["pos"]), int(state["emitted"]), bool(state["head_pending"])
