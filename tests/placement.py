"""Operand placement for the kernel tests: where a tensor lies in memory, and what lies around it.

A fresh ``torch.empty`` starts on a 256-byte boundary and is followed by allocator slack nobody looks at, so a suite
that only ever hands such tensors to the library cannot see (1) a kernel that assumes more alignment than a float's,
(2) a store before / after an output, (3) an output element that was never written, (4) a read of somebody else's
memory.  ``Arena`` makes all four visible:

* one byte buffer, filled with 0xFF before every case -- 0xFFFFFFFF is a NaN as fp32 / fp16 pair / bf16 pair and
  0xFFFFFFFFFFFFFFFF one as fp64, so whatever is read from outside a payload poisons a result;
* ``place`` / ``put`` carve contiguous payloads out of it, each ``shift_floats * 4`` bytes behind a 256-byte boundary
  and with at least ``guard_bytes(shape)`` of sentinel on either side;
* ``check`` asserts that every word outside the payloads is still the sentinel, ``unwritten`` counts the words of an
  output that still are;
* ``allocating(module)`` swaps a module's global ``torch`` for a proxy whose ``empty`` / ``empty_like`` / ``zeros`` /
  ``zeros_like`` come out of the arena, so the outputs and scratch the wrappers allocate are guarded as well
  (``zeros*`` are zeroed, ``empty*`` stay poisoned).

``PLACEMENT`` is the declared contract: per public callable of ``sudo_rm_rf_amd.ops`` (and the loss / metric /
augmentation / optimiser entry points that take caller tensors) and per pointer operand, what a base that is float
aligned but not 16-byte aligned must do.  tests/test_placement_host.py proves the checker and the table's completeness
on the CPU; tests/test_gpu_placement.py runs the table on the GPU.
"""
import contextlib
from collections import namedtuple

import torch

SENTINEL_BYTE = 0xFF
SENTINEL_WORD = -1          # 0xFFFFFFFF as int32

FALLBACK, REFUSES, NA = "FALLBACK", "REFUSES", "N/A"


def guard_bytes(shape, itemsize=4):
    """Guard on each side of a payload: two rows of its innermost length plus 256 floats (a condition, not a knob: a
    store one or two rows past the end still lands in a guard), rounded up to a multiple of 256 bytes."""
    inner = int(shape[-1]) if len(shape) else 1
    if itemsize == 1:           # a byte buffer (scratch, a packed image) has no rows: 64 KiB stands in for two of them
        inner = min(inner, 8192)
    need = 2 * inner * max(int(itemsize), 4) + 256 * 4
    return (need + 255) // 256 * 256


_Payload = namedtuple("_Payload", "name start end w0 w1 ptr shape")


class PlacementError(AssertionError):
    pass


class Arena:
    def __init__(self, device, nbytes):
        nbytes = (int(nbytes) + 255) // 256 * 256
        self.device = torch.device(device)
        self._raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._raw.data_ptr()) % 256
        self.bytes = self._raw[off:off + nbytes]          # starts on a 256-byte boundary
        self.words = self.bytes.view(torch.int32)
        self.nbytes = nbytes
        self.reset()

    # ---- layout -----------------------------------------------------------------------------------------------------
    def reset(self):
        self.bytes.fill_(SENTINEL_BYTE)
        self.payloads = []
        self._cursor = 0

    def place(self, shape, dtype=torch.float32, shift_floats=0, guard=0, name=None, zero=False):
        """A contiguous view of `shape`, 4 * shift_floats bytes behind a 256-byte boundary, sentinel all around."""
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        assert 0 <= shift_floats <= 3, shift_floats
        itemsize = torch.empty((), dtype=dtype).element_size()
        assert (4 * shift_floats) % itemsize == 0 or itemsize < 4, "a %s cannot start %d floats in" % (dtype, shift_floats)
        numel = 1
        for s in shape:
            numel *= s
        guard = max(int(guard), guard_bytes(shape, itemsize))
        start = (self._cursor + guard + 255) // 256 * 256 + 4 * shift_floats
        end = start + numel * itemsize
        if end + guard > self.nbytes:
            raise PlacementError("arena of %d bytes is too small for %s %s" % (self.nbytes, name, shape))
        self._cursor = end + guard
        view = self.bytes[start:end].view(dtype).view(shape)
        name = name or "operand%d" % len(self.payloads)
        self.payloads.append(_Payload(name, start, end, start // 4, (end + 3) // 4, view.data_ptr(), shape))
        if zero:
            view.zero_()
        return view

    def put(self, tensor, dtype=torch.float32, shift_floats=0, guard=0, name=None):
        """place() + a copy of a host (or device) tensor of any floating type."""
        view = self.place(tuple(tensor.shape), dtype, shift_floats, guard, name)
        view.copy_(tensor.to(dtype))
        return view

    # ---- checks -----------------------------------------------------------------------------------------------------
    def _payload_of(self, view):
        for p in self.payloads:
            if p.ptr == view.data_ptr() and p.end - p.start == view.numel() * view.element_size():
                return p
        raise PlacementError("tensor %s at %#x was not placed in this arena" % (tuple(view.shape), view.data_ptr()))

    def name_of(self, view):
        return self._payload_of(view).name

    def owns(self, view):
        lo = self.bytes.data_ptr()
        return lo <= view.data_ptr() < lo + self.nbytes

    def unwritten(self, view):
        """Number of 32-bit words of a payload that still hold the sentinel."""
        p = self._payload_of(view)
        assert p.start % 4 == 0 and p.end % 4 == 0, "unwritten() needs a payload of whole words"
        return int((self.words[p.w0:p.w1] == SENTINEL_WORD).sum().item())

    def check(self):
        """Every word outside the payloads still 0xFFFFFFFF, bit for bit; names the operand and the first / last offending
        byte offsets relative to the payload edge (negative: before its start; positive: past its end)."""
        w = self.words.clone()
        for p in self.payloads:
            w[p.w0:p.w1] = SENTINEL_WORD
        bad = (w != SENTINEL_WORD).nonzero().flatten()
        if bad.numel() == 0:
            return
        bad = bad.cpu().tolist()
        msgs = []
        edges = [0] + [p.w1 for p in self.payloads]
        for i, p in enumerate(self.payloads):
            nxt = self.payloads[i + 1].w0 if i + 1 < len(self.payloads) else self.nbytes // 4
            before = [b for b in bad if edges[i] <= b < p.w0]
            after = [b for b in bad if p.w1 <= b < nxt]
            # a word in the gap between two payloads is charged to the nearer edge
            if i + 1 < len(self.payloads):
                after = [b for b in after if b - p.w1 <= nxt - 1 - b]
            if i > 0:
                before = [b for b in before if p.w0 - 1 - b < b - edges[i]]
            if before:
                msgs.append("%d word(s) written BEFORE operand '%s' %s: byte offsets %d .. %d relative to its start"
                            % (len(before), p.name, p.shape, before[0] * 4 - p.start, before[-1] * 4 - p.start))
            if after:
                msgs.append("%d word(s) written AFTER operand '%s' %s: byte offsets +%d .. +%d past its end"
                            % (len(after), p.name, p.shape, after[0] * 4 - p.end, after[-1] * 4 - p.end))
        raise PlacementError("guard band damaged: " + "; ".join(msgs))

    def assert_written(self, view, what=None):
        n = self.unwritten(view)
        if n:
            raise PlacementError("operand '%s': %d of %d word(s) of the output were never written"
                                 % (what or self.name_of(view), n, view.numel() * view.element_size() // 4))

    def assert_untouched(self, view, what=None):
        """For refusals: the whole output still holds the sentinel."""
        p = self._payload_of(view)
        n = int((self.bytes[p.start:p.end] != SENTINEL_BYTE).sum().item())
        if n:
            raise PlacementError("operand '%s': %d byte(s) were written although the call was refused" % (what or p.name, n))

    def assert_clean(self, view, what=None):
        """No NaN in a floating output (a NaN = something read from outside a payload, or an unwritten element)."""
        n = int(torch.isnan(view).sum().item())
        if n:
            idx = torch.isnan(view).nonzero()[0].tolist()
            raise PlacementError("operand '%s': %d NaN value(s), first at index %s -- poison was read (an access outside "
                                 "an input) or the element was never written" % (what or self.name_of(view), n, idx))

    # ---- the wrappers' own allocations ------------------------------------------------------------------------------
    @contextlib.contextmanager
    def allocating(self, *modules, names=(), shifts=None):
        """Inside the block `module.torch` is a proxy whose empty / empty_like / zeros / zeros_like allocate from this
        arena; the n-th allocation is called names[n] (``alloc<n>`` beyond the list) and starts shifts.get(name, 0)
        floats behind a 256-byte boundary.  Yields the list of (name, view) in allocation order."""
        proxy = _TorchProxy(self, tuple(names), dict(shifts or {}))
        saved = [(m, m.torch) for m in modules]
        for m in modules:
            m.torch = proxy
        try:
            yield proxy.made
        finally:
            for m, t in saved:
                m.torch = t


class _Made(list):
    """(name, view) of every allocation, in order; .zeroed = the names that came from zeros / zeros_like."""

    def __init__(self):
        super().__init__()
        self.zeroed = set()


class _TorchProxy:
    """`torch` with the four allocating calls the wrappers use redirected into an Arena; everything else is torch's."""

    def __init__(self, arena, names, shifts):
        self._arena, self._names, self._shifts = arena, names, shifts
        self.made = _Made()

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device, zero):
        if device is not None and torch.device(device).type != self._arena.device.type:
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
        n = len(self.made)
        name = self._names[n] if n < len(self._names) else "alloc%d" % n
        itemsize = torch.empty((), dtype=dtype).element_size()
        shift = self._shifts.get(name, 0)
        if itemsize == 8 and shift:
            shift = 2                        # a double cannot start on an odd float: one double in
        view = self._arena.place(shape, dtype or torch.float32, shift % 4, name=name, zero=zero)
        self.made.append((name, view))
        if zero:
            self.made.zeroed.add(name)
        return view

    @staticmethod
    def _shape(size):
        if len(size) == 1 and not isinstance(size[0], int):
            return tuple(size[0])
        return tuple(size)

    def empty(self, *size, dtype=torch.float32, device=None):
        return self._alloc(self._shape(size), dtype, device, False)

    def zeros(self, *size, dtype=torch.float32, device=None):
        return self._alloc(self._shape(size), dtype, device, True)

    def empty_like(self, t):
        return self._alloc(tuple(t.shape), t.dtype, t.device, False)

    def zeros_like(self, t):
        return self._alloc(tuple(t.shape), t.dtype, t.device, True)


# =====================================================================================================================
# The declared placement contract.
#
# PLACEMENT[entry] = {"allocs": names of the tensors the wrapper allocates itself, in allocation order (outputs and
#                               scratch: they are operands of the C entry point like any other),
#                     "operands": {operand: (kind, note)}}
# kind, for a base that is float aligned (fp64 statistics: double aligned) but NOT 16-byte aligned:
#   FALLBACK  the result is correct.  note = the kernel family the trace must then show (a prefix; a tuple = either), or SAME when the host
#             code runs the same launch either way (scalar accesses only, or a run-time flag / an under-aligned vector type
#             inside one kernel: the note then says which).
#   REFUSES   _lib.SrfError before anything is launched; its text names the operand (note = the name it uses).
#   NA        not a device pointer.
# Read off the host code of every entry point (csrc/*.hip: the srf_aligned16 predicates and SRF_CHECK_ALIGNED16), see
# include/sudormrf_hip.h "Operand placement".  A list-valued operand (levels, weights, params ...) stands for each member.
# =====================================================================================================================
SAME = "same launch"
_S = (FALLBACK, SAME)
_SUMS_IN = (REFUSES, "sums")          # GlobLN statistics are read as pairs of doubles (srf_finalize_stats)
_SUMS_OUT = (FALLBACK, SAME)          # ... and accumulated one double at a time


def _e(allocs, **operands):
    return {"allocs": tuple(allocs), "operands": operands}


_PRO = dict(in_sums=_SUMS_IN, in_gamma=_S, in_beta=_S, in_prelu=_S)
_PAIR = dict(x=(REFUSES, "'x'"), bias1=_S, residual=(REFUSES, "'residual'"), bias2=_S, y=(REFUSES, "'y'"),
             y2=(REFUSES, "'y2'"), **_PRO)

PLACEMENT = {
    "encoder": _e(("out",), wav=_S, weight=_S, sums=_SUMS_OUT, out=_S),
    "gln_stats": _e(("sums",), x=_S, sums=_SUMS_OUT),
    "gln_apply": _e(("y",), x=_S, sums=_SUMS_IN, gamma=_S, beta=_S, prelu=_S, residual=_S, y=_S),
    "glob_ln": _e(("sums", "y"), x=_S, gamma=_S, beta=_S, sums=(NA, "allocated 256-byte aligned by the wrapper"), y=_S),
    "pack_pw_weight": _e(("packed",), weight=_S, packed=(REFUSES, "'packed'")),
    "pack3_pw_weight": _e(("packed",), weight=_S, packed=(REFUSES, "'packed'")),
    # srf_pw_conv_packed: x / weight / y / residual / mask_mul off the grid -> the scalar kernel; an unaligned packed
    # image -> the kernels that split the fp32 weight themselves
    "pw_conv": _e(("y",), x=(FALLBACK, "pw_conv_generic"), weight=(FALLBACK, ("pw_conv_generic", "pw_conv_x3w")), bias=_S,
                  residual=(FALLBACK, "pw_conv_generic"), out_sums=_SUMS_OUT, mask_mul=(FALLBACK, "pw_conv_generic"),
                  packed=(FALLBACK, "pw_conv_bf16x3"), y=(FALLBACK, "pw_conv_generic"), **_PRO),
    # (the three-part kernel reads the packed image only: an fp32 weight off the grid changes nothing where it serves)
    "pw_conv3": _e(("y",), x=(FALLBACK, "pw_conv_generic"), weight=(FALLBACK, ("pw_conv_generic", "pw_conv_x3w")),
                   packed3=(FALLBACK, "pw_conv_bf16x3"), bias=_S, residual=(FALLBACK, "pw_conv_generic"),
                   out_sums=_SUMS_OUT, y=(FALLBACK, "pw_conv_generic"), **_PRO),
    "pw_conv_pair": _e(("y", "y2"), packed1=(REFUSES, "'w1_packed'"), packed2=(REFUSES, "'w2_packed'"),
                       out_sums2=_SUMS_OUT, **_PAIR),
    "pw_conv_pair3": _e(("y", "y2"), packed3_1=(REFUSES, "'w1_packed3'"), packed3_2=(REFUSES, "'w2_packed3'"),
                        out_sums2=_SUMS_OUT, **_PAIR),
    "dwconv5": _e(("y",), x=(FALLBACK, "dwconv5_generic"), weight=_S, bias=_S, out_sums=_SUMS_OUT,
                  y=(FALLBACK, "dwconv5_generic"), **_PRO),
    "conv1d": _e(("y",), x=_S, weight=_S, bias=_S, out_sums=_SUMS_OUT, y=_S),
    "merge": _e(("y",), levels=(FALLBACK, "merge_generic"), sums=_SUMS_IN, gammas=_S, betas=_S, out_sums=_SUMS_OUT,
                y=(FALLBACK, "merge_generic")),
    "pyramid": _e(("merged", "scratch"), y1=(REFUSES, "'y1'"), weights=_S, biases=_S, gammas=_S, betas=_S,
                  out_sums=_SUMS_OUT, merged=(REFUSES, "'merged'"), scratch=(REFUSES, "'scratch'"), **_PRO),
    # the frame GEMM is srf_pw_conv on v (-> its scalar kernel); the overlap-add stores through an under-aligned vector type
    "decoder": _e(("scratch", "out"), v=(FALLBACK, "pw_conv_generic"), weight=_S, scratch=(REFUSES, "'scratch'"), out=_S),
    # n = 16, G = 16: the MFMA form moves x / q as 16-byte buffer rows -> the VALU kernel "tac"; its weight loads test the
    # address themselves (srf_tac.hip: two float4 or eight floats)
    "tac": _e(("q",), x4=(FALLBACK, "tac"), params=_S, out_sums=_SUMS_OUT, q=(FALLBACK, "tac")),
    "mixture_consistency": _e(("out", "work"), pr_batch=_S, input_mixture=_S, out=_S, work=_S),
    # dw / scratch off the grid: the scalar instance of the partial-sum fold (same family name pw_wgrad_reduce)
    "pw_wgrad": _e(("dw", "dbias", "scratch"), g=(REFUSES, "'g'"), x=(REFUSES, "'x'"), dw=(FALLBACK, "pw_wgrad_reduce"),
                   dbias=_S, scratch=(FALLBACK, "pw_wgrad_reduce"), **_PRO),
    # gout / gout2 / x / gx off the grid: the scalar reduce / apply kernels (same family names)
    "gln_bwd": _e(("gx", "dgamma", "dbeta", "dslope", "scratch"), gout=(FALLBACK, "gln_bwd_reduce"),
                  x=(FALLBACK, "gln_bwd_reduce"), sums=_SUMS_IN, gamma=_S, beta=_S, prelu=_S,
                  gout2=(FALLBACK, "gln_bwd_reduce"), gx=(FALLBACK, "gln_bwd_apply"), dgamma=_S, dbeta=_S, dslope=_S,
                  scratch=(REFUSES, "'scratch'")),
    # off the grid: the chain of pair-sum launches instead of the one-pass kernel (same family name)
    "merge_bwd": _e(("levels",), g_merged=(FALLBACK, "merge_bwd"), levels=(FALLBACK, "merge_bwd")),
    "dwconv5_bwd": _e(("gin", "dw", "dbias", "scratch"), gd=(FALLBACK, "dwconv5_bwd"), xin=(FALLBACK, "dwconv5_bwd"),
                      weight=_S, dw=_S, dbias=_S, gin=(FALLBACK, "dwconv5_bwd"), scratch=_S, **_PRO),
    "mask_apply": _e(("v",), m=_S, enc=_S, v=_S),
    "mask_bwd": _e(("genc", "gm"), gv=_S, m=_S, enc=_S, genc=_S, gm=_S),
    # one kernel, run-time flag `vec` (n % 4 == 0 and gout, x, gx on the grid)
    "prelu_bwd": _e(("gx", "dslope"), gout=(FALLBACK, "prelu_bwd"), x=(FALLBACK, "prelu_bwd"), slope=_S, dslope=_S,
                    gx=(FALLBACK, "prelu_bwd")),
    "frames_gather": _e(("out",), src=_S, out=_S),
    # x and the scratch slices feed srf_pw_wgrad, go / gx move as 16-byte rows in the MFMA kernel
    "tac_bwd": _e(("grads", "gx", "scratch"), x=(REFUSES, "'x'"), go=(REFUSES, "'go'"), params=_S, grads=_S,
                  gx=(REFUSES, "'gx'"), scratch=(REFUSES, "'scratch'")),
    "wav_normalize": _e(("out", "stats"), wav=_S, out=_S, stats=_S),
    "wav_denormalize": _e(("out",), est=_S, stats=_S, mix_norm=_S, out=_S),
    "causal_encoder": _e(("out",), wav=_S, weight=_S, out=_S),
    "causal_dwconv": _e(("y",), x=_S, weight=_S, bias=_S, in_prelu=_S, out_prelu=_S, y=_S),
    "causal_merge": _e(("y",), levels=_S, y=_S),
    # one kernel, run-time flag a.vec (L % 4 == 0 and y1 on the grid): quad loads or scalar loads of y1
    "causal_pyramid": _e(("merged",), y1=(FALLBACK, "causal_pyramid"), in_prelu=_S, weights=_S, biases=_S, prelus=_S,
                         merged=_S),
    "causal_stream_pyramid": _e(("merged",), y1=_S, state=_S, in_prelu=_S, weights=_S, biases=_S, prelus=_S, merged=_S),
    "causal_scale": _e(("dst",), src=_S, dscale=_S, dst=_S),
    "prelu": _e(("y",), x=_S, slope=_S, y=_S),
    # ---- beyond ops: the loss / metric / augmentation / optimiser entry points that take caller tensors --------------
    # rows are read with 16-byte loads only when T % 4 == 0 AND the bases are on the grid (srf_loss_fuss.hip `vec`)
    "losses.snr.zeroref_snr": _e((), est=(FALLBACK, "zeroref_snr"), tgt=(FALLBACK, "zeroref_snr"),
                                 grad_est=(FALLBACK, "zeroref_snr")),
    "losses.sisdr.stab_sisdr": _e((), pr=(FALLBACK, "stab_sisdr"), tgt=(FALLBACK, "stab_sisdr")),
    "losses.sisdr.pit_sisdr": _e((), est=_S, tgt=_S),
    "losses.sisdr.perm_inv_sisdr": _e((), pr=_S, tgt=_S, mix=_S),
    "augment.fuss_augment": _e((), clean=(FALLBACK, "fuss_augment"), out=(FALLBACK, "fuss_augment"),
                               mix=(FALLBACK, "fuss_augment")),
    "augment.online_remix": _e((), clean=_S, out=_S, mix=_S),
    # parameters / gradients / moments are addressed element by element through the tensor table
    "optim.FusedClipAdam": _e((), p=_S, g=_S, m=_S, v=_S),
}

# public names of ops that take no caller tensors
EXCLUDED = {
    "set_debug_flags": "a process-wide switch, no tensor",
    "DebugFlag": "the names of that switch's bits, no tensor",
    "debug_flags": "that switch as a context manager, no tensor",
    "set_kernel_mode": "a process-wide switch, no tensor",
    "get_kernel_mode": "a query, no tensor",
    "kernel_trace": "the in-library profiler's context manager, no tensor",
    "new_sums": "allocates a zeroed statistics tensor, calls no kernel",
    "pw_conv_pair_supported": "a shape query, no tensor",
    "pw_conv_pair3_supported": "a shape query, no tensor",
    "causal_pyramid_supported": "a shape query, no tensor",
}


def public_ops():
    """The public callables sudo_rm_rf_amd.ops defines itself, by introspection."""
    import inspect

    from sudo_rm_rf_amd import ops
    return {n for n, o in vars(ops).items()
            if not n.startswith("_") and (inspect.isfunction(o) or inspect.isclass(o)) and o.__module__ == ops.__name__}


@contextlib.contextmanager
def poisoned_allocations(*modules):
    """Inside the block every tensor `module.torch.empty` / `empty_like` hands out is filled with 0xFF first (the caching
    allocator would otherwise return blocks that still hold an earlier, correct answer); zeros* are torch's."""
    class _Poison:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def _fill(t):
            if t.numel():
                t.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
            return t

        def empty(self, *a, **kw):
            t = torch.empty(*a, **kw)
            return t if kw.get("pin_memory") or t.device.type == "cpu" else self._fill(t)

        def empty_like(self, *a, **kw):
            return self._fill(torch.empty_like(*a, **kw))
    proxy = _Poison()
    saved = [(m, m.torch) for m in modules]
    for m in modules:
        m.torch = proxy
    try:
        yield
    finally:
        for m, t in saved:
            m.torch = t
