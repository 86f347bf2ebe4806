"""Stream, event and scratch protocol of one training step on one MI355X: the device workspaces, the process-wide HIP
streams, the cross-stream hand-over events, the parity ring of scratch sets a side stream may still be reading, and the
arenas of small accumulators that start every pass at zero.  StepSchedule owns the order in which work may touch memory and
nothing else: it knows no model, no parameter and no kernel; whoever derives from it says what runs."""
import math
from typing import Dict

import torch

_STREAMS = {}


def shared_stream(dev, kind, high=False):
    """One HIP stream per (device, role) for the whole process.  HIP maps streams onto a small pool of hardware queues
    (GPU_MAX_HW_QUEUES, 4 by default) round-robin: a process that builds a second engine / trainer with streams of its own
    gets a main and a side stream on the SAME hardware queue sooner or later and the two-stream schedule silently runs as
    one (bench.py's configs[3] leg, the third trainer of its process: 84 ms per step instead of 66)."""
    idx = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    key = (idx, kind)
    if key not in _STREAMS:
        pr = torch.cuda.Stream.priority_range()[1] if high else 0
        _STREAMS[key] = torch.cuda.Stream(device=dev, priority=pr)
    return _STREAMS[key]


class _FastEvent:
    """Cross-stream hand-over event created with hipEventDisableTiming | hipEventDisableSystemFence: the marker packet of
    a default-flag event costs the queue it is recorded on ~7.3 us between two kernels, this one ~5.2 (tools/event_cost.py,
    rocprofv3 kernel trace); the engine records ~110 of them per step on the main stream.  Same interface as the two methods
    of torch.cuda.Event the engine uses (torch's own events are the fallback when libamdhip64.so cannot be loaded by that name)."""
    _hip = None
    _pools = {}        # device -> [events, next]: an event belongs to the device that was current when it was created

    @classmethod
    def create(cls):
        """A fresh event that belongs to its caller (never handed out again)."""
        import ctypes
        if cls._hip is None:
            cls._hip = ctypes.CDLL("libamdhip64.so")
        h = ctypes.c_void_p()
        if cls._hip.hipEventCreateWithFlags(ctypes.byref(h), ctypes.c_uint(0x2 | 0x20000000)) != 0:
            raise RuntimeError("hipEventCreateWithFlags failed")
        e = cls.__new__(cls)
        e.h = h
        return e

    @classmethod
    def get(cls):
        """An event from the per-device ring, for hand-overs that are recorded and waited for back to back (a wait captures
        the record that precedes it, so re-recording a ring event later is safe).  Anything a holder keeps across other
        hand-overs must NOT come from here (StepSchedule._owned_event): 1024 later get() calls would re-record it."""
        pool = cls._pools.setdefault(torch.cuda.current_device(), [[], 0])
        if len(pool[0]) < 1024:
            e = cls.create()
            pool[0].append(e)
            return e
        pool[1] = (pool[1] + 1) % len(pool[0])
        return pool[0][pool[1]]

    def record(self, stream=None):
        import ctypes
        st = stream if stream is not None else torch.cuda.current_stream()
        if self._hip.hipEventRecord(self.h, ctypes.c_void_p(st.cuda_stream)) != 0:
            raise RuntimeError("hipEventRecord failed")

    def wait_on(self, stream):
        import ctypes
        if self._hip.hipStreamWaitEvent(ctypes.c_void_p(stream.cuda_stream), self.h, 0) != 0:
            raise RuntimeError("hipStreamWaitEvent failed")


class _TorchEvent:
    def __init__(self):
        self.e = torch.cuda.Event()

    def record(self, stream=None):
        self.e.record(stream) if stream is not None else self.e.record()

    def wait_on(self, stream):
        stream.wait_event(self.e)


def _new_event(owned=False):
    global _FAST_EVENTS
    if _FAST_EVENTS:
        try:
            return _FastEvent.create() if owned else _FastEvent.get()
        except (OSError, RuntimeError):          # no libamdhip64 by that name: torch's events do the same job
            _FAST_EVENTS = False
    return _TorchEvent()


_FAST_EVENTS = True


class Workspace:
    """Named device buffers, allocated on first use and reused every step (static shapes)."""

    def __init__(self, device):
        self.device = device
        self.bufs: Dict[tuple, torch.Tensor] = {}

    def get(self, name, shape, dtype=torch.float32, zero=False, zero_once=False):
        """zero: cleared on every call; zero_once: cleared when allocated only (buffers with entries nobody writes)."""
        key = (name, tuple(shape), dtype)
        t = self.bufs.get(key)
        if t is None:
            t = (torch.zeros if (zero or zero_once) else torch.empty)(tuple(shape), dtype=dtype, device=self.device)
            self.bufs[key] = t
        elif zero:
            t.zero_()
        return t

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.bufs.values())


class _RowWorkspace(Workspace):
    """Workspace whose buffers keep their storage across sequence lengths: one grow-only allocation per (name, dtype),
    viewed at the requested shape (the engine's Workspace would keep one buffer set per distinct length)."""

    def __init__(self, device):
        super().__init__(device)
        self.shapes = {}

    def get(self, name, shape, dtype=torch.float32, zero=False, zero_once=False):
        shape = tuple(shape)
        n, key = math.prod(shape), (name, dtype)
        t = self.bufs.get(key)
        if t is None or t.numel() < n:
            t = torch.zeros(max(n, 1), dtype=dtype, device=self.device)
            self.bufs[key] = t
            self.shapes.pop(key, None)
        v = t[:n].view(shape)
        if zero or (zero_once and self.shapes.get(key) != shape):
            v.zero_()
        self.shapes[key] = shape
        return v


class _Arena:
    """Small accumulators (BatchNorm sums, rel-pos projection gradient) that must start every pass at zero.  Instead of ~45
    tiny fill launches per step they live in one buffer that is cleared with ONE fill at the start of forward or of backward;
    a slot keeps its offset for the lifetime of the schedule."""

    def __init__(self, dtype, device):
        self.dtype, self.device, self.buf, self.used, self.slots = dtype, device, None, 0, {}

    def slot(self, name, numel):
        if name not in self.slots:
            self.slots[name] = (self.used, numel)
            self.used += (numel + 63) // 64 * 64
            if self.buf is None or self.used > self.buf.numel():   # grow (first step only): re-create and clear
                self.buf = torch.zeros(max(2 * self.used, 1 << 16), dtype=self.dtype, device=self.device)
        o, n = self.slots[name]
        return self.buf[o:o + n]

    def clear(self):
        if self.buf is not None and self.used:
            self.buf[:self.used].zero_()


class StepSchedule:
    def __init__(self, dev, side_stream=True, side2=True, depth=48):
        """Weight-gradient GEMMs feed nothing until the optimizer, so the backward schedule launches them on a second HIP
        stream: they fill the partially empty last round of the data-gradient GEMMs' grids and overlap the HBM-bound row
        kernels (LayerNorm / softmax backward).  Scratch tensors they read are buffered `depth` deep by sub-layer parity.
        `side` / `side2` are read at every call: side = None on a live schedule makes the next step a one-stream one."""
        self.dev = dev
        self.ws = Workspace(dev)
        self.side = self.side2 = None
        if dev.type == "cuda" and side_stream:
            self.side = shared_stream(dev, "side")
            # results the main stream waits for inside the sub-layer (dV, dK of the attention backward) get a stream of their own:
            # queued behind the weight gradients they would hand the main stream the whole backlog to wait for
            self.side2 = shared_stream(dev, "side2", high=True) if side2 else self.side
        self._owned = {}       # events a holder keeps across other hand-overs: one per role, owned by this schedule
        self._par = 0
        self._depth = depth    # scratch sets the main stream may run ahead by
        self._side_ev = [None] * depth
        self._arena = {k: _Arena(dt, dev) for k, dt in
                       (("fwd64", torch.float64), ("bwd64", torch.float64), ("bwd32", torch.float32))}

    def _arena_slot(self, kind, name, numel):
        return self._arena[kind].slot(name, numel)

    def _arena_clear(self, kind):
        self._arena[kind].clear()

    def _t(self, name):
        """Scratch tensor name for the current sub-layer parity (tensors a side-stream GEMM reads)."""
        return f"{name}.{self._par}"

    def _sub_begin(self):
        """Start of a sub-layer backward: flip the parity; its scratch set was last read by the side-stream work
        issued `depth` sub-layers ago, which must have drained before the main stream overwrites it."""
        self._par = (self._par + 1) % self._depth
        ev = self._side_ev[self._par]
        if ev is not None:
            ev.wait_on(torch.cuda.current_stream())
            self._side_ev[self._par] = None

    def _owned_event(self, key):
        """The schedule's own event for one long-lived role (scratch-set slot, weight casts, positional projections): held from
        its record to a wait that may come a whole backward later, so it cannot be a ring event (_FastEvent.get)."""
        ev = self._owned.get(key)
        if ev is None:
            ev = self._owned[key] = _new_event(owned=True)
        return ev

    def _sub_end(self):
        if self.side is not None:
            ev = self._owned_event(("slot", self._par))
            ev.record(self.side)
            self._side_ev[self._par] = ev

    def _side(self, fn, want_event=False, urgent=False):
        """Run fn (work whose inputs are complete on the main stream NOW) on the side stream; with want_event the
        returned event marks its completion (for results the main stream consumes later).  urgent: the main stream joins
        this work before the sub-layer ends -- it goes to the second side stream, in front of no backlog."""
        if self.side is None:
            fn()
            return None
        ev = _new_event()
        ev.record()
        st = self.side2 if urgent else self.side
        with torch.cuda.stream(st):
            ev.wait_on(st)
            fn()
            if want_event:     # True: waited for inside the same sub-layer (ring event); a key: kept by the caller (owned event)
                done = _new_event() if want_event is True else self._owned_event(("side", want_event))
                done.record()
                return done
        return None

    def _wg_flush(self):
        """Hook: hand over what the derived class has collected for the side stream (called before every join)."""

    def join_side(self):
        """Make the current stream wait for every weight gradient issued so far (for on_group_done hooks that read gradients)."""
        self._wg_flush()
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)
            if self.side2 is not self.side:
                torch.cuda.current_stream().wait_stream(self.side2)
            self._side_ev = [None] * self._depth
