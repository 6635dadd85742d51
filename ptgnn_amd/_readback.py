"""Device integers looked at on the host WITHOUT stalling the stream, and the back-offs driven by them.

A few launches decide something from numbers that exist on the device only (row counts, a hub count, a bad-id count,
halo sizes).  `Readback` copies them into a pooled host buffer behind the producing kernels and lets the host look later;
`Backoff` is the "skip the next N decisions" counter two of those looks drive; `take_arrived` polls a list of pending
looks.  Two Python threads on this path are a real configuration (threaded minibatch iterators), so the pool, the pending
lists and the counters are all guarded by ONE lock -- which is never held across a HIP call or an event synchronise:
every critical section is list and dict work on host memory.
"""
import threading
from typing import List, Optional

import torch

LOCK = threading.Lock()
_POOL = {}      # (dtype, elements, pinned) -> host buffers not in flight (pinning host memory costs far more than the kernels)


def _allocate(dtype, n: int, pinned: bool) -> torch.Tensor:
    t = torch.empty(n, dtype=dtype)
    return t.pin_memory() if pinned else t


class Readback:
    """The values of a small integer tensor, on their way to the host.  A device tensor is copied asynchronously into a
    pooled pinned buffer and an event is recorded behind the copy on the current stream of the tensor's device; a CPU
    tensor is ready at once (`event` lets a caller that has one of its own, or a test, say when).  `tag`: what the
    values are about, for whoever takes the read-back off a pending list."""
    __slots__ = ("_host", "_event", "_values", "_key", "tag")

    def __init__(self, values: torch.Tensor, event=None, tag=None):
        self._values, self.tag = None, tag
        self._key = key = (values.dtype, values.numel(), values.is_cuda)
        with LOCK:
            free = _POOL.get(key)
            self._host = free.pop() if free else None
        if self._host is None:
            self._host = _allocate(*key)        # pinning is a HIP call: outside the lock
        if values.is_cuda:
            with torch.cuda.device(values.device):      # the copy and its event belong to the stream of the tensor's device
                self._host.copy_(values, non_blocking=True)
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(values.device))
        else:
            self._host.copy_(values)
        self._event = event

    def ready(self) -> bool:
        """Whether the values are on the host.  Never blocks."""
        ev = self._event
        if ev is not None and ev.query():
            self._event = ev = None             # asked once: later looks cost no HIP call
        return ev is None

    def values(self, wait: bool = False) -> Optional[List[int]]:
        """The values as Python ints once they have arrived, None before.  `wait` blocks on the read-back's own event --
        not on the stream: work enqueued behind it keeps running.  The buffer goes back to the pool exactly once,
        however many callers (or threads) ask."""
        if self._values is None:
            if wait:
                ev = self._event
                if ev is not None:
                    ev.synchronize()
            elif not self.ready():
                return None
            with LOCK:
                if self._values is None:
                    self._values = self._host.tolist()
                    _POOL.setdefault(self._key, []).append(self._host)
                    self._host = self._event = None
        return self._values


class Backoff:
    """"Skip the next N decisions": tripped by a look that came back unfavourable, consumed one decision at a time."""
    __slots__ = ("steps",)

    def __init__(self):
        self.steps = 0

    def trip(self, n: int) -> None:
        with LOCK:
            self.steps = int(n)

    def consume(self) -> bool:
        """One decision: True = skip it (one step fewer is left); False once the back-off has run out."""
        with LOCK:
            if self.steps > 0:
                self.steps -= 1
                return True
            return False


def take_arrived(pending: List[Readback], keep: int) -> List[Readback]:
    """Remove from `pending` the read-backs that have arrived and return them -- each to ONE caller, whichever thread
    asks -- then forget all but the newest `keep` of those still in flight.  The events are queried outside the lock."""
    with LOCK:
        snapshot = list(pending)
    done = []
    for item in snapshot:
        ev = item._event            # Readback.ready() spelled out: the loop runs over up to 24 entries per layer call, and
        if ev is None or ev.query():     # a Python call per entry cost the small-minibatch benchmark 1 to 2 us a call
            item._event = None
            done.append(item)
    if not done and len(snapshot) <= keep:      # the usual call: nothing to take, nothing to forget
        return done
    with LOCK:
        mine = [item for item in done if item in pending]       # another thread may have taken some meanwhile
        pending[:] = [p for p in pending if p not in mine][-keep:]
    return mine
