"""Python host wrappers over the C ABI (include/ptgnn_amd.h).

torch is plumbing here: it owns device memory (outputs/workspaces are torch tensors so the caching
allocator and stream semantics are preserved) and supplies the current HIP stream.  All compute
happens in libptgnn_amd.so; there is no eager fallback.
"""
import ctypes
import os
import weakref
from typing import List, Optional, Sequence, Tuple

import torch

from ptgnn_amd import _lib
from ptgnn_amd._readback import LOCK, Backoff, Readback, take_arrived

REDUCE_IDS = {"sum": 0, "add": 0, "mean": 1, "max": 2, "min": 3}
EPI_NONE, EPI_GELU, EPI_LAYERNORM, EPI_GELU_LAYERNORM = 0, 1, 2, 3
ACT_IDS = {None: 0, "none": 0, "tanh": 1, "relu": 2}


GEMM_MODES = {"tile": 0, "stream": 1}


def set_gemm_mode(mode) -> int:
    """Kernel family of the dense blocks (ptgnn_amd_set_gemm_mode): "tile" = round-1 128x128 tile kernels, "stream" =
    weight-stationary streaming kernels; both exact fp32 MFMA with the same bits.  Returns the previous mode id.
    (The opt-in 3 x bf16 split arithmetic of rounds 2-4 was removed in round 5.)"""
    lib = _lib.load()
    prev = lib.ptgnn_amd_get_gemm_mode()
    if isinstance(mode, str) and mode not in GEMM_MODES:
        raise _lib.PtgnnAmdError(f"unknown GEMM mode {mode!r} (have {sorted(GEMM_MODES)}; the split mode was removed)")
    _lib.check(lib.ptgnn_amd_set_gemm_mode(int(GEMM_MODES.get(mode, mode))), "ptgnn_amd_set_gemm_mode")
    return prev


def get_gemm_mode() -> int:
    return _lib.load().ptgnn_amd_get_gemm_mode()


_AGG_FAMILY_FIRST = 64   # PTGNN_AMD_KERNEL_AGG_FIRST_: the aggregation families' id range (include/ptgnn_amd.h)


_CHAR_FAMILY_FIRST = 128  # PTGNN_AMD_KERNEL_CHAR_FIRST_: the char-CNN kernels' id range


_HEAD_FAMILY_FIRST = 192  # PTGNN_AMD_KERNEL_HEAD_FIRST_: the task heads' id range


_SEQ_FAMILY_FIRST = 256  # PTGNN_AMD_KERNEL_SEQ_FIRST_: the copying decoder's loss kernels


_DECODE_FAMILY_FIRST = 320  # PTGNN_AMD_KERNEL_DECODE_FIRST_: the copying decoder's greedy-decoding step


_BEAM_FAMILY_FIRST = 384  # PTGNN_AMD_KERNEL_BEAM_FIRST_: the copying decoder's beam-search step


_HALF_FAMILY_FIRST = 448  # PTGNN_AMD_KERNEL_HALF_FIRST_: the opt-in 16-bit-input dense blocks


_EDGE16_FAMILY_FIRST = 512  # PTGNN_AMD_KERNEL_EDGE16_FIRST_: the opt-in 16-bit-input grouped per-edge GEMM


_HALF_TRAIN_FAMILY_FIRST = 576  # PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_: the opt-in 16-bit-input training launches


_EDGE16_DST_FAMILY_FIRST = 640  # PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_: the 16-bit per-edge GEMM with a target-state half


_BEAM_FINISH_FAMILY_FIRST = 704  # PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_: the beam search's finishing route


_ATTENTION16_FAMILY_FIRST = 768  # PTGNN_AMD_KERNEL_ATTENTION16_FIRST_: the opt-in 16-bit-input block attention


_EDGE16_TRAIN_FAMILY_FIRST = 832  # PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_: the 16-bit-input edge-form training launches


def launch_counts(aggregation: bool = False, char_cnn: bool = False, heads: bool = False,
                  sequence: bool = False, decode: bool = False, beam: bool = False, half: bool = False,
                  edge16: bool = False, half_training: bool = False, edge16_dst: bool = False,
                  beam_finish: bool = False, attention16: bool = False, edge16_training: bool = False) -> dict:
    """{kernel family: launches made by this process} (ptgnn_amd_launch_count): tests take differences around a call
    to assert which kernel a shape / size / mode was dispatched to.  `aggregation=True` adds the aggregation families
    (k_gather_reduce, egc_gather_combine, egc_combine, egc_combine_backward, pna_aggregate, pna_aggregate_backward,
    attention_pool, attention_pool_backward, head_projection, graph_norm, graph_norm_backward, block_attention,
    block_attention_backward, segment_scores, segment_scores_backward, embedding_bag, embedding_bag_backward);
    `char_cnn=True` adds the char-CNN embedder's (char_embed, char_embed_backward, window_max, window_max_backward);
    `heads=True` the task heads' (logit_loss, logit_loss_backward, candidate_scores, candidate_scores_backward);
    `sequence=True` the copying decoder's loss kernels (vocab_loss, vocab_loss_backward, copy_loss_finish);
    `decode=True` its greedy-decoding step (decode_step); `beam=True` its beam-search step (beam_step);
    `half=True` the 16-bit-input dense blocks (half_linear, half_gru); `edge16=True` the 16-bit-input grouped per-edge
    GEMM's two launch forms (edge16, edge16_shared); `half_training=True` the 16-bit-input training launches
    (half_wgrad, half_gru_train, half_linear_add); `edge16_dst=True` the 16-bit-input per-edge GEMM with a target-state
    half (edge16_dst: the MLP-MP message Linear); `beam_finish=True` the beam search's finishing route (beam_step_links,
    beam_backtrack); `attention16=True` the 16-bit-input block attention (block_attention16); `edge16_training=True`
    the 16-bit-input edge-form training launches (edge16_masked: the masked per-edge GEMM in its forward and
    input-gradient modes; edge_wgrad16: the per-type weight gradient)."""
    lib = _lib.load()
    out = {}
    for first in (0,) + ((_AGG_FAMILY_FIRST,) if aggregation else ()) + ((_CHAR_FAMILY_FIRST,) if char_cnn else ()) \
            + ((_HEAD_FAMILY_FIRST,) if heads else ()) + ((_SEQ_FAMILY_FIRST,) if sequence else ()) \
            + ((_DECODE_FAMILY_FIRST,) if decode else ()) + ((_BEAM_FAMILY_FIRST,) if beam else ()) \
            + ((_HALF_FAMILY_FIRST,) if half else ()) + ((_EDGE16_FAMILY_FIRST,) if edge16 else ()) \
            + ((_HALF_TRAIN_FAMILY_FIRST,) if half_training else ()) \
            + ((_EDGE16_DST_FAMILY_FIRST,) if edge16_dst else ()) \
            + ((_BEAM_FINISH_FAMILY_FIRST,) if beam_finish else ()) \
            + ((_ATTENTION16_FAMILY_FIRST,) if attention16 else ()) \
            + ((_EDGE16_TRAIN_FAMILY_FIRST,) if edge16_training else ()):
        i = first
        while True:
            name = lib.ptgnn_amd_launch_name(i)
            if name is None:
                break
            out[name.decode()] = int(lib.ptgnn_amd_launch_count(i))
            i += 1
    return out


def launches_since(before: dict) -> dict:
    """Kernel families of `before = launch_counts(...)` launched since -> {name: count}, zero entries dropped."""
    now = launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True, beam=True, half=True,
                        edge16=True, half_training=True, edge16_dst=True, beam_finish=True, attention16=True,
                        edge16_training=True)
    return {k: now[k] - v for k, v in before.items() if now[k] != v}


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class KernelTimer:
    """Optional HIP-event bracket around every C-ABI launch (bench.py's live roofline numbers).
    Events are recorded on the stream the kernel is launched on; nothing synchronises until
    `summary()` is called."""

    def __init__(self):
        self.records = []   # (name, start_event, end_event, work dict)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, s, e, work in self.records:
            d = out.setdefault(name, {"calls": 0, "ms": 0.0, "bytes": 0.0, "flops": 0.0})
            d["calls"] += 1
            d["ms"] += s.elapsed_time(e)
            b, f = work.get("bytes", 0.0), work.get("flops", 0.0)
            d["bytes"] += b() if callable(b) else b
            d["flops"] += f() if callable(f) else f
        return out


_TIMER: Optional[KernelTimer] = None


def set_kernel_timer(timer: Optional[KernelTimer]):
    global _TIMER
    _TIMER = timer


class _timed:
    __slots__ = ("name", "work", "s")

    def __init__(self, name, **work):
        self.name, self.work = name, work

    def __enter__(self):
        if _TIMER is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if _TIMER is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _TIMER.records.append((self.name, self.s, e, self.work))
        return False


def _require_cuda_f32(name: str, t: torch.Tensor, dims: int = 2):
    if not t.is_cuda:
        raise _lib.PtgnnAmdError(
            f"{name} must live on the GPU: the C-ABI wrappers have no CPU path (got device {t.device}; CPU tensors are served "
            "one level up, by the layers' and the facade's plain-torch route)")
    if t.dtype != torch.float32:
        raise _lib.PtgnnAmdError(f"{name} must be float32 (got {t.dtype})")
    if t.dim() != dims:
        raise _lib.PtgnnAmdError(f"{name} must be {dims}-D (got shape {tuple(t.shape)})")


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    """Accept row-major 2-D views with unit inner stride (e.g. column slices); copy otherwise."""
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    if t.shape[1] == 1 and t.stride(0) >= 1:
        return t
    return t.contiguous()


def _ptr_or(t: torch.Tensor, stand_in: torch.Tensor) -> int:
    """Device pointer of `t`; a tensor WITHOUT elements (the message table of a minibatch whose edge types are all empty)
    has none, so a stand-in that is never dereferenced (no CSR slot refers to a row of it) is passed instead."""
    return t.data_ptr() if t.numel() else stand_in.data_ptr()


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _rows_arg(t: torch.Tensor, d: int):
    """(data pointer, leading dimension) of an [n, d] operand of a library call: (None, d) when it has no rows."""
    return (t.data_ptr(), _ld(t)) if t.numel() else (None, d)


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Scratch bytes of one library call; never empty, so that its pointer is not NULL."""
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


class _DeviceState:
    """What the host keeps about ONE GPU between calls: the node-id guard's accumulator and its read-back (at most one
    in flight), the shared-message and hub back-offs with the read-backs that drive them, the side stream of the
    overlapped plan build and the plan-build control blocks per stream.  The back-offs, the pending lists and the guard's
    read-back slot are changed under `_readback.LOCK` only.  Device objects are created on first use, outside the lock
    (looking a state up touches no GPU); of two accumulators created at once the first one stored is the one used."""
    __slots__ = ("device", "bad_ids", "bad_readback", "uniq_backoff", "uniq_pending", "hub_backoff", "hub_pending",
                 "side_stream", "plan_control")

    def __init__(self, index: int):
        self.device = torch.device("cuda", index)
        self.bad_ids = self.bad_readback = self.side_stream = None     # bad_ids: int32 [1] device accumulator
        self.uniq_backoff, self.uniq_pending = Backoff(), []     # row counts in flight, tag = (edges, edge types)
        self.hub_backoff, self.hub_pending = Backoff(), []       # hub counts in flight, tag = weakref to the plan
        self.plan_control = {}                                   # stream handle -> zero-at-rest control block


_STATES = {}    # device index -> _DeviceState


def _device_state(device) -> _DeviceState:
    key = torch.device(device).index or 0
    st = _STATES.get(key)
    if st is None:
        with LOCK:
            st = _STATES.setdefault(key, _DeviceState(key))
    return st


# ------------------------------------------------------------------------------------------------
# graph plan
# ------------------------------------------------------------------------------------------------
class GraphPlan:
    """Destination-sorted CSR of all edge types of one minibatch (see ptgnn_amd_csr_build).

    rowptr int32 [N+1]; col int32 [E] = (src << type_bits) | type; perm int32 [E] = position of
    the CSR slot's edge in the type-major concatenation of the adjacency lists.
    """

    __slots__ = ("rowptr", "col", "perm", "type_bits", "num_nodes", "num_edges", "num_types",
                 "num_src_rows", "_backward", "_adj", "_adj_refs", "_inv_perm", "_ready", "_waited",
                 "_hub_tickets", "hub_entries", "hub_count", "_slot_rows", "_ident", "_transposed", "_uniq", "_hub_posted",
                 "_has_hubs", "_hdrs", "__weakref__")

    def __init__(self, rowptr, col, perm, type_bits, num_nodes, num_edges, num_types):
        self.rowptr, self.col, self.perm = rowptr, col, perm
        self.type_bits, self.num_nodes = type_bits, num_nodes
        self.num_edges, self.num_types = num_edges, num_types
        self.num_src_rows = num_nodes
        self._backward = None
        self._adj = None       # the adjacency tensors the plan was built from (for the backward plan)
        self._adj_refs = None
        self._inv_perm = None
        self._ready = None     # event recorded on the plan stream after the build (None = same stream)
        self._waited = set()
        self._hub_tickets = {}
        self.hub_entries = self.hub_count = None   # (chunk, row) pairs of rows > HUB_THRESHOLD
        self._slot_rows = self._ident = self._transposed = None
        self._uniq = None      # UniqueMessages | pending read-back | False (not worth it / not applicable)
        self._hub_posted = False   # the hub count's Readback is pending on the device's state (ops.gather_update_supported)
        self._has_hubs = None      # ... and has arrived: True / False (None = not known on the host)
        self._hdrs = {}            # "col" / "perm" -> row headers int32 [N, 8] of that slot array (row_header)

    def may_have_hubs(self) -> bool:
        """Only plans with more edges than the threshold can contain a hub row (whether they do is
        known on the device: `hub_count`)."""
        return self.hub_entries is not None

    def hub_tickets(self, msg_dim: int) -> torch.Tensor:
        """Arrival counters of the hub chunks: zeroed once, left zero by every launch -- and owned by the launches of ONE
        stream at a time (include/ptgnn_amd.h), so they are kept per (size, current stream): two streams that
        aggregate over the same plan concurrently must not count each other's chunks."""
        n = _lib.load().ptgnn_amd_hub_ticket_count(self.num_edges, msg_dim)
        dev = self.rowptr.device
        key = (n, torch.cuda.current_stream(dev).cuda_stream)
        t = self._hub_tickets.get(key)
        if t is None:
            t = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            self._hub_tickets[key] = t
        return t

    def wait(self) -> None:
        """Make the current stream wait for a plan that was built on the side stream (once per stream).
        Consumers call this right before their first launch that reads rowptr/col/perm."""
        if self._ready is not None:
            cur = torch.cuda.current_stream(self.rowptr.device)
            if cur.cuda_stream not in self._waited:
                cur.wait_event(self._ready)
                self._waited.add(cur.cuda_stream)

    def row_header(self, entries: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """int32 [N, 8] row headers of a forward plan for the slot array the aggregation is about to read (`entries`:
        the plan's col -- the default --, its perm, or the slot_row of its UniqueMessages): hdr[r, k] is the entry of slot
        rowptr[r] + k, clamped to the row's last slot, zeros for an empty row (ptgnn_amd_row_headers).  One launch on the
        first call per slot array, behind the plan build, shared by every layer of the minibatch; no host
        synchronisation.  None for the plans that keep the plain walk (backward, transposed, pooling) and for a slot
        array the plan does not know."""
        if self._adj is None:
            return None
        uniq = self._uniq or None
        if entries is None or entries is self.col:
            key, entries = "col", self.col
        elif entries is self.perm:
            key = "perm"
        elif uniq is not None and entries is uniq.slot_row:
            if uniq.hdr is None:
                uniq.hdr = _launch_row_headers(self, entries)
            return uniq.hdr
        else:
            return None
        hdr = self._hdrs.get(key)
        if hdr is None:
            hdr = self._hdrs[key] = _launch_row_headers(self, entries)
        return hdr

    def unique_messages(self) -> Optional["UniqueMessages"]:
        """Message rows of the layers whose message depends on (edge type, source) only (GGNN without edge features /
        per-edge dropout): one row per pair that occurs instead of one per edge -- see ptgnn_amd_unique_sources.  Built
        on the first call behind the plan build and shared by all layers of the minibatch; everything the de-duplicated
        launches need stays on the device (no host synchronisation).  None when it does not apply (small batches, more
        than 64 edge types) or when recent minibatches saved fewer than UNIQUE_MIN_SAVING of their rows."""
        if self._uniq is None:
            self._uniq = _launch_unique_sources(self) or False
        return self._uniq or None

    def backward_plan(self) -> "GraphPlan":
        """Plan of the transposed problem, rows = src * T + type, col = dst: row r of the [N*T, M] view
        of the message-table gradient sums the output gradients of its out-edges.  Built lazily on the
        first backward of a minibatch and shared by all layers."""
        if self._backward is None:
            if self._adj is None:
                raise _lib.PtgnnAmdError("this plan was built without keeping its adjacency lists")
            self.wait()
            self._backward = build_plan(self._adj, self.num_src_rows * self.num_types, mode=2)
        return self._backward

    def forward_slot_of_backward_slot(self) -> torch.Tensor:
        """int32 [E]: for slot i of the backward plan, the forward-plan slot of the same edge."""
        bp = self.backward_plan()
        if bp._inv_perm is None:   # reuse the field on the backward plan as the cache
            inv = self.inverse_perm()
            bp._inv_perm = inv[bp.perm[: self.num_edges].to(torch.int64)].to(torch.int32).contiguous()
        return bp._inv_perm

    def slot_rows(self) -> torch.Tensor:
        """int32 [E]: destination row of every CSR slot (rowptr expanded); built on the first backward
        of a minibatch, shared by all layers."""
        if self._slot_rows is None:
            self.wait()
            E = self.num_edges
            deg = (self.rowptr[1:] - self.rowptr[:-1]).to(torch.int64)
            rows = torch.arange(self.num_nodes, device=self.rowptr.device, dtype=torch.int32)
            self._slot_rows = torch.repeat_interleave(rows, deg, output_size=E) if E > 0 else rows[:0]
        return self._slot_rows

    def identity_index(self) -> List[torch.Tensor]:
        """Per-type views of arange(E) (int64): the "source index" that makes the grouped edge GEMM
        read its A rows in message order (backward of the message Linear)."""
        if self._ident is None:
            if self._adj is None:
                raise _lib.PtgnnAmdError("this plan was built without keeping its adjacency lists")
            ar = torch.arange(max(self.num_edges, 1), device=self.rowptr.device, dtype=torch.int64)
            out, off = [], 0
            for s_, _ in self._adj:
                n = int(s_.shape[0])
                out.append(ar[off: off + n])
                off += n
            self._ident = out
        return self._ident

    def transposed_plan(self) -> "GraphPlan":
        """rows = source node, col/perm over the same message order: segment-sums per-edge input
        gradients back onto the source rows."""
        if self._transposed is None:
            if self._adj is None:
                raise _lib.PtgnnAmdError("this plan was built without keeping its adjacency lists")
            self.wait()
            self._transposed = build_plan(self._adj, self.num_src_rows, mode=1)
        return self._transposed

    def inverse_perm(self) -> torch.Tensor:
        """original edge position -> CSR slot (int64)."""
        if self._inv_perm is None:
            self.wait()
            inv = torch.empty(max(self.num_edges, 1), dtype=torch.int64, device=self.perm.device)
            inv[self.perm[: self.num_edges].to(torch.int64)] = torch.arange(
                self.num_edges, device=self.perm.device)
            self._inv_perm = inv
        return self._inv_perm


class UniqueMessages:
    """slot_row int32 [E]: message row of every CSR slot; unique_src int64: source node of every message row
    (type-major); edge_table: the device-resident launch table of ptgnn_amd_edge_linear_shared_f32; capacity: rows the
    message table must hold; counts: device int64 [T + 1] rows per type and in all (`_readback`: their Readback, posted
    with the build unless it was captured); hdr: the row headers of slot_row (GraphPlan.row_header), None until an
    aggregation asks for them."""
    __slots__ = ("slot_row", "unique_src", "edge_table", "capacity", "counts", "num_edges", "num_types", "_readback",
                 "_counts", "hdr")

    def __init__(self, slot_row, unique_src, edge_table, capacity, counts, num_edges, num_types):
        self.slot_row, self.unique_src, self.edge_table = slot_row, unique_src, edge_table
        self.capacity, self.counts, self.num_edges, self.num_types = capacity, counts, num_edges, num_types
        self._readback = self._counts = self.hdr = None

    def host_counts(self, wait: bool = False) -> Optional[List[int]]:
        """Rows per edge type + the total, once the asynchronous read-back has arrived (None before).  `wait` blocks
        on the read-back's own event -- not on the stream: work enqueued after the bookkeeping keeps running."""
        if self._counts is None:
            if self._readback is not None:
                self._counts = self._readback.values(wait)
            elif wait:                          # built under graph capture: no read-back was posted
                self._counts = [int(c) for c in self.counts.tolist()]
        return self._counts

    def rows(self, wait: bool = False) -> Optional[int]:
        """Rows of the message table (None while the read-back is in flight, unless `wait`)."""
        c = self.host_counts(wait)
        return None if c is None else c[self.num_types]

    def adjacency(self):
        """Per edge type (unique source ids, same): the adjacency input of the host-sized launches (weight gradient,
        tests).  Waits for the row counts."""
        adj, off = [], 0
        for c in self.host_counts(wait=True)[:-1]:
            adj.append((self.unique_src[off: off + c], self.unique_src[off: off + c]))
            off += c
        return adj


# Sharing message rows costs ~6 small launches per minibatch.  Whether it pays is only known afterwards (the row counts
# come back asynchronously): when the minibatches seen so far saved fewer than UNIQUE_MIN_SAVING of their rows, the
# next UNIQUE_BACKOFF plans of that device keep the per-edge form, then one is probed again.
UNIQUE_MIN_SAVING = float(os.environ.get("PTGNN_AMD_UNIQUE_MIN_SAVING", "0.05"))
UNIQUE_MIN_EDGES = int(os.environ.get("PTGNN_AMD_UNIQUE_MIN_EDGES", "65536"))
UNIQUE_BACKOFF = 16


def _poll_unique_stats(st: _DeviceState) -> None:
    for readback in take_arrived(st.uniq_pending, keep=8):
        num_edges, num_types = readback.tag
        if num_edges > 0 and readback.values()[num_types] > (1.0 - UNIQUE_MIN_SAVING) * num_edges:
            st.uniq_backoff.trip(UNIQUE_BACKOFF)


def _launch_unique_sources(plan: "GraphPlan") -> Optional[UniqueMessages]:
    lib = _lib.load()
    E, T, ns = plan.num_edges, plan.num_types, plan.num_src_rows
    if plan._adj is None or E < UNIQUE_MIN_EDGES or T > 64:
        return None
    capturing = torch.cuda.is_current_stream_capturing()
    dev = plan.col.device
    st = _device_state(dev)
    if not capturing:
        _poll_unique_stats(st)
        if st.uniq_backoff.consume():
            return None
    plan.wait()
    cap = max(1, min(E, ns * T))
    slot_row = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    unique_src = torch.empty(cap, dtype=torch.int64, device=dev)
    counts = torch.empty(T + 1, dtype=torch.int64, device=dev)
    table = torch.empty(int(lib.ptgnn_amd_edge_table_bytes()), dtype=torch.uint8, device=dev)
    ws_bytes = int(lib.ptgnn_amd_unique_sources_workspace_bytes(ns, T))
    ws = _workspace(ws_bytes, dev)
    with _timed("unique_sources", bytes=E * 12.0 + ns * T / 4.0):
        rc = lib.ptgnn_amd_unique_sources(plan.col.data_ptr(), E, plan.type_bits, T, ns, slot_row.data_ptr(),
                                          unique_src.data_ptr(), cap, counts.data_ptr(), table.data_ptr(),
                                          ws.data_ptr(), ws_bytes, _stream(slot_row))
    _lib.check(rc, "ptgnn_amd_unique_sources")
    u = UniqueMessages(slot_row, unique_src, table, cap, counts, E, T)
    if not capturing:
        u._readback = Readback(counts, tag=(E, T))
        with LOCK:
            st.uniq_pending.append(u._readback)
    return u


# Row headers (GraphPlan.row_header): the aggregation's lane groups request a row's first eight slot entries together
# with its rowptr pair.  PTGNN_AMD_ROW_HEADERS=0 (or ops.ROW_HEADERS = False, looked at per call) keeps the plain walk:
# same bits, one more dependent round trip per row (A/B + tests).
ROW_HEADERS = os.environ.get("PTGNN_AMD_ROW_HEADERS", "1") not in ("", "0")


def _launch_row_headers(plan: "GraphPlan", entries: torch.Tensor) -> torch.Tensor:
    N = plan.num_nodes
    plan.wait()
    hdr = torch.empty(max(N, 1), 8, dtype=torch.int32, device=plan.rowptr.device)
    with _timed("row_headers", bytes=N * (32.0 + 4) + 4.0 * min(plan.num_edges, 8 * N)):
        rc = _lib.load().ptgnn_amd_row_headers(plan.rowptr.data_ptr(), entries.data_ptr(), N, hdr.data_ptr(),
                                               _stream(hdr))
    _lib.check(rc, "ptgnn_amd_row_headers")
    return hdr


def edge_linear_shared_supported(state_dim: int, msg_dim: int, num_types: int) -> bool:
    return bool(_lib.load().ptgnn_amd_edge_linear_shared_supported(state_dim, msg_dim, num_types))


def edge_linear16_supported(state_dim: int, msg_dim: int, num_types: int, dtype) -> bool:
    """Whether the 16-bit-input grouped per-edge GEMM takes the shape (ptgnn_amd_edge_linear16_supported; no device)."""
    if dtype not in HALF_IDS:
        return False
    return bool(_lib.load().ptgnn_amd_edge_linear16_supported(int(state_dim), int(msg_dim), int(num_types),
                                                             HALF_IDS[dtype]))


def edge_linear16_dst_supported(state_dim: int, msg_dim: int, num_types: int, dtype) -> bool:
    """Whether the 16-bit-input grouped per-edge GEMM with a target-state half takes the shape
    (ptgnn_amd_edge_dst_linear16_supported; no device).  `state_dim` is H: the weights are [msg_dim, 2 H]."""
    if dtype not in HALF_IDS:
        return False
    return bool(_lib.load().ptgnn_amd_edge_dst_linear16_supported(int(state_dim), int(msg_dim), int(num_types),
                                                                 HALF_IDS[dtype]))


def edge_linear16_masked_supported(state_dim: int, msg_dim: int, num_types: int, dtype, mode: int) -> bool:
    """Whether the 16-bit grouped per-edge GEMM takes the shape with the per-edge dropout mask in `mode` (1: on the
    gathered input, the forward; 2: on the output, the input gradient) -- ptgnn_amd_edge_masked_linear16_supported;
    needs no device."""
    if dtype not in HALF_IDS:
        return False
    return bool(_lib.load().ptgnn_amd_edge_masked_linear16_supported(int(state_dim), int(msg_dim), int(num_types),
                                                                     HALF_IDS[dtype], int(mode)))


def edge_weight_grad16_supported(state_dim: int, msg_dim: int, num_types: int, dtype) -> bool:
    """Whether the 16-bit per-type weight gradient takes the shape (ptgnn_amd_edge_weight_grad16_supported; needs no
    device)."""
    if dtype not in HALF_IDS:
        return False
    return bool(_lib.load().ptgnn_amd_edge_weight_grad16_supported(int(state_dim), int(msg_dim), int(num_types),
                                                                   HALF_IDS[dtype]))


def edge_wgrad16_chunk_edges(num_edges: int, num_types: int, msg_dim: int, state_dim: int) -> int:
    """Edges one workgroup partial of the 16-bit per-type weight gradient covers -- a type of n edges is ceil(n / it)
    partials (ptgnn_amd_edge_wgrad16_chunk_edges; needs no device); 0 for a shape the kernel does not take."""
    return int(_lib.load().ptgnn_amd_edge_wgrad16_chunk_edges(int(num_edges), int(num_types), int(msg_dim),
                                                              int(state_dim)))


def _edge16_stack(ws: Sequence[torch.Tensor], dtype: torch.dtype, given: Optional[torch.Tensor]) -> torch.Tensor:
    """The [T, M, H] stack ([T, M, 2 H] with a target-state half) of the per-type weights rounded to `dtype` by torch
    (round to nearest even), or the caller's cached copy of exactly that."""
    shape = (len(ws),) + tuple(ws[0].shape)
    if given is None:
        return torch.stack(list(ws)).to(dtype)          # two launches, whatever T; the rounding of w.to(dtype)
    if given.dtype != dtype or tuple(given.shape) != shape or given.device != ws[0].device:
        raise _lib.PtgnnAmdError(f"rounded weights must be {dtype} {shape} on {ws[0].device} "
                                 f"(got {given.dtype} {tuple(given.shape)} on {given.device})")
    return given.contiguous()


def edge_linear_shared(x: torch.Tensor, uniq: UniqueMessages, weights: Sequence[torch.Tensor],
                       act: Optional[str] = None, inputs=None, rounded: Optional[torch.Tensor] = None) -> torch.Tensor:
    """msg[r] = act(W_t x[unique_src[r]]) over the message rows of `uniq` (GraphPlan.unique_messages): the grouped
    per-edge GEMM of `edge_linear` with one row per distinct (edge type, source) pair; rows beyond the table's count
    are not written.  The launch geometry comes from the device-resident table: no host synchronisation.
    `inputs` = torch.bfloat16 / torch.float16: the gathered rows and the weights are rounded to that type and multiplied
    on the 16-bit matrix cores (fp32 accumulation and output) where `edge_linear16_supported` takes the shape and x has
    16-byte aligned rows; otherwise the fp32 kernel runs, silently.  `rounded`: the caller's [T, M, H] stack of
    `weight.to(inputs)`, to save the conversion."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    T, H, M = uniq.num_types, x.shape[1], weights[0].shape[0]
    if len(weights) != T:
        raise _lib.PtgnnAmdError(f"edge_linear_shared: {len(weights)} weights for {T} edge types")
    ws = [w.detach().contiguous() for w in weights]
    for w in ws:
        if tuple(w.shape) != (M, H) or not w.is_cuda or w.dtype != torch.float32:
            raise _lib.PtgnnAmdError(f"edge_linear_shared: weight shape {tuple(w.shape)} does not match [{M}, {H}]")
    msg = torch.empty(uniq.capacity, M, dtype=torch.float32, device=x.device)

    def rows():                       # resolved when the timer is summarised: the count is back by then
        r = uniq.rows(wait=True)
        return float(r if r is not None else uniq.num_edges)
    half = _half_inputs(inputs)
    if half is not None and edge_linear16_supported(H, M, T, half) and _half_rows_ok(x):
        w16 = _edge16_stack(ws, half, rounded)
        with _timed("edge_linear16_shared", flops=lambda: 2.0 * rows() * H * M,
                    bytes=lambda: 4.0 * (rows() * H + rows() * M) + 2.0 * T * M * H + 8.0 * rows()):
            rc = lib.ptgnn_amd_edge_linear16_shared(x.data_ptr(), _ld(x), x.shape[0], H, uniq.edge_table.data_ptr(),
                                                    w16.data_ptr(), T, M, ACT_IDS[act], HALF_IDS[half],
                                                    msg.data_ptr(), M, _stream(msg))
        _lib.check(rc, "ptgnn_amd_edge_linear16_shared")
        return msg
    wp = (ctypes.c_void_p * T)(*[w.data_ptr() for w in ws])
    with _timed("edge_linear_shared", flops=lambda: 2.0 * rows() * H * M,
                bytes=lambda: 4.0 * (rows() * H + rows() * M + T * M * H) + 8.0 * rows()):
        rc = lib.ptgnn_amd_edge_linear_shared_f32(x.data_ptr(), _ld(x), x.shape[0], H, uniq.edge_table.data_ptr(),
                                                  ctypes.cast(wp, ctypes.c_void_p), T, M, ACT_IDS[act],
                                                  msg.data_ptr(), M, _stream(msg))
    _lib.check(rc, "ptgnn_amd_edge_linear_shared_f32")
    return msg


# ------------------------------------------------------------------------------------------------
# index range guard
# ------------------------------------------------------------------------------------------------
# The reference device-asserts on an out-of-range node id (F.embedding, gatedmessagepassing.py:54-56).
# Here the plan build clamps such ids to row 0 (nothing is ever read or written out of bounds) and counts
# them in a per-device accumulator (`_DeviceState.bad_ids`); the count travels back through a Readback WITHOUT a sync
# and is looked at on later plan builds (or on demand: `check_indices(sync=True)`).  A non-zero count raises
# PtgnnAmdError: the results of the offending minibatch are garbage, like the reference's would be.
VALIDATE_INDICES = os.environ.get("PTGNN_AMD_VALIDATE", "async")   # "async" | "sync" | "off"


def _bad_accumulator(st: _DeviceState) -> torch.Tensor:
    if st.bad_ids is None:
        fresh = torch.zeros(1, dtype=torch.int32, device=st.device)
        with LOCK:
            if st.bad_ids is None:
                st.bad_ids = fresh
    return st.bad_ids


def _raise_bad(st: _DeviceState, count: int):
    st.bad_ids.zero_()
    with LOCK:
        st.bad_readback = None      # one still in flight carries the count that is being reported here
    raise _lib.PtgnnAmdError(
        f"{count} node id(s) outside [0, num_nodes) reached the graph plan build (adjacency lists / scatter "
        "index / dim_size too small). They were clamped to row 0 so no memory was touched out of bounds, but "
        "the outputs of that minibatch are wrong.")


def check_indices(device=None, sync: bool = False) -> None:
    """Raise if a plan build on `device` (None: any device) saw an out-of-range node id.  sync=True reads the device's
    accumulator; sync=False only looks at a read-back that has already arrived (no host-device synchronisation)."""
    for st in list(_STATES.values()) if device is None else [_device_state(device)]:
        if st.bad_ids is None:
            continue
        if sync:
            n = int(st.bad_ids.item())
        else:
            rb = st.bad_readback
            got = rb.values() if rb is not None else None
            if got is None:
                continue
            with LOCK:
                mine = st.bad_readback is rb
                if mine:
                    st.bad_readback = None
            n = got[0] if mine else 0       # the thread that cleared the slot reports the count, no other
        if n:
            _raise_bad(st, n)


def _post_bad_readback(st: _DeviceState) -> None:
    if st.bad_readback is None:     # one read-back in flight at a time
        rb = Readback(st.bad_ids)   # (a HIP call: outside the lock)
        with LOCK:
            if st.bad_readback is None:
                st.bad_readback = rb
        # a thread that lost this race drops its copy of the same accumulator; its buffer is still being written, so it
        # does not go back to the pool


def _plan_control(dev: torch.device) -> torch.Tensor:
    """The control block ptgnn_amd_csr_build wants (include/ptgnn_amd.h): zero-filled once, then owned by the
    builds of ONE stream -- stream order serialises them and every build leaves it zero-filled.  Under graph
    capture a fresh zero-filled block is captured with the build instead (a cached one could be shared with
    eager builds that run while the graph replays)."""
    nbytes = int(_lib.load().ptgnn_amd_csr_control_bytes())
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    blocks, key = _device_state(dev).plan_control, torch.cuda.current_stream(dev).cuda_stream
    ctl = blocks.get(key)
    if ctl is None:
        ctl = blocks.setdefault(key, torch.zeros(nbytes, dtype=torch.uint8, device=dev))
    return ctl


def build_plan(adjacency_lists: Sequence[Tuple[torch.Tensor, torch.Tensor]], num_nodes: int,
               transposed: bool = False, want_perm: bool = True,
               num_src_rows: Optional[int] = None, mode: Optional[int] = None) -> GraphPlan:
    """One stable sort per minibatch; reused by every layer of the forward.  mode: 0 forward plan
    (rows = dst), 1 transposed (rows = src), 2 backward plan (rows = src * T + type, col = dst;
    `num_nodes` must then be source rows * T)."""
    if mode is None:
        mode = 1 if transposed else 0
    lib = _lib.load()
    T = len(adjacency_lists)
    if T == 0:
        raise _lib.PtgnnAmdError("build_plan: at least one edge type is required")
    dev = None
    srcs, dsts, counts = [], [], []
    for t, (s, d) in enumerate(adjacency_lists):
        if not (s.is_cuda and d.is_cuda):
            raise _lib.PtgnnAmdError("build_plan: adjacency lists must be CUDA tensors (no CPU path)")
        if s.dtype != torch.int64 or d.dtype != torch.int64:
            raise _lib.PtgnnAmdError("build_plan: adjacency lists must be int64 "
                                     "(GraphNeuralNetworkModel.finalize_minibatch layout)")
        if s.dim() != 1 or s.shape != d.shape:
            raise _lib.PtgnnAmdError(f"build_plan: edge type {t}: src/dst must be equal-length 1-D")
        s, d = s.contiguous(), d.contiguous()
        dev = s.device if dev is None else dev
        srcs.append(s)
        dsts.append(d)
        counts.append(int(s.shape[0]))
    E = sum(counts)
    type_bits = lib.ptgnn_amd_type_bits(T)
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    perm = torch.empty(max(E, 1), dtype=torch.int32, device=dev) if want_perm else None
    ws_bytes = lib.ptgnn_amd_csr_workspace_bytes(E, num_nodes)
    ws = _workspace(ws_bytes, dev)
    control = _plan_control(dev)
    hub_entries = hub_count = None
    if HUB_THRESHOLD > 0 and E > HUB_THRESHOLD:
        hub_entries = torch.empty(2 * ((E + 1023) // 1024), 2, dtype=torch.int32, device=dev)
        hub_count = torch.empty(1, dtype=torch.int32, device=dev)
    PtrArr, CntArr = ctypes.c_void_p * T, ctypes.c_int64 * T
    src_ptrs = PtrArr(*[s.data_ptr() if s.numel() else None for s in srcs])
    dst_ptrs = PtrArr(*[d.data_ptr() if d.numel() else None for d in dsts])
    cnts = CntArr(*counts)
    bad = None
    capturing = torch.cuda.is_current_stream_capturing()
    if VALIDATE_INDICES != "off":
        bad = _device_state(dev)
        if not capturing:
            check_indices(dev)      # surfaces an earlier minibatch's bad ids (never blocks)
    # algorithmic bytes: read 16 B/edge (int64 src+dst), write 4 B/edge col (+4 perm) + rowptr
    with _timed("csr_build", bytes=E * (16 + 4 + (4 if want_perm else 0)) + 4.0 * (num_nodes + 1)):
        rc = lib.ptgnn_amd_csr_build(ctypes.cast(src_ptrs, ctypes.c_void_p),
                                     ctypes.cast(dst_ptrs, ctypes.c_void_p),
                                     ctypes.cast(cnts, ctypes.c_void_p), T, num_nodes,
                                     int(num_src_rows or 0),
                                     mode, rowptr.data_ptr(), col.data_ptr(),
                                     perm.data_ptr() if perm is not None else None, None,
                                     HUB_THRESHOLD if hub_entries is not None else 0,
                                     hub_entries.data_ptr() if hub_entries is not None else None,
                                     hub_count.data_ptr() if hub_count is not None else None,
                                     _bad_accumulator(bad).data_ptr() if bad is not None else None,
                                     control.data_ptr(),
                                     ws.data_ptr(), ws_bytes, _stream(rowptr))
    if rc != 0:
        _device_state(dev).plan_control.clear()     # a build that stopped half-way may have left its block non-zero
    _lib.check(rc, "ptgnn_amd_csr_build")
    if bad is not None:
        if capturing:
            pass                    # a captured plan build keeps counting; read-backs resume outside the graph
        elif VALIDATE_INDICES == "sync":
            check_indices(dev, sync=True)
        else:
            _post_bad_readback(bad)
    # `ws`, `srcs`, `dsts` are stream-ordered: torch's caching allocator only hands their memory to
    # later work on the same stream, so dropping the references here is safe.
    # col/perm keep >= 1 element so their base pointer is never null (E == 0 batches are legal)
    plan = GraphPlan(rowptr, col, perm, 0 if mode == 2 else type_bits, num_nodes, E, T)
    plan.hub_entries, plan.hub_count = hub_entries, hub_count
    if mode == 0:
        plan.num_src_rows = int(num_src_rows or num_nodes)
        plan._adj = list(zip(srcs, dsts))
    return plan


def shard_index(adjacency_lists: Sequence[Tuple[torch.Tensor, torch.Tensor]], lo: int, hi: int,
                bounds: torch.Tensor, total_nodes: int):
    """ptgnn_amd_shard_index: (local_src [E], local_dst [E], need_ids buffer, stats) of a dst-range shard whose
    edges are given in global ids; see include/ptgnn_amd.h.  No host synchronisation."""
    lib = _lib.load()
    T = len(adjacency_lists)
    srcs = [a[0].contiguous() for a in adjacency_lists]
    dsts = [a[1].contiguous() for a in adjacency_lists]
    for s_, d_ in zip(srcs, dsts):
        if not (s_.is_cuda and d_.is_cuda and s_.dtype == torch.int64 and d_.dtype == torch.int64 and s_.shape == d_.shape):
            raise _lib.PtgnnAmdError("shard_index: adjacency lists must be equal-length CUDA int64 tensors")
    dev = srcs[0].device
    counts = [int(s_.shape[0]) for s_ in srcs]
    E = sum(counts)
    world = int(bounds.shape[0]) - 1
    local_src = torch.empty(max(E, 1), dtype=torch.int64, device=dev)
    local_dst = torch.empty(max(E, 1), dtype=torch.int64, device=dev)
    cap = max(0, min(E, total_nodes - (hi - lo)))
    need = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    stats = torch.empty(world + 2 + T, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.ptgnn_amd_shard_index_workspace_bytes(total_nodes))
    ws = _workspace(ws_bytes, dev)
    PtrArr, CntArr = ctypes.c_void_p * T, ctypes.c_int64 * T
    sp = PtrArr(*[s_.data_ptr() if s_.numel() else None for s_ in srcs])
    dp = PtrArr(*[d_.data_ptr() if d_.numel() else None for d_ in dsts])
    cn = CntArr(*counts)
    # global source ids outside [0, total_nodes) are counted like the plan build's bad ids (after the remap they are
    # ordinary own / halo rows, which that guard can no longer see)
    bad = _device_state(dev) if VALIDATE_INDICES != "off" else None
    with _timed("shard_index", bytes=E * 32.0 + total_nodes / 4.0):
        rc = lib.ptgnn_amd_shard_index(ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(dp, ctypes.c_void_p),
                                       ctypes.cast(cn, ctypes.c_void_p), T, int(lo), int(hi), bounds.data_ptr(), world,
                                       int(total_nodes), local_src.data_ptr(), local_dst.data_ptr(), need.data_ptr(),
                                       cap, stats.data_ptr(), _bad_accumulator(bad).data_ptr() if bad is not None else None,
                                       ws.data_ptr(), ws_bytes, _stream(local_src))
    _lib.check(rc, "ptgnn_amd_shard_index")
    if bad is not None and not torch.cuda.is_current_stream_capturing():
        if VALIDATE_INDICES == "sync":
            check_indices(dev, sync=True)
        else:
            _post_bad_readback(bad)
    return local_src[:E], local_dst[:E], counts, need, stats


def plan_from_sorted_index(index: torch.Tensor, num_segments: int) -> GraphPlan:
    """Plan of a segment reduce whose index is already sorted (node_to_graph_idx of a disjoint-union
    batch): no sort -- rowptr is a searchsorted over the index, col/perm are the identity."""
    if not index.is_cuda or index.dtype != torch.int64 or index.dim() != 1:
        raise _lib.PtgnnAmdError("plan_from_sorted_index: expected a 1-D CUDA int64 index")
    n = int(index.shape[0])
    bounds = torch.arange(num_segments + 1, device=index.device, dtype=torch.int64)
    rowptr = torch.searchsorted(index, bounds).to(torch.int32)
    ident = torch.arange(max(n, 1), device=index.device, dtype=torch.int32)
    plan = GraphPlan(rowptr, ident, ident, 0, num_segments, n, 1)
    if HUB_THRESHOLD > 0 and n > HUB_THRESHOLD:   # graphs are long segments: reuse the hub machinery
        lib = _lib.load()
        plan.hub_entries = torch.empty(2 * ((n + 1023) // 1024), 2, dtype=torch.int32, device=index.device)
        plan.hub_count = torch.zeros(1, dtype=torch.int32, device=index.device)
        rc = lib.ptgnn_amd_hub_list(rowptr.data_ptr(), num_segments, HUB_THRESHOLD,
                                    plan.hub_entries.data_ptr(), plan.hub_count.data_ptr(), _stream(rowptr))
        _lib.check(rc, "ptgnn_amd_hub_list")
    return plan


_PLAN_CACHE: List[GraphPlan] = []
_PLAN_CACHE_SIZE = 4

# Rows longer than this are reduced chunk-parallel by the hub kernels (see gather_reduce.hip).
HUB_THRESHOLD = 2048

# The plan (sort) is latency-bound integer work and the first dense block of a layer (pre-transform /
# per-edge GEMM) does not read it, so the build CAN run on a side HIP stream under that GEMM, the
# aggregation kernel waiting on the plan's event (PTGNN_AMD_OVERLAP_PLAN=1).
# Off: measured again in round 2 with the streaming GEMMs (one 8-wave workgroup per CU, so the plan kernels do fit
# beside them): cfg2 0.411 -> 0.456 ms per step, cfg3 4.34 -> 4.39 ms -- the co-resident plan workgroups take LDS
# bandwidth and issue slots from the MFMA kernel for longer than the plan build lasts on an idle chip.
OVERLAP_PLAN_BUILD = os.environ.get("PTGNN_AMD_OVERLAP_PLAN", "0") not in ("", "0")


def _side_stream(device) -> "torch.cuda.Stream":
    st = _device_state(device)
    if st.side_stream is None:
        st.side_stream = torch.cuda.Stream(device=device)
    return st.side_stream


def _build_plan_overlapped(adjacency_lists, num_nodes: int) -> GraphPlan:
    dev = adjacency_lists[0][0].device
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    side.wait_stream(main)                      # the adjacency tensors' producers ran on `main`
    with torch.cuda.stream(side):
        plan = build_plan(adjacency_lists, num_nodes)
        plan._ready = torch.cuda.Event()
        plan._ready.record(side)
    for s, d in adjacency_lists:                # read by side-stream kernels: defer allocator reuse
        s.record_stream(side)
        d.record_stream(side)
    for t in (plan.rowptr, plan.col, plan.perm, plan.hub_entries, plan.hub_count):  # alloc on `side`, used on `main`
        if t is not None:
            t.record_stream(main)
    return plan


def plan_for(adjacency_lists: Sequence[Tuple[torch.Tensor, torch.Tensor]], num_nodes: int) -> GraphPlan:
    """Plan lookup keyed on the *identity and version* of the adjacency tensors, so the L layers of
    one forward (which all receive the same tensors, graphneuralnetwork.py:122-131) share one
    sort.  Weak references guarantee a freed-and-reallocated tensor can never alias a stale plan."""
    for plan in _PLAN_CACHE:
        refs = plan._adj_refs
        if plan.num_nodes != num_nodes or len(refs) != len(adjacency_lists):
            continue
        ok = True
        for (rs, vs, rd, vd), (s, d) in zip(refs, adjacency_lists):
            if rs() is not s or rd() is not d or s._version != vs or d._version != vd:
                ok = False
                break
        if ok:
            return plan
    plan = _build_plan_overlapped(adjacency_lists, num_nodes) if OVERLAP_PLAN_BUILD else \
        build_plan(adjacency_lists, num_nodes)
    plan._adj_refs = [(weakref.ref(s), s._version, weakref.ref(d), d._version)
                      for s, d in adjacency_lists]
    _PLAN_CACHE.insert(0, plan)
    del _PLAN_CACHE[_PLAN_CACHE_SIZE:]
    return plan


def clear_plan_cache():
    del _PLAN_CACHE[:]


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
def _hub_args(plan: GraphPlan, msg_dim: int, with_arg: bool, device):
    """(workspace, tail): the seven trailing hub arguments of the aggregation entry points (num_edges, hub_threshold,
    hub_entries, hub_count, hub_ws, hub_ws_bytes, hub_tickets) and the chunk-partial buffer they point into, which the
    caller holds until the launch is enqueued; (None, hub-free tail) when the plan is known hub-free."""
    if not plan.may_have_hubs():
        return None, (plan.num_edges, 0, None, None, None, 0, None)
    nbytes = _lib.load().ptgnn_amd_hub_workspace_bytes(plan.num_edges, msg_dim, 1 if with_arg else 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws, (plan.num_edges, HUB_THRESHOLD, plan.hub_entries.data_ptr(), plan.hub_count.data_ptr(), ws.data_ptr(),
                nbytes, plan.hub_tickets(msg_dim).data_ptr())


def _slot_map(plan: GraphPlan, type_bits: Optional[int], col: Optional[torch.Tensor]):
    """(type_bits, col) of a call: the plan's own table-form pair unless the caller passes the edge form's."""
    return plan.type_bits if type_bits is None else type_bits, plan.col if col is None else col


def gather_reduce(ysrc: torch.Tensor, plan: GraphPlan, msg_dim: int, reduce: str,
                  ydst: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE,
                  ln_weight: Optional[torch.Tensor] = None, ln_bias: Optional[torch.Tensor] = None,
                  ln_eps: float = 1e-5, return_arg: bool = False, type_bits: Optional[int] = None,
                  col: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                  rows: Optional[Tuple[int, int]] = None):
    """out[v] = EPI(reduce_{slots of v} ysrc[src, t*M:(t+1)*M] (+ ydst[v, t*M:(t+1)*M])).
    `out`: optional caller-owned [num_nodes, msg_dim] fp32 destination (e.g. one half of a stacked buffer).
    `rows` = (lo, hi): only the destination rows [lo, hi) are computed and written (needs `out`, no arg)."""
    lib = _lib.load()
    _require_cuda_f32("ysrc", ysrc)
    ysrc = _rowmajor(ysrc)
    ld_y = _ld(ysrc)
    ld_yd = ld_y
    if ydst is not None:
        _require_cuda_f32("ydst", ydst)
        ydst = _rowmajor(ydst)
        ld_yd = _ld(ydst)
    if reduce not in REDUCE_IDS:
        raise ValueError(f"unknown aggregation function {reduce!r}")
    N = plan.num_nodes
    caller_out = out
    if out is None:
        out = torch.empty(N, msg_dim, dtype=torch.float32, device=ysrc.device)
    elif tuple(out.shape) != (N, msg_dim) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.PtgnnAmdError(f"gather_reduce: `out` must be a contiguous float32 [{N}, {msg_dim}] tensor")
    arg = None
    if return_arg:
        arg = torch.empty(N, msg_dim, dtype=torch.int32, device=ysrc.device)
    if epilogue & EPI_LAYERNORM:
        ln_weight, ln_bias = ln_weight.contiguous(), ln_bias.contiguous()
    plan.wait()
    tb, colt = _slot_map(plan, type_bits, col)
    # algorithmic bytes (SURVEY.md 8d "(L)"): per edge one message row + its col entry; per node the
    # output row, the rowptr entry and (MLP-MP) the destination-term row; gathers get no cache credit
    nbytes = (plan.num_edges * (4.0 * msg_dim + 4) + N * (4.0 * msg_dim + 4)
              + (N * 4.0 * msg_dim if ydst is not None else 0.0)
              + (N * 4.0 * msg_dim if arg is not None else 0.0))
    lo, hi = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
    if rows is not None:
        if caller_out is None or return_arg:
            raise _lib.PtgnnAmdError("gather_reduce: a row range needs a caller-owned `out` (the other rows are not "
                                     "written) and returns no arg")
        nbytes *= (hi - lo) / max(N, 1)
    hub_ws, hub = _hub_args(plan, msg_dim, arg is not None, ysrc.device)
    # the kernel variants with a header-first walk (gather_reduce_core.h, hdr_walk): float4 rows in one column chunk,
    # no destination term, no arg output -- every other call would build a header that its kernel ignores
    hdr = None
    if (ROW_HEADERS and ydst is None and arg is None and msg_dim % 4 == 0 and msg_dim <= 256 and ld_y % 4 == 0
            and ysrc.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0):
        hdr = plan.row_header(colt)
    with _timed("gather_reduce", bytes=nbytes):
        rc = lib.ptgnn_amd_gather_reduce_hdr_f32(
            _ptr_or(ysrc, plan.rowptr), ld_y, ydst.data_ptr() if ydst is not None else None, ld_yd,
            plan.rowptr.data_ptr(), colt.data_ptr(), tb, N, msg_dim,
            REDUCE_IDS[reduce], epilogue,
            ln_weight.data_ptr() if ln_weight is not None else None,
            ln_bias.data_ptr() if ln_bias is not None else None, float(ln_eps),
            out.data_ptr(), msg_dim, arg.data_ptr() if arg is not None else None,
            *hub, lo, hi, hdr.data_ptr() if hdr is not None else None, _stream(out))
    _lib.check(rc, "ptgnn_amd_gather_reduce_hdr_f32")
    return (out, arg) if return_arg else out


# The fused aggregation + node update serves minibatch-sized plans (every row folds serially: no hub launches)
GATHER_UPDATE = os.environ.get("PTGNN_AMD_GATHER_UPDATE", "1") not in ("", "0")
GATHER_UPDATE_MAX_EDGES = 1 << 21


# ... and plans without hub rows: the fused kernel folds every row serially, so a row of > HUB_THRESHOLD in-edges (which the
# unfused aggregation splits over chunk workgroups) would set its duration.  Whether a plan has such rows is known on the
# device only (`plan.hub_count`); it is read back asynchronously once per plan, and a non-zero count sends the next
# GATHER_UPDATE_BACKOFF calls on that device to the unfused pair (both forms are exact: this is a speed decision, never a
# correctness one).
GATHER_UPDATE_BACKOFF = 64


def _poll_hub_counts(st: _DeviceState) -> None:
    for readback in take_arrived(st.hub_pending, keep=16):
        hubs = readback.values()[0] > 0
        plan = readback.tag()
        if plan is not None:
            plan._has_hubs = hubs            # a fact of THIS plan: decides every later call over it
        if hubs:
            st.hub_backoff.trip(GATHER_UPDATE_BACKOFF)


def gather_update_supported(msg_dim: int, out_dim: int, plan: "GraphPlan") -> bool:
    """Whether the fused aggregation + update launch serves this call.  Callers evaluate their cheaper conditions
    (gradients needed, dropout) FIRST: a call whose plan does not know its own hub count yet consumes one step of the hub
    back-off of the plan's device (`_DeviceState.hub_backoff`; under stream capture it is only looked at)."""
    if not (GATHER_UPDATE and plan.num_edges < GATHER_UPDATE_MAX_EDGES
            and bool(_lib.load().ptgnn_amd_gather_update_supported(int(msg_dim), int(out_dim)))):
        return False
    if plan.hub_count is None:              # too few edges for a hub row to exist
        return True
    if plan._has_hubs is not None:          # the plan's own count has come back (a cached plan of full-graph inference)
        return not plan._has_hubs
    st = _device_state(plan.hub_count.device)
    if torch.cuda.is_current_stream_capturing():
        return st.hub_backoff.steps == 0
    _poll_hub_counts(st)
    if plan._has_hubs is not None:
        return not plan._has_hubs
    with LOCK:
        post, plan._hub_posted = not plan._hub_posted, True
    if post:
        plan.wait()
        readback = Readback(plan.hub_count, tag=weakref.ref(plan))
        with LOCK:
            st.hub_pending.append(readback)
    # this plan's count is still in flight: go by what the recent plans of this device reported
    return not st.hub_backoff.consume()


def gather_update(msgs: torch.Tensor, plan: GraphPlan, reduce: str, col: torch.Tensor, type_bits: int, epilogue: int,
                  ln_weight: Optional[torch.Tensor], ln_bias: Optional[torch.Tensor], ln_eps: float,
                  weight: torch.Tensor, bias: Optional[torch.Tensor], act: Optional[str],
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(W . EPI(reduce_{slots of v} msgs[col >> type_bits]) + b) in ONE launch (ptgnn_amd_gather_update_f32): the
    aggregation of `gather_reduce` and the Linear of `linear`, same bits, without the [N, M] aggregate in memory."""
    lib = _lib.load()
    _require_cuda_f32("msgs", msgs)
    _require_cuda_f32("weight", weight)
    msgs, weight = _rowmajor(msgs), weight.contiguous()
    N, M, out_dim = plan.num_nodes, weight.shape[1], weight.shape[0]      # msgs: [E, M] rows or a [rows, T * M] table
    if msgs.shape[1] % M != 0 or reduce not in REDUCE_IDS:
        raise _lib.PtgnnAmdError(f"gather_update: weight {tuple(weight.shape)} / reduce {reduce!r} do not fit messages of "
                                 f"width {msgs.shape[1]}")
    if out is None:
        out = torch.empty(N, out_dim, dtype=torch.float32, device=msgs.device)
    elif tuple(out.shape) != (N, out_dim) or out.dtype != torch.float32 or out.stride(1) != 1 or not out.is_cuda:
        raise _lib.PtgnnAmdError(f"gather_update: `out` must be a float32 CUDA [{N}, {out_dim}] view with unit inner stride")
    if epilogue & EPI_LAYERNORM:
        ln_weight, ln_bias = ln_weight.contiguous(), ln_bias.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    plan.wait()
    E = plan.num_edges
    with _timed("gather_update", bytes=E * (4.0 * M + 4) + N * (4.0 * out_dim + 4) + 4.0 * out_dim * M,
                flops=2.0 * N * M * out_dim):
        rc = lib.ptgnn_amd_gather_update_f32(
            _ptr_or(msgs, plan.rowptr), _ld(msgs), plan.rowptr.data_ptr(), col.data_ptr(), int(type_bits), N, M, REDUCE_IDS[reduce],
            int(epilogue), ln_weight.data_ptr() if epilogue & EPI_LAYERNORM else None,
            ln_bias.data_ptr() if epilogue & EPI_LAYERNORM else None, float(ln_eps), weight.data_ptr(),
            bias.data_ptr() if bias is not None else None, out_dim, ACT_IDS[act], out.data_ptr(), _ld(out), _stream(out))
    _lib.check(rc, "ptgnn_amd_gather_update_f32")
    return out


def gather_reduce_masked(grad: torch.Tensor, arg: torch.Tensor, bplan: GraphPlan,
                         slot_of: torch.Tensor, msg_dim: int) -> torch.Tensor:
    """out[r] = sum_{i in row r} [arg[col_i] == slot_of[i]] * grad[col_i] over a backward plan."""
    lib = _lib.load()
    _require_cuda_f32("grad", grad)
    grad = _rowmajor(grad)
    bplan.wait()
    out = torch.empty(bplan.num_nodes, msg_dim, dtype=torch.float32, device=grad.device)
    hub_ws, hub = _hub_args(bplan, msg_dim, False, grad.device)
    with _timed("gather_reduce_masked", bytes=bplan.num_edges * (8.0 * msg_dim + 8) + bplan.num_nodes * (4.0 * msg_dim + 4)):
        rc = lib.ptgnn_amd_gather_reduce_masked_f32(_ptr_or(grad, bplan.rowptr), _ld(grad), _ptr_or(arg, bplan.rowptr),
                                                    bplan.rowptr.data_ptr(), bplan.col.data_ptr(),
                                                    slot_of.data_ptr(), bplan.num_nodes, msg_dim,
                                                    out.data_ptr(), msg_dim, *hub, _stream(out))
    _lib.check(rc, "ptgnn_amd_gather_reduce_masked_f32")
    return out


def segment_reduce(messages: torch.Tensor, plan: GraphPlan, reduce: str, return_arg: bool = False):
    """The torch_scatter seam over a plan: messages [E, D] are in the type-major concatenation
    order of the adjacency lists (abstractmessagepassing.py:38-50)."""
    _require_cuda_f32("messages", messages)
    if messages.shape[0] != plan.num_edges:
        raise _lib.PtgnnAmdError("segment_reduce: messages rows != number of edges in the plan")
    if plan.perm is None:
        raise _lib.PtgnnAmdError("segment_reduce: plan was built without perm")
    return gather_reduce(messages, plan, messages.shape[1], reduce, return_arg=return_arg,
                         type_bits=0, col=plan.perm)


def segment_mul(messages: torch.Tensor, plan: GraphPlan) -> torch.Tensor:
    """reduce="mul" of the torch_scatter seam over a plan (ptgnn_amd_segment_mul_f32): per destination row the product
    of its messages in edge order; rows without in-edges are 1, like torch_scatter's scatter_mul."""
    lib = _lib.load()
    _require_cuda_f32("messages", messages)
    if messages.shape[0] != plan.num_edges:
        raise _lib.PtgnnAmdError("segment_mul: messages rows != number of edges in the plan")
    if plan.perm is None:
        raise _lib.PtgnnAmdError("segment_mul: plan was built without perm")
    plan.wait()
    msg = _rowmajor(messages)
    n, d, E = plan.num_nodes, messages.shape[1], plan.num_edges
    out = torch.empty(n, d, dtype=torch.float32, device=messages.device)
    with _timed("segment_mul", bytes=E * (4.0 * d + 4) + n * 4.0 * d):
        rc = lib.ptgnn_amd_segment_mul_f32(msg.data_ptr() if E > 0 else None, _ld(msg) if E > 0 else d,
                                           plan.rowptr.data_ptr(), plan.perm.data_ptr(), n, E, d, out.data_ptr(), d,
                                           _stream(out))
    _lib.check(rc, "ptgnn_amd_segment_mul_f32")
    return out


def _egc_dims(coef: torch.Tensor, num_heads: int, num_bases: int, head_dim: int):
    K, B, Dh = int(num_heads), int(num_bases), int(head_dim)
    if K <= 0 or B <= 0 or Dh <= 0:
        raise _lib.PtgnnAmdError(f"EGC combine: bad heads / bases / head_dim ({K}, {B}, {Dh})")
    if coef.shape[1] != K * B:
        raise _lib.PtgnnAmdError(f"EGC combine: coefficients have {coef.shape[1]} columns, need heads*bases = {K * B}")
    return K, B, Dh


def gather_combine(ysrc: torch.Tensor, plan: GraphPlan, num_heads: int, num_bases: int, head_dim: int, reduce: str,
                   coef: torch.Tensor, type_bits: Optional[int] = None, col: Optional[torch.Tensor] = None,
                   return_agg: bool = False, return_arg: bool = False):
    """EGC aggregation with the head / basis combination as its row finish (ptgnn_amd_egc_gather_combine_f32):
        out[v, k*Dh + d] = sum_b coef[v, k*B + b] * (reduce_{slots of v} ysrc[src, t*M:(t+1)*M])[k*B*Dh + b*Dh + d]
    with M = heads * bases * head_dim; `ysrc` / `type_bits` / `col` as in `gather_reduce`.  Returns out, or
    (out, agg, arg) when `return_agg` (training: the aggregate and, for max / min with `return_arg`, its arg).  Message
    widths beyond one lane group's row aggregate with `gather_reduce` and combine with `basis_combine` (both HIP)."""
    lib = _lib.load()
    _require_cuda_f32("ysrc", ysrc)
    _require_cuda_f32("coef", coef)
    if reduce not in REDUCE_IDS:
        raise ValueError(f"unknown aggregation function {reduce!r}")
    K, B, Dh = _egc_dims(coef, num_heads, num_bases, head_dim)
    M, D, N = K * B * Dh, K * Dh, plan.num_nodes
    if return_arg and (not return_agg or REDUCE_IDS[reduce] < REDUCE_IDS["max"]):
        raise _lib.PtgnnAmdError("gather_combine: return_arg needs return_agg and max / min")
    ysrc, coef = _rowmajor(ysrc), _rowmajor(coef)
    if coef.shape[0] != N:
        raise _lib.PtgnnAmdError(f"gather_combine: coef has {coef.shape[0]} rows, the plan {N} nodes")
    out = torch.empty(N, D, dtype=torch.float32, device=ysrc.device)
    agg = torch.empty(N, M, dtype=torch.float32, device=ysrc.device) if return_agg else None
    arg = torch.empty(N, M, dtype=torch.int32, device=ysrc.device) if return_arg else None
    plan.wait()
    tb, colt = _slot_map(plan, type_bits, col)
    # algorithmic bytes: per edge one message row + its col entry; per node the coefficients, the output row, the rowptr
    # entry (and the aggregate / arg when asked for)
    nbytes = (plan.num_edges * (4.0 * M + 4) + N * (4.0 * (K * B + D) + 4)
              + (N * 4.0 * M if agg is not None else 0.0) + (N * 4.0 * M if arg is not None else 0.0))
    hub_ws, hub = _hub_args(plan, M, arg is not None, ysrc.device)
    with _timed("egc_gather_combine", bytes=nbytes):
        rc = lib.ptgnn_amd_egc_gather_combine_f32(
            _ptr_or(ysrc, plan.rowptr), _ld(ysrc), plan.rowptr.data_ptr(), colt.data_ptr(), tb, N, K, B, Dh,
            REDUCE_IDS[reduce], coef.data_ptr(), _ld(coef), out.data_ptr(), D,
            agg.data_ptr() if agg is not None else None, arg.data_ptr() if arg is not None else None,
            *hub, _stream(out))
    if rc == _lib.EUNSUPPORTED:
        res = gather_reduce(ysrc, plan, M, reduce, return_arg=return_arg, type_bits=tb, col=colt)
        agg, arg = res if return_arg else (res, None)
        out = basis_combine(agg, coef, K, B, Dh)
    else:
        _lib.check(rc, "ptgnn_amd_egc_gather_combine_f32")
    return (out, agg, arg) if return_agg else out


def basis_combine(agg: torch.Tensor, coef: torch.Tensor, num_heads: int, num_bases: int, head_dim: int) -> torch.Tensor:
    """out[v, k*Dh + d] = sum_b coef[v, k*B + b] * agg[v, k*B*Dh + b*Dh + d]  (ptgnn_amd_egc_combine_f32, any shape)."""
    lib = _lib.load()
    _require_cuda_f32("agg", agg)
    _require_cuda_f32("coef", coef)
    K, B, Dh = _egc_dims(coef, num_heads, num_bases, head_dim)
    agg, coef = _rowmajor(agg), _rowmajor(coef)
    n = agg.shape[0]
    if agg.shape[1] != K * B * Dh or coef.shape[0] != n:
        raise _lib.PtgnnAmdError(f"basis_combine: agg {tuple(agg.shape)} / coef {tuple(coef.shape)} do not match "
                                 f"({K}, {B}, {Dh})")
    out = torch.empty(n, K * Dh, dtype=torch.float32, device=agg.device)
    with _timed("egc_combine", bytes=4.0 * n * (K * B * Dh + K * B + K * Dh)):
        rc = lib.ptgnn_amd_egc_combine_f32(agg.data_ptr() if n else None, _ld(agg), coef.data_ptr() if n else None,
                                           _ld(coef), n, K, B, Dh, out.data_ptr() if n else None, K * Dh, _stream(out))
    _lib.check(rc, "ptgnn_amd_egc_combine_f32")
    return out


def basis_combine_backward(agg: torch.Tensor, coef: torch.Tensor, grad: torch.Tensor, num_heads: int, num_bases: int,
                           head_dim: int):
    """(grad_agg, grad_coef) of `basis_combine` in one pass (ptgnn_amd_egc_combine_backward_f32):
    grad_agg[v, k,b,d] = coef[v, k*B + b] * grad[v, k*Dh + d],  grad_coef[v, k*B + b] = sum_d agg[v, k,b,d] grad[v, k*Dh + d]."""
    lib = _lib.load()
    _require_cuda_f32("agg", agg)
    _require_cuda_f32("coef", coef)
    _require_cuda_f32("grad", grad)
    K, B, Dh = _egc_dims(coef, num_heads, num_bases, head_dim)
    agg, coef, grad = _rowmajor(agg), _rowmajor(coef), _rowmajor(grad)
    n = agg.shape[0]
    if agg.shape[1] != K * B * Dh or tuple(grad.shape) != (n, K * Dh) or coef.shape[0] != n:
        raise _lib.PtgnnAmdError(f"basis_combine_backward: agg {tuple(agg.shape)} / coef {tuple(coef.shape)} / grad "
                                 f"{tuple(grad.shape)} do not match ({K}, {B}, {Dh})")
    g_agg = torch.empty(n, K * B * Dh, dtype=torch.float32, device=agg.device)
    g_coef = torch.empty(n, K * B, dtype=torch.float32, device=agg.device)
    with _timed("egc_combine_backward", bytes=4.0 * n * (2 * K * B * Dh + K * Dh + 2 * K * B)):
        rc = lib.ptgnn_amd_egc_combine_backward_f32(
            agg.data_ptr() if n else None, _ld(agg), coef.data_ptr() if n else None, _ld(coef),
            grad.data_ptr() if n else None, _ld(grad), n, K, B, Dh, g_agg.data_ptr() if n else None, K * B * Dh,
            g_coef.data_ptr() if n else None, K * B, _stream(g_agg))
    _lib.check(rc, "ptgnn_amd_egc_combine_backward_f32")
    return g_agg, g_coef


PNA_ROUND = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def pna_aggregate(ysrc: torch.Tensor, plan: GraphPlan, msg_dim: int, delta: float = 1.0,
                  ydst: Optional[torch.Tensor] = None, type_bits: Optional[int] = None, col: Optional[torch.Tensor] = None,
                  epilogue: int = EPI_NONE, ln_weight: Optional[torch.Tensor] = None,
                  ln_bias: Optional[torch.Tensor] = None, ln_eps: float = 1e-5, return_arg: bool = False,
                  round_to: torch.dtype = torch.float32, agg_out: Optional[torch.Tensor] = None):
    """PNA aggregation (pna_aggregation.py:27-56) in one launch (ptgnn_amd_pna_aggregate_f32): per destination v
        A = [sum, mean, max, min, std] of the messages of v,  out = EPI([A | A*s | A*s'])   [N, 15 * msg_dim]
    with s = log(d + 1) / delta, s' = 1 / (s + 1e-3).  Messages as in `gather_reduce` (table form `ysrc` [+ `ydst`] or
    the edge form with col = plan.perm, type_bits = 0).  `epilogue` = EPI_GELU | EPI_LAYERNORM (msg_dim <= 256) fuses
    the MLP layer's activation and LayerNorm(15 * msg_dim).  `round_to` (float16 / bfloat16) rounds A to the message
    dtype before the scalers; `agg_out` (contiguous fp32 [N, 5 * msg_dim], no epilogue) then receives A unrounded, as
    the backward needs it.  Returns out, or (out, argmax, argmin) with `return_arg` (int32 [N, msg_dim] slots)."""
    lib = _lib.load()
    _require_cuda_f32("ysrc", ysrc)
    ysrc = _rowmajor(ysrc)
    ld_yd = _ld(ysrc)
    if ydst is not None:
        _require_cuda_f32("ydst", ydst)
        ydst = _rowmajor(ydst)
        ld_yd = _ld(ydst)
    if float(delta) == 0.0:
        raise _lib.PtgnnAmdError("pna_aggregate: delta must be non-zero")
    if round_to not in PNA_ROUND:
        raise _lib.PtgnnAmdError(f"pna_aggregate: messages of dtype {round_to} are not supported")
    M, N = int(msg_dim), plan.num_nodes
    out = torch.empty(N, 15 * M, dtype=torch.float32, device=ysrc.device)
    amax = torch.empty(N, M, dtype=torch.int32, device=ysrc.device) if return_arg else None
    amin = torch.empty(N, M, dtype=torch.int32, device=ysrc.device) if return_arg else None
    if epilogue & EPI_LAYERNORM:
        if ln_weight is None or ln_bias is None:
            raise _lib.PtgnnAmdError("pna_aggregate: the LayerNorm epilogue needs ln_weight and ln_bias")
        ln_weight, ln_bias = ln_weight.contiguous(), ln_bias.contiguous()
    if agg_out is not None and (tuple(agg_out.shape) != (N, 5 * M) or agg_out.dtype != torch.float32
                                or not agg_out.is_contiguous() or agg_out.device != ysrc.device):
        raise _lib.PtgnnAmdError(f"pna_aggregate: `agg_out` must be a contiguous float32 [{N}, {5 * M}] tensor")
    plan.wait()
    tb, colt = _slot_map(plan, type_bits, col)
    # algorithmic bytes: per edge one message row + its col entry; per node the rowptr entry, the 15M-wide output row
    # (and the destination-term row, the two arg rows)
    nbytes = (plan.num_edges * (4.0 * M + 4) + N * (60.0 * M + 4) + (N * 4.0 * M if ydst is not None else 0.0)
              + (N * 8.0 * M if return_arg else 0.0))
    with _timed("pna_aggregate", bytes=nbytes):
        rc = lib.ptgnn_amd_pna_aggregate_f32(
            _ptr_or(ysrc, plan.rowptr), _ld(ysrc), ydst.data_ptr() if ydst is not None else None, ld_yd,
            plan.rowptr.data_ptr(), colt.data_ptr(), tb, N, M, float(delta), int(epilogue),
            ln_weight.data_ptr() if ln_weight is not None else None,
            ln_bias.data_ptr() if ln_bias is not None else None, float(ln_eps), PNA_ROUND[round_to],
            out.data_ptr() if N else None, 15 * M, amax.data_ptr() if amax is not None and N else None,
            amin.data_ptr() if amin is not None and N else None,
            agg_out.data_ptr() if agg_out is not None and N else None, plan.num_edges, _stream(out))
    _lib.check(rc, "ptgnn_amd_pna_aggregate_f32")
    return (out, amax, amin) if return_arg else out


def pna_aggregate_backward(messages: torch.Tensor, plan: GraphPlan, agg: torch.Tensor, argmax: torch.Tensor,
                           argmin: torch.Tensor, grad: torch.Tensor, delta: float = 1.0,
                           round_to: torch.dtype = torch.float32) -> torch.Tensor:
    """Gradient of `pna_aggregate` (edge form) w.r.t. the [E, M] messages in message order, in one pass per row
    (ptgnn_amd_pna_aggregate_backward_f32).  `agg` holds the forward's UNROUNDED A in its first 5M columns: the
    forward's [N, 15M] output when it ran without rounding, else its `agg_out` [N, 5M].  `grad` = dL/dout [N, 15M];
    `round_to` as in the forward (the block gradients are then rounded as the reference's autograd rounds them)."""
    lib = _lib.load()
    for name, t in (("messages", messages), ("agg", agg), ("grad", grad)):
        _require_cuda_f32(name, t)
    messages, agg, grad = _rowmajor(messages), _rowmajor(agg), _rowmajor(grad)
    E, M, N = plan.num_edges, messages.shape[1], plan.num_nodes
    if round_to not in PNA_ROUND:
        raise _lib.PtgnnAmdError(f"pna_aggregate_backward: messages of dtype {round_to} are not supported")
    if messages.shape[0] != E or tuple(agg.shape) not in ((N, 5 * M), (N, 15 * M)) or tuple(grad.shape) != (N, 15 * M):
        raise _lib.PtgnnAmdError(f"pna_aggregate_backward: messages {tuple(messages.shape)} / agg {tuple(agg.shape)} / "
                                 f"grad {tuple(grad.shape)} do not match the plan ({N} nodes, {E} edges)")
    out = torch.empty(E, M, dtype=torch.float32, device=messages.device)
    if E == 0:
        return out
    plan.wait()
    nbytes = E * (3 * 4.0 * M + 8) + N * (4.0 * (15 * M + 2 * M) + 8.0 * M + 4)
    with _timed("pna_aggregate_backward", bytes=nbytes):
        rc = lib.ptgnn_amd_pna_aggregate_backward_f32(
            messages.data_ptr(), _ld(messages), plan.rowptr.data_ptr(), plan.perm.data_ptr(), N, M, float(delta),
            agg.data_ptr(), _ld(agg), argmax.contiguous().data_ptr(), argmin.contiguous().data_ptr(),
            grad.data_ptr(), _ld(grad), out.data_ptr(), M, PNA_ROUND[round_to], E, _stream(out))
    _lib.check(rc, "ptgnn_amd_pna_aggregate_backward_f32")
    return out


# The opt-in 16-bit matrix-core inputs (include/ptgnn_amd.h: ptgnn_amd_half_*; ptgnn_amd/precision.py is the switch the
# LAYERS read -- nothing here does: `inputs=` is explicit, because inside an autograd Function.forward grad mode is off
# and an op cannot tell inference from training).
HALF_IDS = {torch.bfloat16: 1, torch.float16: 2}     # PTGNN_AMD_HALF_BF16 / _F16
HALF_KIND_LINEAR, HALF_KIND_GRU = 0, 1               # PTGNN_AMD_HALF_KIND_*
HALF_KIND_WGRAD = 3                                  # PTGNN_AMD_HALF_KIND_WGRAD (id 2 stays an unknown kind)


def half_supported(kind: int, k_or_m: int, n_out_or_hd: int, dtype) -> bool:
    """Whether the 16-bit-input kernels take the shape (ptgnn_amd_half_supported; needs no device)."""
    if dtype not in HALF_IDS:
        return False
    return bool(_lib.load().ptgnn_amd_half_supported(kind, int(k_or_m), int(n_out_or_hd), HALF_IDS[dtype]))


def _half_inputs(inputs) -> Optional[torch.dtype]:
    """The `inputs=` keyword of linear / gru_cell / aggregate_gru: None and float32 mean the fp32 kernels."""
    if inputs is None or inputs == torch.float32:
        return None
    if inputs not in HALF_IDS:
        raise _lib.PtgnnAmdError(f"inputs must be None, torch.float32, torch.bfloat16 or torch.float16 (got {inputs!r})")
    return inputs


def _half_rows_ok(t: torch.Tensor) -> bool:
    """An fp32 operand the 16-bit kernels' fragment loads can read: 16-byte aligned rows."""
    return t.data_ptr() % 16 == 0 and _ld(t) % 4 == 0


def _rounded_weight(w: torch.Tensor, dtype: torch.dtype, given: Optional[torch.Tensor]) -> torch.Tensor:
    """`w` rounded to `dtype` by torch (round to nearest even), or the caller's cached copy of exactly that."""
    if given is None:
        return w.detach().to(dtype).contiguous()
    if given.dtype != dtype or given.shape != w.shape or given.device != w.device:
        raise _lib.PtgnnAmdError(f"rounded weight must be {dtype} {tuple(w.shape)} on {w.device} "
                                 f"(got {given.dtype} {tuple(given.shape)} on {given.device})")
    return given.contiguous()


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           act: Optional[str] = None, out: Optional[torch.Tensor] = None, inputs=None,
           rounded: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(x W^T + b) on fp32 MFMA.  weight is nn.Linear layout [n_out, k].
    `inputs` = torch.bfloat16 / torch.float16: x and the weight are rounded to that type and multiplied on the 16-bit
    matrix cores (fp32 accumulation and output) where `half_supported` takes the shape and x has 16-byte aligned rows;
    otherwise the fp32 kernel runs, silently.  `rounded`: the caller's `weight.to(inputs)`, to save the conversion."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    _require_cuda_f32("weight", weight)
    x, weight = _rowmajor(x), weight.contiguous()
    rows, k = x.shape
    n_out = weight.shape[0]
    if weight.shape[1] != k:
        raise _lib.PtgnnAmdError(f"linear: x has {k} columns but weight expects {weight.shape[1]}")
    if out is None:
        out = torch.empty(rows, n_out, dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = bias.contiguous()
    half = _half_inputs(inputs)
    if half is not None and half_supported(HALF_KIND_LINEAR, k, n_out, half) and _half_rows_ok(x):
        w16 = _rounded_weight(weight, half, rounded)
        with _timed("half_linear", flops=2.0 * rows * k * n_out, bytes=4.0 * rows * (k + n_out) + 2.0 * n_out * k):
            rc = lib.ptgnn_amd_half_linear(x.data_ptr(), rows, k, _ld(x), w16.data_ptr(), n_out,
                                           bias.data_ptr() if bias is not None else None, ACT_IDS[act],
                                           HALF_IDS[half], out.data_ptr(), _ld(out), _stream(out))
        _lib.check(rc, "ptgnn_amd_half_linear")
        return out
    with _timed("linear", flops=2.0 * rows * k * n_out, bytes=4.0 * (rows * k + n_out * k + rows * n_out)):
        rc = lib.ptgnn_amd_linear_f32(x.data_ptr(), rows, k, _ld(x), weight.data_ptr(), n_out,
                                      bias.data_ptr() if bias is not None else None, ACT_IDS[act],
                                      out.data_ptr(), _ld(out), _stream(out))
    _lib.check(rc, "ptgnn_amd_linear_f32")
    return out


def linear_add(x: torch.Tensor, weight: torch.Tensor, addend: torch.Tensor, bias: Optional[torch.Tensor] = None,
               act: Optional[str] = None, inputs=None, rounded: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x W^T + b) + addend.  One launch where the streaming GEMM takes the shape (the add rides its store epilogue:
    ptgnn_amd_linear_add_f32), else the GEMM followed by torch's add -- the same sum either way.
    `inputs` / `rounded`: as `linear` -- one launch of the 16-bit Linear with the fp32 addend in its store epilogue
    (ptgnn_amd_linear_add16) where `half_supported` takes the shape and x has 16-byte aligned rows; otherwise the fp32
    route, silently."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    _require_cuda_f32("weight", weight)
    _require_cuda_f32("addend", addend)
    x, weight, addend = _rowmajor(x), weight.contiguous(), _rowmajor(addend)
    rows, k = x.shape
    n_out = weight.shape[0]
    if weight.shape[1] != k or tuple(addend.shape) != (rows, n_out):
        raise _lib.PtgnnAmdError(f"linear_add: shapes x {tuple(x.shape)}, weight {tuple(weight.shape)}, addend "
                                 f"{tuple(addend.shape)} do not agree")
    out = torch.empty(rows, n_out, dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = bias.contiguous()
    half = _half_inputs(inputs)
    if half is not None and half_supported(HALF_KIND_LINEAR, k, n_out, half) and _half_rows_ok(x):
        w16 = _rounded_weight(weight, half, rounded)
        with _timed("half_linear_add", flops=2.0 * rows * k * n_out,
                    bytes=4.0 * rows * (k + 2 * n_out) + 2.0 * n_out * k):
            rc = lib.ptgnn_amd_linear_add16(x.data_ptr(), rows, k, _ld(x), w16.data_ptr(), n_out,
                                            bias.data_ptr() if bias is not None else None, ACT_IDS[act],
                                            HALF_IDS[half], addend.data_ptr(), _ld(addend), out.data_ptr(), _ld(out),
                                            _stream(out))
        _lib.check(rc, "ptgnn_amd_linear_add16")
        return out
    with _timed("linear", flops=2.0 * rows * k * n_out, bytes=4.0 * (rows * k + n_out * k + 2 * rows * n_out)):
        rc = lib.ptgnn_amd_linear_add_f32(x.data_ptr(), rows, k, _ld(x), weight.data_ptr(), n_out,
                                          bias.data_ptr() if bias is not None else None, ACT_IDS[act],
                                          addend.data_ptr(), _ld(addend), out.data_ptr(), _ld(out), _stream(out))
    if rc == _lib.EUNSUPPORTED:
        return linear(x, weight, bias, act=act, out=out).add_(addend)
    _lib.check(rc, "ptgnn_amd_linear_add_f32")
    return out


def dropout_bitmask(rows: int, width: int, p: float, seed: int, device) -> Optional[torch.Tensor]:
    """Keep mask of the per-edge dropout as one bit per element: int32 [rows, width / 32], bit b of word c = column
    32 c + b (ptgnn_amd_dropout_bitmask; the same hash of (seed, row, column) the seed-taking entry points evaluate).
    None when `width` is not a multiple of 32 (callers then stay on the hash form)."""
    if width % 32 != 0 or rows <= 0 or p <= 0.0:
        return None
    lib = _lib.load()
    bits = torch.empty(rows, width // 32, dtype=torch.int32, device=device)
    with _timed("dropout_bitmask", bytes=rows * width / 8.0):
        rc = lib.ptgnn_amd_dropout_bitmask(rows, width, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, bits.data_ptr(),
                                           _stream(bits))
    _lib.check(rc, "ptgnn_amd_dropout_bitmask")
    return bits


def edge_linear_masked_supported(state_dim: int, msg_dim: int, mode: int) -> bool:
    return bool(_lib.load().ptgnn_amd_edge_linear_masked_supported(int(state_dim), int(msg_dim), int(mode)))


def edge_weight_grad_masked_supported(state_dim: int, msg_dim: int) -> bool:
    return bool(_lib.load().ptgnn_amd_edge_weight_grad_masked_supported(int(state_dim), int(msg_dim)))


def edge_linear(x: torch.Tensor, adjacency_lists, weights: Sequence[torch.Tensor], use_dst: bool,
                act: Optional[str] = None, dropout: Optional[Tuple[int, float, int]] = None,
                mask_bits: Optional[torch.Tensor] = None,
                edge_feats: Optional[Sequence[Optional[torch.Tensor]]] = None, inputs=None,
                rounded: Optional[torch.Tensor] = None) -> torch.Tensor:
    """msg[off_t + e] = act([x[src_t[e]] ; x[dst_t[e]] (if use_dst)] W_t^T) for every edge type in one
    launch; rows in type-major message order.  weights[t] is the type's nn.Linear weight.
    `edge_feats[t]` = [E_t, F] per-edge feature rows appended to the message input (weights [M, H (+H) + F];
    gatedmessagepassing.py:57-61, mlpmessagepassing.py:96-98) -- see `_edge_linear_feat`.
    dropout = (mode, p, seed): nn.Dropout(p) on the gathered input rows (mode 1) or on the output rows
    (mode 2, the input-gradient form) with the hash mask of ptgnn_amd_edge_linear_dropout_f32; with
    `mask_bits` (`dropout_bitmask` of the same p and seed) the streaming kernel applies the mask from its bits.
    `inputs` / `rounded`: the 16-bit matrix-core form, as `edge_linear_shared` takes them; with `use_dst` the launch is
    ptgnn_amd_edge_dst_linear16 (`edge_linear16_dst_supported`; `rounded` is then the [T, M, 2 H] stack).  With
    `dropout` AND `mask_bits` (no target half) the launch is ptgnn_amd_edge_masked_linear16 where
    `edge_linear16_masked_supported` takes the shape -- mode 1 rounds (keep ? x * scale : 0), mode 2 masks and scales the
    fp32 accumulator -- and the fp32 masked route otherwise, silently.  With edge features, with dropout but no
    `mask_bits`, or with dropout and a target half, a 16-bit `inputs` raises, and with `use_dst` it wants GPU states."""
    half = _half_inputs(inputs)
    dropping = dropout is not None and dropout[0] != 0 and dropout[1] > 0.0
    if half is not None and edge_feats is not None and any(f is not None and f.shape[-1] > 0 for f in edge_feats):
        raise _lib.PtgnnAmdError("edge_linear: 16-bit inputs take neither dropout nor edge features")
    if half is not None and dropping and (use_dst or mask_bits is None):
        raise _lib.PtgnnAmdError("edge_linear: 16-bit inputs take dropout only as mask_bits (`dropout_bitmask`) and "
                                 "without a target-state half")
    if half is not None and use_dst and not x.is_cuda:
        raise _lib.PtgnnAmdError("edge_linear: 16-bit inputs with a target-state half run on the GPU kernel only "
                                 f"(got states on {x.device})")
    if edge_feats is not None and any(f is not None and f.shape[-1] > 0 for f in edge_feats):
        if dropout is not None and dropout[0] != 0 and dropout[1] > 0.0:
            raise _lib.PtgnnAmdError("edge_linear: the dropout forms take no edge features")
        return _edge_linear_feat(x, adjacency_lists, weights, use_dst, act, edge_feats)
    lib = _lib.load()
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    T = len(adjacency_lists)
    H = x.shape[1]
    M = weights[0].shape[0]
    counts = [int(a[0].shape[0]) for a in adjacency_lists]
    E = sum(counts)
    msg = torch.empty(max(E, 1), M, dtype=torch.float32, device=x.device)
    ws = [w.detach().contiguous() for w in weights]
    for w in ws:
        if tuple(w.shape) != (M, H * (2 if use_dst else 1)) or not w.is_cuda or w.dtype != torch.float32:
            raise _lib.PtgnnAmdError(f"edge_linear: weight shape {tuple(w.shape)} does not match "
                                     f"[{M}, {H * (2 if use_dst else 1)}]")
    srcs = [a[0].contiguous() for a in adjacency_lists]
    dsts = [a[1].contiguous() for a in adjacency_lists]
    PtrArr, CntArr = ctypes.c_void_p * T, ctypes.c_int64 * T
    sp = PtrArr(*[s.data_ptr() if s.numel() else None for s in srcs])
    cn = CntArr(*counts)
    if half is not None and use_dst and edge_linear16_dst_supported(H, M, T, half) and _half_rows_ok(x):
        w16 = _edge16_stack(ws, half, rounded)
        if any(d.numel() != c for d, c in zip(dsts, counts)):
            raise _lib.PtgnnAmdError("edge_linear: source and target id lists differ in length")
        dp = PtrArr(*[d.data_ptr() if d.numel() else None for d in dsts])
        with _timed("edge_linear16_dst", flops=4.0 * E * H * M,
                    bytes=4.0 * (2 * E * H + E * M) + 4.0 * T * M * H + 16.0 * E):
            rc = lib.ptgnn_amd_edge_dst_linear16(x.data_ptr(), _ld(x), x.shape[0], H,
                                                 ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(dp, ctypes.c_void_p),
                                                 ctypes.cast(cn, ctypes.c_void_p), w16.data_ptr(), T, M,
                                                 ACT_IDS[act], HALF_IDS[half], msg.data_ptr(), M, _stream(msg))
        _lib.check(rc, "ptgnn_amd_edge_dst_linear16")
        return msg[:E] if E > 0 else msg[:0]
    if (half is not None and dropping and not use_dst and act is None and mask_bits is not None and E > 0
            and edge_linear16_masked_supported(H, M, T, half, dropout[0]) and _half_rows_ok(x)):
        words = (M if dropout[0] == 2 else H) // 32
        if tuple(mask_bits.shape) != (E, words) or mask_bits.dtype != torch.int32 or not mask_bits.is_cuda:
            raise _lib.PtgnnAmdError(f"edge_linear: mask_bits must be int32 [{E}, {words}] on the device")
        mask_bits = mask_bits.contiguous()
        w16 = _edge16_stack(ws, half, rounded)
        with _timed("edge_linear16_masked", flops=2.0 * E * H * M,
                    bytes=4.0 * (E * H + E * M) + 2.0 * T * M * H + 8.0 * E + 4.0 * E * words):
            rc = lib.ptgnn_amd_edge_masked_linear16(x.data_ptr(), _ld(x), x.shape[0], H,
                                                    ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(cn, ctypes.c_void_p),
                                                    w16.data_ptr(), T, M, HALF_IDS[half], msg.data_ptr(), M,
                                                    int(dropout[0]), float(dropout[1]), mask_bits.data_ptr(),
                                                    _stream(msg))
        _lib.check(rc, "ptgnn_amd_edge_masked_linear16")
        return msg[:E]
    if half is not None and not dropping and not use_dst and edge_linear16_supported(H, M, T, half) and _half_rows_ok(x):
        w16 = _edge16_stack(ws, half, rounded)
        with _timed("edge_linear16", flops=2.0 * E * H * M, bytes=4.0 * (E * H + E * M) + 2.0 * T * M * H + 8.0 * E):
            rc = lib.ptgnn_amd_edge_linear16(x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p),
                                             ctypes.cast(cn, ctypes.c_void_p), w16.data_ptr(), T, M, ACT_IDS[act],
                                             HALF_IDS[half], msg.data_ptr(), M, _stream(msg))
        _lib.check(rc, "ptgnn_amd_edge_linear16")
        return msg[:E] if E > 0 else msg[:0]
    dp = PtrArr(*[d.data_ptr() if d.numel() else None for d in dsts])
    wp = PtrArr(*[w.data_ptr() for w in ws])
    K = H * (2 if use_dst else 1)
    if dropping:
        if use_dst or act is not None:
            raise _lib.PtgnnAmdError("edge_linear: dropout supports the GGNN form only (no target half, no act)")
        if mask_bits is not None and E > 0 and edge_linear_masked_supported(H, M, dropout[0]):
            words = (M if dropout[0] == 2 else H) // 32
            if tuple(mask_bits.shape) != (E, words) or mask_bits.dtype != torch.int32 or not mask_bits.is_cuda:
                raise _lib.PtgnnAmdError(f"edge_linear: mask_bits must be int32 [{E}, {words}] on the device")
            mask_bits = mask_bits.contiguous()
            with _timed("edge_linear", flops=2.0 * E * K * M, bytes=4.0 * (E * K + E * M + T * M * K) + 8.0 * E):
                rc = lib.ptgnn_amd_edge_linear_masked_f32(
                    x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p),
                    ctypes.cast(cn, ctypes.c_void_p), ctypes.cast(wp, ctypes.c_void_p), T, M, msg.data_ptr(), M,
                    int(dropout[0]), float(dropout[1]), mask_bits.data_ptr(), _stream(msg))
            if rc != _lib.EUNSUPPORTED:
                _lib.check(rc, "ptgnn_amd_edge_linear_masked_f32")
                return msg[:E]
            # the streaming kernel declined at run time (first use inside a graph capture, an operand that is not
            # 16-byte aligned, PTGNN_AMD_* developer switches): the seed form below evaluates the SAME hash inside the
            # tile kernels -- bit-identical mask -- and rewrites every output row
        with _timed("edge_linear", flops=2.0 * E * K * M, bytes=4.0 * (E * K + E * M + T * M * K) + 8.0 * E):
            rc = lib.ptgnn_amd_edge_linear_dropout_f32(
                x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p),
                ctypes.cast(cn, ctypes.c_void_p),
                ctypes.cast(wp, ctypes.c_void_p), T, M, msg.data_ptr(), M, int(dropout[0]),
                float(dropout[1]), int(dropout[2]) & 0xFFFFFFFFFFFFFFFF, _stream(msg))
        _lib.check(rc, "ptgnn_amd_edge_linear_dropout_f32")
        return msg[:E] if E > 0 else msg[:0]
    with _timed("edge_linear", flops=2.0 * E * K * M, bytes=4.0 * (E * K + E * M + T * M * K) + 8.0 * E):
        rc = lib.ptgnn_amd_edge_linear_f32(x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p),
                                           ctypes.cast(dp, ctypes.c_void_p) if use_dst else None,
                                           ctypes.cast(cn, ctypes.c_void_p),
                                           ctypes.cast(wp, ctypes.c_void_p), T, M, ACT_IDS[act],
                                           msg.data_ptr(), M, _stream(msg))
    _lib.check(rc, "ptgnn_amd_edge_linear_f32")
    return msg[:E] if E > 0 else msg[:0]


def _edge_linear_feat(x, adjacency_lists, weights, use_dst: bool, act, edge_feats) -> torch.Tensor:
    """The grouped per-edge GEMM with feature rows as a third K range of its A operand: nothing of the reference's
    [E, H (+H) + F] message input is materialised.  Feature widths that are not a multiple of 4 are zero-padded (the
    [E_t, F] block and the weight's feature columns: exact zeros in the products), so only the small block is copied."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    T = len(adjacency_lists)
    H, M = x.shape[1], weights[0].shape[0]
    Hs = H * (2 if use_dst else 1)
    counts = [int(a[0].shape[0]) for a in adjacency_lists]
    E = sum(counts)
    if len(edge_feats) != T:
        raise _lib.PtgnnAmdError(f"edge_linear: {len(edge_feats)} feature blocks for {T} edge types")
    F = max(int(f.shape[-1]) for f in edge_feats if f is not None)
    F4 = (F + 3) // 4 * 4
    feats, ws = [], []
    for t, (f, w, n) in enumerate(zip(edge_feats, weights, counts)):
        w = w.detach()
        if tuple(w.shape) != (M, Hs + F) or not w.is_cuda or w.dtype != torch.float32:
            raise _lib.PtgnnAmdError(f"edge_linear: weight shape {tuple(w.shape)} does not match [{M}, {Hs + F}]")
        if f is None or tuple(f.shape) != (n, F) or not f.is_cuda:
            raise _lib.PtgnnAmdError(f"edge_linear: features of type {t} must be a device tensor [{n}, {F}]")
        f = f.detach().float()
        if F4 != F:
            f = torch.nn.functional.pad(f, (0, F4 - F))
            w = torch.nn.functional.pad(w, (0, F4 - F))
        feats.append(f.contiguous())
        ws.append(w.contiguous())
    msg = torch.empty(max(E, 1), M, dtype=torch.float32, device=x.device)
    srcs = [a[0].contiguous() for a in adjacency_lists]
    dsts = [a[1].contiguous() for a in adjacency_lists]
    PtrArr, CntArr = ctypes.c_void_p * T, ctypes.c_int64 * T
    sp = PtrArr(*[s.data_ptr() if s.numel() else None for s in srcs])
    dp = PtrArr(*[d.data_ptr() if d.numel() else None for d in dsts])
    fp = PtrArr(*[f.data_ptr() if f.numel() else None for f in feats])
    wp = PtrArr(*[w.data_ptr() for w in ws])
    cn = CntArr(*counts)
    K = Hs + F
    with _timed("edge_linear_feat", flops=2.0 * E * K * M, bytes=4.0 * (E * K + E * M + T * M * K) + 8.0 * E):
        rc = lib.ptgnn_amd_edge_linear_feat_f32(
            x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p),
            ctypes.cast(dp, ctypes.c_void_p) if use_dst else None, ctypes.cast(fp, ctypes.c_void_p), F4, F4,
            ctypes.cast(cn, ctypes.c_void_p), ctypes.cast(wp, ctypes.c_void_p), T, M, ACT_IDS[act], msg.data_ptr(), M,
            _stream(msg))
    _lib.check(rc, "ptgnn_amd_edge_linear_feat_f32")
    return msg[:E] if E > 0 else msg[:0]


def edge_weight_grad(x: torch.Tensor, adjacency_lists, grad_msg: torch.Tensor, use_dst: bool,
                     dropout_p: float = 0.0, dropout_seed: int = 0,
                     mask_bits: Optional[torch.Tensor] = None, inputs=None) -> torch.Tensor:
    """grad_w[t] = grad_msg_t^T . [x[src_t] ; x[dst_t] (if use_dst)]  for all types -> [T, M, K].
    `mask_bits`: the dropout keep mask as bits (`dropout_bitmask` of the same p and seed) instead of the hash.
    `inputs` = torch.bfloat16 / torch.float16: both operands -- grad_msg and the gathered, masked, scaled x -- are rounded
    to that type in the kernel and multiplied on the 16-bit matrix cores (ptgnn_amd_edge_weight_grad16: fp32 accumulation
    and output, deterministic) where `edge_weight_grad16_supported` takes the shape, there is no target half, the rows are
    16-byte aligned and dropout (if any) comes with `mask_bits`; otherwise the fp32 kernels run, silently."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    _require_cuda_f32("grad_msg", grad_msg)
    x, grad_msg = _rowmajor(x), _rowmajor(grad_msg)
    T, H, M = len(adjacency_lists), x.shape[1], grad_msg.shape[1]
    K = H * (2 if use_dst else 1)
    counts = [int(a[0].shape[0]) for a in adjacency_lists]
    E = sum(counts)
    if grad_msg.shape[0] != E:
        raise _lib.PtgnnAmdError("edge_weight_grad: grad_msg rows != number of edges")
    srcs = [a[0].contiguous() for a in adjacency_lists]
    dsts = [a[1].contiguous() for a in adjacency_lists]
    PtrArr, CntArr = ctypes.c_void_p * T, ctypes.c_int64 * T
    sp = PtrArr(*[s.data_ptr() if s.numel() else None for s in srcs])
    dp = PtrArr(*[d.data_ptr() if d.numel() else None for d in dsts])
    cn = CntArr(*counts)
    grad_w = torch.empty(T, M, K, dtype=torch.float32, device=x.device)
    half = _half_inputs(inputs)
    if (half is not None and not use_dst and E > 0 and (dropout_p <= 0.0 or mask_bits is not None)
            and edge_weight_grad16_supported(H, M, T, half) and _half_rows_ok(x) and _half_rows_ok(grad_msg)):
        if dropout_p > 0.0:
            if tuple(mask_bits.shape) != (E, H // 32) or mask_bits.dtype != torch.int32 or not mask_bits.is_cuda:
                raise _lib.PtgnnAmdError(f"edge_weight_grad: mask_bits must be int32 [{E}, {H // 32}] on the device")
            mask_bits = mask_bits.contiguous()
        ws_bytes = lib.ptgnn_amd_edge_wgrad16_workspace_bytes(E, T, M, H)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
        # roofline bytes: the fp32 operand rows once, the ids, the mask, the result, and the partials written and read once
        with _timed("edge_weight_grad16", flops=2.0 * E * H * M,
                    bytes=4.0 * (E * H + E * M + T * M * H) + 8.0 * E + (E * H / 8.0 if dropout_p > 0.0 else 0.0)
                    + 2.0 * ws_bytes):
            rc = lib.ptgnn_amd_edge_weight_grad16(
                x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(cn, ctypes.c_void_p),
                grad_msg.data_ptr(), _ld(grad_msg), T, M, HALF_IDS[half], float(dropout_p),
                mask_bits.data_ptr() if dropout_p > 0.0 else None, grad_w.data_ptr(), ws.data_ptr(), ws_bytes,
                _stream(grad_w))
        _lib.check(rc, "ptgnn_amd_edge_weight_grad16")
        return grad_w
    ws_bytes = lib.ptgnn_amd_edge_wgrad_workspace_bytes(E, T, M, K)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
    gm_ptr = grad_msg.data_ptr() if E > 0 else x.data_ptr()
    if (mask_bits is not None and dropout_p > 0.0 and E > 0 and not use_dst
            and edge_weight_grad_masked_supported(H, M)):
        if tuple(mask_bits.shape) != (E, H // 32) or mask_bits.dtype != torch.int32 or not mask_bits.is_cuda:
            raise _lib.PtgnnAmdError(f"edge_weight_grad: mask_bits must be int32 [{E}, {H // 32}] on the device")
        mask_bits = mask_bits.contiguous()
        with _timed("edge_weight_grad", flops=2.0 * E * K * M, bytes=4.0 * (E * K + E * M + T * M * K) + 8.0 * E):
            rc = lib.ptgnn_amd_edge_weight_grad_masked_f32(
                x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p),
                ctypes.cast(cn, ctypes.c_void_p), gm_ptr, _ld(grad_msg), T, M, float(dropout_p),
                mask_bits.data_ptr(), grad_w.data_ptr(), ws.data_ptr(), ws_bytes, _stream(grad_w))
        if rc != _lib.EUNSUPPORTED:
            _lib.check(rc, "ptgnn_amd_edge_weight_grad_masked_f32")
            return grad_w
        # declined at run time (see edge_linear): the seed form computes the same mask from its hash
    with _timed("edge_weight_grad", flops=2.0 * E * K * M, bytes=4.0 * (E * K + E * M + T * M * K) + 8.0 * E):
        rc = lib.ptgnn_amd_edge_weight_grad_f32(
            x.data_ptr(), _ld(x), x.shape[0], H, ctypes.cast(sp, ctypes.c_void_p),
            ctypes.cast(dp, ctypes.c_void_p) if use_dst else None, ctypes.cast(cn, ctypes.c_void_p),
            gm_ptr, _ld(grad_msg) if E > 0 else M, T, M, float(dropout_p),
            int(dropout_seed) & 0xFFFFFFFFFFFFFFFF, grad_w.data_ptr(), ws.data_ptr(), ws_bytes, _stream(grad_w))
    _lib.check(rc, "ptgnn_amd_edge_weight_grad_f32")
    return grad_w


def linear_weight_grad(x: torch.Tensor, grad_y: torch.Tensor, want_bias: bool = False):
    """grad_w [n_out, k] = grad_y^T . x  (weight gradient of y = x W^T), deterministic split-row MFMA GEMM;
    with `want_bias` also grad_b [n_out] = column sums of grad_y from the same pass -> (grad_w, grad_b)."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    _require_cuda_f32("grad_y", grad_y)
    x, grad_y = _rowmajor(x), _rowmajor(grad_y)
    rows, k = x.shape
    n_out = grad_y.shape[1]
    if grad_y.shape[0] != rows:
        raise _lib.PtgnnAmdError("linear_weight_grad: x and grad_y row counts differ")
    if rows == 0:
        gw = torch.zeros(n_out, k, dtype=torch.float32, device=x.device)
        return (gw, torch.zeros(n_out, dtype=torch.float32, device=x.device)) if want_bias else gw
    grad_w = torch.empty(n_out, k, dtype=torch.float32, device=x.device)
    grad_b = torch.empty(n_out, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = lib.ptgnn_amd_edge_wgrad_workspace_bytes(rows, 1, n_out, k)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
    with _timed("linear_weight_grad", flops=2.0 * rows * k * n_out, bytes=4.0 * (rows * k + rows * n_out + n_out * k)):
        rc = lib.ptgnn_amd_linear_weight_grad_f32(x.data_ptr(), _ld(x), k, grad_y.data_ptr(), _ld(grad_y),
                                                  rows, n_out, grad_w.data_ptr(),
                                                  grad_b.data_ptr() if want_bias else None,
                                                  ws.data_ptr(), ws_bytes, _stream(grad_w))
    _lib.check(rc, "ptgnn_amd_linear_weight_grad_f32")
    return (grad_w, grad_b) if want_bias else grad_w


def half_wgrad_chunk_rows(rows: int, n_out: int, k: int) -> int:
    """Rows one workgroup partial of `half_linear_weight_grad` covers (ptgnn_amd_wgrad16_chunk_rows; needs no device);
    0 for a shape the 16-bit kernel does not take."""
    return int(_lib.load().ptgnn_amd_wgrad16_chunk_rows(int(rows), int(n_out), int(k)))


def half_linear_weight_grad(x: torch.Tensor, grad_y: torch.Tensor, dtype, want_bias: bool = False):
    """grad_w [n_out, k] = rnd(grad_y)^T . rnd(x) with both fp32 operands rounded to `dtype` (torch.bfloat16 /
    torch.float16) in the kernel, on the 16-bit matrix cores with fp32 accumulation (csrc/wgrad16.hip: deterministic
    two-stage reduction); with `want_bias` also grad_b [n_out] = column sums of the UNROUNDED fp32 grad_y from the same
    pass -> (grad_w, grad_b).  Where `half_supported(HALF_KIND_WGRAD, ...)` refuses the widths, or a row is not 16-byte
    aligned, or `dtype` is None / float32: `linear_weight_grad` on the unrounded operands, silently."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    _require_cuda_f32("grad_y", grad_y)
    x, grad_y = _rowmajor(x), _rowmajor(grad_y)
    rows, k = x.shape
    n_out = grad_y.shape[1]
    if grad_y.shape[0] != rows:
        raise _lib.PtgnnAmdError("half_linear_weight_grad: x and grad_y row counts differ")
    half = _half_inputs(dtype)
    if half is None or not half_supported(HALF_KIND_WGRAD, k, n_out, half) or not (_half_rows_ok(x)
                                                                                   and _half_rows_ok(grad_y)):
        return linear_weight_grad(x, grad_y, want_bias=want_bias)
    if rows == 0:
        gw = torch.zeros(n_out, k, dtype=torch.float32, device=x.device)
        return (gw, torch.zeros(n_out, dtype=torch.float32, device=x.device)) if want_bias else gw
    grad_w = torch.empty(n_out, k, dtype=torch.float32, device=x.device)
    grad_b = torch.empty(n_out, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = lib.ptgnn_amd_wgrad16_workspace_bytes(rows, n_out, k)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
    # roofline bytes: the fp32 operand rows once, the result, and the partial tiles written and read once
    with _timed("half_linear_weight_grad", flops=2.0 * rows * k * n_out,
                bytes=4.0 * (rows * k + rows * n_out + n_out * k) + 2.0 * ws_bytes):
        rc = lib.ptgnn_amd_linear_weight_grad16(x.data_ptr(), _ld(x), k, grad_y.data_ptr(), _ld(grad_y), rows, n_out,
                                                HALF_IDS[half], grad_w.data_ptr(),
                                                grad_b.data_ptr() if want_bias else None, ws.data_ptr(), ws_bytes,
                                                _stream(grad_w))
    _lib.check(rc, "ptgnn_amd_linear_weight_grad16")
    return (grad_w, grad_b) if want_bias else grad_w


def segment_spread(grad: torch.Tensor, arg: Optional[torch.Tensor], plan: GraphPlan) -> torch.Tensor:
    """Backward of `segment_reduce` w.r.t. the messages: [N, D] row gradients -> [E, D] in message order
    (max/min: only the recorded winner slot of each (row, column) receives the gradient)."""
    lib = _lib.load()
    _require_cuda_f32("grad", grad)
    grad = _rowmajor(grad)
    E, D = plan.num_edges, grad.shape[1]
    out = torch.empty(E, D, dtype=torch.float32, device=grad.device)
    if E == 0:
        return out
    if arg is not None:
        arg = arg.contiguous()
    plan.wait()
    with _timed("segment_spread", bytes=E * (4.0 * D + 8) + plan.num_nodes * 4.0 * D * (2 if arg is not None else 1)):
        rc = lib.ptgnn_amd_segment_spread_f32(grad.data_ptr(), _ld(grad),
                                              arg.data_ptr() if arg is not None else None,
                                              plan.slot_rows().data_ptr(), plan.perm.data_ptr(), E, D,
                                              out.data_ptr(), D, _stream(out))
    _lib.check(rc, "ptgnn_amd_segment_spread_f32")
    return out


def row_epilogue(x: torch.Tensor, flags: int, ln_weight: Optional[torch.Tensor] = None,
                 ln_bias: Optional[torch.Tensor] = None, ln_eps: float = 1e-5) -> torch.Tensor:
    """y = LayerNorm(GELU(x)) over the rows of x (`flags`: EPI_GELU | EPI_LAYERNORM) -- the training-time twin of
    the fused aggregation epilogue (mlpmessagepassing.py:114-116)."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    n, d = x.shape
    y = torch.empty(n, d, dtype=torch.float32, device=x.device)
    if flags & EPI_LAYERNORM:
        ln_weight, ln_bias = ln_weight.contiguous(), ln_bias.contiguous()
    with _timed("row_epilogue", bytes=8.0 * n * d):
        rc = lib.ptgnn_amd_row_epilogue_f32(x.data_ptr(), _ld(x), n, d, flags,
                                            ln_weight.data_ptr() if flags & EPI_LAYERNORM else None,
                                            ln_bias.data_ptr() if flags & EPI_LAYERNORM else None, float(ln_eps),
                                            y.data_ptr(), d, _stream(y))
    _lib.check(rc, "ptgnn_amd_row_epilogue_f32")
    return y


def row_epilogue_backward(x: torch.Tensor, grad_y: torch.Tensor, flags: int, ln_weight: Optional[torch.Tensor] = None,
                          ln_eps: float = 1e-5):
    """(grad_x, grad_gamma, grad_beta) of `row_epilogue`; the last two are None without LayerNorm."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    _require_cuda_f32("grad_y", grad_y)
    x, grad_y = _rowmajor(x), _rowmajor(grad_y)
    n, d = x.shape
    gx = torch.empty(n, d, dtype=torch.float32, device=x.device)
    ln = bool(flags & EPI_LAYERNORM)
    gg = gb = ws = None
    ws_bytes = 0
    if ln:
        ln_weight = ln_weight.contiguous()
        gg = torch.empty(d, dtype=torch.float32, device=x.device)
        gb = torch.empty(d, dtype=torch.float32, device=x.device)
        ws_bytes = int(lib.ptgnn_amd_row_epilogue_workspace_bytes(n, d))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
    with _timed("row_epilogue_backward", bytes=12.0 * n * d):
        rc = lib.ptgnn_amd_row_epilogue_backward_f32(x.data_ptr(), _ld(x), grad_y.data_ptr(), _ld(grad_y), n, d, flags,
                                                     ln_weight.data_ptr() if ln else None, float(ln_eps),
                                                     gx.data_ptr(), d, gg.data_ptr() if ln else None,
                                                     gb.data_ptr() if ln else None,
                                                     ws.data_ptr() if ln else None, ws_bytes, _stream(gx))
    _lib.check(rc, "ptgnn_amd_row_epilogue_backward_f32")
    return gx, gg, gb


def act_dropout_backward(grad: torch.Tensor, y: torch.Tensor, keep: Optional[torch.Tensor], scale: float,
                         act: Optional[str], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad * (keep ? scale : 0) * act'(y) in one pass (ptgnn_amd_act_dropout_backward_f32); `y` is the activation's
    output, `keep` the dropout's bool mask or None; `out`: optional contiguous fp32 destination of grad's size (the
    rows of a gradient frame)."""
    lib = _lib.load()
    _require_cuda_f32("grad", grad)
    grad, y = grad.contiguous(), y.contiguous()
    n = grad.numel()
    if out is None:
        out = torch.empty_like(grad)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n):
        raise _lib.PtgnnAmdError("act_dropout_backward: out must be a contiguous float32 CUDA tensor of grad's size")
    if keep is not None:
        keep = keep.contiguous()
        if keep.dtype != torch.bool or keep.numel() != n:
            raise _lib.PtgnnAmdError("act_dropout_backward: keep must be a bool mask of grad's shape")
    with _timed("act_dropout_backward", bytes=(12.0 + (1.0 if keep is not None else 0.0)) * n):
        rc = lib.ptgnn_amd_act_dropout_backward_f32(grad.data_ptr(), y.data_ptr(),
                                                    keep.data_ptr() if keep is not None else None, float(scale),
                                                    ACT_IDS[act], n, out.data_ptr(), _stream(out))
    _lib.check(rc, "ptgnn_amd_act_dropout_backward_f32")
    return out


def gru_cell(a: torch.Tensor, h: torch.Tensor, w_ih, w_hh, b_ih, b_hh, out: Optional[torch.Tensor] = None,
             inputs=None, rounded=None) -> torch.Tensor:
    """`out`: optional caller-owned [n, hd] fp32 destination with unit inner stride (e.g. the right half of the
    buffer a concat residual returns).
    `inputs` = torch.bfloat16 / torch.float16: a, h and both weights are rounded to that type in the gate GEMMs (16-bit
    matrix cores; fp32 accumulation, gate math and blend with the unrounded h) where `half_supported` takes the widths
    and a, h have 16-byte aligned rows; otherwise the fp32 cell runs, silently.  `rounded`: the caller's
    (w_ih.to(inputs), w_hh.to(inputs))."""
    lib = _lib.load()
    _require_cuda_f32("a", a)
    _require_cuda_f32("h", h)
    a, h = _rowmajor(a), _rowmajor(h)
    n, m = a.shape
    hd = h.shape[1]
    if out is None:
        out = torch.empty(n, hd, dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != (n, hd) or out.dtype != torch.float32 or out.stride(1) != 1 or not out.is_cuda:
        raise _lib.PtgnnAmdError(f"gru_cell: `out` must be a float32 CUDA [{n}, {hd}] view with unit inner stride")
    half = _half_inputs(inputs)
    if half is not None and half_supported(HALF_KIND_GRU, m, hd, half) and _half_rows_ok(a) and _half_rows_ok(h):
        given = rounded if rounded is not None else (None, None)
        wi16, wh16 = _rounded_weight(w_ih, half, given[0]), _rounded_weight(w_hh, half, given[1])
        with _timed("half_gru_cell", flops=2.0 * n * 3 * hd * (m + hd), bytes=4.0 * n * (m + 2 * hd) + 6.0 * hd * (m + hd)):
            rc = lib.ptgnn_amd_half_gru_cell(a.data_ptr(), _ld(a), h.data_ptr(), _ld(h), wi16.data_ptr(), wh16.data_ptr(),
                                             b_ih.contiguous().data_ptr(), b_hh.contiguous().data_ptr(), n, m, hd,
                                             HALF_IDS[half], out.data_ptr(), _ld(out), _stream(out))
        _lib.check(rc, "ptgnn_amd_half_gru_cell")
        return out
    with _timed("gru_cell", flops=2.0 * n * 3 * hd * (m + hd), bytes=4.0 * (n * (m + 2 * hd) + 3 * hd * (m + hd))):
        rc = lib.ptgnn_amd_gru_cell_f32(a.data_ptr(), _ld(a), h.data_ptr(), _ld(h),
                                        w_ih.contiguous().data_ptr(), w_hh.contiguous().data_ptr(),
                                        b_ih.contiguous().data_ptr(), b_hh.contiguous().data_ptr(),
                                        n, m, hd, out.data_ptr(), _ld(out), _stream(out))
    _lib.check(rc, "ptgnn_amd_gru_cell_f32")
    return out


# Aggregation -> GRU of one GGNN layer, pipelined over destination-row ranges (round 5; OFF by default -- it measured
# slower).  The aggregation is latency / HBM-bound (cfg3: 73-76 us, most wave cycles waiting on memory), the fused GRU cell
# MFMA-bound (191-240 us), and after the aggregation the layer is row-wise (gatedmessagepassing.py:63-69): row range i
# of the GRU only needs row range i of the aggregate.  So the ranges' aggregations can run back to back on a side stream
# while the main stream runs the GRU of the ranges that are done.  Same kernels, same per-row arithmetic: bit-identical to
# the unsplit pair (tests/test_gpu_pipeline.py).  Measured on the cfg3 headline step (profiles/r05_notes.md 1): 3.93 ms
# unsplit, 4.19 ms with 2 ranges, 4.25 with 3, 4.36 with 4 -- the persistent GRU workgroups hold every CU's LDS and most
# of its wave slots, so the co-resident aggregation crawls (99 us per HALF against 76 us for the whole matrix alone) and
# each extra GRU launch pays its weight-slab fill again (2 x 136 us against 240 us).  PTGNN_AMD_AGG_PIPELINE = number of row
# ranges (default 1 = the unsplit pair).
AGG_PIPELINE = int(os.environ.get("PTGNN_AMD_AGG_PIPELINE", "1"))
AGG_PIPELINE_MIN_ROWS = int(os.environ.get("PTGNN_AMD_AGG_PIPELINE_MIN_ROWS", "65536"))


def aggregate_gru(ysrc: torch.Tensor, plan: GraphPlan, msg_dim: int, reduce: str, h: torch.Tensor, w_ih, w_hh, b_ih,
                  b_hh, type_bits: Optional[int] = None, col: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, inputs=None, rounded=None) -> torch.Tensor:
    """GRUCell(aggregate(ysrc over plan), h) -- `gather_reduce` followed by `gru_cell`, pipelined over row ranges on
    large minibatches (see above).  `inputs` / `rounded`: as `gru_cell` (the 16-bit cell is row-independent, so the
    row ranges give the bits of one launch there too)."""
    N = plan.num_nodes
    pieces = AGG_PIPELINE
    if (pieces < 2 or N < AGG_PIPELINE_MIN_ROWS or N < 64 * pieces or torch.cuda.is_current_stream_capturing()):
        agg = gather_reduce(ysrc, plan, msg_dim, reduce, type_bits=type_bits, col=col)
        return gru_cell(agg, h, w_ih, w_hh, b_ih, b_hh, out=out, inputs=inputs, rounded=rounded)
    dev = h.device
    hd = h.shape[1]
    agg = torch.empty(N, msg_dim, dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty(N, hd, dtype=torch.float32, device=dev)
    bounds = [min(N, (N * i // pieces + 31) // 32 * 32) for i in range(pieces)] + [N]
    main, side = torch.cuda.current_stream(dev), _side_stream(dev)
    plan.wait()
    gather_reduce(ysrc, plan, msg_dim, reduce, type_bits=type_bits, col=col, out=agg, rows=(bounds[0], bounds[1]))
    first_done = torch.cuda.Event()
    first_done.record(main)
    ready = []
    with torch.cuda.stream(side):
        side.wait_event(first_done)          # the ranges' aggregations never overlap each other (shared hub tickets)
        for i in range(1, pieces):
            gather_reduce(ysrc, plan, msg_dim, reduce, type_bits=type_bits, col=col, out=agg,
                          rows=(bounds[i], bounds[i + 1]))
            ev = torch.cuda.Event()
            ev.record(side)
            ready.append(ev)
    for i in range(pieces):
        if i > 0:
            main.wait_event(ready[i - 1])
        lo, hi = bounds[i], bounds[i + 1]
        if hi > lo:
            gru_cell(agg[lo:hi], h[lo:hi], w_ih, w_hh, b_ih, b_hh, out=out[lo:hi], inputs=inputs, rounded=rounded)
    return out


def gru_cell_train(a: torch.Tensor, h: torch.Tensor, w_ih, w_hh, b_ih, b_hh, inputs=None, rounded=None):
    """Fused GRU cell that also returns the gates the backward needs: (h', gates [n, 4*hd] = r|z|n|gh_n).
    `inputs` / `rounded`: as `gru_cell` -- the 16-bit cell in its training form (ptgnn_amd_gru_cell_train16): h' has
    the bits of `gru_cell(..., inputs=inputs)`, gates holds the fp32 values its gate math used."""
    lib = _lib.load()
    _require_cuda_f32("a", a)
    _require_cuda_f32("h", h)
    a, h = _rowmajor(a), _rowmajor(h)
    n, m = a.shape
    hd = h.shape[1]
    out = torch.empty(n, hd, dtype=torch.float32, device=a.device)
    gates = torch.empty(n, 4 * hd, dtype=torch.float32, device=a.device)
    half = _half_inputs(inputs)
    if half is not None and half_supported(HALF_KIND_GRU, m, hd, half) and _half_rows_ok(a) and _half_rows_ok(h):
        given = rounded if rounded is not None else (None, None)
        wi16, wh16 = _rounded_weight(w_ih, half, given[0]), _rounded_weight(w_hh, half, given[1])
        with _timed("half_gru_cell_train", flops=2.0 * n * 3 * hd * (m + hd),
                    bytes=4.0 * n * (m + 2 * hd + 4 * hd) + 6.0 * hd * (m + hd)):
            rc = lib.ptgnn_amd_gru_cell_train16(a.data_ptr(), _ld(a), h.data_ptr(), _ld(h), wi16.data_ptr(),
                                                wh16.data_ptr(), b_ih.contiguous().data_ptr(),
                                                b_hh.contiguous().data_ptr(), n, m, hd, HALF_IDS[half], out.data_ptr(),
                                                _ld(out), gates.data_ptr(), _stream(out))
        _lib.check(rc, "ptgnn_amd_gru_cell_train16")
        return out, gates
    with _timed("gru_cell", flops=2.0 * n * 3 * hd * (m + hd),
                bytes=4.0 * (n * (m + 2 * hd + 4 * hd) + 3 * hd * (m + hd))):
        rc = lib.ptgnn_amd_gru_cell_train_f32(a.data_ptr(), _ld(a), h.data_ptr(), _ld(h),
                                              w_ih.contiguous().data_ptr(), w_hh.contiguous().data_ptr(),
                                              b_ih.contiguous().data_ptr(), b_hh.contiguous().data_ptr(),
                                              n, m, hd, out.data_ptr(), hd, gates.data_ptr(), _stream(out))
    _lib.check(rc, "ptgnn_amd_gru_cell_train_f32")
    return out, gates


def gru_gates_backward(grad_out: torch.Tensor, gates: torch.Tensor, h: torch.Tensor):
    """Backward of the GRU gate math: (d_gi [n, 3hd], d_gh [n, 3hd], d_h_direct [n, hd])."""
    lib = _lib.load()
    _require_cuda_f32("grad_out", grad_out)
    _require_cuda_f32("h", h)
    grad_out, h = _rowmajor(grad_out), _rowmajor(h)
    n, hd = h.shape
    d_gi = torch.empty(n, 3 * hd, dtype=torch.float32, device=h.device)
    d_gh = torch.empty(n, 3 * hd, dtype=torch.float32, device=h.device)
    d_h = torch.empty(n, hd, dtype=torch.float32, device=h.device)
    with _timed("gru_gates_backward", bytes=4.0 * n * hd * 13):
        rc = lib.ptgnn_amd_gru_cell_backward_gates_f32(grad_out.data_ptr(), _ld(grad_out), gates.data_ptr(),
                                                       h.data_ptr(), _ld(h), n, hd, d_gi.data_ptr(),
                                                       d_gh.data_ptr(), d_h.data_ptr(), _stream(d_h))
    _lib.check(rc, "ptgnn_amd_gru_cell_backward_gates_f32")
    return d_gi, d_gh, d_h


def gather_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    if idx.dtype != torch.int64 or not idx.is_cuda:
        raise _lib.PtgnnAmdError("gather_rows: idx must be a CUDA int64 tensor")
    idx = idx.contiguous()
    out = torch.empty(idx.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
    rc = lib.ptgnn_amd_gather_rows_f32(x.data_ptr(), _ld(x), idx.data_ptr(), idx.shape[0],
                                       x.shape[1], out.data_ptr(), x.shape[1], _stream(out))
    _lib.check(rc, "ptgnn_amd_gather_rows_f32")
    return out


def weighted_pool(x: torch.Tensor, w: torch.Tensor, plan: GraphPlan) -> torch.Tensor:
    """out[g] = sum_{i in segment g} sigmoid(x_i . w) x_i over the plan of an element -> sample map
    (ptgnn_amd_weighted_pool_f32: WeightedSumVarSizedElementReduce, varsizedsummary.py:68-81, in one pass over x)."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    n, d = x.shape
    if n != plan.num_edges or w.numel() != d or plan.perm is None:
        raise _lib.PtgnnAmdError(f"weighted_pool: x {tuple(x.shape)}, w {tuple(w.shape)} do not fit a plan over "
                                 f"{plan.num_edges} elements")
    w = w.detach().reshape(-1).contiguous()
    G = plan.num_nodes
    out = torch.empty(G, d, dtype=torch.float32, device=x.device)
    ws_bytes = int(lib.ptgnn_amd_weighted_pool_workspace_bytes(G, n, d))
    ws = _workspace(ws_bytes, x.device)
    plan.wait()
    with _timed("weighted_pool", bytes=4.0 * (n * d + G * d + d) + 4.0 * n):
        rc = lib.ptgnn_amd_weighted_pool_f32(*_rows_arg(x, d), w.data_ptr(),
                                             plan.rowptr.data_ptr(), plan.perm.data_ptr(), G, n, d, out.data_ptr(), d,
                                             ws.data_ptr(), ws_bytes, _stream(out))
    _lib.check(rc, "ptgnn_amd_weighted_pool_f32")
    return out


def weighted_pool_backward(x: torch.Tensor, w: torch.Tensor, index: torch.Tensor, grad_out: torch.Tensor):
    """(grad_x [n, d], grad_w [d]) of `weighted_pool` from grad_out [G, d] and the int64 element -> sample map."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    _require_cuda_f32("grad_out", grad_out)
    x, grad_out = _rowmajor(x), _rowmajor(grad_out)
    n, d = x.shape
    if index.dtype != torch.int64 or not index.is_cuda or index.shape[0] != n:
        raise _lib.PtgnnAmdError("weighted_pool_backward: the map must be a CUDA int64 tensor with one entry per element")
    index = index.contiguous()
    w = w.detach().reshape(-1).contiguous()
    gx = torch.empty(n, d, dtype=torch.float32, device=x.device)
    gw = torch.empty(d, dtype=torch.float32, device=x.device)
    ws_bytes = int(lib.ptgnn_amd_weighted_pool_backward_workspace_bytes(n, d))
    ws = _workspace(ws_bytes, x.device)
    with _timed("weighted_pool_backward", bytes=4.0 * (3 * n * d) + 8.0 * n):
        rc = lib.ptgnn_amd_weighted_pool_backward_f32(*_rows_arg(x, d), w.data_ptr(),
                                                      index.data_ptr() if n else None,
                                                      *_rows_arg(grad_out, d), n, d,
                                                      gx.data_ptr() if n else None, d, gw.data_ptr(), ws.data_ptr(),
                                                      ws_bytes, _stream(gx))
    _lib.check(rc, "ptgnn_amd_weighted_pool_backward_f32")
    return gx, gw


def attention_pool_supported(dim: int, num_heads: int) -> bool:
    """Whether the fused attention pool takes (dim, heads) (ptgnn_amd_attention_pool_supported: heads <= 8, dim <= 1024)."""
    return bool(_lib.load().ptgnn_amd_attention_pool_supported(int(dim), int(num_heads)))


def _attention_pool_args(x: torch.Tensor, u: torch.Tensor, plan: GraphPlan, what: str):
    _require_cuda_f32("x", x)
    _require_cuda_f32("u", u, dims=3)
    x = _rowmajor(x)
    n, d = x.shape
    G, H = plan.num_nodes, u.shape[1]
    if n != plan.num_edges or tuple(u.shape) != (G, H, d) or plan.perm is None:
        raise _lib.PtgnnAmdError(f"{what}: x {tuple(x.shape)}, u {tuple(u.shape)} do not fit a plan of "
                                 f"{plan.num_edges} elements in {G} samples")
    return x, u.contiguous(), n, d, G, H


def attention_pool(x: torch.Tensor, u: torch.Tensor, plan: GraphPlan):
    """Multi-head segment-softmax pool over the plan of an element -> sample map (ptgnn_amd_attention_pool_f32):
        s[i,h] = u[g(i),h] . x_i,   p = softmax of s[., h] within each sample,   P[g,h] = sum_{i in g} p[i,h] x_i
    in one pass over x.  Returns (P [G, heads, D], stats [G, 2 * heads] = per-(g, h) max score | log-sum-exp)."""
    lib = _lib.load()
    x, u, n, d, G, H = _attention_pool_args(x, u, plan, "attention_pool")
    out = torch.empty(G, H, d, dtype=torch.float32, device=x.device)
    stats = torch.empty(G, 2 * H, dtype=torch.float32, device=x.device)
    if G == 0:
        return out, stats
    ws_bytes = int(lib.ptgnn_amd_attention_pool_workspace_bytes(G, n, d, H))
    ws = _workspace(ws_bytes, x.device)
    plan.wait()
    with _timed("attention_pool", bytes=4.0 * (n * d + 2 * G * H * d) + 4.0 * n):
        rc = lib.ptgnn_amd_attention_pool_f32(*_rows_arg(x, d), u.data_ptr(),
                                              plan.rowptr.data_ptr(), plan.perm.data_ptr() if n else None, G, n, d, H,
                                              out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes, _stream(out))
    _lib.check(rc, "ptgnn_amd_attention_pool_f32")
    return out, stats


def attention_pool_backward(x: torch.Tensor, u: torch.Tensor, plan: GraphPlan, pooled: torch.Tensor,
                            stats: torch.Tensor, grad_out: torch.Tensor):
    """(grad_x [n, D], grad_u [G, heads, D]) of `attention_pool` from grad_out = dL/dP [G, heads, D] and the forward's P
    and stats (ptgnn_amd_attention_pool_backward_f32: one pass over x, grad_u folded in a fixed order)."""
    lib = _lib.load()
    x, u, n, d, G, H = _attention_pool_args(x, u, plan, "attention_pool_backward")
    _require_cuda_f32("grad_out", grad_out, dims=3)
    pooled, stats, grad_out = pooled.contiguous(), stats.contiguous(), grad_out.contiguous()
    if tuple(grad_out.shape) != (G, H, d) or tuple(pooled.shape) != (G, H, d) or tuple(stats.shape) != (G, 2 * H):
        raise _lib.PtgnnAmdError(f"attention_pool_backward: grad_out {tuple(grad_out.shape)} / pooled "
                                 f"{tuple(pooled.shape)} / stats {tuple(stats.shape)} do not match ({G}, {H}, {d})")
    gx = torch.empty(n, d, dtype=torch.float32, device=x.device)
    gu = torch.empty(G, H, d, dtype=torch.float32, device=x.device)
    if G == 0:
        return gx, gu
    ws_bytes = int(lib.ptgnn_amd_attention_pool_backward_workspace_bytes(G, n, d, H))
    ws = _workspace(ws_bytes, x.device)
    plan.wait()
    with _timed("attention_pool_backward", bytes=4.0 * (2 * n * d + 4 * G * H * d) + 4.0 * n):
        rc = lib.ptgnn_amd_attention_pool_backward_f32(
            *_rows_arg(x, d), u.data_ptr(), plan.rowptr.data_ptr(),
            plan.perm.data_ptr() if n else None, G, n, d, H, pooled.data_ptr(), stats.data_ptr(), grad_out.data_ptr(),
            gx.data_ptr() if n else None, d, gu.data_ptr(), ws.data_ptr(), ws_bytes, _stream(gu))
    _lib.check(rc, "ptgnn_amd_attention_pool_backward_f32")
    return gx, gu


def segment_scores_supported(dim: int, num_vectors: int) -> bool:
    """Whether the fused segment scores take (dim, vectors) (ptgnn_amd_segment_scores_supported: vectors <= 8,
    dim <= 1024)."""
    return bool(_lib.load().ptgnn_amd_segment_scores_supported(int(dim), int(num_vectors)))


def _segment_scores_args(y: torch.Tensor, v: torch.Tensor, plan: GraphPlan, what: str):
    _require_cuda_f32("y", y)
    _require_cuda_f32("v", v, dims=3)
    y = _rowmajor(y)
    n, k = y.shape
    G, L = plan.num_nodes, v.shape[1]
    if n != plan.num_edges or tuple(v.shape) != (G, L, k) or plan.perm is None:
        raise _lib.PtgnnAmdError(f"{what}: y {tuple(y.shape)}, v {tuple(v.shape)} do not fit a plan of "
                                 f"{plan.num_edges} elements in {G} samples")
    return y, v.contiguous(), n, k, G, L


def segment_scores(y: torch.Tensor, v: torch.Tensor, plan: GraphPlan):
    """Scores of every element against the vectors of its sample over the plan of an element -> sample map, and their
    per-sample log-sum-exp (ptgnn_amd_segment_scores_f32):
        scores[i,l] = v[g(i),l] . y_i,   lse[g,l] = log sum_{i in g} exp(scores[i,l])   (-inf for an empty sample)
    in one pass over y.  Returns (scores [n, L] in element order, lse [G, L])."""
    lib = _lib.load()
    y, v, n, k, G, L = _segment_scores_args(y, v, plan, "segment_scores")
    scores = torch.empty(n, L, dtype=torch.float32, device=y.device)
    lse = torch.empty(G, L, dtype=torch.float32, device=y.device)
    ws_bytes = int(lib.ptgnn_amd_segment_scores_workspace_bytes(G, n, k, L))
    ws = _workspace(ws_bytes, y.device)
    plan.wait()
    with _timed("segment_scores", bytes=4.0 * (n * k + n * L + G * L * (k + 1)) + 4.0 * n):
        rc = lib.ptgnn_amd_segment_scores_f32(*_rows_arg(y, k), v.data_ptr() if G else None, plan.rowptr.data_ptr(),
                                              plan.perm.data_ptr() if n else None, G, n, k, L,
                                              scores.data_ptr() if n else None, lse.data_ptr() if G else None,
                                              ws.data_ptr(), ws_bytes, _stream(lse))
    _lib.check(rc, "ptgnn_amd_segment_scores_f32")
    return scores, lse


def segment_scores_backward(y: torch.Tensor, v: torch.Tensor, plan: GraphPlan, scores: torch.Tensor, lse: torch.Tensor,
                            grad_scores: torch.Tensor, grad_lse: torch.Tensor):
    """(grad_y [n, K], grad_v [G, L, K]) of `segment_scores` from grad_scores [n, L], grad_lse [G, L] and the forward's
    scores and lse (ptgnn_amd_segment_scores_backward_f32: one pass over y, grad_v folded in a fixed order)."""
    lib = _lib.load()
    y, v, n, k, G, L = _segment_scores_args(y, v, plan, "segment_scores_backward")
    _require_cuda_f32("grad_scores", grad_scores)
    _require_cuda_f32("grad_lse", grad_lse)
    scores, lse, grad_scores, grad_lse = (t.contiguous() for t in (scores, lse, grad_scores, grad_lse))
    if tuple(scores.shape) != (n, L) or tuple(grad_scores.shape) != (n, L) or tuple(lse.shape) != (G, L) \
            or tuple(grad_lse.shape) != (G, L):
        raise _lib.PtgnnAmdError(f"segment_scores_backward: scores {tuple(scores.shape)} / grad_scores "
                                 f"{tuple(grad_scores.shape)} / lse {tuple(lse.shape)} / grad_lse "
                                 f"{tuple(grad_lse.shape)} do not match ({n}, {L}) and ({G}, {L})")
    gy = torch.empty(n, k, dtype=torch.float32, device=y.device)
    gv = torch.empty(G, L, k, dtype=torch.float32, device=y.device)
    ws_bytes = int(lib.ptgnn_amd_segment_scores_backward_workspace_bytes(G, n, k, L))
    ws = _workspace(ws_bytes, y.device)
    plan.wait()
    with _timed("segment_scores_backward", bytes=4.0 * (2 * n * k + 2 * n * L + 2 * G * L * (k + 1)) + 4.0 * n):
        rc = lib.ptgnn_amd_segment_scores_backward_f32(
            *_rows_arg(y, k), v.data_ptr() if G else None, plan.rowptr.data_ptr(),
            plan.perm.data_ptr() if n else None, G, n, k, L, scores.data_ptr() if n else None,
            lse.data_ptr() if G else None, grad_scores.data_ptr() if n else None,
            grad_lse.data_ptr() if G else None, gy.data_ptr() if n else None, k, gv.data_ptr() if G else None,
            ws.data_ptr(), ws_bytes, _stream(gv))
    _lib.check(rc, "ptgnn_amd_segment_scores_backward_f32")
    return gy, gv


BAG_MODES = {"sum": 0, "mean": 1, "max": 2}


def embedding_bag_supported(dim: int, slots: int) -> bool:
    """Whether the fused embedding bag takes (dim, slots) (ptgnn_amd_embedding_bag_supported: dim % 4 == 0,
    4 <= dim <= 1024, slots <= 32)."""
    return bool(_lib.load().ptgnn_amd_embedding_bag_supported(int(dim), int(slots)))


def _embedding_bag_args(table: torch.Tensor, ids: torch.Tensor, lengths: torch.Tensor, mode: str, what: str):
    _require_cuda_f32("table", table)
    if mode not in BAG_MODES:
        raise ValueError(f"unknown subtoken combination {mode!r}")
    for name, t, dims in (("ids", ids, 2), ("lengths", lengths, 1)):
        if not t.is_cuda or t.dtype != torch.int64 or t.dim() != dims:
            raise _lib.PtgnnAmdError(f"{what}: {name} must be a {dims}-D CUDA int64 tensor")
    if lengths.shape[0] != ids.shape[0]:
        raise _lib.PtgnnAmdError(f"{what}: {lengths.shape[0]} lengths for {ids.shape[0]} bags")
    return _rowmajor(table), ids.contiguous(), lengths.contiguous()


def embedding_bag(table: torch.Tensor, ids: torch.Tensor, lengths: torch.Tensor, mode: str, return_arg: bool = False):
    """out[b] = sum / mean / max of table[ids[b, s]] over the slots s < lengths[b] (ptgnn_amd_embedding_bag_f32: the pool of
    SubtokenUnitEmbedder without the [B, S, D] tensor).  `return_arg` (max): also the int32 [B, D] winning slots."""
    lib = _lib.load()
    table, ids, lengths = _embedding_bag_args(table, ids, lengths, mode, "embedding_bag")
    (B, S), (V, D) = ids.shape, table.shape
    out = torch.empty(B, D, dtype=torch.float32, device=table.device)
    arg = torch.empty(B, D, dtype=torch.int32, device=table.device) if return_arg and mode == "max" else None
    with _timed("embedding_bag", bytes=B * (8.0 * S + 8) + 4.0 * min(B * S, V) * D + 4.0 * B * D * (2 if arg is not None else 1)):
        rc = lib.ptgnn_amd_embedding_bag_f32(table.data_ptr() if V else None, _ld(table), V, ids.data_ptr() if B else None,
                                             lengths.data_ptr() if B else None, B, S, D, BAG_MODES[mode],
                                             out.data_ptr() if B else None, D,
                                             arg.data_ptr() if arg is not None and B else None, _stream(out))
    _lib.check(rc, "ptgnn_amd_embedding_bag_f32")
    return (out, arg) if return_arg else out


def embedding_bag_plan(ids: torch.Tensor, lengths: torch.Tensor, vocabulary_size: int) -> GraphPlan:
    """The backward plan of a bag: its elements as (bag, token) edges (ptgnn_amd_embedding_bag_keys), stably sorted by token
    with the dead slots keyed to the extra row `vocabulary_size` (which no launch walks)."""
    lib = _lib.load()
    B, S = ids.shape
    src = torch.empty(max(B * S, 1), dtype=torch.int64, device=ids.device)
    key = torch.empty(max(B * S, 1), dtype=torch.int64, device=ids.device)
    rc = lib.ptgnn_amd_embedding_bag_keys(ids.data_ptr() if B else None, lengths.data_ptr() if B else None, B, S,
                                          int(vocabulary_size), src.data_ptr(), key.data_ptr(), _stream(src))
    _lib.check(rc, "ptgnn_amd_embedding_bag_keys")
    return build_plan([(src[:B * S], key[:B * S])], int(vocabulary_size) + 1, num_src_rows=max(B, 1))


def embedding_bag_backward(grad: torch.Tensor, ids: torch.Tensor, lengths: torch.Tensor, mode: str, vocabulary_size: int,
                           arg: Optional[torch.Tensor] = None, plan: Optional[GraphPlan] = None) -> torch.Tensor:
    """dL/dtable [V, D] of `embedding_bag` from grad = dL/dout [B, D] (ptgnn_amd_embedding_bag_backward_f32): a segment sum
    over the bag's plan (`embedding_bag_plan`, built here when not given), every vocabulary row folded in element order;
    `arg`: the forward's winning slots (max)."""
    lib = _lib.load()
    _require_cuda_f32("grad", grad)
    grad = _rowmajor(grad)
    _, ids, lengths = _embedding_bag_args(grad, ids, lengths, mode, "embedding_bag_backward")
    (B, S), D, V = ids.shape, grad.shape[1], int(vocabulary_size)
    if grad.shape[0] != B:
        raise _lib.PtgnnAmdError(f"embedding_bag_backward: grad {tuple(grad.shape)} for {B} bags")
    if mode == "max":
        if arg is None or tuple(arg.shape) != (B, D) or arg.dtype != torch.int32 or not arg.is_cuda:
            raise _lib.PtgnnAmdError("embedding_bag_backward: max needs the forward's int32 [B, D] arg")
        arg = arg.contiguous()
    out = torch.empty(V, D, dtype=torch.float32, device=grad.device)
    if V == 0:
        return out
    if not embedding_bag_supported(D, S):     # before the plan build: an unsupported shape does no device work
        raise _lib.PtgnnAmdError(f"embedding_bag_backward: dim {D} / {S} slots outside the kernel range")
    if plan is None:
        plan = embedding_bag_plan(ids, lengths, V)
    if plan.num_nodes != V + 1 or plan.num_edges != B * S:
        raise _lib.PtgnnAmdError("embedding_bag_backward: the plan is not this bag's")
    plan.wait()
    ws_bytes = int(lib.ptgnn_amd_embedding_bag_backward_workspace_bytes(B, S, D, BAG_MODES[mode]))
    ws = _workspace(ws_bytes, grad.device)
    hub_ws, hub = _hub_args(plan, D, False, grad.device)
    with _timed("embedding_bag_backward", bytes=B * S * (4.0 * D + 4) + V * (4.0 * D + 4)):
        rc = lib.ptgnn_amd_embedding_bag_backward_f32(
            grad.data_ptr() if B else None, _ld(grad) if B else D, lengths.data_ptr() if B else None,
            arg.data_ptr() if mode == "max" and B else None, B, S, V, D, BAG_MODES[mode], plan.rowptr.data_ptr(),
            plan.col.data_ptr(), plan.perm.data_ptr(), out.data_ptr(), D, *hub[1:], ws.data_ptr(), ws_bytes, _stream(out))
    _lib.check(rc, "ptgnn_amd_embedding_bag_backward_f32")
    return out


# ------------------------------------------------------------------------------------------------
# char-CNN embedder (csrc/char_conv.hip and the windowed GEMM entries)
# ------------------------------------------------------------------------------------------------
def char_embed_supported(num_chars: int, window: int, dim: int) -> bool:
    """Whether the char-embed kernels take the shape (ptgnn_amd_char_embed_supported: dim % 4 == 0, 4 <= dim <= 1024,
    window <= 16, a table tile of (window * num_chars + 1) x 64 floats within one CU's LDS)."""
    return bool(_lib.load().ptgnn_amd_char_embed_supported(int(num_chars), int(window), int(dim)))


def char_embed_backward_chunk() -> int:
    """Samples per chunk of the char-embed backward (ptgnn_amd_char_embed_backward_chunk)."""
    return int(_lib.load().ptgnn_amd_char_embed_backward_chunk())


def _char_args(chars: torch.Tensor, table: torch.Tensor, window: int, what: str):
    _require_cuda_f32("table", table)
    if not chars.is_cuda or chars.dtype != torch.int64 or chars.dim() != 2:
        raise _lib.PtgnnAmdError(f"{what}: chars must be a 2-D CUDA int64 tensor")
    window = int(window)
    if window < 1 or table.shape[0] % window != 0 or chars.shape[1] < window:
        raise _lib.PtgnnAmdError(f"{what}: a [{table.shape[0]}, {table.shape[1]}] table and {chars.shape[1]} chars do not "
                                 f"fit a window of {window}")
    return chars.contiguous(), table.contiguous(), window, table.shape[0] // window


def _frame_rows(frame: torch.Tensor, first_row: int, rows: int, what: str) -> torch.Tensor:
    """The contiguous [rows, width] block of `frame` that starts at `first_row` (the destination of a launch)."""
    if not frame.is_contiguous() or first_row < 0 or first_row + rows > frame.shape[0]:
        raise _lib.PtgnnAmdError(f"{what}: rows [{first_row}, {first_row + rows}) are not inside a contiguous frame of "
                                 f"{frame.shape[0]} rows")
    return frame[first_row:first_row + rows]


def char_embed(chars: torch.Tensor, table: torch.Tensor, bias: Optional[torch.Tensor], window: int,
               act: Optional[str] = "relu", out: Optional[torch.Tensor] = None, out_first_row: int = 0) -> torch.Tensor:
    """a1[b R + p] = act(bias + sum_k table[k C + chars[b, p + k]]), R = L - window + 1 (ptgnn_amd_char_embed_f32: the first
    convolution of CharUnitEmbedder over its one-hot input as a table sum).  `out`: a contiguous frame whose rows
    [out_first_row, out_first_row + B R) receive the result (returned as a view); allocated when None."""
    lib = _lib.load()
    chars, table, window, C = _char_args(chars, table, window, "char_embed")
    (B, L), D = chars.shape, table.shape[1]
    R = L - window + 1
    if out is None:
        out, out_first_row = torch.empty(B * R, D, dtype=torch.float32, device=table.device), 0
    _require_cuda_f32("out", out)
    dst = _frame_rows(out, int(out_first_row), B * R, "char_embed")
    if dst.shape[1] != D:
        raise _lib.PtgnnAmdError(f"char_embed: the frame has {dst.shape[1]} columns, the table {D}")
    if bias is not None:
        _require_cuda_f32("bias", bias, 1)
        if bias.shape[0] != D:
            raise _lib.PtgnnAmdError(f"char_embed: a bias of {bias.shape[0]} entries for {D} columns")
        bias = bias.contiguous()
    with _timed("char_embed", bytes=8.0 * B * L + 4.0 * table.numel() + 4.0 * B * R * D):
        rc = lib.ptgnn_amd_char_embed_f32(chars.data_ptr() if B else None, B, L, C, window, table.data_ptr(),
                                          bias.data_ptr() if bias is not None else None, D, ACT_IDS[act],
                                          dst.data_ptr() if B else None, D, _stream(out))
    _lib.check(rc, "ptgnn_amd_char_embed_f32")
    return dst


def char_embed_backward(grad: torch.Tensor, a1: Optional[torch.Tensor], chars: torch.Tensor, num_chars: int, window: int,
                        act: Optional[str] = "relu", want_bias: bool = True):
    """(d table [window C, D], d bias [D] or None) of `char_embed` from grad = dL/da1 [B R, D] and the saved a1 (the ReLU
    mask a1 > 0; not read for act None): ptgnn_amd_char_embed_backward_f32, deterministic."""
    lib = _lib.load()
    _require_cuda_f32("grad", grad)
    grad = _rowmajor(grad)
    D = grad.shape[1]
    if not chars.is_cuda or chars.dtype != torch.int64 or chars.dim() != 2:
        raise _lib.PtgnnAmdError("char_embed_backward: chars must be a 2-D CUDA int64 tensor")
    chars = chars.contiguous()
    B, L = chars.shape
    window, C = int(window), int(num_chars)
    R = L - window + 1
    relu = ACT_IDS[act] != 0
    if R < 1 or grad.shape[0] != B * R:
        raise _lib.PtgnnAmdError(f"char_embed_backward: grad {tuple(grad.shape)} for {B} samples of {R} rows")
    if relu:
        _require_cuda_f32("a1", a1)
        a1 = _rowmajor(a1)
        if tuple(a1.shape) != (B * R, D):
            raise _lib.PtgnnAmdError(f"char_embed_backward: a1 {tuple(a1.shape)} is not grad's shape")
    g_table = torch.empty(window * C, D, dtype=torch.float32, device=grad.device)
    g_bias = torch.empty(D, dtype=torch.float32, device=grad.device) if want_bias else None
    ws_bytes = int(lib.ptgnn_amd_char_embed_backward_workspace_bytes(B, C, window, D))
    ws = _workspace(ws_bytes, grad.device)
    with _timed("char_embed_backward", bytes=8.0 * B * R * D + 8.0 * B * L + 2.0 * ws_bytes):
        rc = lib.ptgnn_amd_char_embed_backward_f32(grad.data_ptr() if B else None, _ld(grad) if B else D,
                                                   a1.data_ptr() if relu and B else None, _ld(a1) if relu and B else D,
                                                   chars.data_ptr() if B else None, B, L, C, window, D, ACT_IDS[act],
                                                   g_table.data_ptr(), g_bias.data_ptr() if want_bias else None,
                                                   ws.data_ptr(), ws_bytes, _stream(g_table))
    _lib.check(rc, "ptgnn_amd_char_embed_backward_f32")
    return g_table, g_bias


def _window_frame(x: torch.Tensor, first_row: int, rows: int, window: int, what: str):
    _require_cuda_f32("x", x)
    first_row, rows, window = int(first_row), int(rows), int(window)
    if not x.is_contiguous():
        raise _lib.PtgnnAmdError(f"{what}: the frame must be contiguous (a window spans packed rows; a strided view would "
                                 "have to be copied)")
    if window < 1 or rows < 0 or first_row < 0 or first_row + rows + window - 1 > x.shape[0]:
        raise _lib.PtgnnAmdError(f"{what}: rows [{first_row}, {first_row + rows}) with a window of {window} reach outside "
                                 f"the frame's {x.shape[0]} rows")
    return first_row, rows, window


def window_linear(x: torch.Tensor, first_row: int, rows: int, window: int, weight: torch.Tensor,
                  bias: Optional[torch.Tensor] = None, act: Optional[str] = None, out: Optional[torch.Tensor] = None,
                  out_first_row: int = 0) -> torch.Tensor:
    """y[r] = act(W . x[first_row + r .. first_row + r + window - 1] + b) for r < rows (ptgnn_amd_window_linear_f32): a
    Conv1d over the channel-last frame `x` [T, c_in] (the frame itself and the window, not an as_strided view), weight
    [n_out, window * c_in].  `out`: a contiguous frame whose rows [out_first_row, out_first_row + rows) receive y."""
    lib = _lib.load()
    first_row, rows, window = _window_frame(x, first_row, rows, window, "window_linear")
    _require_cuda_f32("weight", weight)
    weight = weight.contiguous()
    c_in, n_out = x.shape[1], weight.shape[0]
    if weight.shape[1] != window * c_in:
        raise _lib.PtgnnAmdError(f"window_linear: weight {tuple(weight.shape)} for a window of {window} x {c_in} columns")
    if out is None:
        out, out_first_row = torch.empty(rows, n_out, dtype=torch.float32, device=x.device), 0
    _require_cuda_f32("out", out)
    dst = _frame_rows(out, int(out_first_row), rows, "window_linear")
    if dst.shape[1] != n_out:
        raise _lib.PtgnnAmdError(f"window_linear: the output frame has {dst.shape[1]} columns, the weight {n_out} rows")
    if bias is not None:
        _require_cuda_f32("bias", bias, 1)
        if bias.shape[0] != n_out:
            raise _lib.PtgnnAmdError(f"window_linear: a bias of {bias.shape[0]} entries for {n_out} output columns")
        bias = bias.contiguous()
    k = window * c_in
    with _timed("linear", flops=2.0 * rows * k * n_out, bytes=4.0 * (rows * c_in + n_out * k + rows * n_out)):
        rc = lib.ptgnn_amd_window_linear_f32(x[first_row:].data_ptr() if rows else None, rows, c_in, window, c_in,
                                             weight.data_ptr(), n_out, bias.data_ptr() if bias is not None else None,
                                             ACT_IDS[act], dst.data_ptr() if rows else None, n_out, _stream(out))
    _lib.check(rc, "ptgnn_amd_window_linear_f32")
    return dst


def window_weight_grad(x: torch.Tensor, first_row: int, rows: int, window: int, grad_y: torch.Tensor,
                       want_bias: bool = False):
    """grad_w [n_out, window * c_in] = sum_r grad_y[r]^T . x[first_row + r .. + window - 1] (and grad_b = column sums of
    grad_y with `want_bias`): the weight gradient of `window_linear` (ptgnn_amd_window_weight_grad_f32)."""
    lib = _lib.load()
    first_row, rows, window = _window_frame(x, first_row, rows, window, "window_weight_grad")
    _require_cuda_f32("grad_y", grad_y)
    grad_y = _rowmajor(grad_y)
    c_in, n_out = x.shape[1], grad_y.shape[1]
    if grad_y.shape[0] != rows:
        raise _lib.PtgnnAmdError("window_weight_grad: grad_y does not have `rows` rows")
    k = window * c_in
    if rows == 0:
        gw = torch.zeros(n_out, k, dtype=torch.float32, device=x.device)
        return (gw, torch.zeros(n_out, dtype=torch.float32, device=x.device)) if want_bias else gw
    grad_w = torch.empty(n_out, k, dtype=torch.float32, device=x.device)
    grad_b = torch.empty(n_out, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = lib.ptgnn_amd_edge_wgrad_workspace_bytes(rows, 1, n_out, k)
    ws = _workspace(ws_bytes, x.device)
    with _timed("linear_weight_grad", flops=2.0 * rows * k * n_out, bytes=4.0 * (rows * c_in + rows * n_out + n_out * k)):
        rc = lib.ptgnn_amd_window_weight_grad_f32(x[first_row:].data_ptr(), rows, c_in, window, grad_y.data_ptr(),
                                                  _ld(grad_y), n_out, grad_w.data_ptr(),
                                                  grad_b.data_ptr() if want_bias else None, ws.data_ptr(), ws_bytes,
                                                  _stream(grad_w))
    _lib.check(rc, "ptgnn_amd_window_weight_grad_f32")
    return (grad_w, grad_b) if want_bias else grad_w


def window_max(x: torch.Tensor, first_row: int, num_samples: int, rows_per_sample: int, valid: int,
               return_arg: bool = False):
    """out[b] = max over the first `valid` of the `rows_per_sample` rows of sample b, which start at row `first_row` of the
    frame `x` (ptgnn_amd_window_max_f32); `return_arg`: also the int32 [B, D] lowest winning positions."""
    lib = _lib.load()
    _require_cuda_f32("x", x)
    B, R, D = int(num_samples), int(rows_per_sample), x.shape[1]
    src = _frame_rows(x, int(first_row), B * R, "window_max")
    out = torch.empty(B, D, dtype=torch.float32, device=x.device)
    arg = torch.empty(B, D, dtype=torch.int32, device=x.device) if return_arg else None
    with _timed("window_max", bytes=4.0 * B * int(valid) * D + 4.0 * B * D * (2 if return_arg else 1)):
        rc = lib.ptgnn_amd_window_max_f32(src.data_ptr() if B else None, D, B, R, int(valid), D,
                                          out.data_ptr() if B else None, D,
                                          arg.data_ptr() if return_arg and B else None, _stream(out))
    _lib.check(rc, "ptgnn_amd_window_max_f32")
    return (out, arg) if return_arg else out


def window_max_backward(grad: torch.Tensor, arg: torch.Tensor, rows_per_sample: int, out: Optional[torch.Tensor] = None,
                        out_first_row: int = 0) -> torch.Tensor:
    """The [B R, D] gradient rows of `window_max` (ptgnn_amd_window_max_backward_f32): grad[b, d] at row arg[b, d] of
    sample b, exact zeros elsewhere; written into rows [out_first_row, out_first_row + B R) of the frame `out`."""
    lib = _lib.load()
    _require_cuda_f32("grad", grad)
    grad = _rowmajor(grad)
    (B, D), R = grad.shape, int(rows_per_sample)
    if not arg.is_cuda or arg.dtype != torch.int32 or tuple(arg.shape) != (B, D):
        raise _lib.PtgnnAmdError("window_max_backward: arg must be the forward's int32 [B, D] positions")
    arg = arg.contiguous()
    if out is None:
        out, out_first_row = torch.empty(B * R, D, dtype=torch.float32, device=grad.device), 0
    _require_cuda_f32("out", out)
    dst = _frame_rows(out, int(out_first_row), B * R, "window_max_backward")
    if dst.shape[1] != D:
        raise _lib.PtgnnAmdError(f"window_max_backward: the frame has {dst.shape[1]} columns, grad {D}")
    with _timed("window_max_backward", bytes=4.0 * B * R * D + 8.0 * B * D):
        rc = lib.ptgnn_amd_window_max_backward_f32(grad.data_ptr() if B else None, _ld(grad) if B else D,
                                                   arg.data_ptr() if B else None, B, R, D,
                                                   dst.data_ptr() if B else None, D, _stream(out))
    _lib.check(rc, "ptgnn_amd_window_max_backward_f32")
    return dst


def graph_norm_supported(dim: int) -> bool:
    """Whether the fused GraphNorm takes `dim` columns (ptgnn_amd_graph_norm_supported: dim <= 1024)."""
    return bool(_lib.load().ptgnn_amd_graph_norm_supported(int(dim)))


def _graph_norm_args(x: torch.Tensor, params, plan: GraphPlan, what: str):
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    n, d = x.shape
    if d % 4 == 0 and (x.data_ptr() % 16 or (n > 1 and x.stride(0) % 4)):
        x = x.contiguous()     # float4 rows whenever the width allows: one chunk layout per width
    if n != plan.num_edges or plan.perm is None or any(p.numel() != d for p in params):
        raise _lib.PtgnnAmdError(f"{what}: x {tuple(x.shape)} and parameters of {[p.numel() for p in params]} entries do "
                                 f"not fit a plan of {plan.num_edges} elements")
    flat = []
    for name, p in zip(("gamma", "alpha", "bias"), params):
        if not p.is_cuda or p.dtype != torch.float32:
            raise _lib.PtgnnAmdError(f"{what}: {name} must be a float32 GPU tensor (got {p.dtype} on {p.device})")
        flat.append(p.detach().reshape(-1).contiguous())
    return x, flat, n, d, plan.num_nodes


def graph_norm(x: torch.Tensor, gamma: torch.Tensor, alpha: torch.Tensor, bias: torch.Tensor, eps: float,
               plan: GraphPlan, with_mean: bool = False):
    """GraphNorm over the plan of the node -> graph map (ptgnn_amd_graph_norm_f32; graphnorm.py:36-46 in three reads of x
    and one write of y): y [n, D], and with `with_mean` also the per-graph means [G, D], which `graph_norm_backward`
    takes."""
    lib = _lib.load()
    x, (gamma, alpha, bias), n, d, G = _graph_norm_args(x, (gamma, alpha, bias), plan, "graph_norm")
    y = torch.empty(n, d, dtype=torch.float32, device=x.device)
    mean = torch.empty(G, d, dtype=torch.float32, device=x.device) if with_mean else None
    if G > 0:
        ws_bytes = int(lib.ptgnn_amd_graph_norm_workspace_bytes(G, n, d))
        ws = _workspace(ws_bytes, x.device)
        plan.wait()
        with _timed("graph_norm", bytes=4.0 * (4 * n * d) + 3 * 4.0 * n):
            rc = lib.ptgnn_amd_graph_norm_f32(*_rows_arg(x, d), gamma.data_ptr(),
                                              alpha.data_ptr(), bias.data_ptr(), float(eps), plan.rowptr.data_ptr(),
                                              plan.perm.data_ptr() if n else None, G, n, d,
                                              y.data_ptr() if n else None, d,
                                              mean.data_ptr() if with_mean else None, ws.data_ptr(), ws_bytes,
                                              _stream(y))
        _lib.check(rc, "ptgnn_amd_graph_norm_f32")
    return (y, mean) if with_mean else y


def graph_norm_backward(x: torch.Tensor, grad_y: torch.Tensor, gamma: torch.Tensor, alpha: torch.Tensor, eps: float,
                        mean: torch.Tensor, plan: GraphPlan):
    """(grad_x [n, D], grad_gamma [D], grad_alpha [D], grad_bias [D]) of `graph_norm` from grad_y = dL/dy and the
    forward's eps and per-graph means (ptgnn_amd_graph_norm_backward_f32: two reads of (x, grad_y), one write of grad_x; per-graph
    arithmetic in float64; deterministic)."""
    lib = _lib.load()
    x, (gamma, alpha), n, d, G = _graph_norm_args(x, (gamma, alpha), plan, "graph_norm_backward")
    _require_cuda_f32("grad_y", grad_y)
    grad_y = _rowmajor(grad_y)
    if d % 4 == 0 and (grad_y.data_ptr() % 16 or (n > 1 and grad_y.stride(0) % 4)):
        grad_y = grad_y.contiguous()
    mean = mean.contiguous()
    if tuple(grad_y.shape) != (n, d) or tuple(mean.shape) != (G, d) or mean.dtype != torch.float32:
        raise _lib.PtgnnAmdError(f"graph_norm_backward: grad_y {tuple(grad_y.shape)} / mean {tuple(mean.shape)} do not "
                                 f"match x {(n, d)} over {G} graphs")
    gx = torch.empty(n, d, dtype=torch.float32, device=x.device)
    gp = torch.empty(3, d, dtype=torch.float32, device=x.device)
    ws_bytes = int(lib.ptgnn_amd_graph_norm_backward_workspace_bytes(G, n, d))
    ws = _workspace(ws_bytes, x.device)
    plan.wait()
    with _timed("graph_norm_backward", bytes=4.0 * (5 * n * d) + 2 * 4.0 * n):
        rc = lib.ptgnn_amd_graph_norm_backward_f32(
            *_rows_arg(x, d), *_rows_arg(grad_y, d),
            gamma.data_ptr(), alpha.data_ptr(), float(eps), mean.data_ptr() if G else None, plan.rowptr.data_ptr(),
            plan.perm.data_ptr() if n else None, G, n, d, gx.data_ptr() if n else None, d, gp[0].data_ptr(),
            gp[1].data_ptr(), gp[2].data_ptr(), ws.data_ptr(), ws_bytes, _stream(gx))
    _lib.check(rc, "ptgnn_amd_graph_norm_backward_f32")
    return gx, gp[0], gp[1], gp[2]


# csrc/block_attention.hip: a workgroup owns 32, 64 or 128 rows of a window (1, 2 or 4 waves of 32 rows: the most whose
# LDS stays within 64 KiB at the given dk / dv) and walks the window in tiles of 32 rows
BLOCK_ATTENTION_ROW_TILES = (32, 64, 128)
BLOCK_ATTENTION_COL_TILE = 32


def block_attention_supported(dk: int, dv: int) -> bool:
    """Whether the fused block attention takes these key / value widths (ptgnn_amd_block_attention_supported: 1..128)."""
    return bool(_lib.load().ptgnn_amd_block_attention_supported(int(dk), int(dv)))


def block_attention16_supported(dk: int, dv: int, dtype) -> bool:
    """Whether the 16-bit-input block attention takes these widths and this dtype (ptgnn_amd_attention16_block_supported;
    needs no device)."""
    if dtype not in HALF_IDS:
        return False
    return bool(_lib.load().ptgnn_amd_attention16_block_supported(int(dk), int(dv), HALF_IDS[dtype]))


def attention_windows(plan: GraphPlan, max_num_nodes: int) -> torch.Tensor:
    """Window table of selfattmessagepassing.py:59-75 from the plan of a node -> graph map (ptgnn_amd_attention_windows):
    int32 [bound + 1], bound = ceil(N / max_num_nodes) + G.  Entry w is the first row of window w for the W windows of
    the batch (graph g owns the count_g rows after those of the graphs in front of it and is cut every max_num_nodes
    rows; only the counts of the map matter), the entries from W on are N.  No host read-back."""
    lib = _lib.load()
    G, n = int(plan.num_nodes), int(plan.num_edges)
    bound = int(lib.ptgnn_amd_attention_windows_bound(G, n, int(max_num_nodes)))
    if bound < 0:
        raise _lib.PtgnnAmdError(f"attention_windows: bad sizes (graphs {G}, rows {n}, max_num_nodes {max_num_nodes})")
    if G == 0:
        return torch.zeros(1, dtype=torch.int32, device=plan.rowptr.device)
    windows = torch.empty(bound + 1, dtype=torch.int32, device=plan.rowptr.device)
    plan.wait()
    rc = lib.ptgnn_amd_attention_windows(plan.rowptr.data_ptr(), G, n, int(max_num_nodes), windows.data_ptr(),
                                         bound + 1, _stream(windows))
    _lib.check(rc, "ptgnn_amd_attention_windows")
    return windows


def _block_attention_args(kqv: torch.Tensor, windows: torch.Tensor, heads: int, dk: int, dv: int, what: str):
    _require_cuda_f32("kqv", kqv)
    kqv = _rowmajor(kqv)
    if heads < 1 or dk < 1 or dv < 1 or kqv.shape[1] != heads * (2 * dk + dv):
        raise _lib.PtgnnAmdError(f"{what}: kqv {tuple(kqv.shape)} is not [N, {heads} * (2 * {dk} + {dv})]")
    if not block_attention_supported(dk, dv):
        raise _lib.PtgnnAmdError(f"{what}: key / value dimensions ({dk}, {dv}) outside the kernels' 1..128")
    if not windows.is_cuda or windows.dtype != torch.int32 or windows.dim() != 1 or windows.numel() < 1:
        raise _lib.PtgnnAmdError(f"{what}: windows must be the int32 GPU table of attention_windows")
    return kqv, windows.contiguous()


def block_attention(kqv: torch.Tensor, windows: torch.Tensor, max_num_nodes: int, heads: int, dk: int, dv: int,
                    p: float = 0.0, seed: int = 0, inputs=None):
    """Softmax attention among the rows of every window, per head (ptgnn_amd_block_attention_f32;
    selfattmessagepassing.py:104-117): kqv [N, heads (2 dk + dv)] read in place -> (out [N, heads dv], lse [N, heads]).
    `p` > 0 applies the hash dropout mask of `seed` to the probabilities (row r heads + h, column j of a
    [N heads, max_num_nodes rounded up to even] mask).
    `inputs` = torch.bfloat16 / torch.float16: keys, queries, values and the unnormalised probabilities are rounded to
    that type and both products run on the 16-bit matrix cores (ptgnn_amd_attention16_block: fp32 softmax, accumulation
    and output) where p == 0, `block_attention16_supported` takes the widths and kqv has 16-byte aligned rows; otherwise
    the fp32 kernel runs, silently."""
    lib = _lib.load()
    kqv, windows = _block_attention_args(kqv, windows, heads, dk, dv, "block_attention")
    n = kqv.shape[0]
    out = torch.empty(n, heads * dv, dtype=torch.float32, device=kqv.device)
    lse = torch.empty(n, heads, dtype=torch.float32, device=kqv.device)
    half = _half_inputs(inputs)
    if n and half is not None and p == 0 and block_attention16_supported(dk, dv, half) and _half_rows_ok(kqv):
        with _timed("block_attention16", bytes=4.0 * n * heads * (2 * dk + 2 * dv + 1)):
            rc = lib.ptgnn_amd_attention16_block(kqv.data_ptr(), _ld(kqv), windows.data_ptr(), windows.numel() - 1, n,
                                                 int(max_num_nodes), heads, dk, dv, out.data_ptr(), heads * dv,
                                                 lse.data_ptr(), HALF_IDS[half], _stream(out))
        _lib.check(rc, "ptgnn_amd_attention16_block")
        return out, lse
    if n:
        with _timed("block_attention", bytes=4.0 * n * heads * (2 * dk + 2 * dv + 1)):
            rc = lib.ptgnn_amd_block_attention_f32(kqv.data_ptr(), _ld(kqv), windows.data_ptr(), windows.numel() - 1, n,
                                                   int(max_num_nodes), heads, dk, dv, float(p), int(seed), out.data_ptr(),
                                                   heads * dv, lse.data_ptr(), _stream(out))
        _lib.check(rc, "ptgnn_amd_block_attention_f32")
    return out, lse


def block_attention_backward(kqv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, grad_out: torch.Tensor,
                             windows: torch.Tensor, max_num_nodes: int, heads: int, dk: int, dv: int, p: float = 0.0,
                             seed: int = 0) -> torch.Tensor:
    """grad_kqv [N, heads (2 dk + dv)] of `block_attention` from grad_out = dL/dout and the forward's out / lse
    (ptgnn_amd_block_attention_backward_f32: the probabilities are recomputed; deterministic, no float atomics)."""
    lib = _lib.load()
    kqv, windows = _block_attention_args(kqv, windows, heads, dk, dv, "block_attention_backward")
    n = kqv.shape[0]
    _require_cuda_f32("grad_out", grad_out)
    grad_out, out, lse = _rowmajor(grad_out), out.contiguous(), lse.contiguous()
    if tuple(grad_out.shape) != (n, heads * dv) or tuple(out.shape) != (n, heads * dv) or tuple(lse.shape) != (n, heads) \
            or out.dtype != torch.float32 or lse.dtype != torch.float32:
        raise _lib.PtgnnAmdError(f"block_attention_backward: grad_out {tuple(grad_out.shape)} / out {tuple(out.shape)} / "
                                 f"lse {tuple(lse.shape)} do not match kqv {tuple(kqv.shape)}")
    gkqv = torch.empty(n, heads * (2 * dk + dv), dtype=torch.float32, device=kqv.device)
    if n:
        ws_bytes = int(lib.ptgnn_amd_block_attention_backward_workspace_bytes(n, heads))
        ws = _workspace(ws_bytes, kqv.device)
        with _timed("block_attention_backward", bytes=4.0 * n * heads * (4 * dk + 5 * dv + 2)):
            rc = lib.ptgnn_amd_block_attention_backward_f32(
                kqv.data_ptr(), _ld(kqv), out.data_ptr(), heads * dv, lse.data_ptr(), grad_out.data_ptr(), _ld(grad_out),
                windows.data_ptr(), windows.numel() - 1, n, int(max_num_nodes), heads, dk, dv, float(p), int(seed),
                gkqv.data_ptr(), heads * (2 * dk + dv), ws.data_ptr(), ws_bytes, _stream(gkqv))
        _lib.check(rc, "ptgnn_amd_block_attention_backward_f32")
    return gkqv


HEAD_EXPAND, HEAD_CONTRACT, HEAD_WEIGHT_GRAD = 0, 1, 2    # modes of ptgnn_amd_head_projection_f32


def _head_projection(mode: int, a, b, w, rows: int, heads: int, head_dim: int, dim: int, scale: float,
                     out: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    with _timed("head_projection", flops=2.0 * rows * heads * head_dim * dim):
        rc = lib.ptgnn_amd_head_projection_f32(mode, a.data_ptr() if a is not None and a.numel() else None,
                                               b.data_ptr() if b is not None and b.numel() else None,
                                               w.data_ptr() if w is not None else None, rows, heads, head_dim, dim,
                                               float(scale), out.data_ptr() if out.numel() else None, _stream(out))
    _lib.check(rc, "ptgnn_amd_head_projection_f32")
    return out


def _head_dims(hidden: int, num_heads: int, what: str) -> Tuple[int, int]:
    H = int(num_heads)
    if H <= 0 or hidden % H:
        raise _lib.PtgnnAmdError(f"{what}: {hidden} columns do not split into {H} heads")
    return H, hidden // H


def head_expand(a: torch.Tensor, w: torch.Tensor, num_heads: int, scale: float = 1.0) -> torch.Tensor:
    """out[g, h, :] = scale * W[h*dk:(h+1)*dk, :]^T a[g, h*dk:(h+1)*dk]: a [G, hidden], W [hidden, D] -> [G, heads, D]
    (the key projection of the queries, varsizedsummary.py:151-158 moved onto the samples)."""
    _require_cuda_f32("a", a)
    _require_cuda_f32("w", w)
    a, w = a.contiguous(), w.contiguous()
    G, hidden = a.shape
    H, dk = _head_dims(hidden, num_heads, "head_expand")
    if w.shape[0] != hidden:
        raise _lib.PtgnnAmdError(f"head_expand: a {tuple(a.shape)} and W {tuple(w.shape)} do not match")
    out = torch.empty(G, H, w.shape[1], dtype=torch.float32, device=a.device)
    return _head_projection(HEAD_EXPAND, a, None, w, G, H, dk, w.shape[1], scale, out)


def head_contract(b: torch.Tensor, w: torch.Tensor, num_heads: int, scale: float = 1.0) -> torch.Tensor:
    """out[g, h*dk + k] = scale * W[h*dk + k, :] . b[g, h, :]: b [G, heads, D], W [hidden, D] -> [G, hidden]
    (the value Linear of the multi-head reducer applied to the pools, varsizedsummary.py:161-166)."""
    _require_cuda_f32("b", b, dims=3)
    _require_cuda_f32("w", w)
    b, w = b.contiguous(), w.contiguous()
    G, H, D = b.shape
    _, dk = _head_dims(w.shape[0], H, "head_contract")
    if w.shape[1] != D:
        raise _lib.PtgnnAmdError(f"head_contract: b {tuple(b.shape)} and W {tuple(w.shape)} do not match")
    out = torch.empty(G, w.shape[0], dtype=torch.float32, device=b.device)
    return _head_projection(HEAD_CONTRACT, None, b, w, G, H, dk, D, scale, out)


def head_weight_grad(a: torch.Tensor, b: torch.Tensor, num_heads: int, scale: float = 1.0) -> torch.Tensor:
    """grad_W[h*dk + k, :] = scale * sum_g a[g, h*dk + k] b[g, h, :]: a [G, hidden], b [G, heads, D] -> [hidden, D], the
    samples added in a fixed order (the weight gradient of `head_expand` and `head_contract`)."""
    _require_cuda_f32("a", a)
    _require_cuda_f32("b", b, dims=3)
    a, b = a.contiguous(), b.contiguous()
    G, hidden = a.shape
    H, dk = _head_dims(hidden, num_heads, "head_weight_grad")
    if b.shape[0] != G or b.shape[1] != H:
        raise _lib.PtgnnAmdError(f"head_weight_grad: a {tuple(a.shape)} and b {tuple(b.shape)} do not match")
    out = torch.empty(hidden, b.shape[2], dtype=torch.float32, device=a.device)
    return _head_projection(HEAD_WEIGHT_GRAD, a, b, None, G, H, dk, b.shape[2], scale, out)


# ------------------------------------------------------------------------------------------------
# task heads (csrc/task_heads.hip)
# ------------------------------------------------------------------------------------------------
LOSS_MODES = {"softmax": 0, "sigmoid": 1}
HEAD_TOTALS_SLOTS = 8     # PTGNN_AMD_HEAD_TOTALS_BYTES / 8: loss sum (float64 bits) | denominator | three counts | rows | 0 | 0
HEAD_METRICS_SLOTS = 4    # PTGNN_AMD_HEAD_METRICS_BYTES / 8


def head_metrics_block(device) -> torch.Tensor:
    """A zeroed persistent metrics block (int64 [4]; the sigmoid mode keeps float64 bits in the first three slots, read
    them with `.view(torch.float64)`).  The merge step of `logit_loss` / `candidate_scores` adds into it; it belongs to
    one stream at a time."""
    return torch.zeros(HEAD_METRICS_SLOTS, dtype=torch.int64, device=device)


def _metrics_ptr(metrics: Optional[torch.Tensor], device):
    if metrics is None:
        return None
    if not metrics.is_cuda or metrics.device != device or metrics.dtype != torch.int64 \
            or metrics.numel() != HEAD_METRICS_SLOTS or not metrics.is_contiguous():
        raise _lib.PtgnnAmdError("a head metrics block is a contiguous CUDA int64 [4] tensor on the logits' device "
                                 "(ops.head_metrics_block)")
    return metrics.data_ptr()


def _head_targets(logits: torch.Tensor, targets: Optional[torch.Tensor], mode: int, what: str):
    """(targets as the kernel reads them, their leading dimension)."""
    R, C = logits.shape
    if targets is None:
        if mode != 0:
            raise _lib.PtgnnAmdError(f"{what}: the sigmoid mode needs targets")
        return None, 0
    if not targets.is_cuda or targets.device != logits.device:
        raise _lib.PtgnnAmdError(f"{what}: targets must live on the logits' GPU (got {targets.device})")
    if mode == 0:
        if targets.dtype != torch.int64 or tuple(targets.shape) != (R,):
            raise _lib.PtgnnAmdError(f"{what}: softmax targets are int64 [{R}] (got {targets.dtype} "
                                     f"{tuple(targets.shape)})")
        return targets.contiguous(), 0
    if targets.dtype not in (torch.bool, torch.uint8) or tuple(targets.shape) != (R, C):
        raise _lib.PtgnnAmdError(f"{what}: sigmoid targets are bool [{R}, {C}] (got {targets.dtype} "
                                 f"{tuple(targets.shape)})")
    targets = targets.contiguous()
    return (targets.view(torch.uint8) if targets.dtype == torch.bool else targets), C


def logit_loss(logits: torch.Tensor, targets: Optional[torch.Tensor], mode: str = "softmax",
               metrics: Optional[torch.Tensor] = None):
    """Row loss over fp32 logits [R, C] in one pass (ptgnn_amd_logit_loss_f32; graph2class.py:91-102, ppi.py:43-62).
    "softmax": int64 targets [R] (None: predict) -> cross-entropy over the live rows; "sigmoid": bool targets [R, C] ->
    BCE-with-logits summed per row, tp / fp / fn.  Returns (loss [] -- nan without rows or targets --, lse [R], argmax
    int64 [R], max_prob [R], totals int64 [8]); the three per-row tensors are None in the sigmoid mode.  `metrics`: a
    block of `head_metrics_block` to add this call's figures into.  Nothing here waits for the device."""
    lib = _lib.load()
    _require_cuda_f32("logits", logits)
    logits = _rowmajor(logits)
    R, C = logits.shape
    if mode not in LOSS_MODES:
        raise _lib.PtgnnAmdError(f"logit_loss: unknown mode {mode!r} (have {sorted(LOSS_MODES)})")
    m = LOSS_MODES[mode]
    if C < 1:
        raise _lib.PtgnnAmdError("logit_loss: logits need at least one class")
    dev = logits.device
    tg, ld_t = _head_targets(logits, targets, m, "logit_loss")
    mptr = _metrics_ptr(metrics, dev)
    lse = argmax = maxp = None
    if m == 0:
        lse = torch.empty(R, dtype=torch.float32, device=dev)
        argmax = torch.empty(R, dtype=torch.int64, device=dev)
        maxp = torch.empty(R, dtype=torch.float32, device=dev)
    if R == 0 or tg is None:
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        totals = torch.zeros(HEAD_TOTALS_SLOTS, dtype=torch.int64, device=dev)
        if R == 0:
            return loss.view(()), lse, argmax, maxp, totals
    else:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        totals = torch.empty(HEAD_TOTALS_SLOTS, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.ptgnn_amd_logit_loss_workspace_bytes(R))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    with _timed("logit_loss", bytes=4.0 * R * C + (8.0 * R if m == 0 else 1.0 * R * C) + 20.0 * R):
        rc = lib.ptgnn_amd_logit_loss_f32(logits.data_ptr(), _ld(logits), R, C, m, tg.data_ptr() if tg is not None else None,
                                          ld_t, lse.data_ptr() if lse is not None else None,
                                          argmax.data_ptr() if argmax is not None else None,
                                          maxp.data_ptr() if maxp is not None else None, None, loss.data_ptr(),
                                          totals.data_ptr(), mptr, ws.data_ptr(), ws.numel() * 8, _stream(loss))
    _lib.check(rc, "ptgnn_amd_logit_loss_f32")
    return loss.view(()), lse, argmax, maxp, totals


def _device_scalar(t: torch.Tensor, device, what: str) -> torch.Tensor:
    if not t.is_cuda or t.numel() != 1:
        raise _lib.PtgnnAmdError(f"{what} must be a one-element CUDA tensor (it is read on the device)")
    return t.detach().to(device=device, dtype=torch.float32).reshape(1).contiguous()


def logit_loss_backward(logits: torch.Tensor, targets: torch.Tensor, mode: str, lse: Optional[torch.Tensor],
                        totals: torch.Tensor, grad_loss: torch.Tensor) -> torch.Tensor:
    """grad_logits [R, C] of `logit_loss` from the upstream scalar `grad_loss` and the forward's lse and totals, all read
    on the device (ptgnn_amd_logit_loss_backward_f32)."""
    lib = _lib.load()
    _require_cuda_f32("logits", logits)
    logits = _rowmajor(logits)
    R, C = logits.shape
    m = LOSS_MODES[mode]
    tg, ld_t = _head_targets(logits, targets, m, "logit_loss_backward")
    if tg is None:
        raise _lib.PtgnnAmdError("logit_loss_backward: a call without targets has no loss to differentiate")
    if not totals.is_cuda or totals.dtype != torch.int64 or totals.numel() != HEAD_TOTALS_SLOTS:
        raise _lib.PtgnnAmdError("logit_loss_backward: totals must be the forward's CUDA int64 [8] block")
    if m == 0 and (lse is None or not lse.is_cuda or tuple(lse.shape) != (R,)):
        raise _lib.PtgnnAmdError(f"logit_loss_backward: lse must be the forward's CUDA [{R}] tensor")
    g = _device_scalar(grad_loss, logits.device, "logit_loss_backward: grad_loss")
    grad = torch.empty(R, C, dtype=torch.float32, device=logits.device)
    if R == 0:
        return grad
    with _timed("logit_loss_backward", bytes=8.0 * R * C + (8.0 * R if m == 0 else 1.0 * R * C)):
        rc = lib.ptgnn_amd_logit_loss_backward_f32(logits.data_ptr(), _ld(logits), R, C, m, tg.data_ptr(), ld_t,
                                                   lse.contiguous().data_ptr() if m == 0 else None,
                                                   totals.contiguous().data_ptr(), g.data_ptr(), grad.data_ptr(), C,
                                                   _stream(grad))
    _lib.check(rc, "ptgnn_amd_logit_loss_backward_f32")
    return grad


def candidate_scores_supported(dim: int) -> bool:
    """Whether the fused candidate scoring takes node states of width `dim` (a multiple of 4, 4 <= dim <= 1024)."""
    return bool(_lib.load().ptgnn_amd_candidate_scores_supported(int(dim)))


def _candidate_args(x, cand_idx, slot_idx, cand_slot, plan, w, correct, what):
    _require_cuda_f32("x", x)
    x = _rowmajor(x)
    N, D = x.shape
    for name, t in (("cand_idx", cand_idx), ("slot_idx", slot_idx), ("cand_slot", cand_slot), ("correct", correct)):
        if t is not None and (not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1):
            raise _lib.PtgnnAmdError(f"{what}: {name} must be a 1-D CUDA int64 tensor")
    Cn, G = cand_idx.shape[0], slot_idx.shape[0]
    if cand_slot.shape[0] != Cn or plan.num_nodes != G or plan.num_edges != Cn or plan.perm is None \
            or (correct is not None and correct.shape[0] != G):
        raise _lib.PtgnnAmdError(f"{what}: {Cn} candidates / {G} slots do not fit cand_slot {tuple(cand_slot.shape)}, a plan "
                                 f"of {plan.num_edges} elements in {plan.num_nodes} segments or correct")
    if not w.is_cuda or w.dtype != torch.float32 or w.numel() != 2 * D:
        raise _lib.PtgnnAmdError(f"{what}: w must hold 2 * {D} CUDA float32 values")
    return (x, cand_idx.contiguous(), slot_idx.contiguous(), cand_slot.contiguous(), w.detach().reshape(-1).contiguous(),
            correct.contiguous() if correct is not None else None, N, D, Cn, G)


def candidate_scores(x: torch.Tensor, cand_idx: torch.Tensor, slot_idx: torch.Tensor, cand_slot: torch.Tensor,
                     plan: GraphPlan, w: torch.Tensor, correct: Optional[torch.Tensor] = None,
                     metrics: Optional[torch.Tensor] = None):
    """scores[c] = x[cand_idx[c]] . w[:D] + x[slot_idx[cand_slot[c]]] . w[D:], their per-slot log-sum-exp and arg-max
    position over `plan` (the segment plan of cand_slot), and -mean_g(scores[correct[g]] - lse[g]) in one launch plus a
    merge (ptgnn_amd_candidate_scores_f32; varmisuse.py:63-91).  Returns (loss [] -- nan without slots or `correct` --,
    scores [Cn], lse [G], argmax int64 [G], totals int64 [8]).  Nothing here waits for the device."""
    lib = _lib.load()
    x, cand_idx, slot_idx, cand_slot, w, correct, N, D, Cn, G = _candidate_args(
        x, cand_idx, slot_idx, cand_slot, plan, w, correct, "candidate_scores")
    dev = x.device
    mptr = _metrics_ptr(metrics, dev)
    scores = torch.empty(Cn, dtype=torch.float32, device=dev)
    lse = torch.empty(G, dtype=torch.float32, device=dev)
    argmax = torch.empty(G, dtype=torch.int64, device=dev)
    if G == 0 or correct is None:
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    else:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    totals = torch.zeros(HEAD_TOTALS_SLOTS, dtype=torch.int64, device=dev) if G == 0 else \
        torch.empty(HEAD_TOTALS_SLOTS, dtype=torch.int64, device=dev)
    if not lib.ptgnn_amd_candidate_scores_supported(D):
        raise _lib.PtgnnAmdError(f"candidate_scores: node states of width {D} are outside the kernel range (a multiple of 4 "
                                 "up to 1024); compose gather_rows / dense.linear / the scatter facade instead")
    if G == 0:
        return loss.view(()), scores, lse, argmax, totals
    ws_bytes = int(lib.ptgnn_amd_candidate_scores_workspace_bytes(G))
    ws = _workspace(ws_bytes, dev)
    plan.wait()
    with _timed("candidate_scores", bytes=4.0 * (Cn + G) * D + 8.0 * D + 24.0 * Cn + 28.0 * G):
        rc = lib.ptgnn_amd_candidate_scores_f32(
            x.data_ptr() if N else None, _ld(x), N, cand_idx.data_ptr() if Cn else None, slot_idx.data_ptr(),
            cand_slot.data_ptr() if Cn else None, plan.rowptr.data_ptr(), plan.perm.data_ptr() if Cn else None, Cn, G, D,
            w.data_ptr(), correct.data_ptr() if correct is not None else None, scores.data_ptr() if Cn else None,
            lse.data_ptr(), argmax.data_ptr(), loss.data_ptr(), totals.data_ptr(), mptr, ws.data_ptr(), ws_bytes,
            _stream(loss))
    _lib.check(rc, "ptgnn_amd_candidate_scores_f32")
    return loss.view(()), scores, lse, argmax, totals


def candidate_scores_backward(x: torch.Tensor, cand_idx: torch.Tensor, slot_idx: torch.Tensor, cand_slot: torch.Tensor,
                              plan: GraphPlan, w: torch.Tensor, correct: Optional[torch.Tensor], scores: torch.Tensor,
                              lse: torch.Tensor, grad_loss: Optional[torch.Tensor],
                              grad_scores: Optional[torch.Tensor] = None):
    """(row_grad [Cn + G, D] -- the gradient rows of cat(cand_idx, slot_idx), to be segment-summed onto the nodes --,
    grad_w [2 D]) of `candidate_scores` from the upstream scalar `grad_loss` (read on the device; None = 0) and an optional
    extra gradient `grad_scores` [Cn] of the scores (ptgnn_amd_candidate_scores_backward_f32)."""
    lib = _lib.load()
    x, cand_idx, slot_idx, cand_slot, w, correct, N, D, Cn, G = _candidate_args(
        x, cand_idx, slot_idx, cand_slot, plan, w, correct, "candidate_scores_backward")
    dev = x.device
    if tuple(scores.shape) != (Cn,) or tuple(lse.shape) != (G,) or not scores.is_cuda or not lse.is_cuda:
        raise _lib.PtgnnAmdError(f"candidate_scores_backward: scores / lse must be the forward's CUDA [{Cn}] / [{G}] tensors")
    g = _device_scalar(grad_loss, dev, "candidate_scores_backward: grad_loss") if grad_loss is not None else None
    if grad_scores is not None:
        _require_cuda_f32("grad_scores", grad_scores, dims=1)
        if grad_scores.shape[0] != Cn:
            raise _lib.PtgnnAmdError(f"candidate_scores_backward: grad_scores must have {Cn} entries")
        grad_scores = grad_scores.contiguous()
    row_grad = torch.zeros(Cn + G, D, dtype=torch.float32, device=dev)
    grad_w = torch.empty(2 * D, dtype=torch.float32, device=dev)
    ws_bytes = int(lib.ptgnn_amd_candidate_scores_backward_workspace_bytes(G, D))
    ws = _workspace(ws_bytes, dev)
    plan.wait()
    with _timed("candidate_scores_backward", bytes=4.0 * (Cn + G) * D * 2 + 8.0 * G * D + 24.0 * Cn):
        rc = lib.ptgnn_amd_candidate_scores_backward_f32(
            x.data_ptr() if N else None, _ld(x), N, cand_idx.data_ptr() if Cn else None, slot_idx.data_ptr() if G else None,
            cand_slot.data_ptr() if Cn else None, plan.rowptr.data_ptr(), plan.perm.data_ptr() if Cn else None, Cn, G, D,
            w.data_ptr(), correct.data_ptr() if correct is not None else None,
            scores.contiguous().data_ptr() if Cn else None, lse.contiguous().data_ptr() if G else None,
            g.data_ptr() if g is not None else None, grad_scores.data_ptr() if grad_scores is not None and Cn else None,
            row_grad.data_ptr() if Cn + G else None, grad_w.data_ptr(), ws.data_ptr(), ws_bytes, _stream(grad_w))
    _lib.check(rc, "ptgnn_amd_candidate_scores_backward_f32")
    return row_grad, grad_w


# ------------------------------------------------------------------------------------------------
# the copying decoder's loss (csrc/vocab_loss.hip)
# ------------------------------------------------------------------------------------------------
def _vocab_args(scores: torch.Tensor, bias, extra, targets, what: str):
    _require_cuda_f32("scores", scores)
    scores = _rowmajor(scores)
    R, V = scores.shape
    if V < 1:
        raise _lib.PtgnnAmdError(f"{what}: scores need at least one column")
    dev = scores.device
    for name, t, n, dt in (("bias", bias, V, torch.float32), ("extra", extra, R, torch.float32),
                           ("targets", targets, R, torch.int64)):
        if t is not None and (not t.is_cuda or t.device != dev or t.dtype != dt or tuple(t.shape) != (n,)):
            raise _lib.PtgnnAmdError(f"{what}: {name} must be a CUDA {dt} [{n}] tensor on the scores' device (got "
                                     f"{t.dtype} {tuple(t.shape)} on {t.device})")
    return scores, *(t.contiguous() if t is not None else None for t in (bias, extra, targets)), R, V


def _opt_ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None and t.numel() else None


def vocab_loss(scores: torch.Tensor, bias: Optional[torch.Tensor] = None, extra: Optional[torch.Tensor] = None,
               targets: Optional[torch.Tensor] = None):
    """(norm [R], picked [R] or None, stats [R, 2]) over raw vocabulary scores [R, V] (ptgnn_amd_vocab_loss_f32;
    grucopydecoder.py:118-135): with s = scores + bias, norm = logaddexp(logsumexp_v s, extra) and picked =
    s[r, targets[r]] - norm (nan for a target outside [0, V)); stats = (maximum, log of the sum relative to it) with norm =
    their sum, which `vocab_loss_backward` takes.  One read of the scores; the [R, V] log-probabilities are never formed."""
    lib = _lib.load()
    scores, bias, extra, targets, R, V = _vocab_args(scores, bias, extra, targets, "vocab_loss")
    dev = scores.device
    norm = torch.empty(R, dtype=torch.float32, device=dev)
    picked = torch.empty(R, dtype=torch.float32, device=dev) if targets is not None else None
    stats = torch.empty(R, 2, dtype=torch.float32, device=dev)
    if R == 0:
        return norm, picked, stats
    ws_bytes = int(lib.ptgnn_amd_vocab_loss_workspace_bytes(R, V))
    ws = _workspace(ws_bytes, dev)
    with _timed("vocab_loss", bytes=4.0 * R * V + 4.0 * V + 24.0 * R):
        rc = lib.ptgnn_amd_vocab_loss_f32(scores.data_ptr(), _ld(scores), R, V, _opt_ptr(bias), _opt_ptr(extra),
                                          _opt_ptr(targets), norm.data_ptr(), _opt_ptr(picked), stats.data_ptr(),
                                          ws.data_ptr(), ws_bytes, _stream(norm))
    _lib.check(rc, "ptgnn_amd_vocab_loss_f32")
    return norm, picked, stats


def vocab_loss_backward(scores: torch.Tensor, bias: Optional[torch.Tensor], extra: Optional[torch.Tensor],
                        targets: Optional[torch.Tensor], stats: torch.Tensor, g_norm: Optional[torch.Tensor],
                        g_picked: Optional[torch.Tensor], want_bias: bool = True):
    """(grad_scores [R, V], grad_extra [R] or None, grad_bias [V] or None) of `vocab_loss` from its `stats` and the gradients of
    its norm and picked outputs (device tensors, None = 0) in one pass (ptgnn_amd_vocab_loss_backward_f32): grad_bias comes from the pass's own
    per-row-block column sums, added in row-block order."""
    lib = _lib.load()
    scores, bias, extra, targets, R, V = _vocab_args(scores, bias, extra, targets, "vocab_loss_backward")
    dev = scores.device
    for name, t, shape in (("stats", stats, (R, 2)), ("g_norm", g_norm, (R,)), ("g_picked", g_picked, (R,))):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape):
            raise _lib.PtgnnAmdError(f"vocab_loss_backward: {name} must be a CUDA float32 {list(shape)} tensor")
    stats, g_norm, g_picked = (t.contiguous() if t is not None else None for t in (stats, g_norm, g_picked))
    grad = torch.empty(R, V, dtype=torch.float32, device=dev)
    grad_extra = torch.empty(R, dtype=torch.float32, device=dev) if extra is not None else None
    if R == 0:
        return grad, grad_extra, torch.zeros(V, dtype=torch.float32, device=dev) if want_bias else None
    grad_bias = torch.empty(V, dtype=torch.float32, device=dev) if want_bias else None
    ws_bytes = int(lib.ptgnn_amd_vocab_loss_backward_workspace_bytes(R, V)) if want_bias else 0
    ws = _workspace(ws_bytes, dev)
    with _timed("vocab_loss_backward", bytes=8.0 * R * V + (8.0 * ((R + 7) // 8) * V if want_bias else 0.0) + 24.0 * R):
        rc = lib.ptgnn_amd_vocab_loss_backward_f32(scores.data_ptr(), _ld(scores), R, V, _opt_ptr(bias), _opt_ptr(extra),
                                                   _opt_ptr(targets), stats.data_ptr(), _opt_ptr(g_norm), _opt_ptr(g_picked),
                                                   grad.data_ptr(), V, _opt_ptr(grad_extra), _opt_ptr(grad_bias),
                                                   ws.data_ptr(), ws_bytes, _stream(grad))
    _lib.check(rc, "ptgnn_amd_vocab_loss_backward_f32")
    return grad, grad_extra, grad_bias


def copy_loss_finish(gen: torch.Tensor, copied: torch.Tensor, rowptr: Optional[torch.Tensor], targets: torch.Tensor,
                     unk_id: int, lengths: torch.Tensor):
    """(loss [], d_gen [B, L], d_copied [B, L]) of the decoder's [B, L] tail (ptgnn_amd_copy_loss_finish_f32;
    grucopydecoder.py:171-212): gen / copied [B, L] the correct generation / copy log-probabilities, `rowptr` int32
    [B L + 1] the row pointer of the plan of the copyable locations (None: nothing to copy anywhere), targets int64 [B, L],
    lengths int64 [B].  One launch; the two derivatives are those of the returned loss."""
    lib = _lib.load()
    _require_cuda_f32("gen", gen)
    _require_cuda_f32("copied", copied)
    B, L = gen.shape
    dev = gen.device
    if tuple(copied.shape) != (B, L) or tuple(targets.shape) != (B, L) or targets.dtype != torch.int64 \
            or not targets.is_cuda or tuple(lengths.shape) != (B,) or lengths.dtype != torch.int64 or not lengths.is_cuda:
        raise _lib.PtgnnAmdError(f"copy_loss_finish: copied float32 / targets int64 must be CUDA [{B}, {L}] tensors and "
                                 f"lengths a CUDA int64 [{B}] tensor")
    if rowptr is not None and (not rowptr.is_cuda or rowptr.dtype != torch.int32 or rowptr.numel() != B * L + 1):
        raise _lib.PtgnnAmdError(f"copy_loss_finish: rowptr must be a CUDA int32 [{B * L + 1}] tensor")
    gen, copied, targets, lengths = (t.contiguous() for t in (gen, copied, targets, lengths))
    d_gen = torch.empty(B, L, dtype=torch.float32, device=dev)
    d_copied = torch.empty(B, L, dtype=torch.float32, device=dev)
    if B == 0 or L == 0:
        return torch.full((), float("nan"), dtype=torch.float32, device=dev), d_gen, d_copied
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    ws_bytes = int(lib.ptgnn_amd_copy_loss_finish_workspace_bytes(B))
    ws = _workspace(ws_bytes, dev)
    with _timed("copy_loss_finish", bytes=28.0 * B * L + 12.0 * B):
        rc = lib.ptgnn_amd_copy_loss_finish_f32(gen.data_ptr(), copied.data_ptr(),
                                                rowptr.contiguous().data_ptr() if rowptr is not None else None,
                                                targets.data_ptr(), int(unk_id), lengths.data_ptr(), B, L, loss.data_ptr(),
                                                d_gen.data_ptr(), d_copied.data_ptr(), ws.data_ptr(), ws_bytes,
                                                _stream(loss))
    _lib.check(rc, "ptgnn_amd_copy_loss_finish_f32")
    return loss.view(()), d_gen, d_copied


# ------------------------------------------------------------------------------------------------
# the copying decoder's greedy-decoding step (csrc/decode_step.hip)
# ------------------------------------------------------------------------------------------------
def value_groups(index: torch.Tensor, ids: torch.Tensor, num_samples: int, num_ids: int):
    """The memories of a decode call ordered by (sample, value id): (rowptr int32 [B + 1], slot_memory int32 [I],
    slot_ids int64 [I]) with the slots of sample b at rowptr[b] .. rowptr[b + 1] - 1, ascending ids inside a sample and
    the memories of one (sample, id) in memory order -- a value group is a run of equal ids.  Two passes of the stable
    plan build: by id (`num_ids` > every id), then by sample over that order.  Built once per call, no host read-back."""
    I = int(index.shape[0])
    if not (index.is_cuda and ids.is_cuda and index.dtype == torch.int64 and ids.dtype == torch.int64
            and index.dim() == 1 and tuple(ids.shape) == (I,)):
        raise _lib.PtgnnAmdError("value_groups: index and ids must be CUDA int64 tensors with one entry per memory")
    ids = ids.contiguous()
    by_id = plan_for([(ids, ids)], int(num_ids))
    by_id.wait()
    order = by_id.perm[:I].to(torch.int64)                     # memories by id, equal ids in memory order
    index_by_id = index[order]
    by_sample = plan_for([(index_by_id, index_by_id)], int(num_samples))
    by_sample.wait()
    slot_memory = order[by_sample.perm[:I].to(torch.int64)]
    return by_sample.rowptr, slot_memory.to(torch.int32), ids[slot_memory]


def decode_step(scores: torch.Tensor, bias: Optional[torch.Tensor], copy_scores: torch.Tensor, total_copy: torch.Tensor,
                groups, top_k: int, unk_id: int, end_id: int, step: int, done: torch.Tensor, lengths: torch.Tensor,
                logprobs: torch.Tensor, tokens: torch.Tensor, next_tokens: torch.Tensor,
                live: Optional[torch.Tensor] = None) -> None:
    """One greedy-decoding step of the copying decoder in one launch (ptgnn_amd_decode_step_f32;
    grucopydecoder.py:375-457): from the raw vocabulary scores [B, V], the copy scores [I] with their per-sample
    log-sum-exp [B] and `groups = value_groups(...)` to the prediction of every sample that is not done.  Updates the
    state IN PLACE: done int32 [B], lengths int64 [B], logprobs float32 [B], tokens int64 [B, T] (column `step`),
    next_tokens int64 [B].  No host read-back; ids the kernel had to clamp are counted like the plan build's.
    With `live` (int32 [T], zeroed once per call) the step goes through ptgnn_amd_greedy_step_live_f32 -- the same kernel
    and counter family -- and adds the number of samples that are not done after it to live[step]."""
    lib = _lib.load()
    _require_cuda_f32("scores", scores)
    scores = _rowmajor(scores)
    B, V = scores.shape
    dev = scores.device
    rowptr, slot_memory, slot_ids = groups
    I = int(slot_memory.shape[0])
    copy_scores = copy_scores.reshape(-1)
    T = int(tokens.shape[1]) if tokens.dim() == 2 else -1
    for name, t, shape, dt in (("bias", bias, (V,), torch.float32), ("copy_scores", copy_scores, (I,), torch.float32),
                               ("total_copy", total_copy, (B,), torch.float32), ("rowptr", rowptr, (B + 1,), torch.int32),
                               ("slot_memory", slot_memory, (I,), torch.int32), ("slot_ids", slot_ids, (I,), torch.int64),
                               ("done", done, (B,), torch.int32), ("lengths", lengths, (B,), torch.int64),
                               ("logprobs", logprobs, (B,), torch.float32), ("tokens", tokens, (B, T), torch.int64),
                               ("next_tokens", next_tokens, (B,), torch.int64), ("live", live, (T,), torch.int32)):
        if t is not None and (not t.is_cuda or t.device != dev or t.dtype != dt or tuple(t.shape) != shape):
            raise _lib.PtgnnAmdError(f"decode_step: {name} must be a CUDA {dt} {list(shape)} tensor on the scores' device "
                                     f"(got {t.dtype} {tuple(t.shape)} on {t.device})")
    for name, t in (("done", done), ("lengths", lengths), ("logprobs", logprobs), ("tokens", tokens),
                    ("next_tokens", next_tokens)) + ((("live", live),) if live is not None else ()):
        if not t.is_contiguous():
            raise _lib.PtgnnAmdError(f"decode_step: {name} is updated in place and must be contiguous")
    if V < 1 or top_k < 1:
        raise _lib.PtgnnAmdError(f"decode_step: needs at least one column and top_k >= 1 (got V = {V}, top_k = {top_k})")
    if B == 0:
        return
    bias, copy_scores, total_copy, rowptr, slot_memory, slot_ids = (
        t.contiguous() if t is not None else None for t in (bias, copy_scores, total_copy, rowptr, slot_memory, slot_ids))
    K = int(min(top_k, V))
    bad = _bad_accumulator(_device_state(dev)) if VALIDATE_INDICES != "off" else None
    ws_bytes = int(lib.ptgnn_amd_decode_step_workspace_bytes(B, V, K))
    ws = _workspace(ws_bytes, dev)
    if live is not None:
        with _timed("decode_step", bytes=4.0 * B * V * (1 if K >= V else 5) + 4.0 * V + 16.0 * I + 40.0 * B):
            rc = lib.ptgnn_amd_greedy_step_live_f32(
                scores.data_ptr(), _ld(scores), _opt_ptr(bias), _opt_ptr(copy_scores), total_copy.data_ptr(),
                _opt_ptr(slot_memory), rowptr.data_ptr(), _opt_ptr(slot_ids), B, I, V, K, int(unk_id), int(end_id), int(step),
                T, done.data_ptr(), lengths.data_ptr(), logprobs.data_ptr(), tokens.data_ptr(), next_tokens.data_ptr(),
                live.data_ptr(), bad.data_ptr() if bad is not None else None, ws.data_ptr(), ws_bytes, _stream(done))
        _lib.check(rc, "ptgnn_amd_greedy_step_live_f32")
        return
    with _timed("decode_step", bytes=4.0 * B * V * (1 if K >= V else 5) + 4.0 * V + 16.0 * I + 40.0 * B):
        rc = lib.ptgnn_amd_decode_step_f32(scores.data_ptr(), _ld(scores), _opt_ptr(bias), _opt_ptr(copy_scores),
                                           total_copy.data_ptr(), _opt_ptr(slot_memory), rowptr.data_ptr(),
                                           _opt_ptr(slot_ids), B, I, V, K, int(unk_id), int(end_id), int(step), T,
                                           done.data_ptr(), lengths.data_ptr(), logprobs.data_ptr(), tokens.data_ptr(),
                                           next_tokens.data_ptr(), bad.data_ptr() if bad is not None else None,
                                           ws.data_ptr(), ws_bytes, _stream(done))
    _lib.check(rc, "ptgnn_amd_decode_step_f32")


def beam_step(scores: torch.Tensor, bias: Optional[torch.Tensor], copy_scores: torch.Tensor, total_copy: torch.Tensor,
              groups, top_k: int, unk_id: int, end_id: int, step: int, state_in, state_out, next_tokens: torch.Tensor,
              parent_rows: torch.Tensor) -> None:
    """One beam-search step of the copying decoder (ptgnn_amd_beam_step_f32): from the raw vocabulary scores [B W, V] (row
    b W + j: slot j of sample b), the copy scores [I, W] with their per-sample log-sum-exp [B, W] and `groups =
    value_groups(...)` to the W best continuations of every sample.  `state_in` = (scores float32 [B, W], done int32
    [B, W], lengths int64 [B, W], tokens int64 [B, W, T]) is read, `state_out` (the same shapes, other buffers: the slots
    are reordered) is written, with next_tokens int64 [B W] and parent_rows int64 [B W] = b W + the slot's parent, the
    index of the row gather that reorders the hidden states.  No host read-back; clamped ids are counted like the plan
    build's."""
    lib = _lib.load()
    _require_cuda_f32("scores", scores)
    scores = _rowmajor(scores)
    R, V = scores.shape
    dev = scores.device
    rowptr, slot_memory, slot_ids = groups
    I = int(slot_memory.shape[0])
    beam_in, done_in, lengths_in, tokens_in = state_in
    beam_out, done_out, lengths_out, tokens_out = state_out
    if beam_in.dim() != 2 or beam_in.shape[1] < 1 or R % int(beam_in.shape[1]):
        raise _lib.PtgnnAmdError(f"beam_step: the beam scores must be [B, W] with B W = {R} rows of vocabulary scores "
                                 f"(got {tuple(beam_in.shape)})")
    B, W = (int(v) for v in beam_in.shape)
    T = int(tokens_in.shape[2]) if tokens_in.dim() == 3 else -1
    for name, t, shape, dt in (("bias", bias, (V,), torch.float32), ("copy_scores", copy_scores, (I, W), torch.float32),
                               ("total_copy", total_copy, (B, W), torch.float32),
                               ("rowptr", rowptr, (B + 1,), torch.int32), ("slot_memory", slot_memory, (I,), torch.int32),
                               ("slot_ids", slot_ids, (I,), torch.int64), ("scores in", beam_in, (B, W), torch.float32),
                               ("done in", done_in, (B, W), torch.int32), ("lengths in", lengths_in, (B, W), torch.int64),
                               ("tokens in", tokens_in, (B, W, T), torch.int64),
                               ("scores out", beam_out, (B, W), torch.float32), ("done out", done_out, (B, W), torch.int32),
                               ("lengths out", lengths_out, (B, W), torch.int64),
                               ("tokens out", tokens_out, (B, W, T), torch.int64),
                               ("next_tokens", next_tokens, (B * W,), torch.int64),
                               ("parent_rows", parent_rows, (B * W,), torch.int64)):
        if t is not None and (not t.is_cuda or t.device != dev or t.dtype != dt or tuple(t.shape) != shape):
            raise _lib.PtgnnAmdError(f"beam_step: {name} must be a CUDA {dt} {list(shape)} tensor on the scores' device "
                                     f"(got {t.dtype} {tuple(t.shape)} on {t.device})")
    for name, t in (("scores in", beam_in), ("done in", done_in), ("lengths in", lengths_in), ("tokens in", tokens_in),
                    ("scores out", beam_out), ("done out", done_out), ("lengths out", lengths_out),
                    ("tokens out", tokens_out), ("next_tokens", next_tokens), ("parent_rows", parent_rows)):
        if not t.is_contiguous():
            raise _lib.PtgnnAmdError(f"beam_step: {name} is read or written in place and must be contiguous")
    for a, b in zip(state_in, state_out):
        if a.data_ptr() == b.data_ptr() and a.numel():
            raise _lib.PtgnnAmdError("beam_step: the state out must not share buffers with the state in (slots are reordered)")
    K = int(min(top_k, V))
    if V < 1 or top_k < 1 or not 1 <= W <= min(K, 8):
        raise _lib.PtgnnAmdError(f"beam_step: needs top_k >= 1 and 1 <= beam width <= min(top_k, V, 8), the head limit of "
                                 f"the fused attention pool (got V = {V}, top_k = {top_k}, beam width {W})")
    if B == 0:
        return
    bias, copy_scores, total_copy, rowptr, slot_memory, slot_ids = (
        t.contiguous() if t is not None else None for t in (bias, copy_scores, total_copy, rowptr, slot_memory, slot_ids))
    bad = _bad_accumulator(_device_state(dev)) if VALIDATE_INDICES != "off" else None
    ws_bytes = int(lib.ptgnn_amd_beam_step_workspace_bytes(B, I, V, K, W))
    ws = _workspace(ws_bytes, dev)
    passes = 2 + (4 if W < V else 0) + (4 if K < V and K != W else 0)      # normaliser, collect, the radix selects
    with _timed("beam_step", bytes=4.0 * R * V * passes + 4.0 * V + (12.0 + 8.0 * W) * I * W + 20.0 * R * W
                + (16.0 * T + 48.0) * R):
        rc = lib.ptgnn_amd_beam_step_f32(scores.data_ptr(), _ld(scores), _opt_ptr(bias), _opt_ptr(copy_scores),
                                         total_copy.data_ptr(), _opt_ptr(slot_memory), rowptr.data_ptr(),
                                         _opt_ptr(slot_ids), B, I, V, K, W, int(unk_id), int(end_id), int(step), T,
                                         beam_in.data_ptr(), done_in.data_ptr(), lengths_in.data_ptr(),
                                         tokens_in.data_ptr(), beam_out.data_ptr(), done_out.data_ptr(),
                                         lengths_out.data_ptr(), tokens_out.data_ptr(), next_tokens.data_ptr(),
                                         parent_rows.data_ptr(), bad.data_ptr() if bad is not None else None,
                                         ws.data_ptr(), ws_bytes, _stream(beam_out))
    _lib.check(rc, "ptgnn_amd_beam_step_f32")


def beam_step_links(scores: torch.Tensor, bias: Optional[torch.Tensor], copy_scores: torch.Tensor,
                    total_copy: torch.Tensor, groups, top_k: int, unk_id: int, end_id: int, step: int,
                    key_scale: torch.Tensor, state_in, state_out, next_tokens: torch.Tensor, parent_rows: torch.Tensor,
                    links: torch.Tensor, live: Optional[torch.Tensor] = None) -> None:
    """`beam_step` on the finishing route (ptgnn_amd_search_step_links_f32): the state is (scores float32 [B, W], done
    int32 [B, W], lengths int64 [B, W]) without the histories; the candidates are placed by score * key_scale[lengths of
    the parent + 1] (`key_scale` float32 [T + 1], positive; the state keeps the raw sums); slot p of sample b writes
    links[step, b, p] = (the id it appends or -1, its parent slot) into `links` int32 [T, B, W, 2]; and with `live`
    (int32 [T], zeroed once per call) the number of slots that are live after the step is added to live[step]."""
    lib = _lib.load()
    _require_cuda_f32("scores", scores)
    scores = _rowmajor(scores)
    R, V = scores.shape
    dev = scores.device
    rowptr, slot_memory, slot_ids = groups
    I = int(slot_memory.shape[0])
    beam_in, done_in, lengths_in = state_in
    beam_out, done_out, lengths_out = state_out
    if beam_in.dim() != 2 or beam_in.shape[1] < 1 or R % int(beam_in.shape[1]):
        raise _lib.PtgnnAmdError(f"beam_step_links: the beam scores must be [B, W] with B W = {R} rows of vocabulary "
                                 f"scores (got {tuple(beam_in.shape)})")
    B, W = (int(v) for v in beam_in.shape)
    T = int(links.shape[0]) if links.dim() == 4 else -1
    for name, t, shape, dt in (("bias", bias, (V,), torch.float32), ("copy_scores", copy_scores, (I, W), torch.float32),
                               ("total_copy", total_copy, (B, W), torch.float32),
                               ("rowptr", rowptr, (B + 1,), torch.int32), ("slot_memory", slot_memory, (I,), torch.int32),
                               ("slot_ids", slot_ids, (I,), torch.int64), ("key_scale", key_scale, (T + 1,), torch.float32),
                               ("scores in", beam_in, (B, W), torch.float32), ("done in", done_in, (B, W), torch.int32),
                               ("lengths in", lengths_in, (B, W), torch.int64),
                               ("scores out", beam_out, (B, W), torch.float32), ("done out", done_out, (B, W), torch.int32),
                               ("lengths out", lengths_out, (B, W), torch.int64),
                               ("next_tokens", next_tokens, (B * W,), torch.int64),
                               ("parent_rows", parent_rows, (B * W,), torch.int64),
                               ("links", links, (T, B, W, 2), torch.int32), ("live", live, (T,), torch.int32)):
        if t is not None and (not t.is_cuda or t.device != dev or t.dtype != dt or tuple(t.shape) != shape):
            raise _lib.PtgnnAmdError(f"beam_step_links: {name} must be a CUDA {dt} {list(shape)} tensor on the scores' "
                                     f"device (got {t.dtype} {tuple(t.shape)} on {t.device})")
    for name, t in (("key_scale", key_scale), ("scores in", beam_in), ("done in", done_in), ("lengths in", lengths_in),
                    ("scores out", beam_out), ("done out", done_out), ("lengths out", lengths_out),
                    ("next_tokens", next_tokens), ("parent_rows", parent_rows), ("links", links)) \
            + ((("live", live),) if live is not None else ()):
        if not t.is_contiguous():
            raise _lib.PtgnnAmdError(f"beam_step_links: {name} is read or written in place and must be contiguous")
    for a, b in zip(state_in, state_out):
        if a.data_ptr() == b.data_ptr() and a.numel():
            raise _lib.PtgnnAmdError("beam_step_links: the state out must not share buffers with the state in (slots are "
                                     "reordered)")
    K = int(min(top_k, V))
    if V < 1 or top_k < 1 or not 1 <= W <= min(K, 8):
        raise _lib.PtgnnAmdError(f"beam_step_links: needs top_k >= 1 and 1 <= beam width <= min(top_k, V, 8), the head "
                                 f"limit of the fused attention pool (got V = {V}, top_k = {top_k}, beam width {W})")
    if B == 0:
        return
    bias, copy_scores, total_copy, rowptr, slot_memory, slot_ids = (
        t.contiguous() if t is not None else None for t in (bias, copy_scores, total_copy, rowptr, slot_memory, slot_ids))
    bad = _bad_accumulator(_device_state(dev)) if VALIDATE_INDICES != "off" else None
    ws_bytes = int(lib.ptgnn_amd_beam_step_workspace_bytes(B, I, V, K, W))
    ws = _workspace(ws_bytes, dev)
    passes = 2 + (4 if W < V else 0) + (4 if K < V and K != W else 0)      # normaliser, collect, the radix selects
    with _timed("beam_step_links", bytes=4.0 * R * V * passes + 4.0 * V + (12.0 + 8.0 * W) * I * W + 20.0 * R * W
                + 56.0 * R):
        rc = lib.ptgnn_amd_search_step_links_f32(
            scores.data_ptr(), _ld(scores), _opt_ptr(bias), _opt_ptr(copy_scores), total_copy.data_ptr(),
            _opt_ptr(slot_memory), rowptr.data_ptr(), _opt_ptr(slot_ids), B, I, V, K, W, int(unk_id), int(end_id), int(step),
            T, key_scale.data_ptr(), beam_in.data_ptr(), done_in.data_ptr(), lengths_in.data_ptr(), beam_out.data_ptr(),
            done_out.data_ptr(), lengths_out.data_ptr(), next_tokens.data_ptr(), parent_rows.data_ptr(), links.data_ptr(),
            _opt_ptr(live), bad.data_ptr() if bad is not None else None, ws.data_ptr(), ws_bytes, _stream(beam_out))
    _lib.check(rc, "ptgnn_amd_search_step_links_f32")


def beam_backtrack(links: torch.Tensor, steps_run: int, tokens: torch.Tensor) -> None:
    """The histories of the finishing route in one launch (ptgnn_amd_search_backtrack): `links` int32 [T, B, W, 2] as
    `beam_step_links` wrote its first `steps_run` steps -> tokens int64 [B, W, T], every column written (-1 from
    `steps_run` on, and wherever a hypothesis had finished)."""
    lib = _lib.load()
    if not links.is_cuda or links.dtype != torch.int32 or links.dim() != 4 or links.shape[3] != 2 \
            or not links.is_contiguous():
        raise _lib.PtgnnAmdError("beam_backtrack: links must be a contiguous CUDA int32 [T, B, W, 2] tensor (GPU only)")
    T, B, W = (int(v) for v in links.shape[:3])
    if not tokens.is_cuda or tokens.device != links.device or tokens.dtype != torch.int64 \
            or tuple(tokens.shape) != (B, W, T) or not tokens.is_contiguous():
        raise _lib.PtgnnAmdError(f"beam_backtrack: tokens must be a contiguous CUDA int64 {[B, W, T]} tensor on the links' "
                                 f"device (got {tokens.dtype} {tuple(tokens.shape)} on {tokens.device})")
    if not 0 <= int(steps_run) <= T or not 1 <= W <= 8:
        raise _lib.PtgnnAmdError(f"beam_backtrack: needs 0 <= steps_run <= {T} and a beam width in [1, 8] (got {steps_run}, "
                                 f"{W})")
    if B == 0 or T == 0:
        return
    with _timed("beam_backtrack", bytes=(8.0 * steps_run + 8.0 * T) * B * W):
        rc = lib.ptgnn_amd_search_backtrack(links.data_ptr(), B, W, int(steps_run), T, tokens.data_ptr(), _stream(tokens))
    _lib.check(rc, "ptgnn_amd_search_backtrack")


def post_index_check(device) -> None:
    """Send the device's bad-index count on its way to the host (no synchronisation); a later plan build or
    `check_indices` raises on it.  For launches that count into the accumulator without a plan build behind them."""
    if VALIDATE_INDICES != "off" and not torch.cuda.is_current_stream_capturing():
        _post_bad_readback(_device_state(device))
