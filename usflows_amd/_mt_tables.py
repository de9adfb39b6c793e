"""Device chunk tables of the multi-tensor kernels (SophiaG, Adam / AdamW, the gradient clip): every tensor is cut into
chunks of ``CHUNK`` elements, one table row and one 256-thread block each, and a whole parameter group goes through one
launch.  ``ChunkTables`` is the part their owners share: the cache of one table per group keyed on the tensors' addresses,
an optional auxiliary array behind the table (Adam's step counters, the clip's partial sums), and the protocol
``Flow.fit`` drives around the capture of a training step as a hipGraph (``prepare_tables`` / ``defer_uploads`` /
``flush_uploads`` / ``note_graph_replays`` / ``reset_tables``)."""
import numpy as np
import torch

CHUNK = 16384          # elements per block of the multi-tensor kernels


def _round16(n: int) -> int:
    return (n + 15) // 16 * 16


def chunk_rows(bases, n: int, tail=()):
    """the table rows of one tensor group member: ``bases`` are the byte addresses of its fp32 arrays (0: absent), ``n``
    its element count; every row is (addresses advanced to the chunk..., chunk length, *tail)"""
    return [tuple(b + 4 * off if b else 0 for b in bases) + (min(CHUNK, n - off),) + tuple(tail) for off in range(0, n, CHUNK)]


class ChunkTables:
    """mixin; the owner provides ``_chunk_struct`` (the ctypes struct of a row), ``_table_key(gi, tensors)`` -> (key of the
    addresses in play, build) with build() -> (rows as a numpy structured array, auxiliary host tensor or None, meta),
    ``_table_members()`` -> [(gi, tensors the kernel would serve now)] and ``_table_capacity()`` -> {gi: (largest number of
    rows, largest auxiliary bytes, device)}"""

    _chunk_struct = None

    def reset_tables(self) -> None:
        """forget every table (and every upload still pending): the next launch rebuilds from the tensors' current
        addresses -- after a load of state, and after a capture that broke off (a table built during it was never
        uploaded, and a later allocation may land on the addresses it is keyed on)"""
        self._tables = {}           # per group: (key of data pointers, device table, number of chunks, device aux, meta)
        self._pending_uploads = []

    def _table(self, gi: int, tensors):
        """the table entry of group ``gi`` for ``tensors`` (rebuilt when an address moved or the members changed)"""
        from . import _ext
        key, build = self._table_key(gi, tensors)
        hit = self._tables.get(gi)
        if hit is not None and hit[0] == key:
            return hit
        rows, aux, meta = build()
        assert rows.dtype.itemsize == _ext.C.sizeof(self._chunk_struct)
        host = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())
        nb = host.numel()
        aux_host = None if aux is None else aux.contiguous().view(torch.uint8).reshape(-1)
        total = _round16(nb) + (0 if aux_host is None else aux_host.numel())
        device = tensors[0].device
        if getattr(self, "_defer_uploads", False) and torch.cuda.is_current_stream_capturing():
            # Flow.fit captures a step whose gradients are allocated inside the capture (their addresses are known only
            # now): a host-to-device copy is not capturable, and not needed -- nothing runs during a capture.  The table
            # goes into a buffer allocated BEFORE the capture (memory allocated inside one is recycled between the graph's
            # own kernels on every replay: a table uploaded once would be overwritten by whatever shared its block); its
            # contents are uploaded by flush_uploads() before the first replay.
            buf = self._capture_buffers.get(gi)
            if buf is None or buf.numel() < total:
                raise RuntimeError(f"{type(self).__name__}: no pointer-table buffer prepared for this capture (defer_uploads)")
            upload = self._pending_uploads.append
        else:
            buf = torch.empty(total, dtype=torch.uint8, device=device)
            upload = lambda pair: pair[0].copy_(pair[1])      # noqa: E731
        dev = buf[:nb]
        upload((dev, host))
        aux_dev = None
        if aux_host is not None:
            aux_dev = buf[_round16(nb): _round16(nb) + aux_host.numel()]
            upload((aux_dev, aux_host))
            aux_dev = aux_dev.view(aux.dtype)
        entry = (key, dev, len(rows), aux_dev, meta)
        self._tables[gi] = entry
        return entry

    def defer_uploads(self, on: bool) -> None:
        """Flow.fit, around the capture of a training step: table uploads wait for ``flush_uploads``; ``on`` allocates
        one buffer per group, large enough for a table over all of the group's device tensors"""
        from . import _ext
        self._defer_uploads = bool(on)
        if on:
            self._pending_uploads = []
            self._capture_buffers = {}
            for gi, (rows, aux_bytes, device) in self._table_capacity().items():
                if rows:
                    self._capture_buffers[gi] = torch.empty(_round16(rows * _ext.C.sizeof(self._chunk_struct)) + aux_bytes,
                                                            dtype=torch.uint8, device=device)

    def flush_uploads(self) -> None:
        for dev, host in getattr(self, "_pending_uploads", []):
            dev.copy_(host)
        self._pending_uploads = []

    def prepare_tables(self) -> None:
        """(re)build the device chunk tables for the tensors' current buffers now -- Flow.fit calls this before it
        captures a step as a hipGraph: the upload of a table is a host-to-device copy, which a capture refuses"""
        for gi, tensors in self._table_members():
            if tensors:
                self._table(gi, tensors)

    def note_graph_replays(self, n: int = 1) -> None:
        """A hipGraph replay of a captured training step (Flow.fit) runs the update kernels but no Python: the
        per-parameter ``state['step']`` counters (CPU tensors, bumped by ``step()``) do not move.  Flow.fit reports every
        replay here so that ``state_dict()`` stays interchangeable with the reference's / torch's."""
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st is not None and "step" in st and p.grad is not None:
                    st["step"] += n


def param_capacity(param_groups, aux_bytes_per=lambda rows, tensors: 0):
    """``_table_capacity`` of an optimiser: per group the rows of all its fp32 device parameters"""
    cap = {}
    for gi, group in enumerate(param_groups):
        ps = [p for p in group["params"] if p.is_cuda and p.dtype == torch.float32]
        rows = sum((p.numel() + CHUNK - 1) // CHUNK for p in ps)
        if rows:
            cap[gi] = (rows, aux_bytes_per(rows, len(ps)), ps[0].device)
    return cap
