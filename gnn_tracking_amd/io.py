"""Reading the reference's on-disk graphs without PyG.

The reference stores one ``torch_geometric.data.Data`` per event with ``torch.save``
(graph_construction/graph_builder.py:396-455: ``x`` f32[N,14], ``edge_index`` i64[2,E],
``edge_attr`` f32[E,4], ``y``, ``pt``, ``particle_id`` i64, ``reconstructable``, ``sector``,
``evtid``, ``s``, ``eta``, ``layer``) and reads them back in utils/loading.py:17-113.
Such a file is a pickle that references PyG classes; here it is opened with a RESTRICTED
unpickler: tensors and plain containers are rebuilt, the PyG container classes are mapped to
inert stand-ins whose ``_store._mapping`` dict carries the fields, everything else is refused
(no arbitrary code execution from a data file).

``PrefetchLoader`` overlaps disk reads + host-to-device copies of the next graphs with the
training step: a background thread fills pinned host buffers, the copy runs on a side stream.

Writing (``save_graph``, ``save_graphs``, ``GraphWriter``).  A written file is a ``torch.save``
of a plain ``dict``: every field name maps to a CPU tensor, Python ints, floats and strs are kept as they are.  It is
NOT a PyG pickle: ``load_graph`` / ``GraphDataset`` read it (``_fields`` takes a dict), ``torch.load(path,
weights_only=True)`` opens it, a reference user reads it with ``Data(**torch.load(f))`` - the reference's
``TrackingDataset`` does not read it directly, and writing PyG pickles without PyG is out of scope.  A file holds its
own event only: the storage of each of its tensors spans that tensor's bytes of the event's image, never the batch's.
``GraphWriter`` is the mirror image of ``PrefetchLoader``: the events of a collated batch are packed into one byte
image by one launch (``pack_events``: ``gnntrk_pack_segments``, csrc/pack.hip) and copied once into a pinned buffer on
a side stream, and a background thread serialises and writes while the next batch is built.
"""

from __future__ import annotations

import collections
import io as _io
import os
import pathlib
import pickle
import queue
import threading
from typing import Iterable, Iterator, Sequence

import numpy as np
import torch

from . import _capi
from .data import Data, EventLayout, collate, uncollate

_PYG_CONTAINERS = {
    ("torch_geometric.data.data", "Data"), ("torch_geometric.data.data", "DataEdgeAttr"),
    ("torch_geometric.data.data", "DataTensorAttr"), ("torch_geometric.data.storage", "GlobalStorage"),
    ("torch_geometric.data.storage", "BaseStorage"), ("torch_geometric.data.storage", "NodeStorage"),
    ("torch_geometric.data.storage", "EdgeStorage"),
}
_ALLOWED = {
    ("collections", "OrderedDict"), ("collections", "defaultdict"), ("builtins", "dict"),
    ("builtins", "list"), ("builtins", "tuple"), ("builtins", "set"), ("builtins", "int"),
    ("builtins", "float"), ("builtins", "str"), ("builtins", "bool"), ("builtins", "slice"),
    ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_tensor"),
    ("torch._utils", "_rebuild_parameter"), ("torch", "Size"), ("torch", "device"),
    ("torch.serialization", "_get_layout"), ("numpy.core.multiarray", "scalar"),
    ("numpy._core.multiarray", "scalar"), ("numpy", "dtype"),
}


class _Inert:
    """Stand-in for a PyG container: keeps whatever state the pickle assigns."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, st):
        self.__dict__.update(st if isinstance(st, dict) else {"_state": st})


class _RestrictedUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _PYG_CONTAINERS:
            return type(name, (_Inert,), {})
        if (module, name) in _ALLOWED:
            return super().find_class(module, name)
        if module == "torch" and (name.endswith("Storage") or name in (
                "float32", "float64", "float16", "bfloat16", "int64", "int32", "int16", "int8", "uint8",
                "bool")):
            return getattr(torch, name)
        raise pickle.UnpicklingError(f"graph file references {module}.{name}: not a tensor container, refused")


class _RestrictedPickle:
    """Duck-typed ``pickle_module`` for ``torch.load``."""

    __name__ = "gnn_tracking_amd.io.restricted_pickle"
    Unpickler = _RestrictedUnpickler
    UnpicklingError = pickle.UnpicklingError

    @staticmethod
    def load(f, **kw):
        return _RestrictedUnpickler(f, **kw).load()


def _fields(obj) -> dict:
    if isinstance(obj, dict):
        return obj
    store = obj.__dict__.get("_store", None)
    if store is not None:
        mapping = store.__dict__.get("_mapping", None)
        if isinstance(mapping, dict):
            return mapping
    return {k: v for k, v in obj.__dict__.items() if not k.startswith("_")}


def load_graph(path, device=None) -> Data:
    """Read one reference ``.pt`` graph into this package's ``Data`` (no PyG needed)."""
    with open(path, "rb") as f:
        payload = f.read()
    obj = torch.load(_io.BytesIO(payload), map_location="cpu", pickle_module=_RestrictedPickle,
                     weights_only=False)
    fields = {k: v for k, v in _fields(obj).items() if v is not None}
    if "x" not in fields or "edge_index" not in fields:
        raise ValueError(f"{path}: not a graph file (fields: {sorted(fields)})")
    d = Data(**fields)
    return d if device is None else d.to(device)


def renumber_nodes(data: Data, col: int | None = None) -> Data:
    """The hits of ONE event renumbered by a feature column of ``data.x`` (default: the azimuth column the edge
    classifier would sort by itself, ``locality.AUTO_COLUMN``): every node-level attribute is permuted, every
    ``*index*`` attribute relabelled, ``node_order_key`` records the column and ``node_perm`` (new id -> old id) maps
    node results back.  The reference keeps the hits in hit-table order (graph_construction/graph_builder.py:396-455,
    read back unchanged by utils/loading.py:17-113); its datasets are static, so a loader can pay for the geometric
    order ONCE per event (``GraphDataset(renumber=True)``) instead of the 1.4 ms per 64 M-edge step that
    ``ECForGraphTCN`` spends when a batch arrives in file order.  An event that carries
    ``node_order_key`` is not renumbered again in the step (``locality.order_column``).  The order is the stable sort
    of the key's order-preserving integer image; the in-step renumbering of a batch sorts by a QUANTISED image of the
    same key (ties stable), so the two numberings agree in locality, not id for id - results are equal up to
    summation order either way."""
    import copy

    from . import locality

    col = locality.AUTO_COLUMN if col is None else int(col)
    x = data.x
    if x.dim() != 2 or x.dtype != torch.float32 or not 0 <= col < x.shape[1]:
        raise ValueError("renumber_nodes: data.x must be fp32 [N, F] with the key column inside")
    if x.is_cuda:
        from . import ops
        perm, rank = (t.long() for t in ops.node_order(x.contiguous(), col, None))
    else:
        u = x[:, col].contiguous().view(torch.int32).long() & 0xffffffff
        perm = torch.argsort(torch.where(u >> 31 == 1, u ^ 0xffffffff, u ^ 0x80000000), stable=True)
        rank = torch.empty_like(perm)
        rank[perm] = torch.arange(perm.numel(), device=perm.device)
    out = copy.copy(data)
    for k in data.keys():
        v = getattr(data, k)
        if not torch.is_tensor(v):
            continue
        if "index" in k:
            setattr(out, k, rank[v])
        elif data.is_node_attr(k):
            setattr(out, k, v[perm])
    out.node_perm = perm
    out.node_order_key = col
    return out


class GraphDataset:
    """The ``*.pt`` files of one or several directories (utils/loading.py:17-113: sorted by
    name, optional ``start``/``stop`` slice and sector filter).  ``renumber``: every graph goes through
    ``renumber_nodes`` when it is read (True: the default key column, or a column number)."""

    def __init__(self, in_dirs: str | Sequence[str], *, start: int = 0, stop: int | None = None,
                 sector: int | None = None, renumber: bool | int = False):
        self.renumber = renumber
        dirs = [in_dirs] if isinstance(in_dirs, (str, pathlib.Path)) else list(in_dirs)
        files: list[pathlib.Path] = []
        for d in dirs:
            files += sorted(pathlib.Path(d).glob("*.pt"))
        if sector is not None:
            files = [f for f in files if f.stem.endswith(f"_s{sector}")]
        self.files = files[start:stop]

    def __len__(self) -> int:
        return len(self.files)

    def __getitem__(self, i: int) -> Data:
        g = load_graph(self.files[i])
        if self.renumber is not False:
            g = renumber_nodes(g, None if self.renumber is True else int(self.renumber))
        return g


class ResidentDataset:
    """A static dataset kept ON THE DEVICE, with the graph index of every event built ONCE.

    The reference's datasets do not change between epochs (utils/loading.py:97-100: the same files every epoch,
    shuffled), and 288 GB of HBM hold thousands of 2 M-edge events (about 150 MB each with the index).  Every
    event is read, copied and indexed on first use - node order (``locality.py``), 1-byte labels and, for bf16
    storage, the edge features carried into CSR order; ``batches`` collates events as the reference's DataLoader
    does and PLACES their indices into the batch's arrays (``ops.place_graph_indices``: one streaming pass per
    event, the arrays identical to building the index of the collated list) instead of sorting 64 M edges in every
    step.  ``ECForGraphTCN`` finds the placed index through ``ops.placed_graph_index``.

        ds = ResidentDataset(GraphDataset(dirs), "cuda:0")
        for epoch in range(n):
            for batch in ds.batches(32, shuffle=True, seed=epoch):
                module.optimisation_step(batch)
    """

    def __init__(self, events, device, *, bf16: bool = True, order: bool | int = True):
        """``events``: a sequence of ``Data`` (``GraphDataset``, a list); ``bf16``: carry the four fp32 edge features
        as bf16 rows (what ``bf16_storage`` reads; fp32 runs gather ``edge_attr`` through the permutation);
        ``order``: True = follow the node-order policy of ``locality.py`` (column ``AUTO_COLUMN`` unless the policy is
        off - whatever the size: the sort is paid once), a column number, or False."""
        self.source, self.device = events, torch.device(device)
        self.bf16, self.order = bool(bf16), order
        self._events: list = [None] * len(events)
        self._parts: list = [None] * len(events)

    def __len__(self) -> int:
        return len(self._events)

    def _policy_column(self):
        """The column this dataset orders its events by (None: it does not)."""
        from . import locality

        if self.order is False or (self.order is True and locality.mode() == "off"):
            return None
        return int(self.order) if self.order is not True else (
            locality.AUTO_COLUMN if locality.mode() == "auto" else int(locality.mode()))

    def _key_column(self, e: Data):
        col = self._policy_column()
        if col is None or "node_order_key" in e:
            return None
        x = e.x
        return col if x.dim() == 2 and x.dtype == torch.float32 and 0 <= col < x.shape[1] and x.shape[0] >= 2 else None

    def event(self, i: int):
        """``(data, index)`` of event ``i`` on the device (read and indexed on first use)."""
        if self._events[i] is None:
            from . import ops

            e = self.source[i].to(self.device)
            col = self._key_column(e)
            y, ea = getattr(e, "y", None), getattr(e, "edge_attr", None)
            part = ops.graph_index(e.edge_index, e.num_nodes, cache=False,
                                   carry_label=y if torch.is_tensor(y) else None,
                                   carry_rows=ea if self.bf16 and torch.is_tensor(ea) and ea.dim() == 2 and ea.shape[1] == 4 else None,
                                   order_by=None if col is None else (e.x, col, None))
            self._events[i], self._parts[i] = e, part
        return self._events[i], self._parts[i]

    def batches(self, batch_size: int = 1, *, shuffle: bool = False, seed: int = 0) -> Iterator[Data]:
        """Collated batches of ``batch_size`` events with their graph index placed (see the class)."""
        from . import ops

        idx = list(range(len(self)))
        if shuffle:
            idx = torch.randperm(len(idx), generator=torch.Generator().manual_seed(seed)).tolist()
        for s in range(0, len(idx), int(batch_size)):
            evs = [self.event(i) for i in idx[s:s + int(batch_size)]]
            batch = collate([e for e, _ in evs])
            # (events the loader renumbered when it read them keep their order: nothing to place through)
            oc = self._policy_column() if any("node_order_key" not in e for e, _ in evs) else None
            ops.place_graph_indices([p for _, p in evs], batch, order_col=oc)
            yield batch


class PrefetchLoader:
    """Iterate over batches of ``batch_size`` collated graphs on ``device``.  A background
    thread reads and collates the next ``depth`` batches into pinned memory; the
    host-to-device copy is issued on a side stream and joined when the batch is handed out."""

    def __init__(self, dataset, *, batch_size: int = 1, device=None, depth: int = 2, shuffle: bool = False,
                 seed: int = 0, build_index: bool = False):
        """``build_index``: also build the graph index of every staged batch on the side stream
        (``ops.prefetch_graph_index``: it depends on ``edge_index`` only), so the step that
        consumes the batch joins a finished index instead of building it."""
        self.build_index = bool(build_index)
        self.dataset, self.batch_size, self.depth = dataset, int(batch_size), max(1, int(depth))
        self.device = torch.device(device) if device is not None else None
        self.shuffle, self.seed, self._epoch = shuffle, seed, 0

    def __len__(self) -> int:
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _order(self) -> list[int]:
        idx = list(range(len(self.dataset)))
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self._epoch)
            idx = torch.randperm(len(idx), generator=g).tolist()
        return idx

    def __iter__(self) -> Iterator[Data]:
        order = self._order()
        self._epoch += 1
        q: queue.Queue = queue.Queue(maxsize=self.depth)
        cuda = self.device is not None and self.device.type == "cuda"
        side = torch.cuda.Stream(self.device) if cuda else None

        def produce():
            try:
                for s in range(0, len(order), self.batch_size):
                    batch = collate([self.dataset[i] for i in order[s:s + self.batch_size]])
                    if cuda:
                        batch = batch._map(lambda t: t.pin_memory())
                        with torch.cuda.stream(side):
                            dev_batch = batch.to(self.device, non_blocking=True)
                            ev = torch.cuda.Event()
                            ev.record(side)
                        if self.build_index:
                            from . import ops
                            from . import locality
                            # (the same predicate as the step's: events renumbered by the policy's column when they
                            #  were read keep their order - no x, no renumbering in the build)
                            ops.prefetch_graph_index(dev_batch.edge_index, dev_batch.num_nodes, side,
                                                     x=None if locality.order_column(dev_batch) is None else dev_batch.x,
                                                     batch=getattr(dev_batch, "batch", None))
                        q.put((dev_batch, ev, batch))  # keep the pinned source alive until consumed
                    else:
                        q.put((batch if self.device is None else batch.to(self.device), None, None))
                q.put(None)
            except BaseException as e:  # surface loader errors in the consumer
                q.put(e)

        threading.Thread(target=produce, daemon=True).start()
        while True:
            item = q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            batch, ev, _pinned = item
            if ev is not None:
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                # the device tensors were allocated on the side stream: tell the caching
                # allocator that the consumer's stream uses them, or the producer's next
                # copy could be handed the same blocks while kernels queued here still read them
                batch._map(lambda t: (t.record_stream(cur), t)[1])
            yield batch


# ----------------------------------------------------------------------------------------------------------- writing
#: whether a collated batch on the device goes through the packer when ``pack`` is not given (DESIGN.md section 4.21
#: says which the measurement decided); ``GNNTRK_PACK_EVENTS=1`` / ``=0`` overrides it
PACK_BY_DEFAULT = False
_FIELD_ALIGN = 16


def _pack_wanted(pack, data) -> bool:
    if pack is not None:
        return bool(pack)
    env = os.environ.get("GNNTRK_PACK_EVENTS")
    want = PACK_BY_DEFAULT if env is None else env.strip() not in ("", "0")
    x = getattr(data, "x", None)
    return want and torch.is_tensor(x) and x.is_cuda


def _own(t: torch.Tensor) -> torch.Tensor:
    """``t`` on the host in a storage of its own size (``torch.save`` writes whole storages)"""
    t = t.detach().cpu()
    if not t.is_contiguous() or t.untyped_storage().nbytes() != t.numel() * t.element_size():
        t = t.contiguous().clone()
    return t


def _event_dict(data) -> dict:
    """the file content of one event from its fields, one host copy per field: the path without the packer"""
    return {k: _own(v) if torch.is_tensor(v) else v for k, v in ((k, getattr(data, k)) for k in data.keys())
            if v is not None and k not in ("batch", "ptr")}


class PackedEvents:
    """The events of a collated batch as ONE byte image on the device (``image`` uint8), written by one launch of
    ``gnntrk_pack_segments``.  Event ``b`` owns ``image[event_ptr[b]:event_ptr[b + 1]]``; inside it every tensor field
    starts at a 16-byte boundary, in the dtype and event-local shape that ``uncollate`` gives, the index fields with
    event-local ids.  ``event_dicts(host)`` rebuilds the file contents from a host copy of the image."""

    def __init__(self, image, event_ptr, fields, extras, keep):
        self.image, self.event_ptr, self.fields, self.extras, self._keep = image, event_ptr, fields, extras, keep

    @property
    def n_events(self) -> int:
        return len(self.event_ptr) - 1

    def event_dicts(self, host: torch.Tensor) -> list[dict]:
        """``host``: a CPU uint8 copy of ``image``.  Every tensor of event ``b`` gets a storage of its own that spans
        its bytes of the event's image and nothing else (it aliases ``host``: no copy, and ``host`` must outlive it).
        One storage per field, not one per event: ``torch.save`` refuses tensors of different dtypes on one storage."""
        flat = host.numpy()
        out = []
        for b in range(self.n_events):
            at, d = self.event_ptr[b], {}
            for k, meta in self.fields.items():
                if meta is None:
                    d[k] = self.extras[k][b]
                    continue
                dtype, shapes, offs, sizes = meta
                if sizes[b] == 0:
                    d[k] = torch.empty(shapes[b], dtype=dtype)
                else:
                    lo = at + offs[b]
                    d[k] = torch.from_numpy(flat[lo:lo + sizes[b]]).view(dtype).reshape(shapes[b])
            out.append(d)
        return out


def pack_segments(table, image: torch.Tensor, image_bytes: int | None = None):
    """``gnntrk_pack_segments`` for a descriptor table: int64 ``[n_segs, 5]`` rows (device address of the source,
    byte offset in ``image``, byte count, ``sub``, mode ``_capi.PACK_RAW`` / ``PACK_SUB_I64`` / ``PACK_SUB_I32``).  Cuts
    the segments into chunks, uploads descriptors and chunk table as ONE tensor and launches once on the current stream
    of ``image`` (uint8, on the device).  Returns the uploaded plan, which must stay alive until the launch has run."""
    from . import ops

    table = np.ascontiguousarray(table, np.int64).reshape(-1, _capi.PACK_SEG_WORDS)
    n_segs, words = len(table), _capi.PACK_SEG_WORDS
    _capi.require_device(image)
    image_bytes = int(image.numel()) if image_bytes is None else int(image_bytes)
    if image.dtype != torch.uint8 or not image.is_contiguous() or image_bytes > image.numel():
        raise ValueError("pack_segments: `image` must be a contiguous uint8 tensor of at least image_bytes bytes")
    per_seg = -(-np.maximum(table[:, 2], 0) // _capi.PACK_CHUNK_BYTES)
    n_chunks = int(per_seg.sum())
    if n_segs > _capi.PACK_MAX_SEGS or n_chunks > _capi.PACK_MAX_CHUNKS:
        raise NotImplementedError(f"pack_segments: {n_segs} segments in {n_chunks} chunks; at most "
                                  f"{_capi.PACK_MAX_SEGS} and {_capi.PACK_MAX_CHUNKS}: pack fewer events at a time")
    plan = np.empty(n_segs * words + n_chunks, np.int64)
    plan[:n_segs * words] = table.ravel()
    pairs = plan[n_segs * words:].view(np.int32).reshape(n_chunks, 2)
    pairs[:, 0] = np.repeat(np.arange(n_segs, dtype=np.int32), per_seg)
    pairs[:, 1] = np.arange(n_chunks, dtype=np.int64) - np.repeat(np.cumsum(per_seg) - per_seg, per_seg)
    lib = _capi.load()
    plan_dev = torch.from_numpy(plan).to(image.device)
    _capi.check(lib.gnntrk_pack_segments(plan.ctypes.data if n_segs else None, n_segs, ops._p(plan_dev), n_chunks,
                                         ops._p(image), image_bytes, ops._stream(image)), lib)
    return plan_dev


def pack_events(batch, layout: EventLayout | None = None, *, image: torch.Tensor | None = None) -> PackedEvents:
    """Pack the events of a collated batch on the device: the descriptor table of all B x F segments (an index field
    of R rows is R segments per event), ONE ``gnntrk_pack_segments`` launch.  ``image``: a uint8 device buffer to
    write into (at least as large as the image), else one is allocated.  Device tensors only (no CPU path)."""
    from . import ops

    lay = EventLayout(batch, "pack_events") if layout is None else layout
    B = lay.n_events
    node_ptr = np.asarray(lay.node_ptr, np.int64)
    cur = np.zeros(B, np.int64)                              # the bytes of every event's image so far
    segs, fields, extras, keep = [], {}, {}, []
    first = None
    for k, kind in lay.kinds.items():
        v = getattr(batch, k)
        if not torch.is_tensor(v):
            fields[k], extras[k] = None, ([v[b] for b in range(B)] if kind == "list" else [v] * B)
            continue
        _capi.require_device(v)
        t = v.detach().contiguous()
        keep.append(t)
        first = t if first is None else first
        es, base = t.element_size(), t.data_ptr()
        if kind == "copy" or t.dim() == 0:
            lo, hi = np.zeros(B, np.int64), np.full(B, t.numel(), np.int64)
            shapes, rows, row_bytes, stride = [tuple(t.shape)] * B, 1, es, 0
        else:
            ptr = np.asarray([lay.bounds(k, 0)[0]] + [lay.bounds(k, b)[1] for b in range(B)], np.int64)
            lo, hi = ptr[:-1], ptr[1:]
            if kind == "index":
                rows, row_bytes, stride = int(np.prod(t.shape[:-1], dtype=np.int64)), es, int(t.shape[-1]) * es
                shapes = [(*t.shape[:-1], int(h - l)) for l, h in zip(lo, hi)]
            else:
                rows, row_bytes, stride = 1, int(np.prod(t.shape[1:], dtype=np.int64)) * es, 0
                shapes = [(int(h - l), *t.shape[1:]) for l, h in zip(lo, hi)]
        if kind == "index":
            if t.dtype not in (torch.int64, torch.int32):
                raise TypeError(f"pack_events: index field '{k}' must be int64 or int32, got {t.dtype}")
            mode, sub = (_capi.PACK_SUB_I64 if t.dtype == torch.int64 else _capi.PACK_SUB_I32), node_ptr[:-1]
        else:
            mode, sub = _capi.PACK_RAW, np.zeros(B, np.int64)
        n_bytes = (hi - lo) * row_bytes                       # of one row of the field in every event
        offs = cur.copy()
        for r in range(rows):
            segs.append(np.stack([base + r * stride + lo * row_bytes, offs + r * n_bytes, n_bytes, sub,
                                  np.full(B, mode, np.int64), np.arange(B, dtype=np.int64)], axis=1))
        fields[k] = (t.dtype, shapes, offs.tolist(), (rows * n_bytes).tolist())
        cur = (offs + rows * n_bytes + _FIELD_ALIGN - 1) // _FIELD_ALIGN * _FIELD_ALIGN
    event_ptr = np.concatenate([[0], np.cumsum(cur)]).astype(np.int64)
    total = int(event_ptr[-1])
    like = first if first is not None else batch.x
    if image is None:
        image = torch.empty(max(total, _FIELD_ALIGN), dtype=torch.uint8, device=like.device)
    elif image.dtype != torch.uint8 or image.numel() < total or image.device != like.device:
        raise ValueError("pack_events: `image` must be a uint8 buffer of the batch's device that holds the image")
    if segs:
        table = np.concatenate(segs)
        table[:, 1] += event_ptr[table[:, 5]]                 # the event's place in the image
        keep.append(pack_segments(table[table[:, 2] > 0, :_capi.PACK_SEG_WORDS], image, total))
    return PackedEvents(image, event_ptr.tolist(), fields, extras, keep)


def _event_dicts(data, pack) -> list[dict]:
    """the file contents of a list of events, one event or a collated batch (validated before anything is written)"""
    if isinstance(data, (list, tuple)):
        return [_event_dict(d) for d in data]
    if getattr(data, "ptr", None) is None and getattr(data, "batch", None) is None:
        return [_event_dict(data)]
    lay = EventLayout(data, "save_graphs")
    if not _pack_wanted(pack, data):
        return [_event_dict(d) for d in uncollate(data, lay)]
    packed = pack_events(data, lay)
    return packed.event_dicts(packed.image[:packed.event_ptr[-1]].cpu())


def _write(fields: dict, path) -> None:
    path = pathlib.Path(path)
    tmp = path.with_name(path.name + f".tmp{os.getpid()}")
    try:
        torch.save(fields, tmp)
        os.replace(tmp, path)                                # (a reader never sees a half-written file)
    except BaseException:
        tmp.unlink(missing_ok=True)
        raise


def graph_file_name(fields) -> str:
    """``data{evtid}_s{sector}.pt``, the reference's file name (graph_construction/graph_builder.py:484 parses it)"""
    def one(k):
        v = fields[k]
        return int(v.reshape(-1)[0]) if torch.is_tensor(v) else int(v)
    return f"data{one('evtid')}_s{one('s')}.pt"


def save_graph(data, path) -> None:
    """Write ONE event (on either device) in the format the module docstring describes."""
    _write(_event_dict(data), path)


def save_graphs(data, paths, *, pack: bool | None = None) -> None:
    """Write a list of events, or every event of a collated batch, to ``paths`` (one per event).  A collated batch on
    the device goes through the packer where that is the default or ``pack=True`` (one launch, one host copy);
    otherwise through ``uncollate`` and one host copy per field.  A batch whose edges cross events raises
    ``ValueError`` before anything is written."""
    dicts = _event_dicts(data, pack)
    paths = list(paths)
    if len(paths) != len(dicts):
        raise ValueError(f"save_graphs: {len(dicts)} events, {len(paths)} paths")
    for d, p in zip(dicts, paths):
        _write(d, p)


class GraphWriter:
    """Write events to ``outdir`` while the next ones are built: the mirror image of ``PrefetchLoader``.

        with GraphWriter(outdir) as w:
            for clouds in ...:
                w.write(builder.build(clouds, evtid=evtid, s=s))     # returns once the copy is queued

    ``write`` takes one event, a list of events or a collated batch; ``names`` are the file names (default
    ``data{evtid}_s{s}.pt`` from the events' own fields).  With the packer the pack and the ONE copy into a pinned
    buffer run on a side stream and a background thread serialises and writes; without it the per-field copies are made
    in ``write`` and the thread serialises and writes.  Threads only, no child process.  ``close()`` (or leaving the
    ``with`` block) joins the thread; an error in the thread is raised there, and ``outdir`` is not created here."""

    def __init__(self, outdir, *, depth: int = 2, pack: bool | None = None, redo: bool = True):
        self.outdir, self.depth, self.pack, self.redo = pathlib.Path(outdir), max(1, int(depth)), pack, bool(redo)
        self.written: list[pathlib.Path] = []
        self._q: queue.Queue = queue.Queue(maxsize=self.depth)
        self._buffers: queue.Queue = queue.Queue()
        self._n_buffers, self._side, self._error, self._closed = 0, None, None, False
        self._thread = threading.Thread(target=self._consume, daemon=True)
        self._thread.start()

    # ------------------------------------------------------------------------------------------------ the thread
    def _consume(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            make, names, buf = item
            try:
                if self._error is None:
                    dicts = make()
                    names = [graph_file_name(d) for d in dicts] if names is None else names
                    for d, name in zip(dicts, names):
                        path = self.outdir / name
                        if not self.redo and path.is_file():
                            continue
                        _write(d, path)
                        self.written.append(path)
            except BaseException as e:   # kept for close(); later items are dropped, the producers never block
                self._error = e
            finally:
                del make
                if buf is not None:
                    self._buffers.put(buf)

    # ------------------------------------------------------------------------------------------------- producers
    def _buffer(self, nbytes: int) -> torch.Tensor:
        try:
            buf = self._buffers.get_nowait()
        except queue.Empty:
            if self._n_buffers < self.depth:
                self._n_buffers += 1
                buf = None
            else:
                buf = self._buffers.get()
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
        return buf

    def write(self, data, names: Sequence[str] | None = None) -> None:
        if self._closed:
            raise RuntimeError("GraphWriter: closed")
        names = None if names is None else [str(n) for n in names]
        batch = not isinstance(data, (list, tuple)) and (getattr(data, "ptr", None) is not None
                                                         or getattr(data, "batch", None) is not None)
        if batch and _pack_wanted(self.pack, data):
            lay = EventLayout(data, "GraphWriter")
            n = lay.n_events
            if data.x.is_cuda:
                dev = data.x.device
                if self._side is None:
                    self._side = torch.cuda.Stream(dev)
                self._side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(self._side):
                    packed = pack_events(data, lay)
                    total = packed.event_ptr[-1]
                    buf = self._buffer(total)
                    buf[:total].copy_(packed.image[:total], non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(self._side)

                def make(packed=packed, buf=buf, total=total, done=done, data=data):
                    done.synchronize()       # (`data` and `packed` keep the device memory alive until here)
                    return packed.event_dicts(buf[:total])
            else:
                packed, buf = pack_events(data, lay), None

                def make(packed=packed):
                    return packed.event_dicts(packed.image[:packed.event_ptr[-1]])
        else:
            dicts, buf = _event_dicts(data, False), None
            n = len(dicts)

            def make(dicts=dicts):
                return dicts
        if names is not None and len(names) != n:
            if buf is not None:
                self._buffers.put(buf)
            raise ValueError(f"GraphWriter: {n} events, {len(names)} names")
        self._q.put((make, names, buf))

    def close(self) -> None:
        if not self._closed:
            self._closed = True
            self._q.put(None)
            self._thread.join()
        err, self._error = self._error, None
        if err is not None:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                      # the caller's error wins; the thread is still joined
            try:
                self.close()
            except BaseException:
                pass
        return False
