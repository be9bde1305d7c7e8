"""TEST INFRASTRUCTURE ONLY: the cases of the dataset writer (``csrc/pack.hip``, ``data.uncollate``, ``io.save_graphs`` /
``GraphWriter``, ``data_transformer``), shared by the emulator runner (test_dataset_io_emul.py) and the GPU runner
(test_dataset_io_gpu.py); a case takes the device and, where it writes files, a directory.

Every comparison is EXACT: the feature moves bytes and subtracts integers, so tensors are compared byte for byte
(floats through their uint8 image: a NaN equals itself), dtype for dtype and shape for shape.  The packer's oracle is
``pack_ref``, a numpy restatement of the descriptor semantics of include/gnntrk.h; the oracle of the round trips is the
list of events that went in.
"""

from __future__ import annotations

import ctypes
import pathlib

import numpy as np
import torch

import gnn_tracking_amd as G
import graph_builder_cases as GB
import point_cloud_cases as PC
from gnn_tracking_amd import _capi
from gnn_tracking_amd import io as gio
from gnn_tracking_amd.hparams import HyperparametersMixin

GOLDEN_GRAPH = pathlib.Path(__file__).resolve().parent / "golden" / "test_graph.pt"
RAW, SUB64, SUB32 = _capi.PACK_RAW, _capi.PACK_SUB_I64, _capi.PACK_SUB_I32
SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 257, 16385)            # (the last one spans more than one chunk)
DTYPES = (torch.bool, torch.uint8, torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.float64)
POISON = 0xA5


# ----------------------------------------------------------------------------------------------------- the packer
def raw_bytes(t):
    """the bytes of a tensor's elements in order, as numpy uint8"""
    t = t.detach().cpu().contiguous()
    return t.reshape(-1).view(torch.uint8).numpy().copy() if t.numel() else np.zeros(0, np.uint8)


def random_tensor(g, dtype, shape, device):
    """random bits of every dtype (bool: 0 / 1), so that every byte of an element matters"""
    n = int(np.prod(shape))
    es = torch.empty(0, dtype=dtype).element_size()
    if n == 0:
        return torch.empty(shape, dtype=dtype, device=device)
    if dtype == torch.bool:
        return torch.from_numpy(g.integers(0, 2, n).astype(np.bool_)).reshape(shape).to(device)
    b = torch.from_numpy(g.integers(0, 256, n * es, dtype=np.uint8))
    return b.view(dtype).reshape(shape).to(device)


def pack_ref(segs, image_bytes, poison):
    """numpy restatement: segs = [(source tensor, dst_off, mode, sub)]"""
    img = np.full(image_bytes, poison, np.uint8)
    covered = np.zeros(image_bytes, bool)
    for t, off, mode, sub in segs:
        src = raw_bytes(t)
        if mode == SUB64:
            src = (src.view(np.int64) - np.int64(sub)).view(np.uint8)
        elif mode == SUB32:
            src = (src.view(np.int32) - np.int32(sub)).view(np.uint8)
        assert not covered[off:off + len(src)].any(), "the test's segments overlap"
        img[off:off + len(src)] = src
        covered[off:off + len(src)] = True
    return img, covered


def run_pack(device, segs, image_bytes, poison=POISON):
    """the device's image for segs = [(CONTIGUOUS source view, dst_off, mode, sub)] over a poisoned buffer"""
    for t, *_ in segs:
        assert t.is_contiguous()
    table = np.array([[t.data_ptr(), off, t.numel() * t.element_size(), sub, mode] for t, off, mode, sub in segs],
                     np.int64).reshape(-1, 5)
    image = torch.full((max(image_bytes, 16),), poison, dtype=torch.uint8, device=device)
    keep = gio.pack_segments(table, image, image_bytes)
    out = image.cpu().numpy()[:image_bytes].copy()
    del keep
    return out


def check_pack(device, segs, image_bytes, what):
    want, covered = pack_ref(segs, image_bytes, POISON)
    got = run_pack(device, segs, image_bytes, POISON)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{what}: {len(bad)} bytes differ, the first at {bad[0]} (covered: {covered[bad[0]]})"
    # the same bytes twice: again, into a buffer with another poison; what no segment covers keeps the poison
    again = run_pack(device, segs, image_bytes, 0x3C)
    assert np.array_equal(again[covered], want[covered]), f"{what}: the second run differs"
    assert (again[~covered] == 0x3C).all() and (got[~covered] == POISON).all(), f"{what}: a byte outside the segments was written"
    return covered


def layout(tensors, align=16, gap=0):
    """destination offsets, each at a multiple of `align` with `gap` untouched bytes before it"""
    offs, at = [], 0
    for t in tensors:
        at = (at + gap + align - 1) // align * align
        offs.append(at)
        at += t.numel() * t.element_size()
    return offs, at + gap


def case_pack_sizes_and_dtypes(device):
    """every size of SIZES (bytes for the 1-byte dtypes, elements for the others) in every dtype, one launch"""
    g = np.random.default_rng(1)
    ts = [random_tensor(g, dt, (n,), device) for dt in DTYPES for n in SIZES]
    offs, total = layout(ts, gap=5)
    covered = check_pack(device, [(t, o, RAW, 0) for t, o in zip(ts, offs)], total, "sizes x dtypes")
    assert covered.sum() == sum(t.numel() * t.element_size() for t in ts) and not covered.all()


def case_pack_rows_and_views(device):
    """rows of 1, 3, 4 and 14 float32 (12- and 56-byte rows start off 16-byte alignment), sources whose storage offset
    is not 16-aligned (t[1:]), an odd destination offset, source and destination with the same odd misalignment"""
    g = np.random.default_rng(2)
    segs_t = []
    for width in (1, 3, 4, 14):
        for rows in (1, 5, 70, 300):
            t = random_tensor(g, torch.float32, (rows + 1, width), device)
            segs_t += [t[1:], t[:rows]]
    for dt in (torch.uint8, torch.bfloat16, torch.int32, torch.float64):
        t = random_tensor(g, dt, (1031,), device)
        segs_t += [t[1:], t[3:900]]
    assert any(t.data_ptr() % 16 for t in segs_t) and any(t.data_ptr() % 16 == 12 for t in segs_t)
    offs, total = layout(segs_t, gap=3)
    segs = [(t, o, RAW, 0) for t, o in zip(segs_t, offs)]
    b = random_tensor(g, torch.uint8, (20000,), device)
    assert b.data_ptr() % 16 == 0
    total = (total + 15) // 16 * 16
    odd = [(b[1:4000], total + 3), (b[4000:4010], total + 4003 + 7), (b[5003:9000], total + 8003),      # 1|3, 0|6, 11|3
           (b[9001:9002], total + 12001), (b[10005:20000], total + 16 * 800 + 5)]                        # same: 5|5, two chunks
    segs += [(t, o, RAW, 0) for t, o in odd]
    assert (odd[-1][0].data_ptr() - odd[-1][1]) % 16 == 0 and odd[-1][1] % 16 == 5
    check_pack(device, segs, total + 16 * 800 + 5 + 9995 + 11, "rows and views")


def case_pack_sub_modes(device):
    """int64 and int32 elements minus sub: sub 0, positive, and equal to every element (the result is 0); aligned and
    unaligned sources, destinations that are element-aligned only, lengths around the vector width and over one chunk"""
    g = np.random.default_rng(3)
    segs_t = []
    for dt, mode, align in ((torch.int64, SUB64, 8), (torch.int32, SUB32, 4)):
        for n in (0, 1, 2, 3, 4, 5, 64, 65, 2049, 4099):
            base = torch.from_numpy(g.integers(0, 2 ** 31 - 1, n + 1)).to(dt).to(device)
            for view in (base[:n], base[1:]):
                for sub in (0, 12345, None):
                    v = view
                    if sub is None:                          # every element equals sub
                        v, sub = torch.full_like(view, 777), 777
                    segs_t.append((v, mode, sub, 16))
                    segs_t.append((v.clone()[0:], mode, sub, align))
    offs, at = [], 0
    for v, _, _, align in segs_t:
        at = (at + 15) // 16 * 16 + (align if align < 16 else 0)          # element-aligned, off 16 for the narrow ones
        offs.append(at)
        at += v.numel() * v.element_size() + 1
    segs = [(v, o, mode, sub) for (v, mode, sub, _), o in zip(segs_t, offs)]
    check_pack(device, segs, at + 8, "sub modes")
    zero = [s for s in segs if s[3] == 777 and s[0].numel()][0]
    o, n = zero[1], zero[0].numel() * zero[0].element_size()
    assert not run_pack(device, [zero], at + 8)[o:o + n].any(), "element minus itself is not 0"


def case_pack_many_segments(device):
    """several hundred segments of mixed sizes and modes in one launch, placed in shuffled order with gaps"""
    g = np.random.default_rng(4)
    sizes = np.concatenate([g.integers(0, 200, 300), g.integers(200, 40000, 60), [0, 0, 16384, 16384 * 2, 16384 * 3 + 1]])
    g.shuffle(sizes)
    ts = []
    for i, n in enumerate(sizes):
        kind = i % 3
        if kind == 0:
            ts.append((random_tensor(g, torch.uint8, (int(n) + 1,), device)[i % 2:int(n) + i % 2], RAW, 0))
        elif kind == 1:
            ts.append((torch.from_numpy(g.integers(-5, 10 ** 12, int(n) // 8)).to(device), SUB64, int(g.integers(0, 1000))))
        else:
            ts.append((torch.from_numpy(g.integers(0, 10 ** 9, int(n) // 4).astype(np.int32)).to(device), SUB32,
                       int(g.integers(0, 1000))))
    assert len(ts) > 300
    offs, total = layout([t for t, _, _ in ts], gap=1)
    order = g.permutation(len(ts))                                   # (the table's order is not the image's)
    check_pack(device, [(ts[i][0], offs[i], ts[i][1], ts[i][2]) for i in order], total, "many segments")


def case_pack_nothing(device):
    image = torch.full((64,), POISON, dtype=torch.uint8, device=device)
    gio.pack_segments(np.zeros((0, 5), np.int64), image)
    assert (image.cpu().numpy() == POISON).all()
    empty = torch.zeros(0, dtype=torch.int64, device=device)
    assert (run_pack(device, [(empty, 16, SUB64, 3), (empty, 0, RAW, 0)], 64) == POISON).all()


def host_validation(lib):
    """every EINVAL of gnntrk_pack_segments, on host buffers and without a launch (a plan that passes holds no byte)"""
    err = lambda: lib.gnntrk_last_error()   # noqa: E731
    CH = _capi.PACK_CHUNK_BYTES
    src = (ctypes.c_uint8 * 64)()
    dst_raw = (ctypes.c_uint8 * 4096)()
    dst = ctypes.addressof(dst_raw) + (-ctypes.addressof(dst_raw)) % 16
    a = ctypes.addressof(src) + (-ctypes.addressof(src)) % 16

    def call(rows, chunks=None, n_segs=None, n_chunks=None, dst=dst, dst_bytes=2048, plan=True, segs=True):
        rows = np.array(rows, np.int64).reshape(-1, 5)
        if chunks is None:
            chunks = [(s, k) for s, r in enumerate(rows) for k in range(max(0, -(-int(r[2]) // CH)))]
        host = np.concatenate([rows.ravel(), np.array(chunks, np.int32).reshape(-1).view(np.int64)]) if len(rows) else np.zeros(1, np.int64)
        n_segs = len(rows) if n_segs is None else n_segs
        n_chunks = len(chunks) if n_chunks is None else n_chunks
        return lib.gnntrk_pack_segments(host.ctypes.data if segs else None, n_segs, host.ctypes.data if plan else None,
                                        n_chunks, dst, dst_bytes, None)

    assert lib.gnntrk_pack_plan_bytes(3, 7) == 3 * 40 + 7 * 8 and lib.gnntrk_pack_plan_bytes(0, 0) == 0
    assert lib.gnntrk_pack_plan_bytes(-1, 0) == 0 and lib.gnntrk_pack_plan_bytes(_capi.PACK_MAX_SEGS + 1, 0) == 0
    assert lib.gnntrk_pack_plan_bytes(1, _capi.PACK_MAX_CHUNKS + 1) == 0
    assert call([]) == 0 and call([], segs=False, plan=False, dst=None, dst_bytes=0) == 0          # n_segs == 0
    assert call([[a, 0, 0, 0, RAW], [0, 16, 0, 5, SUB64]]) == 0, err()                               # no byte: no launch
    assert call([], n_chunks=1) == 1 and b"without segments" in err()
    assert call([[a, 0, 0, 0, RAW]], segs=False) == 1 and b"NULL" in err()
    assert call([[a, 0, 0, 0, RAW]], plan=False) == 1 and b"NULL" in err()
    assert call([[a, 0, 0, 0, RAW]], dst=None) == 1 and b"NULL dst" in err()
    assert call([[a, 0, 0, 0, RAW]], dst=dst + 4) == 1 and b"16-byte aligned" in err()
    assert call([[0, 0, 8, 0, RAW]]) == 1 and b"NULL source" in err()
    assert call([[a, 0, 0, 0, RAW]], n_segs=-1) == 1 and call([[a, 0, 0, 0, RAW]], dst_bytes=-1) == 1
    assert call([[a, 0, 0, 0, RAW]], n_chunks=-1) == 1 and b"negative" in err()
    assert call([[a, 0, 0, 0, RAW]], n_segs=_capi.PACK_MAX_SEGS + 1) == 1 and str(_capi.PACK_MAX_SEGS).encode() in err()
    assert call([[a, 0, 0, 0, RAW]], n_chunks=_capi.PACK_MAX_CHUNKS + 1) == 1 and str(_capi.PACK_MAX_CHUNKS).encode() in err()
    assert call([[a, 2040, 9, 0, RAW]]) == 1 and b"beyond dst_bytes" in err()                        # offset + size
    assert call([[a, 2049, 0, 0, RAW]]) == 1 and b"beyond dst_bytes" in err()
    assert call([[a, 0, 2 ** 62, 0, RAW]], chunks=[]) == 1 and b"beyond dst_bytes" in err()           # (no overflow)
    assert call([[a, -16, 8, 0, RAW]]) == 1 and call([[a, 0, -8, 0, RAW]], chunks=[]) == 1 and b"negative" in err()
    assert call([[a, 0, 8, 0, 3]]) == 1 and b"unknown mode" in err()
    assert call([[a, 0, 12, 0, SUB64]]) == 1 and b"multiple of the element size" in err()
    assert call([[a, 0, 6, 0, SUB32]]) == 1 and b"multiple of the element size" in err()
    assert call([[a + 4, 0, 8, 0, SUB64]]) == 1 and b"misaligned" in err()
    assert call([[a, 4, 8, 0, SUB64]]) == 1 and b"misaligned" in err()
    assert call([[a + 2, 0, 8, 0, SUB32]]) == 1 and call([[a, 2, 8, 0, SUB32]]) == 1 and b"misaligned" in err()
    assert call([[a, 0, 8, 2 ** 31, SUB32]]) == 1 and b"int32" in err()
    # the chunk table: too few chunks, too many, the wrong segment, the wrong number inside the segment
    assert call([[a, 0, 8, 0, RAW]], chunks=[]) == 1 and b"do not fit" in err()
    assert call([[a, 0, 8, 0, RAW]], chunks=[(0, 0), (0, 1)]) == 1 and b"do not fit" in err()
    assert call([[a, 0, 8, 0, RAW], [a, 16, 8, 0, RAW]], chunks=[(0, 0), (0, 0)]) == 1 and b"chunk table" in err()
    assert call([[a, 0, 8, 0, RAW]], chunks=[(0, 1)]) == 1 and b"chunk table" in err()
    assert bytes(dst_raw) == bytes(4096), "a refused call wrote"


# --------------------------------------------------------------------------------------------- events for round trips
HITS = (5, 0, 70, 64, 257, 1, 2)
EDGES = (63, 0, 257, 64, 65, 1, 0)
TRUE_EDGES = (0, 0, 5, 130, 1, 0, 1)


def make_events(device, evtid0=100):
    """seven events with the node fields of ``graph_builder_cases.make_cloud``, random edges, a second index field with
    counts of its own, a bool and a bf16 field, ``evtid`` / ``s`` as ``GraphBuilder.build`` writes them and a string"""
    g = np.random.default_rng(5)
    out = []
    for i, (n, e, t) in enumerate(zip(HITS, EDGES, TRUE_EDGES)):
        rows = [(30.0 + g.uniform(0, 100), g.uniform(-3, 3), g.uniform(-500, 500), int(g.integers(0, 18)),
                 int(g.integers(0, 9)), float(g.uniform(0.1, 3))) for _ in range(n)]
        d = GB.to_data(GB.make_cloud(rows), device)
        ids = lambda m: torch.from_numpy(g.integers(0, max(n, 1), (2, m))).to(device)   # noqa: E731
        d.edge_index = ids(e)
        d.edge_attr = random_tensor(g, torch.float32, (e, 4), device)
        d.y = torch.from_numpy(g.integers(0, 2, e).astype(np.float32)).to(device)
        d.true_edge_index = ids(t)
        d.flag = random_tensor(g, torch.bool, (n,), device)
        d.emb = random_tensor(g, torch.bfloat16, (n, 3), device)
        d.evtid = torch.tensor([evtid0 + i], dtype=torch.int64, device=device)
        d.s = torch.tensor([i % 2], dtype=torch.int64, device=device)
        d.tag = f"event {i}"
        out.append(d)
    return out


def same_bytes(u, v):
    u, v = u.detach().cpu().contiguous(), v.detach().cpu().contiguous()
    return u.dtype == v.dtype and u.shape == v.shape and np.array_equal(raw_bytes(u), raw_bytes(v))


def assert_same_events(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} events, want {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        assert list(a.keys()) == list(b.keys()), f"{what}: event {i} has the fields {a.keys()}, want {b.keys()}"
        for k in b.keys():
            u, v = getattr(a, k), getattr(b, k)
            if torch.is_tensor(v):
                assert torch.is_tensor(u) and same_bytes(u, v), (
                    f"{what}: event {i}, {k}: {getattr(u, 'dtype', type(u))} {tuple(getattr(u, 'shape', ()))} against "
                    f"{v.dtype} {tuple(v.shape)}")
            else:
                assert type(u) is type(v) and u == v, f"{what}: event {i}, {k}: {u!r} against {v!r}"


def case_uncollate_round_trip(device):
    gs = make_events(device)
    batch = G.collate(gs)
    assert_same_events(G.uncollate(batch), gs, "uncollate(collate)")
    lay = G.EventLayout(batch)
    assert lay.kinds == dict(x="node", layer="node", particle_id="node", pt="node", reconstructable="node", sector="node",
                             eta="node", edge_index="index", edge_attr="edge", y="edge", true_edge_index="index",
                             flag="node", emb="node", evtid="event", s="event", tag="list")
    assert lay.edge_ptr["edge_index"] == np.concatenate([[0], np.cumsum(EDGES)]).tolist()
    assert lay.edge_ptr["true_edge_index"] == np.concatenate([[0], np.cumsum(TRUE_EDGES)]).tolist()
    del batch.ptr                                               # the offsets from `batch`
    assert_same_events(G.uncollate(batch), gs, "uncollate by `batch`")
    for g in (gs[3], gs[1]):                                    # one event; 64 hits and 64 edges: the name rule decides
        assert_same_events(G.uncollate(G.collate([g])), [g], "one event")
    # anything else is copied to every event; the precedence: y of a batch with as many edges as hits is edge-level
    two = G.collate(gs[2:4])
    two.scale = torch.arange(5.0, device=device)
    two.note = "n"
    for d in G.uncollate(two):
        assert torch.equal(d.scale, two.scale) and d.note == "n"
    d = G.uncollate(G.collate([gs[3]]))[0]
    assert d.y.shape[0] == d.pt.shape[0] == 64


def case_uncollate_built(device):
    """graphs from GraphBuilder.build, clouds from PointCloudBuilder.build, tests/golden/test_graph.pt"""
    b = G.GraphBuilder(**GB.WIDE)
    clouds = [GB.to_data(c, device) for c in GB.batch_clouds()]
    graphs = [b.build(c, evtid=5, s=2) for c in clouds]
    assert graphs[0].num_edges > 100 and graphs[1].num_nodes == 0
    assert_same_events(G.uncollate(G.collate(graphs)), graphs, "graphs of GraphBuilder")
    assert_same_events(G.uncollate(b.build(G.collate(clouds), evtid=5, s=2)), graphs, "the graph of a collated batch")
    pcb = G.PointCloudBuilder(detector=G.load_detector(PC.detector_table()), n_sectors=3, add_true_edges=True)
    tables = PC.on(PC.random_event(3, 257), device)
    pcs = pcb.build(tables, evtid=1)
    assert sum(c.num_edges for c in pcs) > 0
    assert_same_events(G.uncollate(G.collate(pcs)), pcs, "clouds of PointCloudBuilder")
    assert_same_events(G.uncollate(pcb.build(tables, evtid=1, collated=True)), pcs, "the collated clouds")
    g = G.load_graph(GOLDEN_GRAPH, device)
    assert_same_events(G.uncollate(G.collate([g, g])), [g, g], "test_graph.pt")


def bad_batches(device):
    """(what, batch): a cross-event edge, an id outside the batch, a negative id, events' edges out of order"""
    gs = make_events(device)
    n0 = HITS[0]

    def with_edges(fn, field="edge_index"):
        b = G.collate(gs)
        setattr(b, field, fn(getattr(b, field).clone()))
        return b

    def cross(e):
        e[1, 3] = n0 + 2
        return e

    def beyond(e):
        e[0, -1] = sum(HITS)
        return e

    def negative(e):
        e[1, 0] = -1
        return e

    def swapped(e):
        return torch.cat([e[:, EDGES[0]:], e[:, :EDGES[0]]], dim=1)

    def far(e):                      # (the second index field has counts of its own: a pair from event 2 to event 0)
        return torch.cat([e[:, :2], torch.tensor([[HITS[0] + HITS[2]], [0]], device=device), e[:, 2:]], dim=1)

    return [("between two events", with_edges(cross)), ("outside", with_edges(beyond)), ("outside", with_edges(negative)),
            ("event order", with_edges(swapped)), ("between two events", with_edges(far, "true_edge_index"))]


def case_bad_edges(device, tmp):
    """cross-event, out-of-range and out-of-order edges raise ValueError before anything is written"""
    out = tmp / "bad"
    out.mkdir()
    for what, batch in bad_batches(device):
        for call in (lambda: G.uncollate(batch), lambda: G.save_graphs(batch, [out / f"{i}.pt" for i in range(len(HITS))], pack=True),
                     lambda: G.save_graphs(batch, [out / f"{i}.pt" for i in range(len(HITS))], pack=False)):
            try:
                call()
            except ValueError as e:
                assert what in str(e), f"{what}: {e}"
            else:
                raise AssertionError(f"{what}: no ValueError")
        w = G.GraphWriter(out, pack=True)
        try:
            w.write(batch)
        except ValueError as e:
            assert what in str(e)
        else:
            raise AssertionError(f"{what}: GraphWriter.write raised nothing")
        finally:
            w.close()
    assert not list(out.iterdir()), "something was written"


def load_all(paths):
    return [G.load_graph(p) for p in paths]


def case_save_graphs(device, tmp):
    """save_graphs (packer and composed path) -> load_graph; weights_only; a file holds its own event only"""
    gs = make_events(device)
    batch = G.collate(gs)
    for pack in (True, False):
        d = tmp / f"pack{int(pack)}"
        d.mkdir()
        paths = [d / f"e{i}.pt" for i in range(len(gs))]
        G.save_graphs(batch, paths, pack=pack)
        assert_same_events(load_all(paths), [g.cpu() for g in gs], f"save_graphs(pack={pack})")
        f = torch.load(paths[2], weights_only=True)
        assert isinstance(f, dict) and list(f) == gs[2].keys() and f["tag"] == "event 2" and f["x"].device.type == "cpu"
        assert same_bytes(f["emb"], gs[2].emb) and f["edge_index"].is_contiguous()
        assert not list(d.glob("*tmp*"))
        alone = d / "alone.pt"
        G.save_graph(gs[4], alone)                                      # the 257-hit event, written alone
        assert_same_events(load_all([alone]), [gs[4].cpu()], "save_graph")
        assert paths[0].stat().st_size < alone.stat().st_size, "the 5-hit event's file carries the batch"
    lst = tmp / "list"
    lst.mkdir()
    G.save_graphs(gs, [lst / f"e{i}.pt" for i in range(len(gs))])
    assert_same_events(load_all([lst / f"e{i}.pt" for i in range(len(gs))]), [g.cpu() for g in gs], "a list of events")
    try:
        G.save_graphs(batch, [lst / "x.pt"], pack=True)
    except ValueError as e:
        assert "7 events, 1 paths" in str(e)
    else:
        raise AssertionError("a wrong number of paths was accepted")


def case_packed_image(device):
    """the packed form: every field of every event at a 16-byte boundary of the event's image, one launch"""
    gs = make_events(device)
    packed = G.pack_events(G.collate(gs))
    assert packed.n_events == len(gs) and all(o % 16 == 0 for o in packed.event_ptr)
    for k, meta in packed.fields.items():
        if meta is not None:
            assert all(o % 16 == 0 for o in meta[2]), k
    dicts = packed.event_dicts(packed.image[:packed.event_ptr[-1]].cpu())
    assert_same_events([G.Data(**d) for d in dicts], [g.cpu() for g in gs], "pack_events")
    for d, (a, z) in zip(dicts, zip(packed.event_ptr, packed.event_ptr[1:])):
        sizes = [t.untyped_storage().nbytes() for t in d.values() if torch.is_tensor(t)]
        assert sizes == [t.numel() * t.element_size() for t in d.values() if torch.is_tensor(t)] and sum(sizes) <= z - a, \
            "a tensor of an event carries more than its own bytes of the event's image"


def case_graph_writer(device, tmp):
    """GraphWriter -> GraphDataset; default names; redo=False leaves files alone; a thread error surfaces at close()"""
    gs = make_events(device)
    want = [g.cpu() for g in gs]
    for pack in (True, False):
        out = tmp / f"writer{int(pack)}"
        out.mkdir()
        with G.GraphWriter(out, pack=pack) as w:
            w.write(G.collate(gs[:3]))
            w.write(gs[3])
            w.write(G.collate(gs[4:]))
        names = [f"data{100 + i}_s{i % 2}.pt" for i in range(len(gs))]
        assert sorted(p.name for p in out.iterdir()) == sorted(names) and [p.name for p in w.written] == names
        ds = G.GraphDataset(out)
        assert_same_events([ds[i] for i in range(len(ds))], want, f"GraphWriter(pack={pack})")
        # redo=False: an existing file keeps its content, a missing one is written
        (out / names[1]).write_bytes(b"sentinel")
        (out / names[2]).unlink()
        with G.GraphWriter(out, pack=pack, redo=False) as w:
            w.write(G.collate(gs[:3]))
        assert (out / names[1]).read_bytes() == b"sentinel" and [p.name for p in w.written] == [names[2]]
        assert_same_events(load_all([out / names[2]]), [want[2]], "redo=False")
        with G.GraphWriter(out, pack=pack) as w:
            w.write(G.collate(gs[:2]), names=["a.pt", "b.pt"])
        assert_same_events(load_all([out / "a.pt", out / "b.pt"]), want[:2], "given names")
        w = G.GraphWriter(tmp / "no" / "such" / "directory", pack=pack)
        w.write(G.collate(gs[:3]))
        w.write(gs[3])
        try:
            w.close()
        except (OSError, RuntimeError) as e:                            # (torch.save's own refusal of the path)
            assert "directory" in str(e), str(e)
        else:
            raise AssertionError("the thread's error did not surface at close()")
        w.close()                                                       # (raised once)
        try:
            w.write(gs[0])
        except RuntimeError as e:
            assert "closed" in str(e)
        else:
            raise AssertionError("write after close")


# --------------------------------------------------------------------------------------------------------- stages
class StubEC(torch.nn.Module, HyperparametersMixin):
    """W is the first edge feature as it is: the test decides every score"""

    def __init__(self, column: int = 0):
        super().__init__()
        self.save_hyperparameters()

    def forward(self, data):
        return {"W": data.edge_attr[:, self.hparams.column].contiguous()}


def scored_events(device):
    gs = make_events(device)
    g = np.random.default_rng(6)
    for d in gs:
        w = g.uniform(0, 1, d.num_edges).astype(np.float32)
        if len(w) > 8:
            w[1], w[5], w[6] = 0.3, np.nan, np.nextafter(np.float32(0.3), np.float32(1))      # == thld, NaN, just above
        d.edge_attr[:, 0] = torch.from_numpy(w).to(device)
    return gs


def restated_cut(d, thld, name=None):
    """edge_subgraph of the restated mask, on the host: strict, float32, NaN kept in no graph"""
    d = d.cpu()
    w = (d.edge_attr[:, 0] if name is None else d[name]).numpy()
    assert w.dtype == np.float32
    mask = torch.from_numpy(w > np.float32(thld))
    if name is None:
        d.ec_score = d.edge_attr[:, 0].clone()
    return d.edge_subgraph(mask), int(mask.sum())


def case_eccut(device):
    gs = scored_events(device)
    cut = G.ECCut(StubEC(), thld=0.3)
    assert dict(cut.hparams) == {"thld": 0.3, "ec": {"class_path": f"{StubEC.__module__}.StubEC", "init_args": {"column": 0}}}
    assert dict(G.ECCutRefine(0.5).hparams) == {"thld": 0.5, "name": "ec_score"}
    n_nan = 0
    for thld in (0.3, -1.0, 2.0):                                       # a cut, all kept (but NaN), none kept
        cut = G.ECCut(StubEC(), thld=thld)
        wants = [restated_cut(d, thld) for d in gs]
        got = [cut(G.Data(**{k: d[k] for k in d.keys()})) for d in gs]
        assert_same_events(got, [w for w, _ in wants], f"ECCut({thld})")
        for d, g_, (w, n) in zip(gs, got, wants):
            assert g_.num_edges == n == g_.ec_score.shape[0] == g_.edge_attr.shape[0] == g_.y.shape[0]
            assert g_.true_edge_index.shape == d.true_edge_index.shape and not torch.isnan(g_.ec_score).any()
            if thld == 0.3 and d.num_edges > 8:
                kept = set(g_.ec_score.cpu().numpy().view(np.uint32).tolist())
                assert np.float32(0.3).view(np.uint32) not in kept and np.nextafter(np.float32(0.3), np.float32(1)).view(np.uint32) in kept
            if thld == -1.0:
                n_nan += d.num_edges - n
            if thld == 2.0:
                assert n == 0
        # the collated batch: the events independently, batch and ptr as they were
        out = cut(G.collate(gs))
        assert_same_events(G.uncollate(out), [w for w, _ in wants], f"ECCut({thld}) of a batch")
    assert n_nan == sum(d.num_edges > 8 for d in gs)
    # ECCutRefine on the output of ECCut with a higher threshold
    first = [G.ECCut(StubEC(), thld=0.3)(G.Data(**{k: d[k] for k in d.keys()})) for d in gs]
    refined = [G.ECCutRefine(0.6)(d) for d in first]
    assert_same_events(refined, [restated_cut(d, 0.6, "ec_score")[0] for d in first], "ECCutRefine")
    assert sum(d.num_edges for d in refined) < sum(d.num_edges for d in first) < sum(d.num_edges for d in gs)


def write_inputs(gs, d):
    d.mkdir()
    names = [f"data{21000 + i}_s0.pt" for i in range(len(gs))]
    G.save_graphs(gs, [d / n for n in names])
    return names


def case_transformer_batching(device, tmp):
    """DataTransformer(ECCut(stub)) with batch_size=3 over 7 files writes the files of batch_size=1"""
    gs = scored_events(device)
    names = write_inputs(gs, tmp / "in")
    dt = G.DataTransformer(G.ECCut(StubEC(), thld=0.3), device=device)
    dt.process_directories([tmp / "in"], [tmp / "one"])
    dt.process_directories([tmp / "in"], [tmp / "three"], batch_size=3)
    one, three = load_all([tmp / "one" / n for n in names]), load_all([tmp / "three" / n for n in names])
    assert_same_events(three, one, "batch_size=3 against batch_size=1")
    assert_same_events(one, [restated_cut(d, 0.3)[0] for d in gs], "the written cut graphs")
    assert sorted(p.name for p in (tmp / "three").iterdir()) == sorted(names + ["hparams"])
    dt.process(names[4], input_dir=tmp / "in", output_dir=tmp / "single")
    assert_same_events(load_all([tmp / "single" / names[4]]), [one[4]], "process")
    (tmp / "single" / names[4]).write_bytes(b"kept")
    dt.process(names[4], input_dir=tmp / "in", output_dir=tmp / "single", redo=False)
    assert (tmp / "single" / names[4]).read_bytes() == b"kept"


def case_smoke_eccut_efmlp(device, tmp):
    """the reference's test_eccut: ECCut(EFMLP(hidden_dim=3, depth=1)) on the test graph; structure only"""
    g = G.load_graph(GOLDEN_GRAPH, device)
    (tmp / "in").mkdir()
    G.save_graph(g, tmp / "in" / "data21000_s0.pt")
    torch.manual_seed(0)
    ec = G.EFMLP(node_indim=g.num_node_features, edge_indim=g.num_edge_features, hidden_dim=3, depth=1).to(device)
    dt = G.DataTransformer(G.ECCut(ec, thld=0.3), device=device)
    dt.process_directories(input_dirs=[tmp / "in"], output_dirs=[tmp / "transformed"], n_files=1, seed=1)
    out = G.load_graph(tmp / "transformed" / "data21000_s0.pt")
    assert out.keys() == [*g.keys(), "ec_score"]
    with torch.no_grad():
        w = ec(g)["W"]
    n = int((w > 0.3).sum())
    assert out.num_edges == n == out.ec_score.shape[0] == out.edge_attr.shape[0] == out.y.shape[0] and out.num_nodes == g.num_nodes
    assert out.ec_score.dtype == torch.float32 and bool((out.ec_score > 0.3).all())
    assert "thld: 0.3" in (tmp / "transformed" / "hparams").read_text()


def case_smoke_ml_graph_construction(device, tmp):
    """the reference's test_data_transformer: MLGraphConstruction(GraphConstructionFCNN, use_embedding_features=True)"""
    g = G.load_graph(GOLDEN_GRAPH, device)
    (tmp / "in").mkdir()
    G.save_graph(g, tmp / "in" / "data21000_s0.pt")
    torch.manual_seed(0)
    ml = G.GraphConstructionFCNN(in_dim=g.num_node_features, out_dim=g.num_node_features, hidden_dim=3, depth=2, alpha=0.5)
    gc = G.MLGraphConstruction(ml=ml.to(device), use_embedding_features=True)
    G.DataTransformer(transform=gc, device=device).process_directories(
        input_dirs=[tmp / "in"], output_dirs=[tmp / "transformed"], n_files=1)
    out = G.load_graph(tmp / "transformed" / "data21000_s0.pt")
    assert {"x", "edge_index", "y", "edge_attr"} <= set(out.keys())
    assert out.num_nodes == g.num_nodes and out.x.shape[1] == 2 * g.num_node_features
    assert out.edge_index.shape[0] == 2 and out.y.shape[0] == out.num_edges == out.edge_attr.shape[0]
    assert out.num_edges == 0 or int(out.edge_index.max()) < out.num_nodes


def write_csv_event(tables, prefix):
    for name, cols in tables.items():
        keys = list(cols)
        with open(f"{prefix}-{name}.csv", "w") as f:
            f.write(",".join(keys) + "\n")
            for row in zip(*[np.asarray(cols[k]).tolist() for k in keys]):
                f.write(",".join(repr(v) for v in row) + "\n")


def case_build_loops(device, tmp):
    """build_point_clouds, then build_graphs, on two tiny synthetic TrackML events written as CSV: the graphs read
    back from disk are GraphBuilder.build(PointCloudBuilder.build(...)) computed in memory"""
    indir, pcdir, gdir = tmp / "csv", tmp / "clouds", tmp / "graphs"
    for d in (indir, pcdir, gdir):
        d.mkdir()
    evtids = (21007, 21003)
    for seed, evtid in enumerate(evtids):
        write_csv_event(PC.random_event(seed + 10, 300), indir / f"event{evtid:09d}")
    det = G.load_detector(PC.detector_table())
    pcb = G.PointCloudBuilder(detector=det, n_sectors=2, measurement_mode=True)
    written = G.build_point_clouds(pcb, indir, pcdir)
    names = [f"data{e}_s{s}.pt" for e in sorted(evtids) for s in (0, 1)]
    assert [p.name for p in written] == names == sorted(p.name for p in pcdir.iterdir())
    mem = G.PointCloudBuilder(detector=det, n_sectors=2, measurement_mode=True)
    clouds = {}
    for e in sorted(evtids):
        tables = PC.on(G.read_event(indir / f"event{e:09d}"), device)
        for s, c in enumerate(mem.build(tables, evtid=e)):
            clouds[f"data{e}_s{s}.pt"] = c
    assert_same_events(load_all([pcdir / n for n in names]), [clouds[n].cpu() for n in names], "the cloud files")
    assert pcb.stats == mem.stats and len(pcb.measurements) == len(mem.measurements) == 4
    assert G.build_point_clouds(pcb, indir, pcdir, redo=False) == [] and G.build_point_clouds(pcb, indir, pcdir, start=1, stop=1) == []

    gb = G.GraphBuilder(measurement_mode=True, **GB.WIDE)
    assert [p.name for p in G.build_graphs(gb, pcdir, gdir)] == names[:1]          # the reference's default: one file
    written = G.build_graphs(gb, pcdir, gdir, start=0, stop=None, batch_size=3, redo=False)
    assert [p.name for p in written] == names[1:] and sorted(p.name for p in gdir.iterdir()) == names
    memb = G.GraphBuilder(measurement_mode=True, **GB.WIDE)
    want = []
    for n in names:
        e, s = (int(v) for v in n[4:-3].split("_s"))
        want.append(memb.build(clouds[n], evtid=e, s=s).cpu())
    assert sum(w.num_edges for w in want) > 20
    got = load_all([gdir / n for n in names])
    assert_same_events(got, want, "the graph files")
    assert [int(g_.evtid) for g_ in got] == [e for e in sorted(evtids) for _ in (0, 1)] and [int(g_.s) for g_ in got] == [0, 1, 0, 1]
    assert len(gb.measurements) == 4
    for a, b in zip(gb.measurements, memb.measurements):
        GB.assert_record(a, b, "measurements of the loop")
    only = tmp / "only"
    only.mkdir()
    assert [p.name for p in G.build_graphs(gb, pcdir, only, stop=None, only_sector=1)] == [names[1], names[3]]
    (pcdir / "cloud7.pt").write_bytes(b"")
    try:
        G.build_graphs(gb, pcdir, only, stop=None)
    except ValueError as e:
        assert str(e) == "cloud7.pt is not a valid file name"
    else:
        raise AssertionError("a badly named file was accepted")
    (pcdir / "notes.txt").write_text("skipped: not .pt")
    (pcdir / "cloud7.pt").unlink()
    assert len(G.build_graphs(gb, pcdir, only, stop=None)) == 4


PACK_CASES = (case_pack_sizes_and_dtypes, case_pack_rows_and_views, case_pack_sub_modes, case_pack_many_segments,
              case_pack_nothing)
CASES = (case_uncollate_round_trip, case_uncollate_built, case_packed_image, case_eccut)
DIR_CASES = (case_bad_edges, case_save_graphs, case_graph_writer, case_transformer_batching, case_smoke_eccut_efmlp,
             case_smoke_ml_graph_construction, case_build_loops)
