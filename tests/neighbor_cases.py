"""Neighbour-search cases shared by the emulator tests (tests/test_neighbor_emul.py) and the GPU tests
(tests/test_neighbor_gpu.py): the kNN search, its collated form, the count scan (csrc/knn.hip), the radius graph and
the DBSCAN labelling (csrc/dbscan.hip) at every padded width, every k class, the tile edges in the number of points,
the batch geometry of the pruned search, and the edge values of the radius (which shape reaches which
kernel, instantiation and loop edge).

Oracles (oracle/ref_cpu.py): ``knn_graph_c`` (oracle/knn_ref.c: fmaf chain, (d2, index) order, ``sqrtf(d2) < r``),
``radius_neighbors`` / ``radius_neighbors_blocked`` (fp64 sequential sum, ``d2 <= r^2``) and ``dbscan_labels``.  Every
comparison is ``torch.equal`` / ``numpy.array_equal``: indices, counts, offsets, fp64 distances, labels.  There is no
tolerance in this file.  Collated batches are compared with the per-event oracle lists, concatenated with their offsets.

Clouds (``cloud``) are drawn as ``parity_cases.case_knn_pruned`` draws them - clustered centres, every eleventh point a
noise hit, exact duplicates (ties by index) - from a generator seeded by the case's own parameters.  Every case asserts
on the ORACLE's output that what it is there for occurs: that k binds (some query has more than k candidates inside
the radius), that the radius binds, that there are at least two 4096-point batches, that an empty event is present."""

from __future__ import annotations

import contextlib
import functools
import math
import zlib

import numpy as np
import torch

from gnn_tracking_amd import _capi, ops, postprocessing
import ref_cpu as O

BRUTE, PRUNED = 2, 1          # ops._KNN_FLAGS / postprocessing.RADIUS_FLAGS
FLAGS = (BRUTE, PRUNED)
EMPTY = torch.empty(2, 0, dtype=torch.int64)

#: 1: both ends of each padded width class (DP = 4, 8, 16, 32; the pruned search covers 4, 8, 16)
KNN_WIDTHS = (1, 3, 4, 5, 8, 9, 16, 17, 31, 32)
KNN_PRUNED_WIDTHS = (1, 4, 5, 8, 9, 16)
FALLBACK_WIDTHS = (17, 32)
#: 2: both ends of each buffer class (cap = 128 up to k = 64, 256 up to 192, 512 up to 448)
K_CLASSES = (1, 63, 64, 65, 192, 193, 448)
K_CLASS_WIDTHS = (3, 12)
OVERFLOW_SHAPES = ((64, 700), (448, 2600))          # (k, n): n >= 5 * cap
#: 3: around the 64-candidate chunk, the 32 / 16 / 8 queries of a wave, the block of 4 waves
KNN_N_EDGES = (2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
KNN_N_EDGE_WIDTHS = (3, 12)
#: 3: n -> (dim, k, radius): around the 64-point sorted chunk and the batch of 64 chunks
KNN_PRUNED_N = {63: (3, 4, 0.05), 64: (3, 4, 0.05), 65: (3, 4, 0.05), 4095: (3, 4, 0.05), 4096: (3, 4, 0.05),
                4097: (3, 4, 0.05), 8192: (3, 16, 0.1), 8193: (3, 16, 0.1), 12289: (8, 8, 0.3)}
#: 4: event sizes of a collated batch
EVENTS = {"empty_events": (0, 5, 0, 0, 70, 1, 64, 0), "tiny_events": (1, 2, 1, 2, 2), "one_event": (77,)}
BIG_EVENTS = (4000, 200, 4100, 1, 3000)
NO_EDGE_RADII = (0.0, -0.5, float("nan"))
#: 7: around the 256-count chunk of a lane group, the 4 x 256 and 4 x 2048 steps of a block, the 256 -> 1024 threads
SCAN_N = (1, 3, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 65535, 65536, 65537)
#: 8: both ends of each padded width class of the radius graph (D = 2, 4, 8, 16, 32; pruned 4, 8, 16)
RADIUS_WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
#: 9: around the 16 / 8 queries of a pruned block, the 64-point chunk, the 256-point tile, two tiles + 1
RADIUS_N_EDGES = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
RADIUS_N_EDGE_WIDTHS = (3, 12)
RADIUS_BOX_LOOP_N = (4095, 4096, 4097)
#: 10: around the ordering kernel's LDS capacity
LIST_LENGTHS = (1023, 1024, 1025)
DBSCAN_SHAPES = ("chain_reversed", "chain_zigzag", "shared_border", "border_first", "all_core", "all_noise",
                 "duplicates", "rescans")


# --------------------------------------------------------------------------------------------------- clouds
def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode())


@functools.lru_cache(maxsize=None)
def cloud(n: int, dim: int, tag: str = "", corner: bool = False) -> torch.Tensor:
    """fp32 [n, dim] (shared between the cases that use it: never written to).  ``corner``: the last three points are
    a clump of 1e-3 at the upper corner of the bounding box - the corner itself has the largest Morton code, so it is
    the last point of the sorted order (alone in the last chunk where n % 64 == 1) and its two neighbours precede it."""
    g = np.random.default_rng(_seed("cloud", n, dim, tag))
    centres = g.uniform(-2, 2, size=(max(n // 30, 1), dim))
    x = centres[g.integers(0, len(centres), size=n)] + 0.05 * g.normal(size=(n, dim))
    x[::11] = g.uniform(-2, 2, size=(len(x[::11]), dim))      # noise hits
    x[5::50] = x[4::50][:len(x[5::50])]                       # exact duplicates: ties by index
    if corner:
        top = x[:-3].max(0) + 0.25
        x[-1] = top
        x[-2] = top - 1e-3
        x[-3] = top - 2e-3
    return torch.from_numpy(x.astype(np.float32))


def cluster_radius(dim: int) -> float:
    """about the median distance of two points of one cluster (0.05 * normal per coordinate)"""
    return 0.05 * math.sqrt(2.0 * dim)


@contextlib.contextmanager
def knn_flags(flags: int):
    old = ops._KNN_FLAGS
    ops._KNN_FLAGS = flags
    try:
        yield
    finally:
        ops._KNN_FLAGS = old


@contextlib.contextmanager
def radius_flags(flags: int):
    old = postprocessing.RADIUS_FLAGS
    postprocessing.RADIUS_FLAGS = flags
    try:
        yield
    finally:
        postprocessing.RADIUS_FLAGS = old


def knn(device, x, k, r, flags, seg_ptr=None):
    with knn_flags(flags):
        ei = ops.knn_graph(x.to(device), k, r, seg_ptr=None if seg_ptr is None else seg_ptr.to(device))
    assert ei.dtype == torch.int64 and ei.dim() == 2 and ei.shape[0] == 2
    return ei.cpu()


# ------------------------------------------------------------------------------------------------ kNN oracle
_ORACLE: dict = {}


def knn_ref(x: torch.Tensor, k: int, r) -> torch.Tensor:
    """the C oracle's edge list, computed once per (cloud, k, radius)"""
    key = (x.data_ptr(), tuple(x.shape), k, r)
    if key not in _ORACLE:
        _ORACLE[key] = (x, O.knn_graph_c(x, k, r) if x.shape[0] > 1 else EMPTY)   # (holds x: the key stays unique)
    return _ORACLE[key][1]


def knn_ref_events(x, sizes, k, r) -> torch.Tensor:
    parts, off = [EMPTY], 0
    for s in sizes:
        if s > 1:
            parts.append(O.knn_graph_c(x[off:off + s].contiguous(), k, r) + off)
        off += s
    return torch.cat(parts, dim=1)


def row_counts(ei, n) -> torch.Tensor:
    return torch.bincount(ei[1], minlength=n)


def assert_k_binds(x, k, r, want):
    """some query has more than k candidates (inside the radius): the oracle finds k + 1 for it"""
    n = x.shape[0]
    assert k + 1 <= n - 1
    assert int(row_counts(want, n).max()) == k
    assert int(row_counts(knn_ref(x, k + 1, r), n).max()) == k + 1, "k does not bind in this cloud"


def assert_radius_binds(x, k, want):
    assert int(row_counts(want, x.shape[0]).min()) < min(k, x.shape[0] - 1), "the radius does not bind in this cloud"


def seg_ptr_of(sizes) -> torch.Tensor:
    return torch.tensor([0, *np.cumsum(sizes)], dtype=torch.int64)


# ------------------------------------------------------------------------------------------- 1: every width
def case_knn_width(device, dim, flags):
    """n = 130, k = 5, without a radius and with one that binds for the noise hits while k binds inside the clusters:
    ``knn_kernel<DP, FULL, false, QW>`` at DP = 4, 8, 16, 32 with dim == DP and dim < DP (QW = 8 up to 8 dimensions,
    0 beyond), ``knn_pruned_kernel<DP, false, QW>`` at DP = 4, 8, 16 (QW = 8 up to 8 dimensions, 4 beyond)."""
    n, k = 130, 5
    x = cloud(n, dim, "width")
    if flags == PRUNED:
        assert int(_capi.load().gnntrk_knn_workspace_bytes(n, dim, k)) > 0
    for r in (None, cluster_radius(dim)):
        want = knn_ref(x, k, r)
        assert_k_binds(x, k, r, want)
        if r is not None:
            assert_radius_binds(x, k, want)
        assert torch.equal(knn(device, x, k, r, flags), want), f"kNN dim={dim} r={r} flags={flags}"


def case_knn_width_fallback(device, dim):
    """beyond 16 dimensions the pruned form has no workspace: the brute-force launch runs, with the same bits"""
    n, k = 130, 5
    x = cloud(n, dim, "width")
    assert int(_capi.load().gnntrk_knn_workspace_bytes(n, dim, k)) == 0
    for r in (None, cluster_radius(dim)):
        got = knn(device, x, k, r, PRUNED)
        assert torch.equal(got, knn(device, x, k, r, BRUTE)), f"fallback dim={dim} r={r}: pruned flag != brute force"
        assert torch.equal(got, knn_ref(x, k, r)), f"fallback dim={dim} r={r}"


def case_knn_width_refused(device, flags):
    x = cloud(40, 33, "width")
    for r in (None, 1.0):
        try:
            knn(device, x, 5, r, flags)
        except NotImplementedError as e:
            assert "dim > 32" in str(e)
        else:
            raise AssertionError(f"33 dimensions were not refused (flags={flags}, r={r})")


# ------------------------------------------------------------------------------------------ 2: every k class
def case_knn_k_class(device, k, dim, flags):
    """n = k + 12: every query has k + 11 candidates, so without a radius k binds everywhere; with the radius 1.5 it
    binds for some queries (small k) or for none (large k).  cap = 128 / 256 / 512 and qw = 8 / 4 / 2: in 3 dimensions
    ``knn_kernel<4, .., QW = 8 / 4 / 0>``, in 12 always QW = 0; ``knn_pruned_kernel<DP, false, 8 / 4 / 2>`` (12
    dimensions: 4 / 4 / 2)."""
    n = k + 12
    x = cloud(n, dim, "k_class")
    for r in (None, 1.5):
        want = knn_ref(x, k, r)
        if r is None:
            assert bool((row_counts(want, n) == k).all())
        elif k >= 63:
            assert_radius_binds(x, k, want)
        assert torch.equal(knn(device, x, k, r, flags), want), f"kNN k={k} dim={dim} r={r} flags={flags}"


def case_knn_k_refused(device, flags):
    x = cloud(500, 3, "k_class")
    try:
        knn(device, x, 449, None, flags)
    except NotImplementedError as e:
        assert "k > 448" in str(e)
    else:
        raise AssertionError(f"k = 449 was not refused (flags={flags})")


def case_knn_k_clipped(device, flags):
    """k > n - 1 is clipped to n - 1: every other point, nearest first"""
    x = cloud(20, 3, "k_class")
    want = knn_ref(x, 19, None)
    assert want.shape[1] == 20 * 19
    for k in (20, 100, 449, 5000):
        assert torch.equal(knn(device, x, k, None, flags), want), f"k={k} at n=20"


@functools.lru_cache(maxsize=None)
def _descending_line(n):
    t = (n - np.arange(n, dtype=np.float64)) * 0.01
    return torch.from_numpy(np.stack([t, 0.5 * t, -0.25 * t], 1).astype(np.float32))


def case_knn_overflow(device, k, n, flags):
    """No radius, points in descending order along a line: for the last query every candidate in index order is
    nearer than all before it, so it passes whatever the threshold has become - the buffer (cap = 128 for k = 64, 512
    for k = 448; n >= 5 * cap) fills and is cut to its k best again and again.  The first queries see the opposite
    (nothing passes after the first cut), those in between both.  (k = 448 takes 16 to 20 s on the emulator - 2600
    queries that sort 512 keys after nearly every chunk - and is run by the device runner only.)"""
    cap = 128
    while cap < k + 64:
        cap <<= 1
    assert n >= 5 * cap
    x = _descending_line(n)
    d2_last = ((x[:-1].double() - x[-1].double()) ** 2).sum(1).numpy()
    assert np.all(np.diff(d2_last) < 0), "every candidate of the last query must beat all earlier ones"
    want = knn_ref(x, k, None)
    assert torch.equal(knn(device, x, k, None, flags), want), f"overflowing buffers k={k} n={n} flags={flags}"


# ------------------------------------------------------------------------------------------ 3: tile edges in n
def case_knn_n_edge(device, n, dim):
    """brute force, k = 4: 3 dimensions (QW = 8: 32 queries per block) and 12 (QW = 0, run-time ``nq``) - the partial
    last wave, nq < QW, nq no multiple of ``kKnnGroup``, the clamped rows of the last candidate chunk"""
    k = 4
    x = cloud(n, dim, "n_edge")
    for r in (None, cluster_radius(dim)):
        want = knn_ref(x, k, r)
        if n > k + 1:
            assert_k_binds(x, k, r, want)
        assert torch.equal(knn(device, x, k, r, BRUTE), want), f"kNN n={n} dim={dim} r={r}"


def case_knn_pruned_n_edge(device, n):
    """The pruned search against the C oracle alone, clustered cloud with a radius: one chunk and its tail (63, 64,
    65), one batch of 64 chunks (4095, 4096), one point in the second batch (4097: the ``b_hi`` round-up, the clamp of
    the invalid chunk lanes), two full batches and a point (8192, 8193: the outward walk from the middle batch), four
    batches (12 289: steps t > 2 of the walk, which are not followed by a cut).  The corner clump (``cloud``) is a
    neighbourhood that straddles the last batch boundary."""
    dim, k, r = KNN_PRUNED_N[n]
    x = cloud(n, dim, "pruned_n", corner=True)
    assert int(_capi.load().gnntrk_knn_workspace_bytes(n, dim, k)) > 0
    assert -(-n // 4096) == {63: 1, 64: 1, 65: 1, 4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, 12289: 4}[n]
    want = knn_ref(x, k, r)
    assert_k_binds(x, k, r, want)
    assert_radius_binds(x, k, want)
    of_corner = want[0][want[1] == n - 1].tolist()
    assert sorted(of_corner) == [n - 3, n - 2], "the corner point's neighbours are its clump"
    assert torch.equal(knn(device, x, k, r, PRUNED), want), f"pruned kNN n={n} dim={dim} k={k} r={r}"


def case_knn_pruned_no_radius(device, n=4097):
    """thresholds start at infinity: the own batch is streamed whole, the second one after the first cut"""
    x = cloud(n, 3, "pruned_n", corner=True)
    assert -(-n // 4096) >= 2
    want = knn_ref(x, 4, None)
    assert bool((row_counts(want, n) == 4).all())
    assert torch.equal(knn(device, x, 4, None, PRUNED), want), f"pruned kNN n={n} without a radius"


# ------------------------------------------------------------------------------------------ 4: collated batches
def case_knn_events(device, name, flags):
    """``knn_kernel<.., BATCH = true, ..>`` / ``knn_pruned_kernel<.., true, ..>``: zero-size events (first, middle,
    last, consecutive), events of 1 and 2 hits, a single event (== no ``seg_ptr``)"""
    sizes = EVENTS[name]
    n = sum(sizes)
    if name == "empty_events":
        assert sizes[0] == 0 and sizes[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(sizes, sizes[1:]))
    sp = seg_ptr_of(sizes)
    for dim, k, r in ((3, 4, None), (8, 6, cluster_radius(8)), (12, 70, 1.5)):
        x = cloud(n, dim, "events")
        want = knn_ref_events(x, sizes, k, r)
        assert want.shape[1] > 0
        got = knn(device, x, k, r, flags, sp)
        assert torch.equal(got, want), f"collated kNN {name} dim={dim} k={k} r={r} flags={flags}"
        if len(sizes) == 1:
            assert torch.equal(got, knn(device, x, k, r, flags)), "n_seg = 1 must equal a search without seg_ptr"


def case_knn_big_events(device):
    """pruned form: events that start, end and straddle a 4096-point batch of the sorted order (the event is the top of
    the sort key, so an event keeps its row range): ``c_lo`` / ``c_hi`` inside a batch, ``b_lo < b_own < b_hi - 1``"""
    sizes = BIG_EVENTS
    n, sp = sum(sizes), seg_ptr_of(sizes)
    ends = sp[1:].tolist()
    assert ends[0] < 4096 < ends[1] and ends[1] < 8192 < ends[2] and sizes[3] == 1 and -(-n // 4096) == 3
    dim, k, r = 3, 4, 0.05
    x = cloud(n, dim, "events")
    want = knn_ref_events(x, sizes, k, r)
    assert int(row_counts(want, n).max()) == k and int(row_counts(want, n).min()) == 0
    assert torch.equal(knn(device, x, k, r, PRUNED, sp), want), "collated pruned kNN over three batches"


def case_radius_graph_batch(device):
    """``losses_ml.radius_graph``: a batch vector that skips an id (the missing id is an empty event), and an unsorted
    one (refused)"""
    from gnn_tracking_amd.losses_ml import radius_graph

    sizes = (5, 0, 70, 64)
    n = sum(sizes)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    assert 1 not in batch.tolist() and bool((batch[1:] >= batch[:-1]).all())
    x = cloud(n, 3, "events")
    r = cluster_radius(3)
    for flags in FLAGS:
        with knn_flags(flags):
            got = radius_graph(x.to(device), r, batch.to(device), 6).cpu()
            assert torch.equal(got, knn_ref_events(x, sizes, 6, r)), f"radius_graph with a skipped id, flags={flags}"
            assert torch.equal(radius_graph(x.to(device), r, None, 6).cpu(), knn_ref(x, 6, r))
    unsorted = batch.clone()
    unsorted[3], unsorted[10] = 2, 0
    try:
        radius_graph(x.to(device), r, unsorted.to(device), 6)
    except ValueError as e:
        assert "sorted" in str(e)
    else:
        raise AssertionError("an unsorted batch vector was not refused")


# ------------------------------------------------------------------------------------------ 5: radius edge values
def case_knn_radius_exact(device, flags):
    """``sqrtf(d2) < r`` is strict: the 3-4-5 point at r = 5.0 is excluded, the one below it is kept"""
    x = torch.tensor([[0.0, 0.0], [3.0, 4.0], [3.0, 3.999], [-6.0, 0.0]])
    want = knn_ref(x, 3, 5.0)
    assert want.t().tolist() == [[2, 0], [2, 1], [1, 2], [0, 2]], "(0, 1) is at distance 5.0 exactly: no edge"
    assert torch.equal(knn(device, x, 3, 5.0, flags), want)
    above = float(np.nextafter(np.float32(5.0), np.float32(6.0)))
    assert [1, 0] in knn_ref(x, 3, above).t().tolist() and [0, 1] in knn_ref(x, 3, above).t().tolist()
    assert torch.equal(knn(device, x, 3, above, flags), knn_ref(x, 3, above))


def case_knn_radius_extremes(device, flags):
    """r = inf keeps everything; r = 1e-20 (r^2 underflows) keeps exact duplicates only"""
    x = cloud(130, 3, "extremes")
    for k in (5, 129):
        assert torch.equal(knn(device, x, k, float("inf"), flags), knn_ref(x, k, None)), f"r = inf, k={k}"
    want = knn_ref(x, 5, 1e-20)
    assert want.shape[1] >= 4 and bool((x[want[0]] == x[want[1]]).all()), "only exact duplicates are that close"
    assert want.shape[1] == int(row_counts(knn_ref(x, 5, 1e-3), 130).sum()), "(and nothing else is closer than 1e-3)"
    assert torch.equal(knn(device, x, 5, 1e-20, flags), want), "r = 1e-20"


def _event(x, device):
    import gnn_tracking_amd as G

    n = x.shape[0]
    g = np.random.default_rng(_seed("event", n))
    ei = torch.from_numpy(g.integers(0, n, size=(2, 3 * n)))
    return G.Data(x=x.to(device), edge_index=ei.to(device),
                  particle_id=torch.from_numpy(g.integers(0, 6, size=n)).to(device),
                  pt=torch.from_numpy(g.uniform(0.1, 3.0, size=n).astype(np.float32)).to(device),
                  eta=torch.from_numpy(g.uniform(-3, 3, size=n).astype(np.float32)).to(device),
                  reconstructable=torch.ones(n, dtype=torch.int64, device=device))


def case_knn_no_edge_radius(device, r, flags):
    """A radius that is 0, negative or NaN keeps no edge (the reference: ``edge_index[:, dists < max_radius]``):
    ``ops.knn_graph``, ``knn_scan``, ``knn_kth_neighbor``, ``losses_ml.radius_graph`` (with and without ``batch``) and
    ``MLGraphConstruction``.  ``None`` is the search without a radius, unchanged."""
    from gnn_tracking_amd.graph_construction import MLGraphConstruction
    from gnn_tracking_amd.losses_ml import radius_graph

    n, k = 50, 4
    x = cloud(n, 3, "no_edge")
    xd = x.to(device)
    assert O.knn_with_max_radius(x, k, r).shape == (2, 0), "the oracle keeps no edge"
    with knn_flags(flags):
        ei = ops.knn_graph(xd, k, r)
        assert ei.dtype == torch.int64 and tuple(ei.shape) == (2, 0) and ei.device == xd.device
        ei = ops.knn_graph(xd, k, r, seg_ptr=seg_ptr_of((20, 30)).to(device))
        assert ei.dtype == torch.int64 and tuple(ei.shape) == (2, 0)
        scan = ops.knn_scan(xd, (1, 4, 200), r)
        assert sorted(scan) == [1, 4, 200]
        assert all(v.dtype == torch.int64 and tuple(v.shape) == (2, 0) for v in scan.values())
        for kk in (1, 4, n - 1, n):
            kth = ops.knn_kth_neighbor(xd, kk, r)
            assert kth.dtype == torch.int32 and kth.cpu().tolist() == [-1] * n
        batch = torch.repeat_interleave(torch.arange(2), torch.tensor((20, 30))).to(device)
        for b in (None, batch):
            ei = radius_graph(xd, r, b, k)
            assert ei.dtype == torch.int64 and tuple(ei.shape) == (2, 0)
        x6 = cloud(n, 6, "no_edge")
        out = MLGraphConstruction(ml=None, embedding_slice=(0, 3), max_radius=r, max_num_neighbors=k)(_event(x6, device))
        assert out.edge_index.dtype == torch.int64 and tuple(out.edge_index.shape) == (2, 0)
        assert tuple(out.y.shape) == (0,) and tuple(out.edge_attr.shape) == (0, 12)
        # None: the search without a radius
        want = knn_ref(x, k, None)
        assert want.shape[1] == n * k
        assert torch.equal(ops.knn_graph(xd, k, None).cpu(), want)
        assert torch.equal(ops.knn_scan(xd, (k,), None)[k].cpu(), want)
        assert torch.equal(ops.knn_kth_neighbor(xd, k, None).cpu().long(), want[0].view(n, k)[:, k - 1])


# ------------------------------------------------------------------------- 6: the k-th neighbour, the largest count
def _kth_of(want, n, k):
    cnt = row_counts(want, n)
    start = torch.cumsum(cnt, 0) - cnt
    out = torch.full((n,), -1, dtype=torch.int64)
    has = cnt >= k
    out[has] = want[0][start[has] + k - 1]
    return out


def case_kth_neighbor(device, flags):
    """``ops.knn_kth_neighbor``: column k - 1 of the oracle's list, -1 where a row has fewer; k = 4 and k = n - 1"""
    n = 60
    x = cloud(n, 3, "kth")
    with knn_flags(flags):
        for k in (4, n - 1):
            for r in (None, cluster_radius(3), 1.5):
                want = _kth_of(knn_ref(x, k, r), n, k)
                if r is None or k == 4:
                    assert bool((want >= 0).any())
                if r == cluster_radius(3):
                    assert bool((want < 0).any())
                got = ops.knn_kth_neighbor(x.to(device), k, r)
                assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want), f"k-th neighbour k={k} r={r}"
        for k in (n, n + 5):
            assert ops.knn_kth_neighbor(x.to(device), k, None).cpu().tolist() == [-1] * n, "n - 1 < k: all -1"


def case_max_radius_count(device):
    """``ops.max_radius_count``: the largest row length of ``radius_neighbors`` minus 1 (fp64, ``d2 <= r^2``): clouds
    with duplicates, the 3-4-5 point (a member here), one point, and a cloud large enough for the pruned count pass"""
    for n, dim, r in ((130, 3, cluster_radius(3)), (300, 8, cluster_radius(8)), (4100, 3, 0.05)):
        x = cloud(n, dim, "count")
        off = O.radius_neighbors_blocked(x.numpy(), r)[0]
        want = int(np.diff(off).max()) - 1
        assert want >= 2
        got = ops.max_radius_count(x.to(device), r)
        assert got.dtype == torch.int32 and int(got) == want, f"max_radius_count n={n} dim={dim}: {int(got)} != {want}"
    x = torch.tensor([[0.0, 0.0], [3.0, 4.0], [-6.0, 0.0]])
    assert int(ops.max_radius_count(x.to(device), 5.0)) == 1 and int(ops.max_radius_count(x.to(device), 4.999)) == 0
    same = torch.ones(9, 3)
    assert int(ops.max_radius_count(same.to(device), 0.0)) == 8, "duplicates are at distance 0 <= 0"
    assert int(ops.max_radius_count(torch.zeros(1, 3).to(device), 1.0)) == 0


# ------------------------------------------------------------------------------------------ 7: the count scan
def _scan(device, cnt: torch.Tensor, k: int) -> torch.Tensor:
    """phase 1 of ``gnntrk_knn_emit`` (``edge_index`` = NULL): it reads ``cnt`` alone"""
    lib = _capi.load()
    n = cnt.numel()
    cd = cnt.to(device)
    assert cd.data_ptr() % 16 == 0
    nbr = torch.zeros(4, dtype=torch.int32, device=device)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=device)
    _capi.check(lib.gnntrk_knn_emit(ops._p(nbr), ops._p(cd), n, k, ops._p(off), None, 0, ops._stream(cd)), lib)
    return off.cpu()


def case_count_scan(device, n, clip):
    """``scan_counts_kernel<true>``: the waves' segments rounded to 256 counts, the step of 8 x 256 counts, 4 waves
    below 65 536 counts and 16 from there on"""
    g = np.random.default_rng(_seed("scan", n))
    cnt = g.integers(0, 21, size=n).astype(np.int32)
    cnt[-1] = 20
    k = 7 if clip else 64
    assert bool((cnt > k).any()) == clip
    want = np.concatenate([[0], np.cumsum(np.minimum(cnt, k).astype(np.int64))])
    got = _scan(device, torch.from_numpy(cnt), k).numpy()
    assert np.array_equal(got, want), f"count scan n={n} k={k}: first difference at {int(np.argmax(got != want))}"


def case_count_scan_beyond_int32(device, n=65537, c=40_000):
    cnt = np.full(n, c, dtype=np.int32)
    want = np.arange(n + 1, dtype=np.int64) * c
    assert want[-1] > 2 ** 31
    got = _scan(device, torch.from_numpy(cnt), 50_000).numpy()
    assert np.array_equal(got, want), f"count scan beyond 2^31: first difference at {int(np.argmax(got != want))}"


# ----------------------------------------------------------------------------- radius graph and DBSCAN: oracle
_GRAPHS: dict = {}


def radius_ref(x: torch.Tensor, r: float):
    key = (x.data_ptr(), tuple(x.shape), r)
    if key not in _GRAPHS:
        _GRAPHS[key] = (x, O.radius_neighbors_blocked(x.numpy(), r))
    return _GRAPHS[key][1]


def labels_ref(x: torch.Tensor, max_eps: float, eps: float, min_pts: int):
    key = (x.data_ptr(), tuple(x.shape), max_eps, eps, min_pts)
    if key not in _GRAPHS:
        _GRAPHS[key] = (x, O.dbscan_labels(x.numpy(), max_eps, eps, min_pts, graph=radius_ref(x, max(max_eps, eps))))
    return _GRAPHS[key][1]


def rescanner(device, x, max_eps, flags):
    with radius_flags(flags):
        return postprocessing.DBSCANFastRescan(x.to(device), max_eps=max_eps, device=device)


def check_graph(fr, x, r, tag):
    off, nbr, dist = radius_ref(x, r)
    m = len(nbr)
    assert fr._n_edges == m, f"{tag}: {fr._n_edges} edges, the oracle has {m}"
    assert np.array_equal(fr._off.cpu().numpy(), off), f"{tag}: offsets"
    assert np.array_equal(fr._nbr.cpu().numpy()[:m].astype(np.int64), nbr), f"{tag}: neighbours"
    assert np.array_equal(fr._dist.cpu().numpy()[:m], dist), f"{tag}: distances (fp64, bit for bit)"


def check_labels(fr, x, max_eps, eps, min_pts, tag, flags):
    with radius_flags(flags):      # (a rescan beyond max_eps builds the graph again)
        lab = fr.cluster(eps, min_pts)
    want = labels_ref(x, max_eps, eps, min_pts)
    assert lab.dtype == np.intp and np.array_equal(lab, want), f"{tag}: labels eps={eps} min_pts={min_pts}"
    return want


def _trials(dim):
    r = 1.3 * cluster_radius(dim)
    return r, ((r, 3), (0.8 * r, 5), (0.5 * r, 2))


# -------------------------------------------------------------------------------------- 8: every width
def case_radius_width(device, dim, flags):
    """n = 300: ``radius_kernel<D, false / true>`` at D = 2, 4, 8, 16, 32, ``radius_pruned_kernel<D, ..>`` at D = 4, 8,
    16 (4 queries per wave, 2 beyond 8 dimensions) + ``radius_order_kernel``; beyond 16 dimensions the pruned flag
    runs the brute-force kernels.  Graph and three labellings, one at ``max_eps`` and two below."""
    n = 300
    x = cloud(n, dim, "radius")
    r, trials = _trials(dim)
    lib = _capi.load()
    assert (int(lib.gnntrk_radius_points_workspace_bytes(n, dim)) > 0) == (dim <= 16)
    fr = rescanner(device, x, r, flags)
    check_graph(fr, x, r, f"radius graph dim={dim} flags={flags}")
    for i, (eps, mp) in enumerate(trials):
        want = check_labels(fr, x, r, eps, mp, f"dim={dim} flags={flags}", flags)
        if i == 0:
            assert want.max() >= 1 and want.min() == -1, "at least two clusters and noise"


def case_radius_width_refused(device, flags):
    x = cloud(40, 33, "radius")
    try:
        rescanner(device, x, 1.0, flags)
    except NotImplementedError as e:
        assert "dim <= 32" in str(e)
    else:
        raise AssertionError(f"33 dimensions were not refused (flags={flags})")


# -------------------------------------------------------------------------------------- 9: tile edges in n
def case_radius_n_edge(device, n, dim, flags):
    """brute force: the 256-point LDS tile (``lim``, the clamped rows of the last tile and of the last block); pruned:
    the 64-point chunk and its -1 tail, 16 (8 beyond 8 dimensions) queries per block, ``nq`` below that"""
    x = cloud(n, dim, "radius_n")
    r, trials = _trials(dim)
    fr = rescanner(device, x, r, flags)
    check_graph(fr, x, r, f"radius graph n={n} dim={dim} flags={flags}")
    check_labels(fr, x, r, *trials[0], f"n={n} dim={dim} flags={flags}", flags)
    check_labels(fr, x, r, *trials[2], f"n={n} dim={dim} flags={flags}", flags)


def case_radius_box_loop(device, n, flags):
    """4095 / 4096 / 4097 points: 64 chunks are one turn of the pruned kernel's box loop, the 65th chunk is alone in
    the second turn (63 clamped lanes) and holds the corner point, whose neighbours are in the first"""
    x = cloud(n, 3, "radius_n", corner=True)
    r = 0.05
    off, nbr, _ = radius_ref(x, r)
    assert nbr[off[n - 1]:off[n]].tolist() == [n - 3, n - 2, n - 1]
    fr = rescanner(device, x, r, flags)
    check_graph(fr, x, r, f"radius graph n={n} flags={flags}")
    want = check_labels(fr, x, r, 0.04, 3, f"n={n} flags={flags}", flags)
    assert want.max() >= 1 and want.min() == -1


# ------------------------------------------------------------------------ 10: list lengths at the LDS capacity
def case_radius_list_length(device, m, flags):
    """An isolated clump of exactly m points inside the radius plus far noise, rows shuffled: ``radius_order_kernel``
    ranks lists of up to ``kCap`` = 1024 ids from LDS and longer ones from memory.  Ids ascending, every distance
    carried with its id."""
    g = np.random.default_rng(_seed("clump", m))
    clump = g.uniform(-0.01, 0.01, size=(m, 3))
    noise = 10.0 + 2.0 * np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    x = np.concatenate([clump, noise + g.uniform(-0.01, 0.01, size=noise.shape)])
    x = torch.from_numpy(x[g.permutation(len(x))].astype(np.float32))
    r = 0.1
    off, nbr, _ = radius_ref(x, r)
    lens = np.diff(off)
    assert lens.max() == m and int((lens == m).sum()) == m and int((lens == 1).sum()) == len(noise)
    assert all(np.all(np.diff(nbr[off[i]:off[i + 1]]) > 0) for i in range(len(x)))
    fr = rescanner(device, x, r, flags)
    check_graph(fr, x, r, f"radius graph with lists of {m}, flags={flags}")
    want = check_labels(fr, x, r, r, 2, f"lists of {m}, flags={flags}", flags)
    assert want.max() == 0 and int((want == 0).sum()) == m


# ------------------------------------------------------------------------------------ 11: exact thresholds
def case_radius_exact(device, flags):
    """``d2 <= r^2``: the 3-4-5 point at radius 5.0 is a member, a point one fp32 ulp further out is not; a rescan with
    ``eps`` equal to a stored distance keeps that edge; radius 0 keeps the point itself and its exact duplicates;
    a negative or NaN radius is refused"""
    up = float(np.nextafter(np.float32(4.0), np.float32(5.0)))
    x = torch.tensor([[0.0, 0.0], [3.0, 4.0], [3.0, up], [-5.0, 0.0], [20.0, 20.0]])
    off, nbr, dist = radius_ref(x, 5.0)
    assert nbr[off[0]:off[1]].tolist() == [0, 1, 3] and dist[off[0]:off[1]].tolist() == [0.0, 5.0, 5.0]
    fr = rescanner(device, x, 5.0, flags)
    check_graph(fr, x, 5.0, f"3-4-5, flags={flags}")
    assert check_labels(fr, x, 5.0, 5.0, 3, "3-4-5", flags).tolist() == [0, 0, 0, 0, -1]

    x = cloud(200, 3, "exact")
    r = 1.3 * cluster_radius(3)
    off, nbr, dist = radius_ref(x, r)
    fr = rescanner(device, x, r, flags)
    check_graph(fr, x, r, f"cloud, flags={flags}")
    stored = np.sort(dist[dist > 0])
    for eps in (float(stored[len(stored) // 2]), float(stored[len(stored) // 5]), float(stored[0])):
        below = float(np.nextafter(eps, 0.0))
        assert int((dist <= eps).sum()) > int((dist <= below).sum())
        check_labels(fr, x, r, eps, 4, f"eps = a stored distance, flags={flags}", flags)
        check_labels(fr, x, r, below, 4, f"eps just below a stored distance, flags={flags}", flags)

    fr = rescanner(device, x, 0.0, flags)
    off, nbr, dist = radius_ref(x, 0.0)
    assert np.diff(off).max() == 2 and np.diff(off).min() == 1 and not dist.any(), "self and exact duplicates"
    check_graph(fr, x, 0.0, f"radius 0, flags={flags}")
    want = check_labels(fr, x, 0.0, 0.0, 2, f"radius 0, flags={flags}", flags)
    assert want.max() >= 1 and int((want >= 0).sum()) == 2 * (int(want.max()) + 1)
    for bad in (-0.5, float("nan")):
        try:
            rescanner(device, x, bad, flags)
        except ValueError as e:
            assert "radius must be >= 0" in str(e)
        else:
            raise AssertionError(f"radius {bad} was not refused (flags={flags})")


# ---------------------------------------------------------------------- 12: component shapes of the labelling
def _chain(order):
    """points 0.9 apart on a line, the point at position p of the line has index order[p]"""
    n = len(order)
    x = np.zeros((n, 2), dtype=np.float32)
    x[np.asarray(order), 0] = 0.9 * np.arange(n, dtype=np.float32)
    return torch.from_numpy(x)


def case_dbscan_shape(device, name, flags):
    """what the label propagation has to get right whatever the cloud looks like"""
    tag = f"{name}, flags={flags}"
    if name in ("chain_reversed", "chain_zigzag"):
        # the component's lowest index travels along 1999 links: more than 32 pointer hops, several host rounds;
        # reversed: from one end; zig-zag: index 0 in the middle, the indices grow outwards on alternating sides
        n = 2000
        if name == "chain_reversed":
            order = np.arange(n)[::-1]
        else:
            order = np.empty(n, dtype=np.int64)
            i = np.arange(n)
            order[n // 2 + np.where(i % 2 == 1, -((i + 1) // 2), i // 2)] = i
            assert order[n // 2] == 0 and sorted(order.tolist()) == list(range(n))
        x = _chain(order)
        fr = rescanner(device, x, 1.0, flags)
        check_graph(fr, x, 1.0, tag)
        assert not check_labels(fr, x, 1.0, 1.0, 2, tag, flags).any(), "one cluster"
        assert not check_labels(fr, x, 1.0, 1.0, 3, tag, flags).any(), "the two ends are border points"
        want = check_labels(fr, x, 1.0, 0.5, 1, tag, flags)
        assert np.array_equal(want, np.arange(n)), "below the spacing every point is its own cluster"
    elif name == "shared_border":
        # two clusters joined by one border point (index 8, 3 neighbours < min_pts = 4): it takes the lower cluster
        # number, which belongs to the cluster with the lower core indices - the one listed second on the line
        pos = [1.2, 1.3, 1.4, 1.5, 0.0, 0.1, 0.2, 0.3, 0.75, 9.0]
        x = torch.tensor([[p, 0.0] for p in pos])
        fr = rescanner(device, x, 0.5, flags)
        check_graph(fr, x, 0.5, tag)
        assert check_labels(fr, x, 0.5, 0.5, 4, tag, flags).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, -1]
        x = torch.tensor([[p, 0.0] for p in pos[4:8] + pos[:4] + pos[8:]])
        fr = rescanner(device, x, 0.5, flags)
        assert check_labels(fr, x, 0.5, 0.5, 4, tag, flags).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, -1]
    elif name == "border_first":
        # index 0 is a border point of the cluster with the HIGHER core indices: numbering goes by the lowest core index
        pos = [-0.45, 5.0, 5.1, 5.2, 5.3, 0.0, 0.1, 0.2, 0.3]
        x = torch.tensor([[p, 1.0, -1.0] for p in pos])
        fr = rescanner(device, x, 0.5, flags)
        check_graph(fr, x, 0.5, tag)
        assert check_labels(fr, x, 0.5, 0.5, 4, tag, flags).tolist() == [1, 0, 0, 0, 0, 1, 1, 1, 1]
    elif name in ("all_core", "all_noise", "duplicates", "rescans"):
        x = cloud(300, 4, "shapes")
        r, trials = _trials(4)
        fr = rescanner(device, x, r, flags)
        if name == "all_core":
            want = check_labels(fr, x, r, r, 1, tag, flags)
            assert want.min() == 0 and len(np.unique(want)) > 20, "every point is core, singletons are clusters"
            want = check_labels(fr, x, r, 0.0, 1, tag, flags)
            assert len(np.unique(want)) == 300 - len(x[5::50]), "eps = 0: duplicates share a cluster"
        elif name == "all_noise":
            longest = int(np.diff(radius_ref(x, r)[0]).max())
            assert (check_labels(fr, x, r, r, longest + 1, tag, flags) == -1).all()
            assert (check_labels(fr, x, r, r, longest, tag, flags) >= 0).any()
        elif name == "duplicates":
            g = np.random.default_rng(_seed("duplicates"))
            x = torch.from_numpy(np.repeat(g.uniform(-1, 1, size=(7, 3)), (1, 2, 3, 10, 64, 65, 5), axis=0)[g.permutation(150)]
                                 .astype(np.float32))
            fr = rescanner(device, x, 0.01, flags)
            check_graph(fr, x, 0.01, tag)
            assert check_labels(fr, x, 0.01, 0.0, 3, tag, flags).max() == 4
            assert check_labels(fr, x, 0.01, 0.01, 65, tag, flags).max() == 0
        else:
            for eps, mp in trials + trials[:1]:       # one graph, several labellings, the first one again
                check_labels(fr, x, r, eps, mp, tag, flags)
            check_labels(fr, x, r, 1.7 * r, 3, tag, flags)      # eps > max_eps: the graph is built again
            check_graph(fr, x, 1.7 * r, tag + " (rebuilt)")
            check_labels(fr, x, 1.7 * r, r, 3, tag, flags)
    else:
        raise KeyError(name)


def case_blocked_oracle():
    """the row-blocked radius oracle equals the dense one, element for element (no device involved)"""
    for n, dim, r, rows in ((300, 3, 0.2, 64), (257, 8, 0.5, 100), (5, 2, 10.0, 512), (130, 3, 0.0, 7)):
        x = cloud(n, dim, "oracle").numpy()
        a, b = O.radius_neighbors(x, r), O.radius_neighbors_blocked(x, r, rows)
        assert all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b)), (n, dim, r)
        g = (b[0], b[1], b[2])
        assert np.array_equal(O.dbscan_labels(x, r, r, 3), O.dbscan_labels(x, r, r, 3, graph=g))
