// DBSCAN post-processing on the device: the radius-neighbourhood graph
// of postprocessing/fastrescanner.py:25-39 (sklearn NearestNeighbors.radius_neighbors) and
// the clustering of :41-66 (sklearn's dbscan_inner) for any (eps, min_pts) <= the graph radius.
//
// Arithmetic contract = sklearn's kd-tree path (what NearestNeighbors picks for <= 15
// features): coordinates widened to fp64, squared distance as a sequential sum over the
// features (no FMA), membership d2 <= r*r, stored distance sqrt(d2); the rescan keeps edges
// with dist <= eps.  Neighbourhoods include the point itself, so min_pts counts it.
//
// dbscan_inner's result does not depend on its traversal order: clusters are the connected
// components of the core points under the eps graph, numbered by their lowest core index;
// a border point takes the lowest-numbered cluster among its core neighbours; everything
// else is noise (-1).  That is what the kernels compute: core flags -> min-label propagation
// with pointer jumping (monotone, so races are benign and the fixpoint is unique) -> root
// compaction -> labels.
//
// A collated batch of events (seg_ptr) is that many independent problems in the same launches: the graph kernels'
// BATCH instantiations keep every neighbourhood inside the query's event, so no component crosses an event and
// init / propagate need no change; the labels are then numbered per event (dbscan_first_kernel: the number of
// roots below every event's first row).
#include "host_util.h"
#include "wave_util.h"

namespace gnntrk {

constexpr int kRTpb = 256;  // one query per thread, candidate tiles of 256 points in LDS

// d2 of query q (registers) against candidate j of the LDS tile [D][256]
template <int D>
__device__ __forceinline__ double dist2(const double (&q)[D], const double *tile, int j) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double t = q[d] - tile[d * kRTpb + j];
        s = s + t * t;  // (-ffp-contract=off: separate multiply and add, as the reference computes)
    }
    return s;
}

// FILL = false: cnt[q] = |{j : d2(q, j) <= r2}|;  FILL = true: the lists themselves, ascending j.
// BATCH: rows are grouped into segments (the events of a collated batch); the block's tiles cover the
// events of its first to its last query, and a query accepts candidates of its own event only
template <int D, bool FILL, bool BATCH>
__global__ __launch_bounds__(kRTpb) void radius_kernel(const float *__restrict__ x, int64_t n, int dim, int stride,
                                                       double r2, const int64_t *__restrict__ seg_ptr, int n_seg,
                                                       int32_t *__restrict__ cnt,
                                                       const int64_t *__restrict__ off, int32_t *__restrict__ nbr,
                                                       double *__restrict__ dist) {
    __shared__ double s_tile[D * kRTpb];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * kRTpb + tid;
    const int64_t qc = q < n ? q : n - 1;
    double xq[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xq[d] = d < dim ? (double)x[qc * stride + d] : 0.0;  // padding adds exactly 0
    int64_t pos = FILL ? off[qc] : 0;
    int32_t c = 0;
    int64_t j_begin = 0, j_end = n, q_lo = 0, q_hi = n;   // the block's candidate rows, the query's own event
    if (BATCH) {
        const int64_t b0 = (int64_t)blockIdx.x * kRTpb, b1 = b0 + kRTpb < n ? b0 + kRTpb - 1 : n - 1;
        j_begin = seg_ptr[segment_of(seg_ptr, n_seg, b0)];
        j_end = seg_ptr[segment_of(seg_ptr, n_seg, b1) + 1];
        const int sg = segment_of(seg_ptr, n_seg, qc);
        q_lo = seg_ptr[sg];
        q_hi = seg_ptr[sg + 1];
    }
    for (int64_t j0 = j_begin; j0 < j_end; j0 += kRTpb) {
        __syncthreads();
        {
            const int64_t j = j0 + tid;
            const int64_t jc = j < j_end ? j : j_end - 1;
#pragma unroll
            for (int d = 0; d < D; ++d) s_tile[d * kRTpb + tid] = d < dim ? (double)x[jc * stride + d] : 0.0;
        }
        __syncthreads();
        const int lim = (int)(j_end - j0 < kRTpb ? j_end - j0 : kRTpb);
        for (int j = 0; j < lim; ++j) {
            const double d2 = dist2<D>(xq, s_tile, j);
            if (d2 <= r2 && (!BATCH || (j0 + j >= q_lo && j0 + j < q_hi))) {
                if (FILL) {
                    if (q < n) {
                        nbr[pos] = (int32_t)(j0 + j);
                        dist[pos] = sqrt(d2);
                    }
                    ++pos;
                } else {
                    ++c;
                }
            }
        }
    }
    if (!FILL && q < n) cnt[q] = c;
}

// ---- the same graph without the N^2 walk --------------------------------------------------------
// Points sorted by Morton code into chunks of 64 with bounding boxes (knn.hip: spatial_chunks_build,
// dim <= 16).  A wave owns four (two beyond 8 dimensions) consecutive sorted QUERIES (coordinates in registers); the candidate
// chunks are tested 64 at a time (lane = chunk) query point against box,
//     LB = sum over d of max(lo_d - q_d, q_d - hi_d, 0)^2     in fp32, compared with r^2 (1 + 1e-5)
// (the fp32 evaluation is within a few 1e-7 of the exact bound, which in turn is <= the fp64 d2 of
// every candidate in the box: with the margin no neighbour can be lost), and only the surviving
// (query, chunk) pairs run the graph's own arithmetic (lane = candidate): fp64 sequential sum,
// member iff d2 <= r^2.  A box-against-box test per chunk of queries does NOT prune in 8 dimensions
// (measured: 92 -> 80 ms; both boxes are wide), the per-query test does (a few per cent survive).
// Lists come out in the order of the sorted chunks; radius_order_kernel puts every list into
// ascending neighbour index (the contract of radius_fill) on its way from the staging arrays to the
// output.
constexpr int kRWaves = kRTpb / 64;
constexpr int radius_queries_per_wave(int d) { return d > 8 ? 2 : 4; }  // (register budget: fp32 + fp64 copies)

// BATCH: the points are sorted by (event, Morton code), so an event keeps its row range in the sorted order; a
// wave walks the chunks of its queries' events only, and since a chunk of 64 may straddle an event edge a
// candidate is also tested for the query's own row range (original index: the events' ranges are the same)
template <int D, bool FILL, bool BATCH>
__global__ __launch_bounds__(kRTpb) void radius_pruned_kernel(const float *__restrict__ xs,
                                                              const int32_t *__restrict__ sidx,
                                                              const float *__restrict__ box, int64_t n, int n_chunks,
                                                              double r2, const int64_t *__restrict__ seg_ptr,
                                                              int n_seg, int32_t *__restrict__ cnt,
                                                              const int64_t *__restrict__ off,
                                                              int32_t *__restrict__ nbr, double *__restrict__ dist) {
    constexpr int kRQ = radius_queries_per_wave(D);
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * kRWaves + wv) * kRQ;  // position in the sorted order
    if (q0 >= n) return;
    const int nq = (int)(n - q0 < kRQ ? n - q0 : kRQ);
    int lane_zero;  // (per-lane copies of the query coordinates: see knn.hip)
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("v_mov_b32 %0, 0" : "=v"(lane_zero));
#else
    lane_zero = 0;
#endif
    float qf[kRQ][D];
    double qd[kRQ][D];
    int64_t pos[kRQ];
    int32_t oq[kRQ], found[kRQ], qlo[kRQ], qhi[kRQ];
#pragma unroll
    for (int u = 0; u < kRQ; ++u) {
        const int64_t r = q0 + (u < nq ? u : nq - 1);
        const float *__restrict__ row = xs + r * D + lane_zero;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            qf[u][d] = row[d];
            qd[u][d] = (double)qf[u][d];
        }
        oq[u] = sidx[r];
        pos[u] = FILL ? off[oq[u]] : 0;
        found[u] = 0;
        qlo[u] = 0;
        qhi[u] = (int32_t)n;
        if (BATCH) {
            const int sg = segment_of(seg_ptr, n_seg, oq[u]);
            qlo[u] = (int32_t)seg_ptr[sg];
            qhi[u] = (int32_t)seg_ptr[sg + 1];
        }
    }
    // (queries ascend in the sorted order and u >= nq repeats the last one: [0] and [kRQ - 1] span the wave's events)
    int c_lo = 0, c_hi = n_chunks;
    if (BATCH) {
        c_lo = (int)__builtin_amdgcn_readfirstlane(qlo[0] >> 6);
        c_hi = (int)__builtin_amdgcn_readfirstlane((qhi[kRQ - 1] + 63) >> 6);
    }
    const float r2m = (float)r2 * 1.00001f + 1e-30f;
    for (int c0 = c_lo; c0 < c_hi; c0 += 64) {
        const int cc = c0 + lane < c_hi ? c0 + lane : c_hi - 1;
        float lo[D], hi[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            lo[d] = box[(int64_t)cc * 2 * D + d];
            hi[d] = box[(int64_t)cc * 2 * D + D + d];
        }
        int qmask = 0;
#pragma unroll
        for (int u = 0; u < kRQ; ++u) {
            float lb = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float gd = fmaxf(fmaxf(lo[d] - qf[u][d], qf[u][d] - hi[d]), 0.f);
                lb = lb + gd * gd;
            }
            if (c0 + lane < c_hi && u < nq && lb <= r2m) qmask |= 1 << u;
        }
        unsigned long long near = __ballot(qmask != 0);
        while (near != 0ull) {
            const int i = __ffsll(near) - 1;
            near &= near - 1ull;
#ifdef __HIP_DEVICE_COMPILE__
            const int qm = __builtin_amdgcn_readlane(qmask, i);
#else
            const int qm = __shfl(qmask, i);
#endif
            const int64_t p2 = (int64_t)(c0 + i) * 64 + lane;
            double xc[D];
#pragma unroll
            for (int d = 0; d < D; ++d) xc[d] = (double)xs[p2 * D + d];
            const int32_t id = sidx[p2];
#pragma unroll
            for (int u = 0; u < kRQ; ++u) {
                if (((qm >> u) & 1) == 0) continue;
                double s2 = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double t = qd[u][d] - xc[d];
                    s2 = s2 + t * t;  // (no FMA: as the reference computes)
                }
                const bool ok = id >= 0 && s2 <= r2 && (!BATCH || (id >= qlo[u] && id < qhi[u]));
                const unsigned long long m = __ballot(ok);
                if (m == 0ull) continue;
                if (FILL) {
                    if (ok) {
                        const int64_t at = pos[u] + __popcll(m & ((1ull << lane) - 1ull));
                        nbr[at] = id;
                        dist[at] = sqrt(s2);
                    }
                    pos[u] += __popcll(m);
                } else {
                    found[u] += __popcll(m);
                }
            }
        }
    }
    if (!FILL && lane == 0) {
#pragma unroll
        for (int u = 0; u < kRQ; ++u)
            if (u < nq) cnt[oq[u]] = found[u];
    }
}

// one wave per query: its list from the staging arrays into the output, ascending neighbour index
// (rank of an entry = number of smaller ids in the list; ids are distinct)
__global__ __launch_bounds__(kRTpb) void radius_order_kernel(const int64_t *__restrict__ off, int64_t n,
                                                             const int32_t *__restrict__ nbr_in,
                                                             const double *__restrict__ dist_in,
                                                             int32_t *__restrict__ nbr, double *__restrict__ dist) {
    constexpr int kCap = 1024;  // list lengths served from LDS
    __shared__ int s_v[kRWaves][kCap];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kRWaves + wv;
    if (q >= n) return;
    const int64_t o = off[q];
    const int64_t len = off[q + 1] - o;
    const bool in_lds = len <= kCap;
    if (in_lds) {
        for (int64_t i = lane; i < len; i += 64) s_v[wv][i] = nbr_in[o + i];
        wave_sync();
    }
    for (int64_t i = lane; i < len; i += 64) {
        const int v = nbr_in[o + i];
        int64_t rank = 0;
        if (in_lds) {
            for (int64_t j = 0; j < len; ++j) rank += s_v[wv][j] < v ? 1 : 0;
        } else {
            for (int64_t j = 0; j < len; ++j) rank += nbr_in[o + j] < v ? 1 : 0;
        }
        nbr[o + rank] = v;
        dist[o + rank] = dist_in[o + i];
    }
}

// core[i] = |{e in list(i): dist[e] <= eps}| >= min_pts;  root[i] = i for core points, else -1
__global__ __launch_bounds__(256) void dbscan_init_kernel(const int64_t *__restrict__ off,
                                                          const double *__restrict__ dist, int64_t n, double eps,
                                                          int min_pts, uint8_t *__restrict__ core,
                                                          int32_t *__restrict__ root) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int32_t c = 0;
        for (int64_t e = off[i]; e < off[i + 1]; ++e) c += dist[e] <= eps ? 1 : 0;
        const bool is_core = c >= min_pts;
        core[i] = is_core ? 1 : 0;
        root[i] = is_core ? (int32_t)i : -1;
    }
}

// one round: root[i] <- min over core eps-neighbours of root[.], then pointer jumping.
// root[.] only ever decreases and always names a core point of the same component, so
// stale reads are harmless; *changed is set when anything moved.
__global__ __launch_bounds__(256) void dbscan_propagate_kernel(const int64_t *__restrict__ off,
                                                               const int32_t *__restrict__ nbr,
                                                               const double *__restrict__ dist, int64_t n,
                                                               double eps, const uint8_t *__restrict__ core,
                                                               int32_t *root, int32_t *__restrict__ changed) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (!core[i]) continue;
        const int32_t old = root[i];
        int32_t m = old;
        for (int64_t e = off[i]; e < off[i + 1]; ++e) {
            const int32_t j = nbr[e];
            if (dist[e] <= eps && core[j]) {
                const int32_t r = root[j];
                m = r < m ? r : m;
            }
        }
        for (int hop = 0; hop < 32; ++hop) {  // follow the chain towards its current end
            const int32_t r = root[m];
            if (r >= m) break;
            m = r;
        }
        if (m < old) {
            root[i] = m;
            *changed = 1;
        }
    }
}

__global__ __launch_bounds__(256) void dbscan_roots_kernel(const uint8_t *__restrict__ core,
                                                           const int32_t *__restrict__ root, int64_t n,
                                                           uint8_t *__restrict__ is_root) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        is_root[i] = (core[i] && root[i] == (int32_t)i) ? 1 : 0;
}

// first[s] = number of roots below seg_ptr[s]: the cluster number of event s's first cluster (one thread per
// event; *n_roots is first[n_seg], written by the compaction)
__global__ __launch_bounds__(256) void dbscan_first_kernel(const int32_t *__restrict__ root_list,
                                                           const int64_t *__restrict__ n_roots,
                                                           const int64_t *__restrict__ seg_ptr, int n_seg,
                                                           int64_t *__restrict__ first) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t row = seg_ptr[s];
    int64_t lo = 0, hi = *n_roots;   // the first root >= row
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (root_list[mid] < row) lo = mid + 1; else hi = mid;
    }
    first[s] = lo;
}

// cluster number = rank of the component's root among the roots (ascending index);
// border point = lowest cluster number among its core neighbours; otherwise -1.
// BATCH: the numbers are local to the event - minus first[event of i] (a border point's core neighbours are of
// its own event)
template <bool BATCH>
__global__ __launch_bounds__(256) void dbscan_labels_kernel(const int64_t *__restrict__ off,
                                                            const int32_t *__restrict__ nbr,
                                                            const double *__restrict__ dist, int64_t n,
                                                            double eps, const uint8_t *__restrict__ core,
                                                            const int32_t *__restrict__ root,
                                                            const int32_t *__restrict__ rank,
                                                            const int64_t *__restrict__ seg_ptr, int n_seg,
                                                            const int64_t *__restrict__ first,
                                                            int64_t *__restrict__ labels) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t base = BATCH ? first[segment_of(seg_ptr, n_seg, i)] : 0;
        int64_t lab = -1;
        if (core[i]) {
            lab = rank[root[i]] - base;
        } else {
            for (int64_t e = off[i]; e < off[i + 1]; ++e) {
                const int32_t j = nbr[e];
                if (dist[e] <= eps && core[j]) {
                    const int64_t l = rank[root[j]] - base;
                    lab = (lab < 0 || l < lab) ? l : lab;
                }
            }
        }
        labels[i] = lab;
    }
}

static int check_points(const float *x, int64_t n, int dim, int stride, double radius, const char *who) {
    if (n < 0 || n > 0x7fffffff) return fail(GNNTRK_EUNSUPPORTED, "radius graph: n must fit int32");
    if (dim < 1 || dim > 32) return fail(GNNTRK_EUNSUPPORTED, "radius graph: 1 <= dim <= 32");
    if (n > 0 && (!x || stride < dim)) return fail(GNNTRK_EINVAL, "radius graph: bad points");
    if (!(radius >= 0.0)) return fail(GNNTRK_EINVAL, "radius graph: radius must be >= 0");
    (void)who;
    return GNNTRK_OK;
}

// the events of a collated batch (ptr == NULL: one event, the kernels' BATCH = false instantiations)
struct Segments {
    const int64_t *ptr;
    int n;
};
static int check_segments(const Segments &sg) {
    if (sg.ptr && sg.n < 1) return fail(GNNTRK_EINVAL, "radius graph: seg_ptr needs n_seg >= 1");
    return GNNTRK_OK;
}

// the N^2 kernel of either pass
template <bool FILL>
static void radius_launch(const float *x, int64_t n, int dim, int stride, double r2, const Segments &sg, int32_t *cnt,
                          const int64_t *off, int32_t *nbr, double *dist, hipStream_t stream) {
    dispatch_dp<2, 4, 8, 16, 32>(dim, [&](auto D) {
        lift_bools([&](auto BATCH) {
            hipLaunchKernelGGL((radius_kernel<decltype(D)::value, FILL, decltype(BATCH)::value>),
                               dim3((unsigned)ceil_div(n, kRTpb)), dim3(kRTpb), 0, stream, x, n, dim, stride, r2, sg.ptr,
                               sg.n, cnt, off, nbr, dist);
        }, sg.ptr != nullptr);
    });
}

// the brute-force passes: what gnntrk_radius_count / _fill run, and what the *_ws entries fall back to
static int radius_count(const float *x, int64_t n, int dim, int x_stride, double radius, const Segments &sg,
                        int32_t *cnt, int64_t *offsets, hipStream_t stream) {
    int rc = check_points(x, n, dim, x_stride, radius, "radius_count");
    if (rc || (rc = check_segments(sg))) return rc;
    if (!offsets) return fail(GNNTRK_EINVAL, "radius_count: NULL offsets");
    if (n == 0) return check_hip(hipMemsetAsync(offsets, 0, sizeof(int64_t), stream), "radius_count");
    if (!cnt) return fail(GNNTRK_EINVAL, "radius_count: NULL counts");
    radius_launch<false>(x, n, dim, x_stride, radius * radius, sg, cnt, nullptr, nullptr, nullptr, stream);
    scan_counts_launch(cnt, 0x7fffffff, n, offsets, stream);
    return check_launch("radius_count");
}

static int radius_fill(const float *x, int64_t n, int dim, int x_stride, double radius, const Segments &sg,
                       const int64_t *offsets, int32_t *nbr, double *dist, hipStream_t stream) {
    int rc = check_points(x, n, dim, x_stride, radius, "radius_fill");
    if (rc || (rc = check_segments(sg)) || n == 0) return rc;
    if (!offsets || !nbr || !dist) return fail(GNNTRK_EINVAL, "radius_fill: NULL argument");
    radius_launch<true>(x, n, dim, x_stride, radius * radius, sg, nullptr, offsets, nbr, dist, stream);
    return check_launch("radius_fill");
}

// ---- pruned graph: workspaces and launch helpers ---------------------------------------------
// ws_points: the sorted chunks (host_util.h: chunks_ws) - filled by the count pass, read by the fill pass;
// ws_edges (fill pass): staging of the unordered lists, m_edges * 12 bytes
struct RadiusEdgesWs {
    int32_t *t_nbr;
    double *t_dist;
    size_t total;
};
static RadiusEdgesWs radius_edges_ws(void *base, int64_t m_edges) {
    const size_t m = (size_t)(m_edges > 0 ? m_edges : 1);
    RadiusEdgesWs w{};
    Carver ws{(char *)base};
    w.t_nbr = ws.take<int32_t>(m);
    w.t_dist = ws.take<double>(m);
    w.total = ws.off;
    return w;
}
constexpr int64_t kRadiusPrunedMinRows = 4096;
constexpr int64_t kRadiusPrunedMaxDegree = 256;  // denser graphs: nothing to prune, ordering would dominate

// the pruned kernel of either pass over the chunks c
template <bool FILL>
static void radius_pruned_launch(const SpatialChunks &c, int64_t n, int dim, double r2, const Segments &sg, int32_t *cnt,
                                 const int64_t *off, int32_t *nbr, double *dist, hipStream_t stream) {
    const unsigned grid = (unsigned)ceil_div(n, (int64_t)kRWaves * radius_queries_per_wave(c.dp));
    dispatch_dp<4, 8, 16>(dim, [&](auto D) {
        lift_bools([&](auto BATCH) {
            hipLaunchKernelGGL((radius_pruned_kernel<decltype(D)::value, FILL, decltype(BATCH)::value>), dim3(grid),
                               dim3(kRTpb), 0, stream, (const float *)c.xs, (const int32_t *)c.sidx, (const float *)c.box,
                               n, c.n_chunks, r2, sg.ptr, sg.n, cnt, off, nbr, dist);
        }, sg.ptr != nullptr);
    });
}

// whether the pruned form runs: the shape is covered, the flags allow it (bit 0: below the size threshold too, bit
// 1: never) and the events fit the sort key (knn.hip: 16 bits)
static bool radius_pruned(const void *ws, int64_t n, int dim, int flags, const Segments &sg) {
    return ws && dim <= 16 && !(flags & 2) && n > 0 && ((flags & 1) || n >= kRadiusPrunedMinRows) &&
           !(sg.ptr && sg.n > 65536);
}

static int radius_count_ws(const float *x, int64_t n, int dim, int x_stride, double radius, const Segments &sg,
                           int32_t *cnt, int64_t *offsets, void *ws_points, size_t ws_points_bytes, int flags,
                           hipStream_t stream) {
    if (!radius_pruned(ws_points, n, dim, flags, sg))
        return radius_count(x, n, dim, x_stride, radius, sg, cnt, offsets, stream);
    int rc = check_points(x, n, dim, x_stride, radius, "radius_count");
    if (rc || (rc = check_segments(sg))) return rc;
    if (!offsets || !cnt) return fail(GNNTRK_EINVAL, "radius_count: NULL argument");
    size_t need;
    const SpatialChunks c = chunks_ws(ws_points, n, dim, &need);
    if (ws_points_bytes < need) return fail(GNNTRK_EINVAL, "radius_count: workspace too small");
    rc = spatial_chunks_build(x, n, dim, x_stride, sg.ptr, sg.n, c, stream);
    if (rc) return rc;
    radius_pruned_launch<false>(c, n, dim, radius * radius, sg, cnt, nullptr, nullptr, nullptr, stream);
    scan_counts_launch(cnt, 0x7fffffff, n, offsets, stream);
    return check_launch("radius_count(pruned)");
}

static int radius_fill_ws(const float *x, int64_t n, int dim, int x_stride, double radius, const Segments &sg,
                          const int64_t *offsets, int64_t m_edges, int32_t *nbr, double *dist, void *ws_points,
                          size_t ws_points_bytes, void *ws_edges, size_t ws_edges_bytes, int flags,
                          hipStream_t stream) {
    const bool pruned = radius_pruned(ws_points, n, dim, flags, sg) && ws_edges &&
                        ((flags & 1) || m_edges <= kRadiusPrunedMaxDegree * n);
    if (!pruned) return radius_fill(x, n, dim, x_stride, radius, sg, offsets, nbr, dist, stream);
    int rc = check_points(x, n, dim, x_stride, radius, "radius_fill");
    if (rc || (rc = check_segments(sg))) return rc;
    if (!offsets || !nbr || !dist || m_edges < 0) return fail(GNNTRK_EINVAL, "radius_fill: bad argument");
    size_t need;
    const SpatialChunks c = chunks_ws(ws_points, n, dim, &need);
    const RadiusEdgesWs e = radius_edges_ws(ws_edges, m_edges);
    if (ws_points_bytes < need || ws_edges_bytes < e.total)
        return fail(GNNTRK_EINVAL, "radius_fill: workspace too small");
    radius_pruned_launch<true>(c, n, dim, radius * radius, sg, nullptr, offsets, e.t_nbr, e.t_dist, stream);
    hipLaunchKernelGGL(radius_order_kernel, dim3((unsigned)ceil_div(n, kRWaves)), dim3(kRTpb), 0, stream, offsets, n,
                       (const int32_t *)e.t_nbr, (const double *)e.t_dist, nbr, dist);
    return check_launch("radius_fill(pruned)");
}

struct LabelsWs {
    uint8_t *is_root;
    int32_t *root_list, *rank;
    char *compact;   // compact_ws_bytes(n)
    size_t total;
};
static LabelsWs labels_ws(void *base, int64_t n) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    LabelsWs w{};
    Carver ws{(char *)base};
    w.is_root = ws.take<uint8_t>(nn);
    w.root_list = ws.take<int32_t>(nn);
    w.rank = ws.take<int32_t>(nn);
    w.compact = ws.take<char>(compact_ws_bytes(n));
    w.total = ws.off;
    return w;
}

// dbscan_labels with or without events; cluster_ptr [n_seg + 1] (one event: the cluster count alone)
static int dbscan_labels(const int64_t *offsets, const int32_t *nbr, const double *dist, int64_t n, double eps,
                         const uint8_t *core, const int32_t *root, const Segments &sg, int64_t *labels,
                         int64_t *cluster_ptr, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (sg.ptr && sg.n < 1) return fail(GNNTRK_EINVAL, "dbscan_labels: seg_ptr needs n_seg >= 1");
    if (!cluster_ptr) return fail(GNNTRK_EINVAL, "dbscan_labels: NULL count output");
    const int n_first = sg.ptr ? sg.n : 0;
    if (n == 0)
        return check_hip(hipMemsetAsync(cluster_ptr, 0, sizeof(int64_t) * (n_first + 1), stream), "dbscan_labels");
    if (!offsets || !core || !root || !labels) return fail(GNNTRK_EINVAL, "dbscan_labels: NULL argument");
    const LabelsWs w = labels_ws(workspace, n);
    if (!workspace || workspace_bytes < w.total) return fail(GNNTRK_EINVAL, "dbscan_labels: workspace too small");
    hipLaunchKernelGGL(dbscan_roots_kernel, dim3(blocks_for(n, 16)), dim3(256), 0, stream, core, root, n, w.is_root);
    int rc = compact_bytes_launch(w.is_root, n, w.root_list, w.rank, cluster_ptr + n_first, w.compact,
                                  compact_ws_bytes(n), stream);
    if (rc) return rc;
    if (sg.ptr) {
        hipLaunchKernelGGL(dbscan_first_kernel, dim3((unsigned)ceil_div(sg.n, 256)), dim3(256), 0, stream,
                           (const int32_t *)w.root_list, (const int64_t *)(cluster_ptr + n_first), sg.ptr, sg.n,
                           cluster_ptr);
        hipLaunchKernelGGL(dbscan_labels_kernel<true>, dim3(blocks_for(n, 16)), dim3(256), 0, stream, offsets, nbr, dist,
                           n, eps, core, root, (const int32_t *)w.rank, sg.ptr, sg.n, (const int64_t *)cluster_ptr,
                           labels);
    } else {
        hipLaunchKernelGGL(dbscan_labels_kernel<false>, dim3(blocks_for(n, 16)), dim3(256), 0, stream, offsets, nbr, dist,
                           n, eps, core, root, (const int32_t *)w.rank, sg.ptr, 0, (const int64_t *)nullptr, labels);
    }
    return check_launch("dbscan_labels");
}

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

int gnntrk_radius_count(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius, int32_t *cnt,
                        int64_t *offsets, void *stream) {
    return radius_count(x, n, dim, x_stride, radius, Segments{}, cnt, offsets, (hipStream_t)stream);
}

int gnntrk_radius_fill(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius, const int64_t *offsets,
                       int32_t *nbr, double *dist, void *stream) {
    return radius_fill(x, n, dim, x_stride, radius, Segments{}, offsets, nbr, dist, (hipStream_t)stream);
}

size_t gnntrk_radius_points_workspace_bytes(int64_t n, int32_t dim) {
    if (n < 1 || n > 0x7fffffff || dim < 1 || dim > 16) return 0;
    size_t total;
    chunks_ws(nullptr, n, dim, &total);
    return total;
}

size_t gnntrk_radius_edges_workspace_bytes(int64_t m_edges) { return radius_edges_ws(nullptr, m_edges).total; }

int gnntrk_radius_count_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius, int32_t *cnt,
                           int64_t *offsets, void *ws_points, size_t ws_points_bytes, int32_t flags, void *stream) {
    return radius_count_ws(x, n, dim, x_stride, radius, Segments{}, cnt, offsets, ws_points, ws_points_bytes, flags,
                           (hipStream_t)stream);
}

int gnntrk_radius_count_batched_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius,
                                   const int64_t *seg_ptr, int32_t n_seg, int32_t *cnt, int64_t *offsets,
                                   void *ws_points, size_t ws_points_bytes, int32_t flags, void *stream) {
    return radius_count_ws(x, n, dim, x_stride, radius, Segments{seg_ptr, n_seg}, cnt, offsets, ws_points,
                           ws_points_bytes, flags, (hipStream_t)stream);
}

int gnntrk_radius_fill_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius,
                          const int64_t *offsets, int64_t m_edges, int32_t *nbr, double *dist, void *ws_points,
                          size_t ws_points_bytes, void *ws_edges, size_t ws_edges_bytes, int32_t flags, void *stream) {
    return radius_fill_ws(x, n, dim, x_stride, radius, Segments{}, offsets, m_edges, nbr, dist, ws_points,
                          ws_points_bytes, ws_edges, ws_edges_bytes, flags, (hipStream_t)stream);
}

int gnntrk_radius_fill_batched_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius,
                                  const int64_t *seg_ptr, int32_t n_seg, const int64_t *offsets, int64_t m_edges,
                                  int32_t *nbr, double *dist, void *ws_points, size_t ws_points_bytes,
                                  void *ws_edges, size_t ws_edges_bytes, int32_t flags, void *stream) {
    return radius_fill_ws(x, n, dim, x_stride, radius, Segments{seg_ptr, n_seg}, offsets, m_edges, nbr, dist,
                          ws_points, ws_points_bytes, ws_edges, ws_edges_bytes, flags, (hipStream_t)stream);
}

int gnntrk_dbscan_init(const int64_t *offsets, const double *dist, int64_t n, double eps, int32_t min_pts,
                       uint8_t *core, int32_t *root, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n > 0x7fffffff) return fail(GNNTRK_EUNSUPPORTED, "dbscan: n must fit int32");
    if (n == 0) return GNNTRK_OK;
    if (!offsets || !core || !root) return fail(GNNTRK_EINVAL, "dbscan_init: NULL argument");
    hipLaunchKernelGGL(dbscan_init_kernel, dim3(blocks_for(n, 16)), dim3(256), 0, stream, offsets, dist, n, eps,
                       min_pts, core, root);
    return check_launch("dbscan_init");
}

int gnntrk_dbscan_propagate(const int64_t *offsets, const int32_t *nbr, const double *dist, int64_t n, double eps,
                            const uint8_t *core, int32_t *root, int32_t rounds, int32_t *changed, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!changed) return fail(GNNTRK_EINVAL, "dbscan_propagate: NULL flag");
    if (n == 0) return check_hip(hipMemsetAsync(changed, 0, sizeof(int32_t), stream), "dbscan_propagate");
    if (!offsets || !core || !root || rounds < 1) return fail(GNNTRK_EINVAL, "dbscan_propagate: bad argument");
    for (int r = 0; r < rounds; ++r) {
        // the flag reports the LAST round only: zero means the fixpoint has been reached
        int rc = check_hip(hipMemsetAsync(changed, 0, sizeof(int32_t), stream), "dbscan_propagate(memset)");
        if (rc) return rc;
        hipLaunchKernelGGL(dbscan_propagate_kernel, dim3(blocks_for(n, 16)), dim3(256), 0, stream, offsets, nbr, dist,
                           n, eps, core, root, changed);
    }
    return check_launch("dbscan_propagate");
}

size_t gnntrk_dbscan_workspace_bytes(int64_t n) { return labels_ws(nullptr, n).total; }

int gnntrk_dbscan_labels(const int64_t *offsets, const int32_t *nbr, const double *dist, int64_t n, double eps,
                         const uint8_t *core, const int32_t *root, int64_t *labels, int64_t *n_clusters,
                         void *workspace, size_t workspace_bytes, void *stream) {
    return dbscan_labels(offsets, nbr, dist, n, eps, core, root, Segments{}, labels, n_clusters, workspace,
                         workspace_bytes, (hipStream_t)stream);
}

int gnntrk_dbscan_labels_batched(const int64_t *offsets, const int32_t *nbr, const double *dist, int64_t n,
                                 double eps, const uint8_t *core, const int32_t *root, const int64_t *seg_ptr,
                                 int32_t n_seg, int64_t *labels, int64_t *cluster_ptr, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    if (!seg_ptr) return fail(GNNTRK_EINVAL, "dbscan_labels_batched: NULL seg_ptr");
    return dbscan_labels(offsets, nbr, dist, n, eps, core, root, Segments{seg_ptr, n_seg}, labels, cluster_ptr,
                         workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
