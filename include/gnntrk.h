/*
 * gnntrk.h - C ABI of libgnntrk.so: the MI355X (gfx950) native hot path of
 * gnn_tracking's Interaction-Network edge classification, kNN graph construction
 * and object-condensation loss reductions.
 *
 * This is the drop-in boundary.  The reference is pure Python; the "FFI" its hot
 * path reaches is ATen / PyG / torch_cluster.  Every entry
 * point below replaces one group of those calls and cites the reference call site
 * (paths relative to /root/reference/src/gnn_tracking).  The Python side
 * (gnn_tracking_amd/_capi.py) binds these with ctypes; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers unless noted;
 *    the library never allocates or frees caller memory: scratch is a caller
 *    workspace whose size comes from the matching *_workspace_bytes() query.
 *  - every call is asynchronous on the given HIP stream (`stream` is a
 *    hipStream_t passed as void*; NULL = default stream) and stateless/re-entrant.
 *  - return value: 0 ok, 1 bad argument, 2 HIP runtime error, 3 out of memory
 *    (message contains "out of memory" so utils/oom.py:12-18 keeps working),
 *    4 unsupported size.  gnntrk_last_error() returns the thread-local message.
 *  - floating point data is fp32 row-major; indices produced by the library are
 *    int32 (graphs up to 2^31-1 nodes/edges), indices consumed from the reference
 *    surface (`edge_index`, `particle_id`) are int64 exactly as PyG stores them.
 */
#ifndef GNNTRK_H
#define GNNTRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNTRK_VERSION 600 /* 0.6.0: + the gfold block of the bf16 backward arguments: target-side gradient fold inside the kernel, mlp_backward_bf16_can_fold, fold_finish_bf16; 0.5.0: + node_order, graph_index_carry.node_rank (node renumbering inside the index build); 0.4.0: + resfcnn_*, hinge_* (metric-learning stage), mlp_*_wide (fp32 in <= 128 / hidden <= 128 / out <= 48); 0.3.0: + graph_index_build_ex / _carry (own counting sort), bce_csr; 0.2.3: + radius_*_ws; 0.2.2: oc_*_spatial; 0.2.1: knn_search_ws / knn_workspace_bytes (0.2.0: edge_targets_csr, knn_search_batched, oc_backward workspace, oc_args.rep_keep_prob/rep_seed) */
#define GNNTRK_MAX_SEGS 10 /* concat segments of one fused MLP input           */
#define GNNTRK_MAX_IN 48   /* max concatenated input width of a fused MLP      */
#define GNNTRK_MAX_HIDDEN 64
#define GNNTRK_MAX_OUT 16

enum {
    GNNTRK_OK = 0,
    GNNTRK_EINVAL = 1,
    GNNTRK_EHIP = 2,
    GNNTRK_ENOMEM = 3,
    GNNTRK_EUNSUPPORTED = 4
};

int gnntrk_version(void);
const char *gnntrk_last_error(void);
/* number of compute units of the current device (grid sizing; 256 on MI355X) */
int gnntrk_device_cu_count(void);

/* ------------------------------------------------------------------ graph index
 * Replaces the bookkeeping PyG's MessagePassing.propagate does per call
 * (models/interaction_network.py:67: x_j = x[edge_index[0]], x_i = x[edge_index[1]],
 * scatter-add onto edge_index[1]) by a one-off index of the COO edge list:
 *
 *   perm[k]      original edge id of the k-th edge in target-sorted ("CSR") order;
 *                the sort is STABLE, so edges of one target keep their COO order
 *   tgt[k],src[k] endpoints of that edge (int32)
 *   rowptr_t[n]  first CSR position whose target is n          (N+1 entries)
 *   rowptr_s[n]  same for the source-sorted order              (N+1 entries)
 *   spos[m]      CSR position of the m-th edge in source-sorted order (stable)
 *
 * With it, aggregation and all gradient scatters become deterministic segment
 * sums (no atomics).  edge_index is int64 [2,E] row-major, unsorted.
 */
typedef struct gnntrk_graph_index {
    int64_t n_nodes;
    int64_t n_edges;
    int32_t *perm;     /* [E]   */
    int32_t *tgt;      /* [E]   */
    int32_t *src;      /* [E]   */
    int32_t *rowptr_t; /* [N+1] */
    int32_t *rowptr_s; /* [N+1] */
    int32_t *spos;     /* [E]   */
    int32_t *spos_inv; /* [E] or NULL: inverse of spos (CSR position -> position in the
                          source-sorted order): lets a backward kernel write per-edge source
                          gradients already source-sorted, so their fold streams */
} gnntrk_graph_index;

size_t gnntrk_graph_index_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int gnntrk_graph_index_build(const int64_t *edge_index, const gnntrk_graph_index *out,
                             void *workspace, size_t workspace_bytes, void *stream);
/* The same with `flags` (tests, measurements; both forms give identical arrays):
 *   bit 0: the library radix-sort form (two stable rocPRIM sorts + gather / boundary passes)
 *   bit 1: the own form also where the library form would be chosen for speed (dense graphs)
 *   default: the library's own two-level counting sort (buckets of 256 nodes ranked in LDS; made
 *   for collated batches - events with disjoint id ranges and contiguous edge ranges -, correct for
 *   any edge list); shapes outside it (more than 2^24 nodes, average degree in the thousands) take
 *   the library form by themselves.
 * The first int32 of the workspace holds the number of node ids outside [0, N) afterwards. */
int gnntrk_graph_index_build_ex(const int64_t *edge_index, const gnntrk_graph_index *out, void *workspace,
                                size_t workspace_bytes, int32_t flags, void *stream);

/* Per-edge inputs of the caller that ride along into CSR order inside the build (instead of a random
 * gather through `perm` afterwards; models/edge_classifier.py:97 reads `data.edge_attr`, training/
 * ec.py:43 `data.y` - both in edge_index order, both needed in CSR order by this library):
 *   edge_label  1-byte labels (the dataset's bool `y`)  ->  label_csr[k] = edge_label[perm[k]] != 0
 *   edge_rows   fp32 [E, 4] rows (`edge_attr`)          ->  rows_csr_bf16[k] = bf16(edge_rows[perm[k]]), RNE
 * Either input may be NULL.  The label travels in bit 31 of the edge id, the row as a second 8-byte
 * record: sequential reads, run-wise writes.  Identical to the gathers (which the library form of the
 * build runs instead). */
typedef struct gnntrk_graph_index_carry {
    const uint8_t *edge_label; /* [E] or NULL */
    uint8_t *label_csr;        /* [E] out */
    const float *edge_rows;    /* [E, 4] fp32, 16-byte aligned, or NULL */
    uint16_t *rows_csr_bf16;   /* [E, out_stride] bf16 out, 8-byte aligned */
    int32_t rows_stride;       /* floats per input row (multiple of 4) */
    int32_t out_stride;        /* bf16 per output row (multiple of 4) */
    const int32_t *node_rank;  /* [N] or NULL: renumbering old node id -> new node id (a permutation of [0, N),
                                  gnntrk_node_order.rank) applied to both endpoints of every edge as they are
                                  read: tgt / src / rowptr_* come out in the NEW numbering, perm / spos still
                                  refer to the caller's edge order.  The caller gathers its node rows through
                                  gnntrk_node_order.perm and hands node results back through rank. */
} gnntrk_graph_index_carry;
/* carry_rows: bit 0 = edge_rows are carried, bit 1 = node_rank is given (room for the translated int32 edge list) */
size_t gnntrk_graph_index_workspace_bytes_carry(int64_t n_nodes, int64_t n_edges, int32_t carry_rows);
int gnntrk_graph_index_build_carry(const int64_t *edge_index, const gnntrk_graph_index *out,
                                   const gnntrk_graph_index_carry *carry, void *workspace, size_t workspace_bytes,
                                   int32_t flags, void *stream);

/* A cached per-event index placed into the arrays of a collated batch.  The reference's datasets are static across
 * epochs (utils/loading.py:97-100) and its DataLoader collates disjoint graphs with shifted ids (utils/loading.py:
 * 233-239, PyG Batch): the batch's stable target sort, source sort and inverses are the events' own, shifted by the
 * event's node / edge offset - so an index built ONCE per event is copied, not sorted again:
 *   batch.perm[eo + k] = part.perm[k] + eo, .tgt / .src + no, .spos / .spos_inv + eo, .rowptr_*[no + n] = part + eo
 *   (n = 0 .. part.n_nodes), carried label_csr / 8-byte rows_csr rows copied (pairs of NULL: not carried),
 *   node_perm / node_rank + no (gnntrk_node_order of the event; NULL: not renumbered).
 * One call per event; the calls of a batch write disjoint ranges (entry n_nodes of an event's row pointers equals
 * entry 0 of the next event's).  Identical to gnntrk_graph_index_build_carry on the collated edge list. */
int gnntrk_graph_index_place(const gnntrk_graph_index *part, int64_t node_offset, int64_t edge_offset,
                             const gnntrk_graph_index *batch, const uint8_t *label_part, uint8_t *label_batch,
                             const uint16_t *rows_part, uint16_t *rows_batch, const int32_t *node_perm_part,
                             int32_t *node_perm_batch, const int32_t *node_rank_part, int32_t *node_rank_batch, void *stream);

/* Node renumbering for gather locality.  The reference keeps the hits of an event in file order
 * (graph_construction/graph_builder.py:396-455: node order = order of the hit table; utils/loading.py:17-113
 * hands the graphs on unchanged), which is unrelated to the geometry; the message passing then gathers
 * x[edge_index[0]] (models/interaction_network.py:67) from random rows.  gnntrk_node_order sorts the nodes
 * of every event by a caller-supplied key (one float per node, row stride key_stride floats; for tracking
 * graphs the azimuth column of data.x - edges join hits of neighbouring azimuth); ties keep the old order:
 *   perm[new] = old, rank[old] = new, events (batch[i] in [0, n_events), non-decreasing, or NULL = one event) keep
 *   their id ranges.  Locality is all the key has to buy (any order gives the same results up to summation order), so
 *   with the event count stated (1 <= n_events <= 64; batch == NULL counts as one event) the key is
 *   QUANTISED to 65 536 levels, q = trunc((key - lo) * (65535 / (hi - lo))) in fp32 with lo / hi the smallest / largest
 *   key of the node's own EVENT (so an event is ordered the same alone and inside a batch; NaN keys: the last level), and the nodes are put in (event, q) order by this library's own
 *   counting sort (the two-level sort of the graph index, records = nodes): nodes of one event that share a level
 *   keep their old order - deterministic, no library sort.  Otherwise (n_events <= 0: not stated - all 32 bits of
 *   batch[i] are sorted; more events; events beyond a million nodes) a stable radix sort of N pairs: with b = ceil(log2(n_events)) <= 8
 *   one 32-bit key {event : b bits, top 32 - b bits of the key's order-preserving integer image} - keys that agree in
 *   those bits keep their old order -, otherwise 32 + b bits of a 64-bit key (the full key).
 * workspace: gnntrk_node_order_workspace_bytes(n_nodes). */
size_t gnntrk_node_order_workspace_bytes(int64_t n_nodes);
int gnntrk_node_order(const float *key, int64_t key_stride, const int64_t *batch, int64_t n_events, int64_t n_nodes,
                      int32_t *perm, int32_t *rank, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------- fused gather-MLP
 * One kernel family replaces, for every MLP site of the path
 * (models/mlp.py:59-62 = addmm + clamp_min chain):
 *   - the gathers feeding it (index_select via PyG _lift, interaction_network.py:67;
 *     h_ec[edge_index[k]], edge_classifier.py:112-113),
 *   - the torch.cat that builds its input (interaction_network.py:86, :102;
 *     edge_classifier.py:110,114),
 *   - the ReLU applied to its inputs by the residual stack (resin.py:103-104),
 *   - its epilogue (residual combination resin.py:17-26; ReLU of the encoders
 *     edge_classifier.py:102-103; clamped sigmoid edge_classifier.py:115-116).
 *
 * Input row m of the MLP is the concatenation over segments j of
 *     act_j( seg[j].ptr[ (seg[j].idx ? seg[j].idx[m] : m) * seg[j].stride + 0..dim ) )
 * Weights are nn.Linear layout [out,in] row-major fp32; bias pointers may be NULL
 * (bias=False encoders, edge_classifier.py:62-67).  n_layers = 2 or 3
 * (Linear-ReLU-Linear[-ReLU-Linear]); hidden <= 64, in <= 48, out <= 16.
 */
typedef struct gnntrk_seg {
    const float *ptr;   /* [rows, stride]                                        */
    const int32_t *idx; /* [M] row gather index, or NULL for identity            */
    int32_t dim;        /* number of features taken from each row                */
    int32_t stride;     /* row stride in floats                                  */
    int32_t relu;       /* apply ReLU to the loaded values                       */
    int32_t rows;       /* rows of the tensor behind ptr, 0 = not stated.  Only read by
                           gnntrk_mlp_backward_bf16: with the sizes of every tensor stated
                           (and below 2 GB each) it addresses them through buffer descriptors
                           - hardware range checks instead of per-lane address arithmetic   */
} gnntrk_seg;

typedef struct gnntrk_mlp {
    int32_t n_layers; /* 2 or 3 */
    int32_t in_dim;   /* must equal the sum of segment dims */
    int32_t hidden;
    int32_t out_dim;
    const float *W[3];
    const float *b[3]; /* NULL = no bias */
} gnntrk_mlp;

enum {
    GNNTRK_EPI_NONE = 0,     /* y                                                 */
    GNNTRK_EPI_RELU = 1,     /* relu(y)                                           */
    GNNTRK_EPI_RESIDUAL = 2, /* ca * res[m] + cb * y        (resin.py:26)         */
    GNNTRK_EPI_SIGMOID = 3   /* ca + cb * sigmoid(y)        (edge_classifier:116) */
};

typedef struct gnntrk_mlp_fwd_args {
    gnntrk_mlp mlp;
    int32_t n_seg;
    int32_t epilogue;
    gnntrk_seg seg[GNNTRK_MAX_SEGS];
    int64_t n_rows; /* M */
    float ca, cb;
    const float *res; /* [M, res_stride] residue rows (EPI_RESIDUAL)              */
    int32_t res_stride;
    int32_t out_stride;
    float *out;             /* [*, out_stride]; row m is written at out_idx[m] or m */
    const int32_t *out_idx; /* optional row scatter (a permutation)               */
    int32_t debug_flags;    /* 0 in production; 1 skip stores, 2 skip input loads  */
    int32_t _pad;
} gnntrk_mlp_fwd_args;

int gnntrk_mlp_forward(const gnntrk_mlp_fwd_args *args, void *stream);

/* bf16-storage variant (BASELINE configs 3/4: "bf16 storage for x, e, e~, aggr and the
 * MFMA inputs, fp32 accumulate"; the reference reaches it through Lightning's
 * precision="bf16-mixed" autocast around the same modules).  Same argument block, read
 * with these changes:
 *   - seg[j].ptr, res and out address bf16 elements (uint16_t storage; the `float *`
 *     field types are reinterpreted), strides are in ELEMENTS, must be multiples of 4 and
 *     >= the feature count rounded up to 4, row starts 8-byte aligned.  Padding elements
 *     of input rows are ignored (forced to 0), padding elements of output rows up to the
 *     next multiple of 4 are written as 0;
 *   - weights/biases are fp32 in memory and rounded to bf16 when loaded; every layer
 *     accumulates in fp32; hidden activations and the output are rounded to bf16 (RNE);
 *   - GNNTRK_EPI_SIGMOID writes an fp32 output [*, out_stride floats] (the edge weights
 *     feed the fp32 loss); GNNTRK_EPI_RESIDUAL reads bf16 res rows;
 *   - limits: <= 16 four-feature input chunks; hidden + the bias row (present when a layer after the
 *     first has a bias; hidden 64 and - with at most eight input chunks - 128 do without it) <= 96, or
 *     <= 128 when the inputs fit eight chunks; above 64 one 16-row tile per iteration and one
 *     workgroup per CU; out <= 16; with hidden + bias row in 33 .. 48 (three hidden tiles) also up to
 *     32 input chunks and out <= 48 (epilogues NONE / RESIDUAL; the forward alone also RELU); n_rows < 2^31. */
int gnntrk_mlp_forward_bf16(const gnntrk_mlp_fwd_args *args, void *stream);

/* Backward of the same fused op with full recompute (nothing but the op inputs is
 * saved): replaces autograd's index_add_ / mm / threshold_backward chain
 * (training/base.py:114-116).
 *
 * Upstream gradient of output row m, feature f:
 *     g[m][f] = sum_t gout[t].ptr[(gout[t].idx ? gout[t].idx[m] : m)*gout[t].stride + f]
 * (two terms let the relational model add "direct" and "through aggr" gradients
 * without materialising their sum).  The epilogue is differentiated inside.
 *
 * Per-row input gradients are written row-aligned: for segment j, if
 * gseg[j].ptr != NULL, row m of the segment's gradient slice goes to
 *     gseg[j].ptr[m * gseg[j].stride + 0..dim)      (ReLU masks of the segment applied;
 * gseg[j].idx and gseg[j].accumulate are reserved and must be NULL / 0 in the fp32 entry
 * point; gnntrk_mlp_backward_bf16 accepts gseg[j].idx (int32[M], a permutation): row m is
 * then written at gseg[j].ptr[gseg[j].idx[m] * stride + ...]).
 * Gathered segments are reduced onto their source rows afterwards with
 * gnntrk_segment_sum (deterministic).  gres (EPI_RESIDUAL) is NOT produced here:
 * it is ca * g, an elementwise op of the caller.
 *
 * Weight/bias gradients are accumulated per wave in registers, written as partials
 * into the workspace and reduced in a fixed order into gW[i]/gb[i]
 * (+= when accumulate_params, else =): bit-reproducible run to run.
 */
typedef struct gnntrk_gterm {
    const float *ptr;
    const int32_t *idx;
    int32_t stride;
    int32_t rows; /* rows of the tensor behind ptr, 0 = not stated (see gnntrk_seg.rows) */
} gnntrk_gterm;

typedef struct gnntrk_gseg {
    float *ptr;
    const int32_t *idx;
    int32_t stride;
    int32_t accumulate;
} gnntrk_gseg;

/* Target-side fold of ONE gathered segment's gradient inside gnntrk_mlp_backward_bf16 (round 6).
 *
 * The rows of an interaction network's relational model / of the edge-weight head are in CSR order, i.e. sorted by
 * target node (models/interaction_network.py:67,75-89; models/edge_classifier.py:108-116), so the gradient of the
 * target-gathered node rows can leave the kernel already summed per node instead of as one row per edge that a
 * segment sum re-reads (16 B written + 16 B read per edge).  With `ids != NULL`:
 *   - gseg[seg].ptr addresses the FOLDED gradient: [n_nodes] padded bf16 rows of gseg[seg].stride = 8 elements
 *     (+ the carry rows, below), ZERO-FILLED by the caller (nodes without an edge are not written); gseg[seg].idx must be NULL;
 *   - ids = the sorted id stream the segment is gathered through (== seg[seg].idx: int32[n_rows], non-decreasing);
 *   - a unit of the kernel is 32 consecutive rows: every run of equal ids that STARTS in a unit is written to its
 *     node's row (its part inside the unit, NOT yet gated by the segment's ReLU); the part of a run that began in
 *     an earlier unit goes to the unit's carry row (8 bf16 = 16 bytes per unit: row n_nodes + unit of the same
 *     allocation - gseg[seg].ptr addresses n_nodes + (n_rows + 31) / 32 rows).  gnntrk_fold_finish_bf16 then
 *     adds, per node, the carries of the units its run continues into (unit order: deterministic, one thread per
 *     node) and applies the relu' gate of the segment - call it on the same stream after the backward;
 *   - arithmetic: the hidden-layer gradient (bf16, as the per-row form uses it) is summed per node in fp32 by an
 *     MFMA against a 0/1 segment matrix, rounded to bf16 once, and goes through W1^T like a row's: one rounding
 *     per node and unit instead of one per edge.
 * Only the launches gnntrk_mlp_backward_bf16_can_fold says 1 for (the buffer-addressed relational / head shapes
 * with two 16-row halves per unit, every gradient segment under the same ReLU flag); everything else rejects a
 * fold with GNNTRK_EUNSUPPORTED. */
typedef struct gnntrk_gfold {
    const int32_t *ids; /* int32[n_rows], non-decreasing; NULL: no fold */
    int64_t n_nodes;    /* node rows behind gseg[seg].ptr; (n_rows + 31) / 32 carry rows follow them */
    int32_t seg;        /* folded segment */
    int32_t _pad;
} gnntrk_gfold;

typedef struct gnntrk_mlp_bwd_args {
    gnntrk_mlp mlp;
    int32_t n_seg;
    int32_t epilogue;
    gnntrk_seg seg[GNNTRK_MAX_SEGS];
    int64_t n_rows;
    float ca, cb;
    int32_t n_gout; /* 1 or 2; gnntrk_mlp_backward_bf16: 3 where gnntrk_mlp_backward_bf16_max_terms says so */
    int32_t accumulate_params;
    gnntrk_gterm gout[3];
    gnntrk_gseg gseg[GNNTRK_MAX_SEGS];
    float *gW[3]; /* may be NULL: skip parameter gradients of that layer */
    float *gb[3];
    int32_t debug_flags; /* 0 in production. Ablation switches for tools/ablate_mlp.py:
                            1 skip input-gradient stores, 2 skip input loads (zeros),
                            8 skip the LDS transposes (weight grads become garbage)      */
    int32_t _pad;
    gnntrk_gfold fold;   /* ids == NULL: off (a zero-filled block is a valid "no fold") */
} gnntrk_mlp_bwd_args;

/* 1 if the launch described by `args` (filled as for the launch, fold included) takes the in-kernel fold. */
int gnntrk_mlp_backward_bf16_can_fold(const gnntrk_mlp_bwd_args *args);
/* Completes a fold: for every node n with rows [rowptr[n], rowptr[n + 1]) (the CSR row pointers of the sorted ids)
 * out[n] = gate(bf16(out[n] + sum of the carry rows out[n_nodes + u] of the units u after the first one its rows reach)), fp32 adds in
 * unit order, one rounding; gate: x != NULL (the folded segment's own input rows, read through a ReLU by the
 * launch) zeroes the features whose input is not positive - the relu' of the segment, applied once per node.
 * out: the folded rows of the launch (gseg[fold.seg].ptr; stride in elements, 8). */
int gnntrk_fold_finish_bf16(uint16_t *out, int32_t out_stride, int64_t n_nodes, const int32_t *rowptr,
                            int64_t n_units, const uint16_t *x, int32_t x_stride, void *stream);

/* How many upstream-gradient terms gnntrk_mlp_backward_bf16 takes for this launch (args filled as for
 * the launch, n_gout ignored): 3 for the shapes that run on buffer descriptors (an edge embedding read by
 * the next interaction network AND by the edge-weight head hands both gradients over without a sum pass in
 * between), else 2. */
int gnntrk_mlp_backward_bf16_max_terms(const gnntrk_mlp_bwd_args *args);
size_t gnntrk_mlp_backward_workspace_bytes(const gnntrk_mlp *mlp);
int gnntrk_mlp_backward(const gnntrk_mlp_bwd_args *args, void *workspace,
                        size_t workspace_bytes, void *stream);

/* Backward of gnntrk_mlp_forward_bf16 (same argument block as gnntrk_mlp_backward):
 *   - seg[j].ptr, gout[t].ptr and gseg[j].ptr address padded bf16 rows (rules of
 *     gnntrk_mlp_forward_bf16); with GNNTRK_EPI_SIGMOID the single upstream term is fp32;
 *   - the forward is recomputed with the forward's rounding; the upstream gradient (after
 *     the epilogue derivative) and the gradient at every hidden layer are rounded to bf16
 *     before they feed the next MFMA; input gradients are written as bf16 (padding
 *     elements as 0); weight / bias gradients are fp32, accumulated in fp32 per wave and
 *     reduced in a fixed order (bit-reproducible). */
size_t gnntrk_mlp_backward_bf16_workspace_bytes(const gnntrk_mlp *mlp);
int gnntrk_mlp_backward_bf16(const gnntrk_mlp_bwd_args *args, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The edge-weight head's backward WITH the head's forward and the gradient of EdgeWeightBCELoss folded into it
 * (models/edge_classifier.py:108-116, metrics/losses/ec.py:95-121): the launch recomputes the head's
 * pre-activation y of every row anyway, so it forms the weight and its own upstream gradient from the 1-byte
 * CSR label instead of reading an fp32 gradient that three earlier launches produced:
 *   sg = sigmoid(y);  W = ca + cb * sg                      (w_out[k], the bits gnntrk_mlp_forward_bf16 stores)
 *   t  = label[k] != 0
 *   gw = ((1 / n_total) * (W - t)) / max((1 - W) * W, 1e-12)  (gnntrk_bce_csr's gw_unit, same operation order)
 *   gw = gw * gscale                                         (the loss's upstream scalar, one fp32 product)
 *   gy = ((gw * cb) * sg) * (1 - sg), rounded to bf16        (as gnntrk_mlp_backward_bf16 with EPI_SIGMOID)
 * Every operation is a separate fp32 rounding in this order (no contraction): with the same inputs the launch
 * writes the gradients gnntrk_mlp_forward_bf16 + gnntrk_bce_csr + (gw_unit * gscale) + gnntrk_mlp_backward_bf16
 * write, bit for bit.  The loss VALUE is not formed here: run gnntrk_bce_csr on w_out with gw_unit = NULL.
 * args: as for gnntrk_mlp_backward_bf16 with epilogue = GNNTRK_EPI_SIGMOID and out_dim = 1; n_gout / gout are
 * ignored (the launch has no upstream tensor).  Only the buffer-addressed shape of the head takes it (h[src] |
 * h[tgt] | four 8-byte edge tensors, every tensor's size stated, n_rows rows each below 2^31 bytes; label
 * 4-byte aligned, w_out != NULL): gnntrk_mlp_backward_bf16_bce_supported says 1 for such a launch, anything else
 * is GNNTRK_EUNSUPPORTED. */
typedef struct gnntrk_head_bce {
    const uint8_t *label; /* uint8[n_rows], CSR order (gnntrk_graph_index_carry.label_csr) */
    float *w_out;         /* float[n_rows], written: the head's output */
    float gscale;         /* upstream scalar of the loss (1, or the weight of a micro-batch) */
    int32_t _pad;
    int64_t n_total;      /* the n of the mean (= n_rows) */
} gnntrk_head_bce;
int gnntrk_mlp_backward_bf16_bce_supported(const gnntrk_mlp_bwd_args *args, const gnntrk_head_bce *bce);
int gnntrk_mlp_backward_bf16_bce(const gnntrk_mlp_bwd_args *args, const gnntrk_head_bce *bce, void *workspace,
                                 size_t workspace_bytes, void *stream);
int gnntrk_mlp_backward_bf16_bce_kernel_name(const gnntrk_mlp_bwd_args *args, const gnntrk_head_bce *bce, char *buf,
                                             size_t len);

/* Helpers of the bf16-storage path. All bf16 row tensors follow the padding rules of
 * gnntrk_mlp_forward_bf16 (uint16_t storage, stride in elements, multiple of 4).
 *  rows_to_bf16:      out[m] = bf16(in[idx ? idx[m] : m]) (RNE), padding written as 0: how the
 *                     dataset's fp32 x / edge_attr (graph_builder.py:440-455) enter the stack,
 *                     edge_attr permuted into CSR order in the same pass.
 *  segment_sum_bf16:  gnntrk_segment_sum over bf16 rows, fp32 accumulation in CSR order, one
 *                     rounding at the end (aggregation and node-gradient folds).
 *  segment_sum_bf16_add: the same with one more bf16 term per segment, out[n] = bf16(addend[n] + sum):
 *                     the two folds of a node embedding that an interaction network gathers by
 *                     target AND by source (interaction_network.py:75-89) leave as one tensor,
 *                     with one rounding, instead of autograd adding two (addend and out must not overlap).
 *  permute_rows_bf16: gnntrk_permute_rows for padded bf16 rows. */
int gnntrk_rows_to_bf16(const float *in, int32_t dim, int32_t in_stride, const int32_t *idx,
                        int64_t n_rows, uint16_t *out, int32_t out_stride, void *stream);
int gnntrk_segment_sum_bf16(const uint16_t *rows, int32_t dim, int32_t row_stride,
                            const int32_t *rowptr, const int32_t *pos, int64_t n_segments,
                            uint16_t *out, int32_t out_stride, void *stream);
int gnntrk_segment_sum_bf16_add(const uint16_t *rows, int32_t dim, int32_t row_stride,
                                const int32_t *rowptr, const int32_t *pos, int64_t n_segments,
                                const uint16_t *addend, int32_t addend_stride, uint16_t *out,
                                int32_t out_stride, void *stream);
int gnntrk_permute_rows_bf16(const uint16_t *in, int32_t dim, int32_t in_stride, const int32_t *idx,
                             int64_t n_rows, uint16_t *out, int32_t out_stride, int32_t scatter,
                             void *stream);

/* Name (as rocprofv3 prints it) of the kernel instantiation gnntrk_mlp_forward /
 * gnntrk_mlp_backward dispatch to for this MLP and input-segment list; written
 * NUL-terminated into buf[len].  backward: 0 forward, 1 backward, +2 for the bf16 entry
 * points.  For matching host-side timings with profiles. */
int gnntrk_mlp_kernel_name(const gnntrk_mlp *mlp, int32_t n_seg, const gnntrk_seg *seg,
                           int32_t backward, char *buf, size_t len);
/* same for the bf16 entry points, whose instantiations also depend on the epilogue, the
 * segment layout (16-byte loads when every chunk pair allows them) and the gradient slices */
int gnntrk_mlp_forward_bf16_kernel_name(const gnntrk_mlp_fwd_args *args, char *buf, size_t len);
int gnntrk_mlp_backward_bf16_kernel_name(const gnntrk_mlp_bwd_args *args, char *buf, size_t len);

/* --------------------------------------------------------------- segment sums
 * out[n][0..dim) (=|+=) sum_{k in [rowptr[n], rowptr[n+1])} rows[(pos ? pos[k] : k)][0..dim)
 * Replaces ATen scatter_add_ (PyG SumAggregation, interaction_network.py:36,67) in
 * the forward, and index_add_ in the backward of the gathers.  Summation order is
 * the CSR order (= COO order per target): deterministic.
 */
int gnntrk_segment_sum(const float *rows, int32_t dim, int32_t row_stride,
                       const int32_t *rowptr, const int32_t *pos, int64_t n_segments,
                       float *out, int32_t out_stride, int32_t accumulate, void *stream);

/* out[m][0..dim) = in[idx[m]][0..dim)  (gather, scatter=0)  or
 * out[idx[m]][0..dim) = in[m][0..dim)  (scatter=1; idx must be a permutation).      */
int gnntrk_permute_rows(const float *in, int32_t dim, int32_t in_stride, const int32_t *idx,
                        int64_t n_rows, float *out, int32_t out_stride, int32_t scatter,
                        void *stream);

/* out = a*x + b*y elementwise (n floats); y may be NULL (then out = a*x).
 * relu_mask (optional, n floats): out is zeroed where relu_mask <= 0.               */
int gnntrk_axpby(float a, const float *x, float b, const float *y, const float *relu_mask,
                 float *out, int64_t n, void *stream);

/* ------------------------------------------------------------------ BCE loss
 * metrics/losses/ec.py:71-121: mean binary cross entropy of edge weights w in
 * (0,1) against y (float 0/1) with torch's log clamp at -100; optional
 * falsify_low_pt_edges: y' = y && pt[src_node[e]] > pt_thld (pt_thld <= 0: off).
 * loss_out: 1 float (device).  workspace >= gnntrk_bce_workspace_bytes().
 * backward: gw[e] = gscale[0] * d/dw mean-BCE  (gscale: 1 device float, the
 * upstream gradient of the scalar loss).
 */
size_t gnntrk_bce_workspace_bytes(int64_t n);
int gnntrk_bce_forward(const float *w, const float *y, const int64_t *src_node,
                       const float *pt, float pt_thld, int64_t n, float *loss_out,
                       void *workspace, size_t workspace_bytes, void *stream);
int gnntrk_bce_backward(const float *w, const float *y, const int64_t *src_node,
                        const float *pt, float pt_thld, int64_t n, const float *gscale,
                        float *gw, void *stream);

/* EdgeWeightBCELoss (metrics/losses/ec.py:95-121) on CSR-ordered edge weights against the 1-byte
 * CSR-ordered labels a graph-index build carried along (gnntrk_graph_index_carry.label_csr), forward
 * and the gradient for a unit upstream value in ONE pass over the edges:
 *   t = label_csr[k] != 0 [&& pt[src_csr[k]] > pt_thld]      (falsify_low_pt_edges, ec.py:71-92)
 *   loss = mean of the per-edge BCE (torch's log clamp at -100);
 *   gw_unit[k] = d loss / d w[k] (NULL: not wanted) - the caller scales it by the upstream gradient.
 * workspace: gnntrk_bce_workspace_bytes(n). */
int gnntrk_bce_csr(const float *w, const uint8_t *label_csr, const int32_t *src_csr, const float *pt, float pt_thld,
                   int64_t n, float *loss, float *gw_unit, void *workspace, size_t workspace_bytes, void *stream);

/* Edge labels in the CSR order of a graph index, pt-falsified (metrics/losses/ec.py:71-92):
 *   out[k] = y[perm[k]]                                           pt_thld <= 0
 *   out[k] = (y[perm[k]] != 0 && pt[src_csr[k]] > pt_thld) ? 1:0  otherwise
 * y: float labels, or (y_is_u8) the dataset's 1-byte bool labels: a quarter of the array, so
 * the random gather mostly hits the Infinity Cache.  perm / src_csr: gnntrk_graph_index.perm /
 * .src.  One gather per batch; the losses then run
 * with src_node = NULL, pt_thld = 0 on the CSR-ordered edge weights the classification head
 * writes (models/edge_classifier.py:108-116 without the scatter back to edge_index order). */
int gnntrk_edge_targets_csr(const void *y, int32_t y_is_u8, const int32_t *perm, const int32_t *src_csr,
                            const float *pt, float pt_thld, int64_t n, float *out, void *stream);

/* ------------------------------------------------------------------ focal loss
 * metrics/losses/ec.py:13-68 (binary_focal_loss), :124-150 (EdgeWeightFocalLoss), :153-183
 * (HaughtyFocalLoss): mean over edges of
 *   -alpha*pw*(1-w)^gamma*t*log(w) - (1-alpha)*w^gamma*(1-t)*log(1-w)        (no log clamp)
 * haughty = 0: t = falsify_low_pt_edges(y), pw = pos_weight (scalar);
 * haughty = 1: t = y, pw = falsify_low_pt_edges(y) per edge.  Workspace as for BCE.      */
int gnntrk_focal_forward(const float *w, const float *y, const int64_t *src_node, const float *pt, float pt_thld,
                         float alpha, float gamma, float pos_weight, int32_t haughty, int64_t n, float *loss_out,
                         void *workspace, size_t workspace_bytes, void *stream);
int gnntrk_focal_backward(const float *w, const float *y, const int64_t *src_node, const float *pt, float pt_thld,
                          float alpha, float gamma, float pos_weight, int32_t haughty, int64_t n,
                          const float *gscale, float *gw, void *stream);

/* ------------------------------------------------------------- kNN graph build
 * models/graph_construction.py:222-237 knn_with_max_radius(x, k, max_radius) =
 * torch_cluster.knn_graph(x, k) (no batch, loop=False, flow source_to_target) followed by
 * the strict L2 filter ||x_j - x_i|| < max_radius.  Arithmetic contract (bit-exact against
 * oracle/knn_ref.c): d2 = fmaf chain over dimensions in order; the k smallest (d2, index)
 * pairs per query, ties -> lower index, self excluded by index; filter sqrtf(d2) < r.
 *
 *  gnntrk_knn_search  : nbr[q*k + i], i < cnt[q]: neighbours of q, ascending distance
 *                       (max_radius <= 0: no radius).  dim <= 32, k <= 448.
 *  gnntrk_knn_emit    : edge_index == NULL: offsets[0..n] = exclusive scan of cnt
 *                       (offsets[n] = number of edges M; read it back to size the output);
 *                       else writes int64 edge_index[2, M]: row 0 = neighbour (source j),
 *                       row 1 = query (target i), grouped by query ascending.
 */
int gnntrk_knn_search(const float *x, int64_t n, int32_t dim, int32_t x_stride, int32_t k,
                      float max_radius, int32_t *nbr, int32_t *cnt, void *stream);
/* The `batch` argument of torch_cluster's knn_graph / radius_graph (metrics/losses/
 * metric_learning.py:97, :232): rows [seg_ptr[s], seg_ptr[s+1]) are event s of a collated batch
 * (seg_ptr: n_seg + 1 ascending int64 offsets on the device, seg_ptr[0] = 0, seg_ptr[n_seg] = n);
 * neighbours are searched inside the query's own event only - all events in ONE launch. */
int gnntrk_knn_search_batched(const float *x, int64_t n, int32_t dim, int32_t x_stride, int32_t k,
                              float max_radius, const int64_t *seg_ptr, int32_t n_seg, int32_t *nbr,
                              int32_t *cnt, void *stream);
/* The same search with a caller-owned workspace (gnntrk_knn_workspace_bytes; 0 = this shape is
 * not covered, pass NULL): for dim <= 16 and at least 8192 rows the points are sorted
 * by (event, Morton code), cut into chunks of 64 with bounding boxes, and a query only streams
 * the chunks whose box can hold a neighbour closer than its current threshold.  The bound is
 * evaluated in the search's own arithmetic (monotone fp32 rounding), so nbr / cnt are
 * bit-identical to gnntrk_knn_search(_batched) - only faster (200 k clustered hits, dim 8: see
 * DESIGN.md 4.6).  seg_ptr may be NULL (one event).  flags: bit 0 = use the pruned search
 * below 8192 rows too, bit 1 = brute force regardless (both for tests / measurements). */
size_t gnntrk_knn_workspace_bytes(int64_t n, int32_t dim, int32_t k);
int gnntrk_knn_search_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, int32_t k, float max_radius,
                         const int64_t *seg_ptr, int32_t n_seg, int32_t *nbr, int32_t *cnt, void *workspace,
                         size_t workspace_bytes, int32_t flags, void *stream);
int gnntrk_knn_emit(const int32_t *nbr, const int32_t *cnt, int64_t n, int32_t k, int64_t *offsets,
                    int64_t *edge_index, int64_t n_edges, void *stream);
/* The k_take <= k_stride nearest neighbours out of a search done with k = k_stride: the same
 * edge list a search with k = k_take returns (neighbours are sorted by the key (d2, index) and
 * the radius filter keeps a prefix).  GraphConstructionKNNScanner scans k = 1..9 with one
 * search per k (graph_construction/k_scanner.py:203-285, :267-269); here ONE search at max(ks)
 * feeds every k. */
int gnntrk_knn_emit_prefix(const int32_t *nbr, const int32_t *cnt, int64_t n, int32_t k_stride,
                           int32_t k_take, int64_t *offsets, int64_t *edge_index, int64_t n_edges,
                           void *stream);

/* MLGraphConstruction.forward, models/graph_construction.py:365-367 and :386-393:
 *   y[e]        = (pid[e0] == pid[e1]) && pid[e0] > 0        (int64 compare, int64 0/1 out)
 *   feat[e]     = [x[e0] - x[e1], x[e0] + x[e1]]             ([M, 2*dim])
 * with e0 = edge_index[0][e], e1 = edge_index[1][e] (int64 [2, M]).                      */
int gnntrk_edge_labels(const int64_t *particle_id, const int64_t *edge_index, int64_t n_edges,
                       int64_t *y, void *stream);
int gnntrk_edge_features(const float *x, int32_t dim, int32_t x_stride, const int64_t *edge_index,
                         int64_t n_edges, float *out, void *stream);

/* ------------------------------------------------------ ModularGraphTCN glue
 * Threshold cut and orphan-node masking between the edge classifier and the track condenser
 * (models/track_condensation_networks.py:251-262).  Deterministic three-pass stream
 * compaction: outputs in ascending index order, exactly what boolean indexing /
 * `unique` return.  Counts are written to device memory (`n_out`); the caller reads them
 * back to size its tensors (the reference's `x[mask]` synchronises in the same place).
 *
 * threshold_compact  replaces `mask = W > ec_threshold; data.edge_subgraph(mask)`:
 *   mask[i] = w[i] > threshold (NaN -> 0), idx[0..n_out[0]) = ascending i with mask[i].
 *   Edge-level attributes are then gathered with idx.
 * connected_nodes    replaces `edge_index.flatten().unique()`, `index_to_mask` and the
 *   relabelling of `data.subgraph(connected)`:
 *   hit[v] = 1 iff node v is an endpoint of an edge; node_idx[0..n_out[0]) = ascending
 *   connected nodes; newid[v] = rank of v among them or -1; edge_index_out = newid[edge_index]
 *   ([2, n_edges] int64); n_out[1] != 0 if an id was outside [0, n_nodes).              */
size_t gnntrk_compact_workspace_bytes(int64_t n);
int gnntrk_threshold_compact(const float *w, int64_t n, float threshold, uint8_t *mask, int32_t *idx,
                             int64_t *n_out, void *workspace, size_t workspace_bytes, void *stream);
int gnntrk_connected_nodes(const int64_t *edge_index, int64_t n_edges, int64_t n_nodes, uint8_t *hit,
                           int32_t *node_idx, int32_t *newid, int64_t *n_out, int64_t *edge_index_out,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------ DBSCAN post-processing
 * postprocessing/fastrescanner.py:6-66 (`DBSCANFastRescan`): the radius-neighbourhood graph
 * at max_eps (sklearn `NearestNeighbors.radius_neighbors`), then for any eps <= max_eps and
 * min_pts the labels of sklearn's `dbscan_inner` on the edges with dist <= eps.
 *
 * Arithmetic = sklearn's kd-tree path (its choice for <= 15 features): fp64 coordinates,
 * d2 = sequential sum of squared differences, member iff d2 <= radius*radius, dist = sqrt(d2);
 * every point is its own neighbour (min_pts counts it).
 *
 *  radius_count : cnt[q] = neighbourhood size, offsets[0..n] = exclusive scan (offsets[n] = M:
 *                 read it back to size nbr / dist).  dim <= 32.
 *  radius_fill  : nbr / dist [M]: the neighbourhoods, CSR by query, ascending neighbour index.
 *  dbscan_init  : core[i] = |{e: dist[e] <= eps}| >= min_pts; root[i] = i (core) or -1.
 *  dbscan_propagate : `rounds` rounds of min-label propagation with pointer jumping over the
 *                 core-core edges; changed[0] != 0 iff the last round still moved a label -
 *                 call again until it is 0 (the fixpoint is unique: root = lowest core index
 *                 of the component).
 *  dbscan_labels: labels[i] (int64) = cluster number (clusters numbered by ascending lowest
 *                 core index, as dbscan_inner discovers them); border points take the lowest
 *                 cluster number among their core neighbours; noise = -1.  n_clusters[0].  */
int gnntrk_radius_count(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius, int32_t *cnt,
                        int64_t *offsets, void *stream);
int gnntrk_radius_fill(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius,
                       const int64_t *offsets, int32_t *nbr, double *dist, void *stream);
/* The same graph with caller-owned workspaces (dim <= 16, from 4096 points on; otherwise these fall
 * back to the two entries above): points sorted into chunks of 64 with bounding boxes; every query
 * walks only the candidate chunks whose box its own point can reach - per-query point-to-box bound
 * `sum_d max(lo_d - q_d, q_d - hi_d, 0)^2 <= r^2 (1 + 1e-5)` evaluated in fp32: the relative margin
 * of 1e-5 covers the fp32 rounding of the bound ((D + 2) ulp) against the graph's fp64 distances,
 * so no neighbour can be lost; the survivors are decided by the graph's own fp64 arithmetic -; the
 * lists are then put into ascending neighbour order.  cnt / offsets / nbr / dist are identical to radius_count / radius_fill.
 * ws_points (gnntrk_radius_points_workspace_bytes; 0 = not covered, pass NULL) is filled by the
 * count pass and read by the fill pass of the same points; ws_edges
 * (gnntrk_radius_edges_workspace_bytes(M)) stages the unordered lists.  flags: bit 0 = pruned form
 * below its size threshold too, bit 1 = brute force regardless. */
size_t gnntrk_radius_points_workspace_bytes(int64_t n, int32_t dim);
size_t gnntrk_radius_edges_workspace_bytes(int64_t m_edges);
int gnntrk_radius_count_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius, int32_t *cnt,
                           int64_t *offsets, void *ws_points, size_t ws_points_bytes, int32_t flags, void *stream);
int gnntrk_radius_fill_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius,
                          const int64_t *offsets, int64_t m_edges, int32_t *nbr, double *dist, void *ws_points,
                          size_t ws_points_bytes, void *ws_edges, size_t ws_edges_bytes, int32_t flags, void *stream);
/* The graph of a collated batch: rows [seg_ptr[s], seg_ptr[s+1]) are event s (seg_ptr as
 * gnntrk_knn_search_batched takes it; NULL: one event, the two entries above) and a query's neighbourhood
 * holds hits of its own event only - all events in ONE launch sequence.  Neighbour ids stay global and
 * ascending, the arithmetic is the one above, so the lists of event s are bit for bit those of its
 * single-event graph with ids shifted by seg_ptr[s].  The pruned form sorts by (event, Morton code) and a
 * wave walks the chunks of its queries' events only; with more than 65 536 events the brute-force form
 * runs.  Workspaces and flags as above. */
int gnntrk_radius_count_batched_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius,
                                   const int64_t *seg_ptr, int32_t n_seg, int32_t *cnt, int64_t *offsets,
                                   void *ws_points, size_t ws_points_bytes, int32_t flags, void *stream);
int gnntrk_radius_fill_batched_ws(const float *x, int64_t n, int32_t dim, int32_t x_stride, double radius,
                                  const int64_t *seg_ptr, int32_t n_seg, const int64_t *offsets, int64_t m_edges,
                                  int32_t *nbr, double *dist, void *ws_points, size_t ws_points_bytes,
                                  void *ws_edges, size_t ws_edges_bytes, int32_t flags, void *stream);
int gnntrk_dbscan_init(const int64_t *offsets, const double *dist, int64_t n, double eps, int32_t min_pts,
                       uint8_t *core, int32_t *root, void *stream);
int gnntrk_dbscan_propagate(const int64_t *offsets, const int32_t *nbr, const double *dist, int64_t n, double eps,
                            const uint8_t *core, int32_t *root, int32_t rounds, int32_t *changed, void *stream);
size_t gnntrk_dbscan_workspace_bytes(int64_t n);
int gnntrk_dbscan_labels(const int64_t *offsets, const int32_t *nbr, const double *dist, int64_t n, double eps,
                         const uint8_t *core, const int32_t *root, int64_t *labels, int64_t *n_clusters,
                         void *workspace, size_t workspace_bytes, void *stream);
/* dbscan_labels on the graph of a collated batch (init and propagate need no events: the graph has no
 * edge between events, so no component crosses one): labels are LOCAL to the event - noise -1, the clusters
 * of event s numbered from 0 by ascending lowest core index inside it - so labels[seg_ptr[s] .. seg_ptr[s+1])
 * is what dbscan_labels gives for event s alone.  cluster_ptr [n_seg + 1] int64: cluster_ptr[s] = number of
 * clusters of the events before s, cluster_ptr[n_seg] = number of clusters.  An event of n_s hits has at most
 * n_s clusters, so (event, label) has the dense slot seg_ptr[s] + label < n (gnntrk_tracking_metrics_batched).
 * workspace: gnntrk_dbscan_workspace_bytes(n). */
int gnntrk_dbscan_labels_batched(const int64_t *offsets, const int32_t *nbr, const double *dist, int64_t n,
                                 double eps, const uint8_t *core, const int32_t *root, const int64_t *seg_ptr,
                                 int32_t n_seg, int64_t *labels, int64_t *cluster_ptr, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* ------------------------------------------------------ condensation losses
 * utils/graph_masks.py:19-28: mask = pt > thld && pid > 0 && reconstructable > 0 && |eta| < max_eta */
int gnntrk_good_node_mask(const float *pt, const int64_t *particle_id, const float *reconstructable,
                          const float *eta, int64_t n, float pt_thld, float max_eta, uint8_t *mask,
                          void *stream);

/* Condensation-point selection (metrics/losses/oc.py:16-43 and :279-292): for every particle
 * id that has at least one masked hit, the hit with the largest score (beta); mode 0 (RG):
 * among its masked hits, mode 1 (Tiger): among all its hits; ties -> lowest hit index.
 * alphas[0..K): CP hit per particle of interest, ascending particle id; gid[h] = k of hit h's
 * particle or -1; n_cp[0] = K (device).  Index work: one stable 64-bit radix sort + scans. */
size_t gnntrk_oc_select_workspace_bytes(int64_t n);
int gnntrk_oc_select_cps(const float *score, const int64_t *particle_id, const uint8_t *mask,
                         int64_t n, int32_t mode, int32_t *alphas, int32_t *gid, int32_t *n_cp,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Potential / background loss terms (metrics/losses/oc.py:46-161 RG with mode 0,
 * :251-347 Tiger with mode 1; q = atanh(beta)^2 + q_min):
 *   out[0] attractive = sum q_j q_k |x_j-x_k|^2 / (1e-9 + n_oi - K)
 *   out[1] repulsive  = sum_{pid_j != pid_k, |x_j-x_k| < radius} q_j q_k (radius - sqrt(eps_sqrt + d2))
 *                       / (1e-9 + (K-1) n)
 *   out[2] coward     = mean(1 - beta[alphas]);  out[3] noise = mean(beta[noise hits])
 *   out[4..8]         = norm_att, norm_rep, K, number of repulsive pairs, number of noise hits
 * backward: gx[n,dim], gbeta[n] = sum_t g[t] * d out[t] / d(x, beta); fwd = forward's out.   */
typedef struct gnntrk_oc_args {
    const float *x;    /* [n, stride] latent coordinates */
    const float *beta; /* [n] */
    const int64_t *particle_id;
    const uint8_t *mask;
    const int32_t *gid;
    const int32_t *alphas;
    const int32_t *n_cp;
    int64_t n;
    int32_t dim, stride;
    float q_min, radius, eps_sqrt;
    int32_t mode;
    /* condensation_loss_tiger's max_n_rep (oc.py:322-328): keep a repulsive pair (hit j, condensation
     * point k) with probability rep_keep_prob, decided by a hash of (rep_seed, j, k) - the same
     * pairs in the forward and both backward passes - and scale norm_rep by it.  >= 1: all pairs. */
    float rep_keep_prob;
    int32_t _pad;
    uint64_t rep_seed;
    /* CondensationLossRG's radius_graph(max_num_neighbors) cap, nearest first (oc.py:115-117): per hit
     * the index of its max_num_neighbors-th nearest hit inside the radius (last neighbour of a
     * gnntrk_knn_search with k = max_num_neighbors), -1 where the hit has fewer.  A condensation point
     * only repels a hit if it is among that hit's nearest max_num_neighbors.  NULL: no cap. */
    const int32_t *cap_nbr;
} gnntrk_oc_args;

size_t gnntrk_oc_forward_workspace_bytes(int64_t n);
int gnntrk_oc_forward(const gnntrk_oc_args *args, float *out /*[9]*/, void *workspace,
                      size_t workspace_bytes, void *stream);
/* backward: hit pass (thread = hit) + condensation-point pass (thread = CP, the hits cut into
 * slices whose partials - the workspace - are added in slice order: deterministic).  max_cps:
 * host-side upper bound of the condensation-point count (n always works). */
size_t gnntrk_oc_backward_workspace_bytes(int64_t n, int32_t dim);
int gnntrk_oc_backward(const gnntrk_oc_args *args, const float *g /*[4]*/, const float *fwd /*[9]*/,
                       float *gx, float *gbeta, int64_t max_cps, void *workspace,
                       size_t workspace_bytes, void *stream);

/* The same on a collated batch of events, every event its own problem.  seg_ptr: int64
 * [n_seg + 1] row offsets of the events' hits (device; seg_ptr[n_seg] = n), the hits sorted by event.
 *   select:   condensation points per (event, particle id); alphas ordered by (event, ascending id) and holding
 *             hit indices of the whole batch, gid[h] = index into alphas of hit h's point or -1, cp_ptr[n_seg + 1]
 *             = offsets of the events' points in alphas, n_cp[0] = their total.  Tie rule, candidates and the
 *             skipped id 0 as gnntrk_oc_select_cps.  Two stable sorts: by id (64 bits), then by event.
 *   forward:  out[n_seg][9], per event the columns of gnntrk_oc_forward's out (norms, K, n of that event).
 *   backward: g[4] is shared by the events (a mean over events carries its 1 / n_seg in g), fwd = that out.
 * A hit only meets the points of its event and a point only the hits of its event; the per-pair arithmetic is
 * that of the entries above.  The events' sizes stay on the device: the launches cover ceil(n / 256) + n_seg
 * tiles and a block finds its (event, tile) from seg_ptr / cp_ptr.  args->n_cp, args->n as above (the whole
 * batch); args->rep_keep_prob in (0, 1) is refused (the sub-sampling is per event); cap_nbr holds indices of
 * the whole batch (gnntrk_knn_search_ws with the same seg_ptr). */
size_t gnntrk_oc_select_batched_workspace_bytes(int64_t n);
int gnntrk_oc_select_cps_batched(const float *score, const int64_t *particle_id, const uint8_t *mask, int64_t n,
                                 int32_t mode, const int64_t *seg_ptr, int32_t n_seg, int32_t *alphas, int32_t *gid,
                                 int32_t *cp_ptr, int32_t *n_cp, void *workspace, size_t workspace_bytes,
                                 void *stream);
size_t gnntrk_oc_forward_batched_workspace_bytes(int64_t n, int32_t n_seg);
int gnntrk_oc_forward_batched(const gnntrk_oc_args *args, const int64_t *seg_ptr, const int32_t *cp_ptr,
                              int32_t n_seg, float *out /*[n_seg, 9]*/, void *workspace, size_t workspace_bytes,
                              void *stream);
size_t gnntrk_oc_backward_batched_workspace_bytes(int64_t n, int32_t dim);
int gnntrk_oc_backward_batched(const gnntrk_oc_args *args, const int64_t *seg_ptr, const int32_t *cp_ptr,
                               int32_t n_seg, const float *g /*[4]*/, const float *fwd /*[n_seg, 9]*/, float *gx,
                               float *gbeta, void *workspace, size_t workspace_bytes, void *stream);

/* The same loss terms and gradients without the N x K walk (dim <= 16; workspace_bytes == 0: not
 * covered, use the entry points above).  A repulsive pair needs |x_j - x_k| < radius: the hits are
 * sorted into chunks of 64 with bounding boxes and a (chunk, condensation point) pair is only
 * looked at when the box reaches into the radius (conservative bound; the exact per-pair test is
 * unchanged); the attractive term is summed over (hit, its own condensation point) directly.  Same
 * pairs and per-pair arithmetic as gnntrk_oc_forward / gnntrk_oc_backward, fixed summation order.
 * `spatial` is ONE caller-owned buffer: the forward fills it (sorted hits, boxes, per-hit and
 * per-point records), the backward of the same inputs reads it and uses its scratch part. */
size_t gnntrk_oc_spatial_workspace_bytes(int64_t n, int32_t dim);
int gnntrk_oc_forward_spatial(const gnntrk_oc_args *args, float *out /*[9]*/, void *spatial, size_t spatial_bytes,
                              void *stream);
int gnntrk_oc_backward_spatial(const gnntrk_oc_args *args, const float *g /*[4]*/, const float *fwd /*[9]*/,
                               float *gx, float *gbeta, int64_t max_cps, void *spatial, size_t spatial_bytes,
                               void *stream);

/* ------------------------------------------------------------------ wide fp32 fused MLP
 * The operator of gnntrk_mlp_forward / gnntrk_mlp_backward (same argument structs, same semantics of
 * segments, epilogues NONE / RELU / RESIDUAL, upstream terms, gradient slices, accumulate_params) for the
 * shapes beyond the register-resident fp32 kernels: in_dim <= 128, hidden <= 128, out_dim <= 48 - e.g. the
 * reference-default GraphConstructionResIN(hidden_dim=40), models/graph_construction.py:136-219, whose
 * relational model is 120 -> 40 -> 40 -> 40, in the reference's own precision.  One forward and one
 * backward launch (+ a fragment-packing and a reduction launch); one layer's weights at a time in LDS,
 * activations in registers (csrc/mlp_wide.hip).  The forward leaves the hidden layers' pre-activations in
 * `acts` ([n_layers - 1][n_rows][gnntrk_mlp_wide_hidden_pad(hidden)] floats, 16-byte aligned; NULL when no
 * backward follows) - the backward walks the layers last to first with one layer's weight-gradient tiles
 * in registers at a time.  out_idx and gseg.idx are not supported (plain per-row slices).
 */
int32_t gnntrk_mlp_wide_hidden_pad(int32_t hidden);
size_t gnntrk_mlp_wide_forward_workspace_bytes(const gnntrk_mlp *mlp);
int gnntrk_mlp_forward_wide(const gnntrk_mlp_fwd_args *args, float *acts, void *workspace, size_t workspace_bytes,
                            void *stream);
size_t gnntrk_mlp_wide_backward_workspace_bytes(const gnntrk_mlp *mlp, int64_t n_rows);
/* `out`: the forward's output (read for EPI_RELU only) */
int gnntrk_mlp_backward_wide(const gnntrk_mlp_bwd_args *args, const float *acts, const float *out, int32_t out_stride,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ residual FCNN
 * ResFCNN (models/mlp.py:65-120) and the embedding networks built on it
 * (models/graph_construction.py:25-132) as ONE forward and ONE backward launch:
 *
 *   x  <- x / max(||x||_2, 1e-12)                      (normalize != 0; mlp.py:116)
 *   h  <- W_enc x + b_enc                              (mlp.py:117)
 *   h  <- sqrt(alpha) h + sqrt(1 - alpha) (W_l relu(h) + b_l),  l = 1 .. n_hidden   (mlp.py:118-119)
 *   y  <- W_dec relu(h) + b_dec                        (mlp.py:120)
 *   y  <- y * out_scale[0]   (out_scale != NULL: GraphConstructionFCNN._latent_normalization,
 *                             graph_construction.py:52)
 *   y  <- relu(y)            (out_relu != 0: the caller's relu(encoder(x)), graph_construction.py:123)
 *
 * fp32 throughout (v_mfma_f32_16x16x4_f32, bit-exact fmaf chains).  A wave keeps the activations
 * of its rows in registers through all layers; the weights of one layer at a time are staged in LDS
 * as MFMA A-operand fragments (packed once per call into the workspace).  Limits: in_dim <= 64,
 * hidden <= 128, out_dim <= 32, n_hidden <= GNNTRK_RESFCNN_MAX_HIDDEN.
 *
 * Backward: the forward optionally leaves the pre-activation residual stream of every layer in
 * `acts` ([n_hidden + 1][n_rows][gnntrk_resfcnn_hidden_pad(hidden)] floats); the backward walks the
 * layers from the decoder down, every wave over its own rows, with the weight gradients of ONE
 * layer at a time in registers (hidden 128: 256 accumulator registers), the gradient of the residual
 * stream in a workspace buffer between layers, per-block partial sums reduced in a fixed order
 * (deterministic, no atomics).  Weight / bias pointers of gnntrk_resfcnn_grads may be NULL (no
 * gradient wanted); accumulate != 0 adds into them.
 */
#define GNNTRK_RESFCNN_MAX_HIDDEN 16 /* hidden (residual) layers = depth - 1 */
#define GNNTRK_RESFCNN_MAX_IN 64
#define GNNTRK_RESFCNN_MAX_WIDTH 128
#define GNNTRK_RESFCNN_MAX_OUT 32

typedef struct gnntrk_resfcnn {
    const float *W_enc, *b_enc;                        /* [hidden, in_dim], [hidden] or NULL     */
    const float *W_hid[GNNTRK_RESFCNN_MAX_HIDDEN];     /* [hidden, hidden]                       */
    const float *b_hid[GNNTRK_RESFCNN_MAX_HIDDEN];     /* [hidden] or NULL                       */
    const float *W_dec, *b_dec;                        /* [out_dim, hidden], [out_dim] or NULL   */
    const float *out_scale;                            /* device scalar or NULL                  */
    int32_t in_dim, hidden, out_dim, n_hidden;
    float alpha;
    int32_t normalize, out_relu, _pad;
} gnntrk_resfcnn;

typedef struct gnntrk_resfcnn_grads {
    float *W_enc, *b_enc;
    float *W_hid[GNNTRK_RESFCNN_MAX_HIDDEN];
    float *b_hid[GNNTRK_RESFCNN_MAX_HIDDEN];
    float *W_dec, *b_dec;
    float *out_scale;
} gnntrk_resfcnn_grads;

int32_t gnntrk_resfcnn_hidden_pad(int32_t hidden); /* floats per row of `acts` (multiple of 16) */
size_t gnntrk_resfcnn_forward_workspace_bytes(const gnntrk_resfcnn *m);
int gnntrk_resfcnn_forward(const gnntrk_resfcnn *m, const float *x, int32_t x_stride, int64_t n_rows, float *out,
                           int32_t out_stride, float *acts /* or NULL */, void *workspace, size_t workspace_bytes,
                           void *stream);
size_t gnntrk_resfcnn_backward_workspace_bytes(const gnntrk_resfcnn *m, int64_t n_rows);
/* `out` is the forward's output (read for out_relu only), `gx` ([n_rows, gx_stride], NULL: not wanted)
 * the gradient w.r.t. the un-normalised input rows */
int gnntrk_resfcnn_backward(const gnntrk_resfcnn *m, const float *x, int32_t x_stride, int64_t n_rows,
                            const float *acts, const float *out, int32_t out_stride, const float *gout,
                            int32_t gout_stride, float *gx, int32_t gx_stride, const gnntrk_resfcnn_grads *grads,
                            int32_t accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ edge filters
 * models/edge_filter.py.  EFMLP (:68-141) is the residual network above on EDGE rows, without biases and
 * without normalisation, with one logit per edge:
 *
 *   v  <- [x[i], x[j], edge_attr[e]]      i = edge_index[0][e], j = edge_index[1][e]      (:124-132)
 *   h  <- W_enc v                                                                         (:133)
 *   h  <- sqrt(beta) W_l relu(h) + sqrt(1 - beta) h,   l = 1 .. n_hidden                  (:134-138)
 *   W  <- 0.001 + 0.998 sigmoid(w_dec . relu(h))                                          (:139)
 *
 * derived != 0: there is no edge_attr array; the third segment is [x[i] - x[j], x[i] + x[j]] (edge_dim =
 * 2 node_dim), formed in registers with the arithmetic of gnntrk_edge_features - bit for bit the W of the
 * materialised features.  Limits: 2 node_dim + edge_dim <= 64, hidden <= 128, n_hidden <=
 * GNNTRK_RESFCNN_MAX_HIDDEN.  Node ids outside [0, n_nodes) are clamped.
 *
 * The forward writes W and nothing else.  The backward produces the weight gradients from dL/dW [n_edges]
 * and keeps no edge-sized state between the two calls: it walks the edges in chunks of
 * gnntrk_efmlp_backward_chunk_rows(m, n_edges, cap_bytes) rows (what fits into cap_bytes of per-row state,
 * a multiple of 64, at least 64), re-runs the forward of a chunk into the workspace, runs the layer-outer
 * backward of gnntrk_resfcnn_backward on it and adds the chunk's reduced partial sums to the gradients in
 * chunk order: deterministic for a given cap, no atomics.  Gradient pointers may be NULL; accumulate != 0
 * adds into them.  No gradient with respect to x or edge_attr.
 */
typedef struct gnntrk_efmlp {
    const float *W_enc;                              /* [hidden, 2 node_dim + edge_dim] */
    const float *W_hid[GNNTRK_RESFCNN_MAX_HIDDEN];   /* [hidden, hidden]                */
    const float *W_dec;                              /* [1, hidden]                     */
    int32_t node_dim, edge_dim, hidden, n_hidden;
    float beta;
    int32_t derived;
} gnntrk_efmlp;

typedef struct gnntrk_efmlp_grads {
    float *W_enc;
    float *W_hid[GNNTRK_RESFCNN_MAX_HIDDEN];
    float *W_dec;
} gnntrk_efmlp_grads;

typedef struct gnntrk_edge_rows {
    const float *x;            /* [n_nodes, x_stride]                                           */
    const int64_t *edge_index; /* [2, n_edges], the two rows edge_stride elements apart         */
    const float *edge_attr;    /* [n_edges, ea_stride], or NULL (edge_dim = 0 or derived)       */
    int64_t n_nodes, n_edges, edge_stride;
    int32_t x_stride, ea_stride;
} gnntrk_edge_rows;

size_t gnntrk_efmlp_forward_workspace_bytes(const gnntrk_efmlp *m);
int gnntrk_efmlp_forward(const gnntrk_efmlp *m, const gnntrk_edge_rows *rows, float *W /* [n_edges] */, void *workspace,
                         size_t workspace_bytes, void *stream);
int64_t gnntrk_efmlp_backward_chunk_rows(const gnntrk_efmlp *m, int64_t n_edges, size_t cap_bytes);
size_t gnntrk_efmlp_backward_workspace_bytes(const gnntrk_efmlp *m, int64_t n_edges, size_t cap_bytes);
int gnntrk_efmlp_backward(const gnntrk_efmlp *m, const gnntrk_edge_rows *rows, const float *gW /* dL/dW [n_edges] */,
                          const gnntrk_efmlp_grads *grads, int32_t accumulate, size_t cap_bytes, void *workspace,
                          size_t workspace_bytes, void *stream);

/* EFDeepSet (:22-65), between its node encoder and its aggregator:
 *   out[e] = [|h[i] - h[j]|, h[i] + h[j]]                              ([n_edges, 2 dim], :56-60)
 * backward: the per-edge gradients at the two ends, for the caller's per-hit segment sums
 *   gi[e] = sign(h[i] - h[j]) g_abs[e] + g_sum[e],  gj[e] = g_sum[e] - sign(h[i] - h[j]) g_abs[e]   (sign(0) = 0)
 */
int gnntrk_pair_invariants_forward(const float *h, int32_t dim, int32_t h_stride, int64_t n_nodes,
                                   const int64_t *edge_index, int64_t edge_stride, int64_t n_edges, float *out,
                                   void *stream);
int gnntrk_pair_invariants_backward(const float *h, int32_t dim, int32_t h_stride, int64_t n_nodes,
                                    const int64_t *edge_index, int64_t edge_stride, int64_t n_edges, const float *gout,
                                    float *gi /* [n_edges, dim] */, float *gj /* [n_edges, dim] */, void *stream);

/* ------------------------------------------------------------------ hinge embedding loss
 * The two edge-list reductions of GraphConstructionHingeEmbeddingLoss
 * (metrics/losses/metric_learning.py:14-55, `_hinge_loss_components`; edge selection :88-110):
 * per edge (a, b) = (edges[0][e], edges[1][e]) with d = ||x[a] - x[b]||_2
 *     attractive (repulsive = 0):  d^p                    (:30-32)
 *     repulsive  (repulsive = 1):  relu(r_emb - d^p)      (:50-53)
 * summed over the edges that pass the reference's selection, applied INSIDE the kernels instead of
 * compacting the edge list first (boolean indexing = a host round trip per mask):
 *     node_mask   != NULL: only edges with node_mask[a] != 0      (`mask[edges[0]]`, :104-106, :109)
 *     particle_id != NULL: only edges with pid[a] != pid[b]       (:107)
 * out[0] = sum / denom, out[1] = number of selected edges, out[2] = denom, with
 * denom = (norm ? norm[0] : out[1]) + 1e-9 (the reference's three normalisations: its own edge count, the
 * hits of interest, the attractive edge count - the latter two handed in as device scalars).
 * Deterministic two-stage sums (fp64 partials).
 *
 * Backward: node-centric, no per-edge intermediate and no atomics.  With the graph index of the SAME
 * edge list (gnntrk_graph_index_build: CSR by edges[1], source-sorted view of edges[0]) one thread owns a
 * node and walks both of its segments, recomputing every incident edge's term:
 *     gx[n] (+)= g[0] / denom * ( sum_{e: a = n} c_e (x[a] - x[b])  -  sum_{e: b = n} c_e (x[a] - x[b]) ),
 *     c_e = s p d^(p-2)  (s = 1 attractive; s = -1 where r_emb - d^p > 0, else 0; c_e = 0 at d = 0, as
 *     torch's norm backward)
 */
typedef struct gnntrk_hinge_args {
    const float *x;             /* [n_nodes, x_stride] embedding, dim <= 32                        */
    int32_t dim, x_stride;
    int64_t n_nodes;
    const uint8_t *node_mask;   /* [n_nodes] or NULL                                               */
    const int64_t *particle_id; /* [n_nodes] or NULL                                               */
    float r_emb, p;
    int32_t repulsive, _pad;
} gnntrk_hinge_args;
size_t gnntrk_hinge_workspace_bytes(int64_t n_edges);
int gnntrk_hinge_forward(const gnntrk_hinge_args *args, const int64_t *edges /* [2, n_edges], rows edge_stride apart */,
                         int64_t n_edges, int64_t edge_stride, const float *norm /* device scalar or NULL */,
                         float *out /* [3] */, void *workspace, size_t workspace_bytes, void *stream);
int gnntrk_hinge_backward(const gnntrk_hinge_args *args, const gnntrk_graph_index *index, const float *g,
                          const float *denom, float *gx, int32_t gx_stride, int32_t accumulate, void *stream);

/* ------------------------------------------------------------ validation metrics
 * The figures of merit of the edge classifier's validation step (training/ec.py:55-84): for every
 * pt cut, get_maximized_bcs (metrics/binary_classification.py:147-195) and get_roc_auc_scores
 * (:198-231) of the masked edges - from two launches and no mask, with exact integer results.
 *
 * Shared edge inputs (n edges, n < 2^31; all device pointers):
 *   w        [n] fp32 scores;
 *   y        labels, read as y[perm[i]] when perm is non-NULL (CSR-ordered w against edge_index-ordered
 *            y, as gnntrk_edge_targets_csr): y_kind 0 = uint8/bool, 1 = fp32.  Positive iff
 *            int(y) == 1 (BinaryClassificationStats: y.int() == 1, :30-35);
 *   src, tgt [n] node ids of the edge's two ends, int32, or int64 with ids_i64 = 1 (edge_index rows
 *            as they are);
 *   pt       per-node fp32 values in the ids' numbering, or NULL = every edge passes every cut;
 *   cuts     HOST array of n_cuts (1..8) ascending pt cuts: cut c <= 0 takes every edge, c > 0 takes
 *            the edge iff pt[src] > c || pt[tgt] > c (ec.py:66-75; a NaN pt fails every c > 0).
 * GNNTRK_EINVAL for n_cuts, n_thr, n_fpr out of range, unordered cuts, NULL required pointers, a small
 * workspace; GNNTRK_EUNSUPPORTED for n >= 2^31. */
#define GNNTRK_METRICS_MAX_CUTS 8
#define GNNTRK_METRICS_MAX_THR 1024
#define GNNTRK_AUC_MAX_FPR 4
#define GNNTRK_AUC_STRIDE 28 /* int64 per cut in gnntrk_roc_auc's output: 4 + 6 * GNNTRK_AUC_MAX_FPR */

/* The threshold scan of get_maximized_bcs (BinaryClassificationStats at every threshold,
 * metrics/binary_classification.py:14-144): ONE pass over the edges.
 *   counts[c][l][k] (int64, [n_cuts][2][n_thr + 1], overwritten) = number of edges passing cut c with
 *   label l whose bin k = #{j : !(w < thr[j])} - the reference predicts true iff !(w < thld), so
 *   TP(thr[j]) = sum over k > j of counts[c][1][k], and a NaN score lands in bin n_thr.
 * thr: DEVICE table of n_thr <= 1024 ascending fp32 thresholds (the caller checks the order). */
int gnntrk_bcs_counts(const float *w, const void *y, int32_t y_kind, const int32_t *perm, const void *src,
                      const void *tgt, int32_t ids_i64, const float *pt, const float *cuts, int32_t n_cuts,
                      const float *thr, int32_t n_thr, int64_t n, int64_t *counts, void *stream);

/* Exact ROC AUC and partial AUCs (get_roc_auc_scores / roc_auc_score, metrics/binary_classification.py:
 * 198-231) of every cut from ONE radix sort of the scores (-0.0 and +0.0 are one tie group) and integer
 * scans over the tie groups.  out (int64, [n_cuts][GNNTRK_AUC_STRIDE], overwritten) per cut:
 *   [0] P, [1] N (positives, negatives passing the cut), [2] U2 = sum over tie groups, highest score
 *   first, of fp_g * (2 tp_before + tp_g): AUC = U2 / (2 P N); [3] number of NaN scores (AUCs NaN if
 *   > 0, as the reference's wrapper turns sklearn's error into NaN; P == 0 or N == 0 likewise).
 *   Per max_fpr m (HOST array of n_fpr <= 4 values in (0, 1]) at [4 + 6m ..]: fp_lim = the largest
 *   count with fp_lim / N <= max_fpr in fp64 (sklearn's fpr), the U2 of the whole groups up to it, and
 *   the group that crosses it as (tp_before, fp_before, tp_g, fp_g) - the caller interpolates linearly
 *   and applies McClish's standardisation in fp64, as sklearn's _binary_roc_auc_score does.
 * workspace: gnntrk_roc_auc_workspace_bytes(n) (16 n bytes of sorted pairs + the sort's scratch). */
size_t gnntrk_roc_auc_workspace_bytes(int64_t n);
int gnntrk_roc_auc(const float *w, const void *y, int32_t y_kind, const int32_t *perm, const void *src, const void *tgt,
                   int32_t ids_i64, const float *pt, const float *cuts, int32_t n_cuts, const double *max_fprs,
                   int32_t n_fpr, int64_t n, int64_t *out, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------ tracking metrics
 * The counts behind the object-condensation stage's TrackingMetrics (metrics/cluster_metrics.py:
 * 76-259) for n_trials cluster labellings of the same n hits at once, as DBSCANHyperParamScanner
 * (postprocessing/dbscanscanner.py:146-187) evaluates them once per DBSCAN trial.  All device pointers
 * except cuts:
 *   labels          [n_trials][n] int64 cluster labels; every label < 0 is noise (no cluster); a label
 *                   >= n is ignored and counted in the last output value;
 *   particle_id     [n] int64 ids of any value (no densification needed);
 *   pt, eta, reconstructable  [n] fp32 per hit;
 *   cuts            HOST array of n_cuts (1..GNNTRK_METRICS_MAX_CUTS) ascending pt cuts.
 * Semantics (the reference's with pandas 2 / numpy 2):
 *   - a cluster is a label >= 0 with at least one hit; valid iff its size >= predicted_count_thld;
 *   - per particle the means over its hits of pt, eta and reconstructable (NaN values skipped, fp64
 *     sums rounded once to fp32); the cluster mask at cut c is: majority particle's mean pt >= c,
 *     mean reconstructable non-zero and not NaN, |mean eta| < max_eta, valid cluster;
 *   - the hit mask at cut c is: pt >= c, reconstructable != 0, |eta| < max_eta; comparisons in fp32;
 *   - the majority particle of a cluster is the one with the most hits in it; TIES go to the
 *     SMALLEST particle id (the reference leaves them to pandas' unstable sort - a tie never decides
 *     a perfect, double-majority or LHC match, only whether the cluster passes the mask);
 *   - perfect: maj_pid_hits == maj_hits && maj_hits / size > 0.99; double majority: maj_hits /
 *     maj_pid_hits > 0.5 && maj_hits / size > 0.5; lhc: maj_hits / size > 0.75 (fp64 ratios).
 * out (int64, n_cuts + n_trials * n_cuts * 4 + 1 values, overwritten):
 *   [c]                              n_particles at cut c: distinct particle ids among the hits that
 *                                    pass the hit mask (independent of the trial);
 *   [n_cuts + (t * n_cuts + c) * 4 + k]  for trial t and cut c: k = 0 clusters passing the cluster
 *                                    mask, 1 perfect, 2 double-majority, 3 lhc matches among them;
 *   [last]                           number of labels >= n over all trials (0 for valid input).
 * workspace: gnntrk_tracking_metrics_workspace_bytes(n, n_trials) (hash tables of 2n..4n slots per
 * trial and for the particles, per-cluster tables).  No host synchronisation.
 * GNNTRK_EINVAL for n_trials or n_cuts out of range, unordered or NaN cuts, NULL required pointers, a
 * small workspace; GNNTRK_EUNSUPPORTED for n >= 2^30. */
#define GNNTRK_TRACKING_MAX_TRIALS 4096
size_t gnntrk_tracking_metrics_workspace_bytes(int64_t n, int32_t n_trials);
int gnntrk_tracking_metrics(const int64_t *labels, int32_t n_trials, const int64_t *particle_id, const float *pt,
                            const float *eta, const float *reconstructable, int64_t n, const float *cuts,
                            int32_t n_cuts, float max_eta, int32_t predicted_count_thld, int64_t *out,
                            void *workspace, size_t workspace_bytes, void *stream);
/* The same counts for every event of a collated batch from one launch sequence: rows [seg_ptr[s],
 * seg_ptr[s+1]) are event s (n_seg >= 1 events, seg_ptr on the device as gnntrk_knn_search_batched takes it).
 * Every event is its own problem:
 *   - a particle is a pair (event, particle id): the hits of one id in two events are two particles, and so is
 *     id 0 (noise) of two events;
 *   - labels are LOCAL to the event, as gnntrk_dbscan_labels_batched writes them: label l of a hit of event s
 *     is the cluster (s, l); a label >= the event's number of hits is ignored and counted in the last output
 *     value (0 <= l < n_s gives the dense cluster slot seg_ptr[s] + l < n).
 * Everything else - masks, means, tie rule (the smallest id of the event), flags - as above, so the values of
 * event s are those of gnntrk_tracking_metrics on its rows alone.
 * out (int64, n_seg * n_cuts + n_trials * n_seg * n_cuts * 4 + 1 values, overwritten):
 *   [s * n_cuts + c]                                        n_particles of event s at cut c;
 *   [n_seg * n_cuts + ((t * n_seg + s) * n_cuts + c) * 4 + k]  trial t, event s, cut c: k as above;
 *   [last]                                                  number of labels >= their event's hits.
 * workspace: gnntrk_tracking_metrics_workspace_bytes(n, n_trials).  No host synchronisation.  Errors as above;
 * GNNTRK_EINVAL also for NULL seg_ptr or n_seg < 1. */
int gnntrk_tracking_metrics_batched(const int64_t *labels, int32_t n_trials, const int64_t *particle_id,
                                    const float *pt, const float *eta, const float *reconstructable, int64_t n,
                                    const int64_t *seg_ptr, int32_t n_seg, const float *cuts, int32_t n_cuts,
                                    float max_eta, int32_t predicted_count_thld, int64_t *out, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* The same counts for two-sided windows instead of nested cuts (tracking_metrics_vs_pt / _vs_eta,
 * metrics/cluster_metrics.py:292-384), arguments as gnntrk_tracking_metrics except:
 *   windows         HOST array of n_win (1..GNNTRK_TRACKING_MAX_WINDOWS) windows, four fp32 each:
 *                   (pt_lo, pt_hi, eta_lo, eta_hi).  A NaN bound means that side is not tested.
 *                   Windows may overlap and need no order.
 *   - a hit is in a window iff pt >= pt_lo, pt < pt_hi, eta >= eta_lo, eta < eta_hi (a NaN value
 *     fails every test that is applied; eta is compared SIGNED, as the reference does there) and
 *     reconstructable != 0 (NaN counts);
 *   - a valid cluster is in a window iff the means of its majority particle pass the same tests and
 *     its mean reconstructable is non-zero and not NaN.  Means, validity, tie rule and flags as above.
 * out (int64, n_win + n_trials * n_win * 4 + 1 values, overwritten): as above with windows for cuts; a
 * particle whose hits lie in several windows counts in each of them.
 * workspace: gnntrk_tracking_metrics_windows_workspace_bytes(n, n_trials).  No host synchronisation.
 * GNNTRK_EINVAL for n_win or n_trials out of range, NULL required pointers, a small workspace;
 * GNNTRK_EUNSUPPORTED for n >= 2^30. */
#define GNNTRK_TRACKING_MAX_WINDOWS 32
size_t gnntrk_tracking_metrics_windows_workspace_bytes(int64_t n, int32_t n_trials);
int gnntrk_tracking_metrics_windows(const int64_t *labels, int32_t n_trials, const int64_t *particle_id,
                                    const float *pt, const float *eta, const float *reconstructable, int64_t n,
                                    const float *windows, int32_t n_win, int32_t predicted_count_thld, int64_t *out,
                                    void *workspace, size_t workspace_bytes, void *stream);
/* The window counts of every event of a collated batch from one launch sequence; events, particles (event, id),
 * local labels and the bad-label count as gnntrk_tracking_metrics_batched, windows as above.  The values of event s
 * are those of gnntrk_tracking_metrics_windows on its rows alone.
 * out (int64, n_seg * n_win + n_trials * n_seg * n_win * 4 + 1 values, overwritten):
 *   [s * n_win + j]                                        n_particles of event s in window j;
 *   [n_seg * n_win + ((t * n_seg + s) * n_win + j) * 4 + k]  trial t, event s, window j: k as above;
 *   [last]                                                 number of labels >= their event's hits.
 * workspace: gnntrk_tracking_metrics_windows_workspace_bytes(n, n_trials).  No host synchronisation.  Errors as
 * above; GNNTRK_EINVAL also for NULL seg_ptr or n_seg < 1. */
int gnntrk_tracking_metrics_windows_batched(const int64_t *labels, int32_t n_trials, const int64_t *particle_id,
                                            const float *pt, const float *eta, const float *reconstructable, int64_t n,
                                            const int64_t *seg_ptr, int32_t n_seg, const float *windows, int32_t n_win,
                                            int32_t predicted_count_thld, int64_t *out, void *workspace,
                                            size_t workspace_bytes, void *stream);

/* The per-cluster rows of tracking_metric_df (metrics/cluster_metrics.py:76-149) of ONE labelling
 * (labels [n], as above) as dense columns of length n indexed by label (device pointers):
 *   cluster_size [n] int64   hits with this label; 0: there is no such cluster (the other columns are 0);
 *   maj_hits     [n] int64   hits of the majority particle in the cluster (tie rule as above);
 *   maj_pid      [n] int64   its id;   maj_pid_hits [n] int64  its hits anywhere;
 *   maj_pt, maj_eta, maj_reconstructable [n] fp32  its means (NaN skipped, fp64 sum rounded once);
 *   n_bad        [1] int64   number of labels >= n (ignored; 0 for valid input).
 * workspace: gnntrk_cluster_table_workspace_bytes(n).  No host synchronisation.
 * GNNTRK_EINVAL for NULL required pointers or a small workspace; GNNTRK_EUNSUPPORTED for n >= 2^30. */
size_t gnntrk_cluster_table_workspace_bytes(int64_t n);
int gnntrk_cluster_table(const int64_t *labels, const int64_t *particle_id, const float *pt, const float *eta,
                         const float *reconstructable, int64_t n, int64_t *cluster_size, int64_t *maj_hits,
                         int64_t *maj_pid, int64_t *maj_pid_hits, float *maj_pt, float *maj_eta,
                         float *maj_reconstructable, int64_t *n_bad, void *workspace, size_t workspace_bytes,
                         void *stream);
/* The same rows for every event of a collated batch from one launch sequence (events, particles and local labels
 * as gnntrk_tracking_metrics_batched): the seven columns keep their length n, row seg_ptr[s] + l is the cluster
 * with the local label l of event s; its majority particle is one of event s (tie: the smallest id of the event).
 * n_bad counts the labels >= their event's number of hits.  The rows of event s are those of gnntrk_cluster_table
 * on its rows alone.  workspace: gnntrk_cluster_table_workspace_bytes(n).  No host synchronisation.  Errors as
 * above; GNNTRK_EINVAL also for NULL seg_ptr or n_seg < 1. */
int gnntrk_cluster_table_batched(const int64_t *labels, const int64_t *particle_id, const float *pt, const float *eta,
                                 const float *reconstructable, int64_t n, const int64_t *seg_ptr, int32_t n_seg,
                                 int64_t *cluster_size, int64_t *maj_hits, int64_t *maj_pid, int64_t *maj_pid_hits,
                                 float *maj_pt, float *maj_eta, float *maj_reconstructable, int64_t *n_bad,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* The size spectra behind the clustering scores of metrics/cluster_metrics.py:400-456 (common_metrics'
 * v_measure, homogeneity, completeness, adjusted_rand and fowlkes_mallows, which the reference hands to
 * sklearn, and count_hits_per_cluster) for n_trials labellings of the same n hits at once.  All five scores
 * are functions of three multisets: the sizes of the truth classes, the sizes of the predicted clusters and
 * the non-zero cells of their contingency table.  Each is returned as its SPECTRUM: the distinct sizes with
 * the number of classes / clusters / cells of exactly that size.  The sizes of a spectrum sum to n, so it has
 * at most D(n) = floor((sqrt(8 n + 1) - 1) / 2) entries = gnntrk_cluster_spectra_capacity(n) (0 for n <= 0).
 * Device pointers:
 *   labels   [n_trials][n] int64 cluster labels;   truth  [n] int64 class ids, may be NULL.
 * Labels and truth ids are CATEGORIES of any int64 value, as sklearn treats what the reference passes it: a
 * negative label is an ordinary cluster (DBSCAN's -1 noise is ONE cluster - unlike gnntrk_tracking_metrics),
 * truth id 0 is an ordinary class, nothing needs densifying and no label is out of range.
 * out (int64, (1 + 2 * n_trials) spectra of 1 + 2 * D(n) values each, overwritten):
 *   spectrum 0            the truth classes;
 *   spectrum 1 + 2 t      the clusters of trial t;
 *   spectrum 2 + 2 t      the contingency cells of trial t;
 *   inside a spectrum     [0] = d, the number of entries, then d pairs (size, multiplicity) in NO particular
 *                         order (every size once); the values behind them are 0.
 * truth == NULL: only the cluster spectra are filled, the class and cell spectra have d = 0.  n == 0 writes
 * d = 0 everywhere and launches nothing.  Integer arithmetic only: the set of pairs does not depend on the
 * order in which atomics land.  workspace: gnntrk_cluster_spectra_workspace_bytes(n, n_trials) (one hash
 * table of 2n..4n slots per spectrum).  No host synchronisation.
 * GNNTRK_EINVAL for n_trials outside 1..GNNTRK_TRACKING_MAX_TRIALS, n < 0, NULL labels, out or workspace, a
 * small workspace; GNNTRK_EUNSUPPORTED for n >= 2^30. */
int64_t gnntrk_cluster_spectra_capacity(int64_t n);
size_t gnntrk_cluster_spectra_workspace_bytes(int64_t n, int32_t n_trials);
int gnntrk_cluster_spectra(const int64_t *labels, int32_t n_trials, const int64_t *truth, int64_t n, int64_t *out,
                           void *workspace, size_t workspace_bytes, void *stream);
/* The spectra of every event of a collated batch from one launch sequence: rows [seg_ptr[s], seg_ptr[s+1]) are
 * event s (n_seg >= 1 events, seg_ptr on the device).  A class is the pair (event, truth id), a cluster the pair
 * (event, label) - labels stay categories of any int64 value, so -1 of two events is two clusters -, a cell
 * belongs to the event of its class.  The spectra of event s are those of gnntrk_cluster_spectra on its rows alone.
 * out (int64, (1 + 2 * n_trials) spectra as above, of 1 + 3 * cap values each, overwritten): a spectrum is ONE
 * pooled list for all events, [0] = d, then d triples (event, size, multiplicity) in NO particular order, every
 * (event, size) once; the values behind them are 0.
 * cap = gnntrk_cluster_spectra_batched_capacity(n, n_seg) = n_seg * (D(ceil(n / n_seg)) + 1), 0 for n <= 0.  It
 * bounds the entries of all events together, sum_s D(n_s): D(x) <= f(x) = (sqrt(8 x + 1) - 1) / 2, f is concave
 * with f(0) = 0, so sum_s D(n_s) <= sum_s f(n_s) <= n_seg f(n / n_seg) < n_seg (D(ceil(n / n_seg)) + 1).
 * workspace: gnntrk_cluster_spectra_workspace_bytes(n, n_trials).  No host synchronisation.  Errors as above;
 * GNNTRK_EINVAL also for NULL seg_ptr or n_seg < 1. */
int64_t gnntrk_cluster_spectra_batched_capacity(int64_t n, int32_t n_seg);
int gnntrk_cluster_spectra_batched(const int64_t *labels, int32_t n_trials, const int64_t *truth, int64_t n,
                                   const int64_t *seg_ptr, int32_t n_seg, int64_t *out, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------ k-scan (metric learning)
 * The device part of GraphConstructionKNNScanner (graph_construction/k_scanner.py:203-285) beyond the
 * neighbour search: connected components and the integer counts behind its records.
 *
 * gnntrk_cc_labels - get_cc_labels (analysis/graphs.py:331-343) and the components of
 * get_largest_segment_fracs (analysis/graphs.py:281-328).  The undirected graph on n nodes is given
 *   - as an edge list: edge_index != NULL, int64 [2, n_edges] (nbr, cnt, k_stride, k ignored), or
 *   - as a prefix of a neighbour table: edge_index == NULL, edges (nbr[q * k_stride + i], q) for
 *     i < min(k, cnt[q]) (the table of gnntrk_knn_search with k = k_stride; 1 <= k <= k_stride),
 * with two optional filters evaluated in the kernel (no filtered edge list is materialised):
 *   same_pid  != NULL: keep an edge only if same_pid[a] == same_pid[b] (k_scanner.py:267-269: plain
 *             equality, two noise hits with id 0 are a true edge);
 *   node_mask != NULL: keep an edge only if both ends pass (Data.subgraph(basic_hit_mask), graphs.py:311-315).
 * labels[i] (int64) = the SMALLEST node index of i's component: unique, independent of the order in which
 * atomics land, and in [0, n) as gnntrk_tracking_metrics takes labels.  (networkx numbers components in
 * discovery order; only the partition is contract there.)  An edge with an end outside [0, n) is skipped
 * and counted in n_bad[0] (device int64, may be NULL).  Lock-free union-find: one pass over the edges,
 * one compression pass, no host read.  workspace: gnntrk_cc_labels_workspace_bytes(n) (4 bytes per node).
 * GNNTRK_EINVAL for n < 0, n_edges < 0, k < 1, k > k_stride, NULL required pointers, a small workspace;
 * GNNTRK_EUNSUPPORTED for n >= 2^30.
 *
 * gnntrk_kscan_counts - everything GraphConstructionKNNScanner._evaluate_graph (k_scanner.py:248-285)
 * counts, for n_ks values of k on ONE neighbour table (nbr / cnt of a search with k = k_stride), in one
 * call without a host read.  ks: HOST array of n_ks (1..GNNTRK_KSCAN_MAX_KS) values in 1..k_stride, any
 * order, repeats allowed.  node_mask: the good-node mask (utils/graph_masks.py:19-28, uint8 [n]).
 * true_edge_index: int64 [2, n_true_edges] (data.true_edge_index; may be NULL with n_true_edges == 0).
 * With y[e] = particle_id[e0] == particle_id[e1] and m = node_mask, row r of
 * out (int64 [n_ks][GNNTRK_KSCAN_COLUMNS], overwritten) holds for k = ks[r]:
 *   [0] n_edges              edges of the k-graph: sum over q of min(k, cnt[q])
 *   [1] n_masked             |{e: m[e0] | m[e1]}|            (metrics/graph_construction.py:18)
 *   [2] n_true_masked        |{e: y[e] and (m[e0] | m[e1])}| (:23-24, numerator of efficiency and purity)
 *   [3] n_true_edges_masked  |{t in true_edge_index: m[t0] & m[t1]}| (:19-21; the same in every row)
 *   [4] n_pids               distinct particle ids among the masked hits (graphs.py:303-305)
 *   [5] n50  [6] n75  [7] n100   particles with 2 s > c, 4 s > 3 c, s == c, where c is the particle's
 *                            number of masked hits and s the size of its largest component in the graph of
 *                            the y edges with both ends masked (graphs.py:311-327; an id without such an
 *                            edge has s = 1, the missing_pids branch) - the integer forms of
 *                            (lsfs > 0.5), (lsfs > 0.75), (lsfs == 1) summed;
 *   [8] n_bad                neighbour or true-edge indices outside [0, n) (skipped; 0 for valid input).
 * labels (int64 [n_ks][n]): row r = gnntrk_cc_labels of the y edges of k = ks[r] on ALL hits - the labels
 * of _evaluate_tracking_metrics_upper_bounds (k_scanner.py:235-246), ready for gnntrk_tracking_metrics
 * with n_trials = n_ks.  The graphs are nested in k: the ks are visited in ascending order and every
 * table edge is united once per call.  workspace: gnntrk_kscan_counts_workspace_bytes(n).
 * GNNTRK_EINVAL for n < 0, n_ks out of range, a k < 1 or > k_stride, NULL required pointers, a small
 * workspace; GNNTRK_EUNSUPPORTED for n >= 2^30.
 *
 * gnntrk_kscan_counts_batched - the same for every event of a collated batch from ONE launch sequence, whose
 * number of launches is that of gnntrk_kscan_counts with the same ks whatever n_seg.  Arguments as above, plus
 *   seg_ptr   device int64 [n_seg + 1], ascending row offsets of the events, seg_ptr[0] = 0 and seg_ptr[n_seg] = n
 *             (as gnntrk_knn_search_batched takes them; empty events are allowed); never read on the host;
 *   n_seg     1..GNNTRK_KSCAN_MAX_EVENTS.
 * out (int64 [n_seg][n_ks][GNNTRK_KSCAN_COLUMNS], overwritten): row (s, r) is what gnntrk_kscan_counts returns for
 * the rows of event s alone with k = ks[r] (an empty event: zeros).  A particle is the pair (event, particle id):
 * ids may repeat from event to event.  labels (int64 [n_ks][n]) are LOCAL to the event, the smallest hit index of
 * the component minus seg_ptr[s]: the slice of event s is the labels of that event alone, in [0, n_s) as
 * gnntrk_tracking_metrics_batched takes them.  Nothing joins two events: a neighbour entry outside its query's
 * event and a true edge whose ends lie in two events are skipped and counted in [8] n_bad - of the query's event
 * and of the event of the true edge's first end - with the indices outside [0, n) (a true edge with one end
 * outside [0, n): the event of the other end; with both: the first event).
 * workspace: gnntrk_kscan_counts_batched_workspace_bytes(n, n_seg, n_ks) - it holds the counter rows of every
 * (event, k).  No host synchronisation; integer arithmetic only, so the outputs do not depend on the order in
 * which atomics land.
 * GNNTRK_EINVAL for NULL seg_ptr, n_seg < 1, a small workspace and everything gnntrk_kscan_counts refuses;
 * GNNTRK_EUNSUPPORTED for n >= 2^30 or n_seg > GNNTRK_KSCAN_MAX_EVENTS. */
#define GNNTRK_KSCAN_COLUMNS 9
#define GNNTRK_KSCAN_MAX_KS 64
#define GNNTRK_KSCAN_MAX_EVENTS 65536
size_t gnntrk_cc_labels_workspace_bytes(int64_t n);
int gnntrk_cc_labels(const int64_t *edge_index, int64_t n_edges, const int32_t *nbr, const int32_t *cnt,
                     int32_t k_stride, int32_t k, const int64_t *same_pid, const uint8_t *node_mask, int64_t n,
                     int64_t *labels, int64_t *n_bad, void *workspace, size_t workspace_bytes, void *stream);
size_t gnntrk_kscan_counts_workspace_bytes(int64_t n);
int gnntrk_kscan_counts(const int32_t *nbr, const int32_t *cnt, int64_t n, int32_t k_stride, const int32_t *ks,
                        int32_t n_ks, const int64_t *particle_id, const uint8_t *node_mask,
                        const int64_t *true_edge_index, int64_t n_true_edges, int64_t *out, int64_t *labels,
                        void *workspace, size_t workspace_bytes, void *stream);
size_t gnntrk_kscan_counts_batched_workspace_bytes(int64_t n, int32_t n_seg, int32_t n_ks);
int gnntrk_kscan_counts_batched(const int32_t *nbr, const int32_t *cnt, int64_t n, int32_t k_stride, const int32_t *ks,
                                int32_t n_ks, const int64_t *particle_id, const uint8_t *node_mask,
                                const int64_t *true_edge_index, int64_t n_true_edges, const int64_t *seg_ptr,
                                int32_t n_seg, int64_t *out, int64_t *labels, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ------------------------------------------------------------ track-graph statistics
 * The device part of get_track_graph_info_from_data (analysis/graphs.py:143-192), which applies
 * get_track_graph_info (graphs.py:86-140) to every selected particle of a built graph: three entries that run
 * back to back on one stream without a host read (csrc/track_graph.hip).  All of them take the events of a
 * collated batch as gnntrk_kscan_counts_batched does (seg_ptr device int64 [n_seg + 1], n_seg in
 * 1..GNNTRK_KSCAN_MAX_EVENTS; one event: seg_ptr = {0, n}); a particle is the pair (event, particle id).
 *
 * gnntrk_track_graph_table - one row per particle that has a hit in node_mask (graphs.py:178-180; the id of such a
 * hit must be > 0, as get_good_node_mask makes it), from
 *   segment_labels    gnntrk_cc_labels of the graph with same_pid = particle_id: the segments (graphs.py:104-108);
 *   component_labels  gnntrk_cc_labels of the graph without a filter (graphs.py:115-119);
 * both int64 [n], the smallest hit index of the component.  table (int64 [n][GNNTRK_TRACK_GRAPH_COLUMNS], the first
 * counts[0] rows are written, in no particular order) holds per row
 *   [0] event   [1] particle id
 *   [2] n_hits                    all hits of the id in the event, masked or not (graphs.py:101-102)
 *   [3] n_segments                (graphs.py:136)
 *   [4] n_hits_largest_segment    (graphs.py:126)
 *   [5] n_hits_largest_component  the largest number of the particle's hits in one component (graphs.py:109-119)
 *   [6] distance_largest_segments 0 for one segment, -1 if the two largest segments lie in different components
 *                                 (no path), -2 if they share one: the row waits for gnntrk_track_graph_distance
 *   [7] [8]                       labels of the largest and the second-largest segment (-1: none); segments of one
 *                                 size rank by ascending label (the reference: by networkx's set order)
 * search (int32 [n]): the counts[1] rows with [6] = -2.  counts: device int64 [2].
 * workspace: gnntrk_track_graph_table_workspace_bytes(n).
 *
 * gnntrk_track_graph_adjacency - the undirected graph of to_networkx(..., to_undirected=True) (graphs.py:172) as
 * rows: rowptr (int64 [n + 1]) and neighbors (int32 [2 * n_edges], the first rowptr[n] are written; the order
 * inside a row is not defined).  An edge with an end outside [0, n) is left out and counted in n_bad[0], one whose
 * ends lie in two events in n_bad[1] (device int64 [2]); a self loop is left out.
 * workspace: gnntrk_track_graph_adjacency_workspace_bytes(n).
 *
 * gnntrk_track_graph_distance - shortest_path_length_multi(graph, segments[0], segments[1]) (graphs.py:121-125) for
 * every row of the search list: the fewest edges on a path in the event's graph from a hit of the largest segment
 * to a hit of the second-largest, written to [6] of the row (-1 if the rows hold no such path).  One workgroup per
 * row runs a level-synchronous breadth-first search over bitmaps of the event's hits, in LDS for an event of at
 * most 163 840 hits, else in the workspace.  gnntrk_track_graph_distance_ex: the same with that capacity given as
 * lds_hits (1..163 840), for tests of the workspace path.
 * workspace: gnntrk_track_graph_distance_workspace_bytes(n, lds_hits) (lds_hits < 1: the default; 0 bytes when
 * n <= lds_hits).
 *
 * GNNTRK_EINVAL for n < 0, n_edges < 0, NULL seg_ptr, n_seg < 1, lds_hits out of range, NULL required pointers and
 * a small workspace; GNNTRK_EUNSUPPORTED for n >= 2^30, n_edges >= 2^30 or n_seg > GNNTRK_KSCAN_MAX_EVENTS. */
#define GNNTRK_TRACK_GRAPH_COLUMNS 9
size_t gnntrk_track_graph_table_workspace_bytes(int64_t n);
int gnntrk_track_graph_table(const int64_t *segment_labels, const int64_t *component_labels, const int64_t *particle_id,
                             const uint8_t *node_mask, int64_t n, const int64_t *seg_ptr, int32_t n_seg, int64_t *table,
                             int32_t *search, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
size_t gnntrk_track_graph_adjacency_workspace_bytes(int64_t n);
int gnntrk_track_graph_adjacency(const int64_t *edge_index, int64_t n_edges, int64_t n, const int64_t *seg_ptr,
                                 int32_t n_seg, int64_t *rowptr, int32_t *neighbors, int64_t *n_bad, void *workspace,
                                 size_t workspace_bytes, void *stream);
size_t gnntrk_track_graph_distance_workspace_bytes(int64_t n, int32_t lds_hits);
int gnntrk_track_graph_distance(int64_t *table, const int32_t *search, const int64_t *counts,
                                const int64_t *segment_labels, const int64_t *rowptr, const int32_t *neighbors, int64_t n,
                                const int64_t *seg_ptr, int32_t n_seg, void *workspace, size_t workspace_bytes,
                                void *stream);
int gnntrk_track_graph_distance_ex(int64_t *table, const int32_t *search, const int64_t *counts,
                                   const int64_t *segment_labels, const int64_t *rowptr, const int32_t *neighbors,
                                   int64_t n, const int64_t *seg_ptr, int32_t n_seg, int32_t lds_hits, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------- EC threshold scan
 * The device part of get_all_ec_stats / collect_all_ec_stats (analysis/edge_classification.py:24-112) for ALL
 * thresholds of a list at once (csrc/ec_scan.hip): per threshold t the binary-classification counts of the edge
 * scores and, per selected particle, three figures of the graph of the edges with w > t.  Two entries on one stream
 * share one caller-owned workspace of gnntrk_ec_scan_prepare_workspace_bytes(n, n_edges, n_thr) bytes, which the
 * caller leaves alone between them; the caller reads head[0] in between to size `steps`.  Events: seg_ptr / n_seg as
 * for the track-graph entries; a particle is the pair (event, particle id).
 *
 * gnntrk_ec_scan_prepare - once per scan.
 *   edge_index  int64 [2][n_edges];  w float32 [n_edges];  y [n_edges]: bytes (y_kind 0, positive iff == 1) or
 *               float32 (y_kind 1, positive iff int(y) == 1), as gnntrk_bcs_counts;  particle_id int64 [n];
 *               node_mask uint8 [n] (the id of a masked hit must be > 0)
 *   thresholds  DEVICE float32 [n_thr], strictly ascending, n_thr in 1..GNNTRK_EC_SCAN_MAX_THR
 *   per_event   0: one set of counts over all events; else one per event
 *   head        device int64 [4]: selected particles P, 0, edges with an end outside [0, n), edges across two events.
 *               Either kind of bad edge is in no graph; the caller refuses the call when one is counted.
 *   particles   int64 [n][3], the first P rows written in no particular order: event, particle id, n_hits (all hits
 *               of the id in the event).  The row number of a particle is its row in `steps`.
 *   bcs         int64 [E][2][2][n_thr + 1] (E = n_seg with per_event, else 1): edges per event (of the first end),
 *               mask class (1: both ends in node_mask), label and bin k = #{j : !(w < t_j)} (a NaN score: bin n_thr).
 *               TP / FP of threshold j are the sums over the bins > j; an edge with an end outside [0, n) is in no bin.
 *   orphans     int64 [E][3]: hits that are no end of any edge of edge_index, outside node_mask | inside | all
 * An edge is in the graph of threshold j iff w > t_j (a NaN weight: in none): its graph bin g = #{j : w > t_j}.
 *
 * gnntrk_ec_scan_steps - the thresholds from the largest to the smallest on two union-find forests that are never
 * reset (every edge is united once).  steps: int32 [n_thr][n_particles][3], n_particles = head[0]; steps[j][r] =
 * n_segments, n_hits_largest_segment, n_hits_largest_component of the particle of row r in the graph of threshold j
 * (the columns of gnntrk_track_graph_table).  distance_largest_segments is not part of the scan.
 *
 * GNNTRK_EINVAL for n < 0, n_edges < 0, n_thr < 1, NULL seg_ptr, n_seg < 1, y_kind not 0 / 1, n_particles outside
 * 0..n, NULL required pointers and a small or NULL workspace; GNNTRK_EUNSUPPORTED for n >= 2^30, n_edges >= 2^30,
 * n_thr > GNNTRK_EC_SCAN_MAX_THR or n_seg > GNNTRK_KSCAN_MAX_EVENTS.  n == 0 and n_edges == 0 succeed. */
#define GNNTRK_EC_SCAN_MAX_THR 256
size_t gnntrk_ec_scan_prepare_workspace_bytes(int64_t n, int64_t n_edges, int32_t n_thr);
int gnntrk_ec_scan_prepare(const int64_t *edge_index, int64_t n_edges, const float *w, const void *y, int32_t y_kind,
                           const int64_t *particle_id, const uint8_t *node_mask, int64_t n, const int64_t *seg_ptr,
                           int32_t n_seg, const float *thresholds, int32_t n_thr, int32_t per_event, int64_t *head,
                           int64_t *particles, int64_t *bcs, int64_t *orphans, void *workspace, size_t workspace_bytes,
                           void *stream);
int gnntrk_ec_scan_steps(const int64_t *edge_index, int64_t n_edges, const int64_t *particle_id, int64_t n,
                         int32_t n_thr, int64_t n_particles, int32_t *steps, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------- geometric graph builder
 * The device part of GraphBuilder.build_edges / correct_truth_labels / get_n_truth_edges and of the measurement
 * record (graph_construction/graph_builder.py:162-394, 457-469, 531-549): the edges between the hits of the layer
 * pairs of a list that pass the cuts, in the reference's order (csrc/graph_builder.hip).  Events: seg_ptr / n_seg as
 * for the track-graph entries; pairs are formed inside an event only and the edges are event-major.
 *
 *   x        float32 [n][x_stride], columns 0..2 = r, phi, z;  layer int64 [n], a hit on a layer outside
 *            [0, GNNTRK_GB_MAX_LAYERS) is counted and takes part in no pair
 *   pairs    HOST int32 [n_pairs][2] (layer 1, layer 2), n_pairs <= GNNTRK_GB_MAX_PAIRS
 *   radius   HOST float64 [n_pairs]: radius of the intersecting-line cut of the pair, 0 for none
 *   cuts     HOST float64 [4]: phi_slope_max, z0_max, dR_max, remove_intersecting (0 / not 0)
 * A pair of hits (1 on layer 1, 2 on layer 2) is an edge iff, all in float64 from the float32 columns with IEEE
 * division: |dphi / dr| < phi_slope_max, |z1 - r1 dz / dr| < z0_max, sqrt(deta^2 + dphi^2) < dR_max and, with
 * remove_intersecting and a radius, NOT -490.975 < radius dz / dr + z0 < 490.975; dphi = phi2 - phi1, reduced by 2 pi
 * if > pi, then raised by 2 pi if < -pi; eta = -log(tan(atan2(r, z) / 2)).  Order: event, pair, hit 1, hit 2, the hits
 * ascending in index.
 *
 * gnntrk_graph_builder_count - groups the hits, counts the edges of every row (event, pair, hit 1) and scans the
 *   counts.  head: device int64 [2] = number of edges, hits on a layer out of range.  The workspace
 *   (gnntrk_graph_builder_count_workspace_bytes, 0 for n <= 0 or no pairs) keeps the groups and the offsets for
 * gnntrk_graph_builder_fill - the same arguments and workspace, n_edges = head[0] read by the caller: writes edge_index
 *   int64 [2][n_edges], edge_attr float32 [4][n_edges] = dr / 1000, dphi / pi, dz / 1000, dR (rounded once from float64),
 *   y float32 [n_edges] = (id 1 == id 2 and id 1 > 0), edge_pt float32 [n_edges] = pt of hit 1 and edge_ptr int64
 *   [n_seg + 1], the first edge of every event.  Count and fill decide with one device function.
 * gnntrk_graph_builder_truth - for the edges of a fill (or none: n_edges = 0): with `relabel`, a true edge of a
 *   particle (event, id > 0) from a barrel layer 7..10 to layer 6 or 11 becomes false when the particle's true edges
 *   hold more than one such layer pair and a pair of a higher barrel layer among them (correct_truth_labels); then
 *   counts int64 [n_seg][GNNTRK_GB_COUNTS] per event: edges, true edges, true edges with edge_pt > 0, 0.1, 0.5, 0.9, 1.0
 *   (float32 comparisons), relabelled edges, the five n_truth_edges of get_n_truth_edges (per particle with id > 0 the
 *   products of its hit counts on consecutive occupied layers, counted where the pt of its first hit is > the cut),
 *   hits on a layer out of range.  workspace: gnntrk_graph_builder_truth_workspace_bytes(n).
 *
 * GNNTRK_EINVAL for n < 0, n_edges < 0, NULL seg_ptr, n_seg < 1, a pair or radius out of range, x_stride < 3, NULL
 * required pointers and a small or NULL workspace; GNNTRK_EUNSUPPORTED for n >= 2^30, n_edges >= 2^30, more than
 * 2^30-1 rows, n_pairs > GNNTRK_GB_MAX_PAIRS or n_seg > GNNTRK_KSCAN_MAX_EVENTS.  n == 0 succeeds. */
#define GNNTRK_GB_MAX_LAYERS 64
#define GNNTRK_GB_MAX_PAIRS 128
#define GNNTRK_GB_COUNTS 14
size_t gnntrk_graph_builder_count_workspace_bytes(int64_t n, int32_t n_seg, const int32_t *pairs, int32_t n_pairs);
int gnntrk_graph_builder_count(const float *x, int64_t x_stride, const int64_t *layer, int64_t n, const int64_t *seg_ptr,
                               int32_t n_seg, const int32_t *pairs, const double *radius, int32_t n_pairs,
                               const double *cuts, int64_t *head, void *workspace, size_t workspace_bytes, void *stream);
int gnntrk_graph_builder_fill(const float *x, int64_t x_stride, const int64_t *layer, const int64_t *particle_id,
                              const float *pt, int64_t n, const int64_t *seg_ptr, int32_t n_seg, const int32_t *pairs,
                              const double *radius, int32_t n_pairs, const double *cuts, int64_t n_edges,
                              int64_t *edge_index, float *edge_attr, float *y, float *edge_pt, int64_t *edge_ptr,
                              void *workspace, size_t workspace_bytes, void *stream);
size_t gnntrk_graph_builder_truth_workspace_bytes(int64_t n);
int gnntrk_graph_builder_truth(const int64_t *edge_index, int64_t n_edges, float *y, const float *edge_pt,
                               const int64_t *layer, const int64_t *particle_id, const float *pt, int64_t n,
                               const int64_t *seg_ptr, int32_t n_seg, int32_t relabel, int64_t *counts, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ---- point cloud builder on the device: the tables of a TrackML event to sector point clouds
 * (preprocessing/point_cloud_builder.py:156-353, 397-450; exatrkx_cell_features.py:174-250; csrc/point_cloud.hip).
 * Every join is by key (hit_id, particle_id as int64), never by position.  All arrays but those marked HOST are device
 * arrays.  One event per call.
 *
 * gnntrk_point_cloud_select - joins the tables, selects the hits and writes the columns of the kept hits in the order
 *   of the hit table:
 *   hit_id int64 [n_hits], hit_xyz float64 [n_hits][3], hit_vlm int32 [n_hits][3] (volume_id, layer_id, module_id);
 *   cell_hit_id int64 [n_cells], cell_ch int32 [n_cells][2] (ch0, ch1), cell_value float64 [n_cells];
 *   part_id int64 [n_particles], part_p float64 [n_particles][3] (px, py, pz);
 *   truth_hit_id, truth_pid int64 [n_truth];
 *   layer_map int32 [GNNTRK_PC_MAX_IDS][GNNTRK_PC_MAX_IDS]: (volume_id, layer_id) -> layer, -1: the hit is dropped;
 *   det_index int32 [det_dims[0]][det_dims[1]][det_dims[2]]: (volume, layer, module) -> row of det_rows or -1, det_dims
 *   HOST int32 [3], det_rows float64 [n_modules][12]: the rotation (row-major 3 x 3), module_t, pitch_u, pitch_v;
 *   feat_code HOST int32 [n_feat] in [0, GNNTRK_PC_FEATURE_CODES): x, y, z, r, phi, eta_rz, u, v, charge_frac,
 *   cell_count, cell_val, leta, lphi, lx, ly, lz, geta, gphi, V7, V8, V9, V12, V13, V14, V16, V17, V18 in this order;
 *   feat_scale HOST float64 [n_feat].  A hit is kept when it has a layer, a truth row, and a particle id that is 0
 *   (unless remove_noise) or in part_id.  Outputs, every one with room for n_hits rows, the first head[0] filled:
 *   x float32 [n_hits][n_feat] (float64 / scale, rounded once), cols int64 [GNNTRK_PC_COLUMNS][n_hits] = layer,
 *   particle_id, reconstructable, n_hits, n_layers_hit (distinct layer_id), index in the hit table; pt_eta float32
 *   [2][n_hits] (noise: 0 and NaN); uv float64 [n_hits][2]; slot int32 [n_hits]: row of the particle, n_particles for
 *   noise.  head int64 [GNNTRK_PC_HEAD]: kept hits, duplicate hit_ids, hits on a layer without a cell, kept hits on a
 *   module that det_index lacks, hits with a volume_id or layer_id outside [0, GNNTRK_PC_MAX_IDS), further truth rows of
 *   one hit, duplicate particle ids, distinct particle ids of the kept hits (0 is one), noise hits; the rest 0.
 * gnntrk_point_cloud_sectors - for the columns of a select (capacity = its n_hits, n_kept = its head): the sector
 *   predicate of every (kept hit, sector), with sector_cs float64 [n_sectors][2] = cos, sin of 2 s pi / n_sectors,
 *   slope = arctan(pi / n_sectors); n_sectors == 1: every hit, nothing evaluated.  counts int64
 *   [n_sectors][GNNTRK_PC_SECTOR_COUNTS]: hits in the wedge, in the extended wedge, distinct ids there, the numerator and
 *   denominator of majority_contained (pt >= thld / pt > thld), pairs of hits of one id > 0 there.  head int64 [2]: rows
 *   of all clouds, pairs of all clouds.  The workspace keeps the rows for
 * gnntrk_point_cloud_gather - n_rows = head[0] read by the caller: x_out float32 [n_rows][n_feat], cols_out int64
 *   [GNNTRK_PC_COLUMNS][n_rows] = layer, particle_id, reconstructable, n_hits, n_layers_hit, sector; pt_eta_out float32
 *   [2][n_rows]: the clouds one after the other, each in hit order.  sector = s where a hit of the particle (id > 0)
 *   lies in the wedge of s, else -1 (n_sectors == 1: 0): the reference divides the hits in the wedge by the length of
 *   the particle's row of its per-particle table, which is 1, before it compares with 0.5; majority_contained likewise.
 * gnntrk_truth_edges_count / _fill - every pair i < j of hits with one non-zero particle id inside a segment
 *   (seg_ptr int64 [n_seg + 1]), in lexicographic order: counts int64 [n_seg]; then, n_edges = their sum, edge_index
 *   int64 [2][n_edges] with global ids (global_ids != 0), or per segment its own block [2][m_s] of ids local to the
 *   segment, the blocks one after the other; edge_ptr int64 [n_seg + 1].
 *
 * GNNTRK_EINVAL for negative sizes, NULL required pointers, a feature code out of range, n_sectors < 1, a small or NULL
 * workspace; GNNTRK_EUNSUPPORTED for a table of 2^30 rows or more, hits x sectors or particles x sectors of 2^30 or more,
 * n_feat > GNNTRK_PC_MAX_FEATURES, n_seg > GNNTRK_KSCAN_MAX_EVENTS.  Empty tables succeed. */
#define GNNTRK_PC_MAX_FEATURES 32
#define GNNTRK_PC_FEATURE_CODES 27
#define GNNTRK_PC_MAX_IDS 64
#define GNNTRK_PC_HEAD 12
#define GNNTRK_PC_COLUMNS 6
#define GNNTRK_PC_SECTOR_COUNTS 6
size_t gnntrk_point_cloud_select_workspace_bytes(int64_t n_hits, int64_t n_cells, int64_t n_particles);
int gnntrk_point_cloud_select(const int64_t *hit_id, const double *hit_xyz, const int32_t *hit_vlm, int64_t n_hits,
                              const int64_t *cell_hit_id, const int32_t *cell_ch, const double *cell_value, int64_t n_cells,
                              const int64_t *part_id, const double *part_p, int64_t n_particles,
                              const int64_t *truth_hit_id, const int64_t *truth_pid, int64_t n_truth,
                              const int32_t *layer_map, const int32_t *det_index, const int32_t *det_dims,
                              const double *det_rows, int64_t n_modules, const int32_t *feat_code, const double *feat_scale,
                              int32_t n_feat, int32_t remove_noise, float *x, int64_t *cols, float *pt_eta, double *uv,
                              int32_t *slot, int64_t *head, void *workspace, size_t workspace_bytes, void *stream);
size_t gnntrk_point_cloud_sectors_workspace_bytes(int64_t capacity, int64_t n_particles, int32_t n_sectors);
int gnntrk_point_cloud_sectors(const double *uv, const int32_t *slot, const int64_t *n_kept,
                               int64_t capacity, const double *part_p, int64_t n_particles, int32_t n_sectors,
                               const double *sector_cs, double slope, double sector_ds, double sector_di, double thld,
                               int64_t *counts, int64_t *head, void *workspace, size_t workspace_bytes, void *stream);
int gnntrk_point_cloud_gather(const float *x, const int64_t *cols, const float *pt_eta, const int32_t *slot,
                              int64_t capacity, int32_t n_feat, int64_t n_particles, int32_t n_sectors, int64_t n_rows,
                              float *x_out, int64_t *cols_out, float *pt_eta_out, void *workspace, size_t workspace_bytes,
                              void *stream);
size_t gnntrk_truth_edges_workspace_bytes(int64_t n);
int gnntrk_truth_edges_count(const int64_t *particle_id, int64_t n, const int64_t *seg_ptr, int32_t n_seg, int64_t *counts,
                             void *workspace, size_t workspace_bytes, void *stream);
int gnntrk_truth_edges_fill(const int64_t *particle_id, int64_t n, const int64_t *seg_ptr, int32_t n_seg, int64_t n_edges,
                            int32_t global_ids, int64_t *edge_index, int64_t *edge_ptr, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ---- dynamic edge convolution on a k-nearest-neighbour table (csrc/edge_conv.hip) ----------------------------------
 * Reference: models/dynamic_edge_conv.py:14-64 (DynamicEdgeConv.forward :36-58 and .message :60-61), as INConvBlock
 * uses it (models/track_condensation_networks.py:35-36, :57-58):
 *     h[i] = aggr_{s < count[i]} nn(cat[x[i], x[j(i, s)] - x[i]]),   nn = Linear(2 dim, hidden) -> ReLU -> Linear(hidden, out_dim)
 * x float32 [n][dim] with row stride x_stride; nbr int32 [n][k_stride] and cnt int32 [n] exactly as gnntrk_knn_search*
 * writes them (cnt is clamped to 0 .. k, ids outside [0, n) are clamped: a bad table reads a wrong hit, never foreign
 * memory).  include_self: slot 0 of every query is the query itself (message input [x[i], 0]), then its cnt[i]
 * neighbours; count[i] = cnt[i] + include_self.  W1 [hidden][2 dim], W2 [out_dim][hidden] in nn.Linear storage, b1 /
 * b2 or NULL.  aggr: 0 add, 1 mean (the sum over the present slots divided by their number), 2 max (ties: the lowest
 * slot).  A query without a slot gives 0.  relu: ReLU on the aggregated row.  The difference x[j] - x[i] is formed in
 * fp32 from the loaded rows and then contracted.
 *
 * gnntrk_edge_conv_forward - h float32 [n][out_dim]; win int32 [n][out_dim] (max only, NULL otherwise): the winning
 *   slot of every (node, feature), -1 for a query without a slot.  Nothing of size n k is written.
 * gnntrk_edge_conv_backward - recomputes the hidden layer per (node, slot).  h, win: what the forward wrote (h is read
 *   for the ReLU gate only, win for max only).  gout float32 [n][out_dim].  gW1, gb1, gW2, gb2: set, or added to with
 *   accumulate != 0; NULL: not wanted.  Per-workgroup partial sums, added in a fixed order (no atomics).
 *   gx_tgt float32 [n][dim] and gx_slot float32 [n][k + include_self][dim] together or both NULL (no input-gradient
 *   work): gx_tgt[i] = sum_s (g_a - g_b) and gx_slot[i][s] = g_b for s < count[i], the gradient of slot s for its
 *   source row j(i, s), which the caller sums per source in a fixed order (rows of absent slots are undefined).
 * gnntrk_edge_conv_workspace_bytes - of either entry (backward != 0: the backward's); 0 for refused shapes.
 *
 * GNNTRK_EINVAL for n < 0, k < 1, k_stride < k, aggr out of range, non-positive widths, NULL required pointers, a small
 * or NULL workspace; GNNTRK_EUNSUPPORTED for 2 dim > GNNTRK_RESFCNN_MAX_IN, hidden > GNNTRK_RESFCNN_MAX_WIDTH, out_dim >
 * GNNTRK_RESFCNN_MAX_OUT, k + include_self > 64, n >= 2^30.  n == 0 returns GNNTRK_OK without a launch. */
size_t gnntrk_edge_conv_workspace_bytes(int32_t dim, int32_t hidden, int32_t out_dim, int64_t n, int32_t backward);
int gnntrk_edge_conv_forward(const float *x, int32_t x_stride, int64_t n, int32_t dim, const int32_t *nbr,
                             const int32_t *cnt, int32_t k, int32_t k_stride, int32_t include_self, const float *W1,
                             const float *b1, const float *W2, const float *b2, int32_t hidden, int32_t out_dim,
                             int32_t aggr, int32_t relu, float *h, int32_t *win, void *workspace, size_t workspace_bytes,
                             void *stream);
int gnntrk_edge_conv_backward(const float *x, int32_t x_stride, int64_t n, int32_t dim, const int32_t *nbr,
                              const int32_t *cnt, int32_t k, int32_t k_stride, int32_t include_self, const float *W1,
                              const float *b1, const float *W2, const float *b2, int32_t hidden, int32_t out_dim,
                              int32_t aggr, int32_t relu, const float *h, const int32_t *win, const float *gout, float *gW1,
                              float *gb1, float *gW2, float *gb2, float *gx_tgt, float *gx_slot, int32_t accumulate,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---- event packer: many byte ranges into one contiguous image, one launch (csrc/pack.hip) --------------------------
 * What the dataset writer (gnn_tracking_amd/io.py) moves off the device: every (event, field) range of a collated batch
 * is one SEGMENT, copied to `dst + dst_off`.  mode GNNTRK_PACK_RAW copies n_bytes bytes; GNNTRK_PACK_SUB_I64 /
 * GNNTRK_PACK_SUB_I32 copy n_bytes / 8 int64 (n_bytes / 4 int32) elements minus `sub` (the node offset of the event,
 * for the `*index*` fields).  `src` is the device address of the first byte.  Bytes of dst that no segment covers are
 * not written; segments must not overlap (the result would depend on the order of the writers).
 *
 * The PLAN is the descriptor table followed by the chunk table: gnntrk_pack_seg [n_segs], then for every segment in
 * order and every k < ceil(n_bytes / GNNTRK_PACK_CHUNK_BYTES) the pair int32 (segment, k), n_chunks pairs in all.  The
 * caller builds it on the host and uploads it as one block:
 *     segs - the plan's HOST image, which the entry checks completely before it launches anything;
 *     plan - the plan's DEVICE image, a copy of the same bytes, which the kernel reads.
 * gnntrk_pack_plan_bytes - the size of either (0 for counts out of range).
 *
 * GNNTRK_EINVAL, before any launch, for: negative sizes; n_segs > GNNTRK_PACK_MAX_SEGS or n_chunks >
 * GNNTRK_PACK_MAX_CHUNKS; NULL segs, plan or dst; a dst that is not 16-byte aligned; a segment with a NULL src and
 * n_bytes > 0, an unknown mode, dst_off + n_bytes beyond dst_bytes, in a sub mode an n_bytes that is no multiple of the
 * element size, a src or dst_off that is not a multiple of it, or (int32) a sub outside int32; a chunk table that is
 * not the one described above (the sizes do not fit n_chunks).  n_segs == 0 returns GNNTRK_OK without a launch. */
#define GNNTRK_PACK_CHUNK_BYTES 16384
#define GNNTRK_PACK_MAX_SEGS 1048576
#define GNNTRK_PACK_MAX_CHUNKS 4194304
#define GNNTRK_PACK_RAW 0
#define GNNTRK_PACK_SUB_I64 1
#define GNNTRK_PACK_SUB_I32 2
typedef struct {
    uint64_t src;     /* device address of the first source byte */
    int64_t dst_off;  /* byte offset in the image */
    int64_t n_bytes;
    int64_t sub;
    int32_t mode;
    int32_t _pad;
} gnntrk_pack_seg;
size_t gnntrk_pack_plan_bytes(int64_t n_segs, int64_t n_chunks);
int gnntrk_pack_segments(const gnntrk_pack_seg *segs, int64_t n_segs, const void *plan, int64_t n_chunks, void *dst,
                         int64_t dst_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNTRK_H */
