// Event packer (gnntrk_pack_segments): many byte ranges of device memory into ONE contiguous byte image, one launch.
//
// A collated batch of B events with F fields leaves the device as B x F small copies otherwise (32 events x 14 fields:
// 448 of them, the index fields after a subtraction of the event's node offset).  Here the caller describes every
// (event, field) range by a segment descriptor, the segments are cut into chunks of GNNTRK_PACK_CHUNK_BYTES on the
// host, and a workgroup copies one chunk at a time: it reads its (segment, chunk of the segment) pair from the chunk
// table of the plan, then streams the chunk with 16-byte loads and stores where source and destination agree modulo
// 16 (a byte-wise head up to the first 16-byte boundary and a byte-wise tail), with 4-byte words where they agree
// modulo 4 only, byte by byte otherwise.  The two index modes subtract `sub` from every int64 / int32 element on the
// way.  No atomics, no LDS: every output byte has one writer and is a pure function of the input; bytes of the image
// that no segment covers are not touched.
//
// HBM-bound: every payload byte is read once and written once, plus 40 bytes per segment and 8 per chunk of plan.
#include "host_util.h"

#include <stdio.h>

static_assert(sizeof(gnntrk_pack_seg) == 40, "gnntrk_pack_seg layout");
static_assert(GNNTRK_PACK_CHUNK_BYTES % 16 == 0, "chunks keep the alignment of their segment");

namespace gnntrk {

constexpr int kPackTpb = 256;                                   // 4 waves
constexpr int kPackChunk = GNNTRK_PACK_CHUNK_BYTES;
constexpr int kPackVecs = kPackChunk / 16 / kPackTpb;           // 16-byte vectors per thread and chunk
static_assert(kPackVecs * 16 * kPackTpb == kPackChunk, "a chunk is a whole number of 16-byte vectors per thread");

struct PackChunk {
    int32_t seg, k;   // the segment and the chunk's number inside it
};

__device__ __forceinline__ void copy_bytes(const uint8_t *src, uint8_t *dst, int64_t lo, int64_t hi) {
    for (int64_t i = lo + threadIdx.x; i < hi; i += kPackTpb) dst[i] = src[i];
}

// The 16-byte vectors [0, nvec) of one chunk, nvec <= kPackVecs * kPackTpb: every thread issues all its loads before
// its first store; f changes a loaded vector in place.  Four named registers, not an array: an array indexed in a loop
// is an alloca, which the compiler may move to LDS.
template <class V, class F>
__device__ __forceinline__ void copy_vecs(const V *__restrict__ s, V *__restrict__ d, int nvec, F f) {
    static_assert(kPackVecs == 4 && sizeof(V) == 16, "four 16-byte vectors per thread and chunk");
    const int i0 = (int)threadIdx.x, i1 = i0 + kPackTpb, i2 = i1 + kPackTpb, i3 = i2 + kPackTpb;
    V v0, v1, v2, v3;
    if (i0 < nvec) v0 = s[i0];
    if (i1 < nvec) v1 = s[i1];
    if (i2 < nvec) v2 = s[i2];
    if (i3 < nvec) v3 = s[i3];
    if (i0 < nvec) { f(v0); d[i0] = v0; }
    if (i1 < nvec) { f(v1); d[i1] = v1; }
    if (i2 < nvec) { f(v2); d[i2] = v2; }
    if (i3 < nvec) { f(v3); d[i3] = v3; }
}

// raw bytes [0, n) of one chunk
__device__ __forceinline__ void pack_raw(const uint8_t *src, uint8_t *dst, int n) {
    const unsigned sa = (unsigned)((uintptr_t)src & 15), da = (unsigned)((uintptr_t)dst & 15);
    if (sa == da) {
        int head = (int)((16 - sa) & 15);
        head = head < n ? head : n;
        const int nvec = (n - head) / 16;
        copy_bytes(src, dst, 0, head);
        copy_vecs(reinterpret_cast<const uint4 *>(src + head), reinterpret_cast<uint4 *>(dst + head), nvec, [](uint4 &) {});
        // (a head moves the body by less than 16 bytes: one more vector than kPackVecs * kPackTpb cannot occur)
        copy_bytes(src, dst, head + 16 * (int64_t)nvec, n);
    } else if (((sa ^ da) & 3) == 0) {
        int head = (int)((4 - (sa & 3)) & 3);
        head = head < n ? head : n;
        const int nw = (n - head) / 4;
        copy_bytes(src, dst, 0, head);
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + head);
        uint32_t *d = reinterpret_cast<uint32_t *>(dst + head);
        for (int i = threadIdx.x; i < nw; i += kPackTpb) d[i] = s[i];
        copy_bytes(src, dst, head + 4 * (int64_t)nw, n);
    } else {
        copy_bytes(src, dst, 0, n);
    }
}

// n bytes of int64 elements minus sub (src and dst 8-byte aligned, n a multiple of 8: the host checked)
__device__ __forceinline__ void pack_sub64(const uint8_t *src, uint8_t *dst, int n, int64_t sub) {
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const int nvec = n / 16;
        copy_vecs(reinterpret_cast<const longlong2 *>(src), reinterpret_cast<longlong2 *>(dst), nvec, [sub](longlong2 &v) {
            v.x -= sub;
            v.y -= sub;
        });
        if (threadIdx.x == 0 && (n & 8))
            reinterpret_cast<int64_t *>(dst)[2 * nvec] = reinterpret_cast<const int64_t *>(src)[2 * nvec] - sub;
    } else {
        const int64_t *s = reinterpret_cast<const int64_t *>(src);
        int64_t *d = reinterpret_cast<int64_t *>(dst);
        for (int i = threadIdx.x; i < n / 8; i += kPackTpb) d[i] = s[i] - sub;
    }
}

// n bytes of int32 elements minus sub (src and dst 4-byte aligned, n a multiple of 4: the host checked)
__device__ __forceinline__ void pack_sub32(const uint8_t *src, uint8_t *dst, int n, int32_t sub) {
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const int nvec = n / 16;
        copy_vecs(reinterpret_cast<const int4 *>(src), reinterpret_cast<int4 *>(dst), nvec, [sub](int4 &v) {
            v.x -= sub;
            v.y -= sub;
            v.z -= sub;
            v.w -= sub;
        });
        const int done = 4 * nvec, rest = n / 4 - done;   // up to three elements
        if ((int)threadIdx.x < rest)
            reinterpret_cast<int32_t *>(dst)[done + threadIdx.x] =
                reinterpret_cast<const int32_t *>(src)[done + threadIdx.x] - sub;
    } else {
        const int32_t *s = reinterpret_cast<const int32_t *>(src);
        int32_t *d = reinterpret_cast<int32_t *>(dst);
        for (int i = threadIdx.x; i < n / 4; i += kPackTpb) d[i] = s[i] - sub;
    }
}

// One chunk per workgroup and turn of the grid-stride loop.  Everything read from the plan is uniform over the
// workgroup.  A pair of the chunk table that names no segment or a range outside the image is skipped: the host
// entry has refused such a plan, so this only bounds what a device image that differs from the checked one can do.
__global__ __launch_bounds__(kPackTpb) void pack_segments_kernel(const gnntrk_pack_seg *__restrict__ segs, int64_t n_segs,
                                                                const PackChunk *__restrict__ chunks, int64_t n_chunks,
                                                                uint8_t *__restrict__ dst, int64_t dst_bytes) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const PackChunk ch = chunks[c];
        if (ch.seg < 0 || ch.seg >= n_segs || ch.k < 0) continue;
        const gnntrk_pack_seg sg = segs[ch.seg];
        const int64_t lo = (int64_t)ch.k * kPackChunk;
        if (sg.n_bytes < 0 || lo >= sg.n_bytes || sg.dst_off < 0 || sg.dst_off > dst_bytes - sg.n_bytes) continue;
        const int64_t left = sg.n_bytes - lo;
        const int n = (int)(left < kPackChunk ? left : kPackChunk);
        const uint8_t *s = reinterpret_cast<const uint8_t *>((uintptr_t)sg.src) + lo;
        uint8_t *d = dst + sg.dst_off + lo;
        if (sg.mode == GNNTRK_PACK_SUB_I64) pack_sub64(s, d, n, sg.sub);
        else if (sg.mode == GNNTRK_PACK_SUB_I32) pack_sub32(s, d, n, (int32_t)sg.sub);
        else pack_raw(s, d, n);
    }
}

static int64_t chunks_of(int64_t n_bytes) { return ceil_div(n_bytes, kPackChunk); }

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

size_t gnntrk_pack_plan_bytes(int64_t n_segs, int64_t n_chunks) {
    if (n_segs < 0 || n_segs > GNNTRK_PACK_MAX_SEGS || n_chunks < 0 || n_chunks > GNNTRK_PACK_MAX_CHUNKS) return 0;
    return (size_t)n_segs * sizeof(gnntrk_pack_seg) + (size_t)n_chunks * sizeof(PackChunk);
}

int gnntrk_pack_segments(const gnntrk_pack_seg *segs, int64_t n_segs, const void *plan, int64_t n_chunks, void *dst,
                         int64_t dst_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    char msg[200];
    if (n_segs < 0 || n_chunks < 0 || dst_bytes < 0) return fail(GNNTRK_EINVAL, "pack_segments: negative size");
    if (n_segs > GNNTRK_PACK_MAX_SEGS) {
        snprintf(msg, sizeof(msg), "pack_segments: %lld segments; at most %d", (long long)n_segs, GNNTRK_PACK_MAX_SEGS);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n_chunks > GNNTRK_PACK_MAX_CHUNKS) {
        snprintf(msg, sizeof(msg), "pack_segments: %lld chunks; at most %d", (long long)n_chunks, GNNTRK_PACK_MAX_CHUNKS);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n_segs == 0) return n_chunks == 0 ? GNNTRK_OK : fail(GNNTRK_EINVAL, "pack_segments: chunks without segments");
    if (!segs || !plan) return fail(GNNTRK_EINVAL, "pack_segments: NULL plan (host image or device image)");
    if (!dst && dst_bytes > 0) return fail(GNNTRK_EINVAL, "pack_segments: NULL dst");
    if (((uintptr_t)dst & 15) != 0) return fail(GNNTRK_EINVAL, "pack_segments: dst must be 16-byte aligned");
    // the host image: the descriptors, then the chunk table, which must list every chunk of every segment in order
    const PackChunk *chunks = reinterpret_cast<const PackChunk *>(segs + n_segs);
    int64_t c = 0;
    for (int64_t s = 0; s < n_segs; ++s) {
        const gnntrk_pack_seg &g = segs[s];
        const char *bad = nullptr;
        if (g.n_bytes < 0 || g.dst_off < 0) bad = "negative size or offset";
        else if (g.dst_off > dst_bytes - g.n_bytes) bad = "offset plus size beyond dst_bytes";
        else if (g.n_bytes > 0 && !g.src) bad = "NULL source";
        else if (g.mode != GNNTRK_PACK_RAW && g.mode != GNNTRK_PACK_SUB_I64 && g.mode != GNNTRK_PACK_SUB_I32) bad = "unknown mode";
        else if (g.mode != GNNTRK_PACK_RAW) {
            const int64_t el = g.mode == GNNTRK_PACK_SUB_I64 ? 8 : 4;
            if (g.n_bytes % el) bad = "size is not a multiple of the element size";
            else if (g.src % el || g.dst_off % el) bad = "source or destination misaligned for the element";
            else if (g.mode == GNNTRK_PACK_SUB_I32 && (g.sub < INT32_MIN || g.sub > INT32_MAX)) bad = "sub does not fit int32";
        }
        if (bad) {
            snprintf(msg, sizeof(msg), "pack_segments: segment %lld: %s", (long long)s, bad);
            return fail(GNNTRK_EINVAL, msg);
        }
        const int64_t nc = chunks_of(g.n_bytes);
        if (nc > n_chunks - c) return fail(GNNTRK_EINVAL, "pack_segments: sizes do not fit n_chunks");
        for (int64_t k = 0; k < nc; ++k, ++c)
            if (chunks[c].seg != s || chunks[c].k != k) {
                snprintf(msg, sizeof(msg), "pack_segments: chunk table entry %lld is not chunk %lld of segment %lld",
                         (long long)c, (long long)k, (long long)s);
                return fail(GNNTRK_EINVAL, msg);
            }
    }
    if (c != n_chunks) return fail(GNNTRK_EINVAL, "pack_segments: sizes do not fit n_chunks");
    if (n_chunks == 0) return GNNTRK_OK;
    const gnntrk_pack_seg *dsegs = reinterpret_cast<const gnntrk_pack_seg *>(plan);
    const int64_t cap = (int64_t)cu_count() * 8;
    launch(pack_segments_kernel, (int)(n_chunks < cap ? n_chunks : cap), kPackTpb, stream, dsegs, n_segs,
           reinterpret_cast<const PackChunk *>(dsegs + n_segs), n_chunks, reinterpret_cast<uint8_t *>(dst), dst_bytes);
    return check_launch("pack_segments");
}

}  // extern "C"
