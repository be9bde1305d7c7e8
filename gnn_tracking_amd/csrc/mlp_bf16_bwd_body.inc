// Body of the bf16 backward kernels (mlp_bf16_kernels.h includes it once per kernel).  Expects the template
// parameters KI, HT, GT, THREE, G32 of the enclosing kernel, constexpr int D, the type IO, constexpr bool BI, kBce
// and the kernel arguments a, part, trash, bp by value; `bce` (gnntrk_head_bce) is read where kBce is set.
    constexpr bool BUF = IO::NL > 0;
    static_assert(!kBce || (BUF && G32 && IO::kEpi == GNNTRK_EPI_SIGMOID && IO::NG == 1),
                  "BCE upstream gradient: the buffer-addressed one-column sigmoid head only");
    constexpr int NW = kWaves, NT = kBlock;   // waves / lanes of the workgroup
    static_assert(!BI || (!BUF && D == 1), "accumulator-initialised biases: generic one-tile form only");
    static_assert(!BUF || KI == 1, "buffer-addressed I/O: one k-step");
    using I = BwdImg<KI, HT, GT, THREE>;
    using F = FwdImg<KI, HT>;
    using S = BwdStage<KI, HT>;
    static_assert(OT == 1 || (!BUF && D == 1 && !G32 && !BI), "output tiles: generic one-tile form, bf16 gradients");
    constexpr int OTX = OT > 1 ? OT - 1 : 1;   // (array extents of the further output tiles)
    __shared__ __attribute__((aligned(16))) uint32_t s_img[I::kTotal + (OT - 1) * HT * 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[NW * D * S::kWave];
    // in-kernel target fold (gnntrk_gfold): the 0/1 segment matrix of a unit's rows, one 16 x 16 bf16 tile per half
    constexpr bool FOLD = BUF && IO::kFold && D == 2;
    static_assert(!IO::kFold || (BUF && D == 2), "the in-kernel fold: buffer-addressed shapes with two halves per unit");
    __shared__ __attribute__((aligned(16))) uint8_t s_fold[FOLD ? NW * 2 * 512 : 16];
    __shared__ SlotPlan s_plan;
    __shared__ gnntrk_seg s_seg[GNNTRK_MAX_SEGS];
    __shared__ gnntrk_gseg s_gseg[GNNTRK_MAX_SEGS];
    __shared__ __attribute__((aligned(16))) float s_btab[BI ? (HT + 1) * 16 : 4];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15, wv = (int)__builtin_amdgcn_readfirstlane(tid >> 6);
    stage_seg_args(s_seg, a.seg, tid);
#pragma unroll
    for (int j = 0; j < GNNTRK_MAX_SEGS; ++j)
        if (tid == 32 + j) s_gseg[j] = a.gseg[j];
    __syncthreads();
    if (tid == 0) make_slot_plan(s_plan, a.mlp, a.n_seg, s_seg, s_gseg);
    __syncthreads();
    {
        const AugWeights w = make_aug(a.mlp, s_plan);
#if !GNNTRK_PROBE_SKIP_PACK   // (timing probe: what the fragment packing costs - results are garbage without it)
        pack_forward_weights<KI, HT, THREE>(s_img, w, s_plan, s_seg, tid, NT);
        pack_backward_weights<KI, HT, GT, THREE>(s_img, w, s_plan, s_seg, tid, NT);
#endif
        if (BI) fill_bias_table<HT>(s_btab, w, tid, NT);
        for (int ot = 1; ot < OT; ++ot)   // W_last'^T of the output features 16 ot ..: [HT] x K16 fragments
            for (int t = 0; t < HT; ++t)
                pack_frag_k16(s_img + I::kTotal + ((ot - 1) * HT + t) * 128,
                              [&](int i, int g_, int e) { return w.wlast(16 * ot + 4 * g_ + e, 16 * t + i); }, tid, NT);
    }
    LaneChunks<KI> L;
    L.init(s_plan, s_seg, g);

    // gradient chunk handled by this lane in dX tile T: q = 4T + g.  Lanes without a chunk
    // (and rows past the end) store to a private 8-byte slot of the trash area instead, so
    // that the store is unconditional (see LaneChunks).
    constexpr int GTA = GT > 0 ? GT : 1;  // (array extents; GT = 0: no input gradient at all)
    gh_ptr gptr[GTA];
    gci_ptr gidx[GTA];  // optional row permutation of the gradient slice (never NULL, see LaneChunks)
    int32_t gstride[GTA], gin_off[GTA];
    uint32_t gkeep[GTA][2];
    uint32_t gmul_and[GTA], gmul_or[GTA];  // relu' multiplier (min(x, 1) & and) | or: branch-free "no ReLU" = 1
    bool gon[GTA], gidx_on[GTA];
    gh_ptr my_trash = (gh_ptr) reinterpret_cast<uint16_t *>(trash + ((int64_t)(blockIdx.x * NW + wv) * 64 + lane) * 8);
#pragma unroll
    for (int T = 0; T < GT; ++T) {
        const int q = 4 * T + g;
        gon[T] = q < s_plan.n_gchunks;
        gptr[T] = my_trash;
        gidx[T] = (gci_ptr) reinterpret_cast<const int32_t *>(a.gout[0].ptr);  // readable int32[n_rows]
        gidx_on[T] = false;
        gstride[T] = 0;
        gin_off[T] = 0;
        bool relu_in = false;
        int d = 0;
        if (gon[T]) {
            const int p = s_plan.gchunk[q], j = s_plan.seg[p];
            d = s_seg[j].dim - 4 * s_plan.first[p];
            d = d > 4 ? 4 : d;
            gptr[T] = (gh_ptr)(reinterpret_cast<uint16_t *>(s_gseg[j].ptr) + 4 * s_plan.first[p]);
            gstride[T] = s_gseg[j].stride;
            if (s_gseg[j].idx) {
                gidx[T] = (gci_ptr)s_gseg[j].idx;
                gidx_on[T] = true;
            }
            gin_off[T] = 8 * p;  // byte offset of the chunk inside a row of the input image
            relu_in = s_seg[j].relu != 0;
        }
        gmul_and[T] = relu_in ? 0xffffffffu : 0u;
        gmul_or[T] = relu_in ? 0u : 0x00010001u;
        gkeep[T][0] = (d >= 1 ? 0x0000ffffu : 0u) | (d >= 2 ? 0xffff0000u : 0u);
        gkeep[T][1] = (d >= 3 ? 0x0000ffffu : 0u) | (d >= 4 ? 0xffff0000u : 0u);
    }
    // buffer-addressed I/O: descriptors (SGPRs) and lane-constant offsets of every access
    constexpr int NLA = BUF ? IO::NL : 1, NIA = IO::NI > 0 ? IO::NI : 1, NSIA = IO::NSI > 0 ? IO::NSI : 1,
                  NSA = IO::NS > 0 ? IO::NS : 1, NGA = IO::NG > 0 ? IO::NG : 1;
    buf_rsrc_t r_ld[NLA], r_id[NIA], r_sid[NSIA], r_go[NGA], r_st[NSA];
    uint32_t v_ld[NLA], v_go[NGA], v_st[NSA];   // lane offsets (kBufOut: the lane takes no part)
    buf_rsrc_t r_fout;   // the in-kernel fold: node rows out, the units' carry rows behind them
    uint32_t v_fold = kBufOut;                       // byte offset of this lane's chunk inside a folded row
    bool b_ld[NLA];                             // the lane reads id stream sb of a two-stream load
    uint32_t ones_v = 0u, rmin_v[2] = {0x80008000u, 0x80008000u};
    const uint32_t v_c4 = 4u * (uint32_t)c;
    if constexpr (BUF) {
        auto lane_off = [&](const BufOpShape &sh, const BufOpArgs &ar, bool gathered) -> uint32_t {
            const bool on = (sh.part >> g) & 1;
            const uint32_t off = g == 0 ? ar.off8[0] : g == 1 ? ar.off8[1] : g == 2 ? ar.off8[2] : ar.off8[3];
            return on ? (gathered ? off : ((uint32_t)c << ar.shift) + off) : kBufOut;
        };
#pragma unroll
        for (int i = 0; i < IO::NL; ++i) {
            r_ld[i] = buf_make(bp.load[i].ptr, bp.load[i].bytes);
            v_ld[i] = lane_off(bp.load_s[i], bp.load[i], IO::load[i].gathered);
            b_ld[i] = (bp.load_s[i].use_b >> g) & 1;
        }
#pragma unroll
        for (int i = 0; i < IO::NI; ++i) r_id[i] = buf_make(bp.ids[i].ptr, bp.ids[i].bytes);
#pragma unroll
        for (int i = 0; i < IO::NSI; ++i) r_sid[i] = buf_make(bp.sids[i].ptr, bp.sids[i].bytes);
#pragma unroll
        for (int i = 0; i < IO::NG; ++i) {
            r_go[i] = buf_make(bp.gout[i].ptr, bp.gout[i].bytes);
            v_go[i] = lane_off(bp.gout_s[i], bp.gout[i], IO::gout[i].gathered);
        }
#pragma unroll
        for (int i = 0; i < IO::NS; ++i) {
            r_st[i] = buf_make(bp.store[i].ptr, bp.store[i].bytes);
            v_st[i] = lane_off(bp.store_s[i], bp.store[i], IO::store[i].gathered);
        }
        if constexpr (FOLD) {
            r_fout = buf_make(bp.fold_out.ptr, bp.fold_out.bytes);
            const bool on = (bp.fold_part >> g) & 1;
            const uint32_t o8 = g == 0 ? bp.fold_out.off8[0] : g == 1 ? bp.fold_out.off8[1] : g == 2 ? bp.fold_out.off8[2] : bp.fold_out.off8[3];
            v_fold = on ? o8 : kBufOut;
        }
        ones_v = g == bp.ones_group ? bp.ones_bits : 0u;
        rmin_v[0] = g == 0 ? bp.rmin[0][0] : g == 1 ? bp.rmin[1][0] : g == 2 ? bp.rmin[2][0] : bp.rmin[3][0];
        rmin_v[1] = g == 0 ? bp.rmin[0][1] : g == 1 ? bp.rmin[1][1] : g == 2 ? bp.rmin[2][1] : bp.rmin[3][1];
    }
    // fused BCE (gnntrk_mlp_backward_bf16_bce): the label bytes of the tile's rows ride in the upstream term's prefetch
    // slot - one dword per four rows, read by the lanes that own the output column; the term's own descriptor (the
    // stand-in the launcher points at w_out) takes the W stores
    buf_rsrc_t r_lab;
    uint32_t v_lab = kBufOut;
    float bce_gs = 0.f;
    if constexpr (kBce) {
        r_lab = buf_make(bce.label, (uint32_t)a.n_rows);
        v_lab = g == 0 ? ((uint32_t)c & ~3u) : kBufOut;
        bce_gs = 1.f / (float)bce.n_total;   // (as bce_csr_kernel forms it)
    }
    const bool any_relu = BUF && bp.any_relu != 0;
    const int gate_mode = BUF ? bp.gate_mode : 2;
    // W1 column of the input slot 16 ts + c (partials of dW1')
    int32_t col1[2 * KI];
#pragma unroll
    for (int ts = 0; ts < 2 * KI; ++ts) col1[ts] = slot_col(s_plan, s_seg, 16 * ts + c);
    const int hid_ones = s_plan.hid_ones;
    const uint32_t k_one = opaque_u32(0x00010001u);
    __syncthreads();
    // Weight fragments of the first layer (forward and W1'^T) and of W_last'^T held in registers for the whole
    // launch where the register file has room (the buffer-addressed two-tile shapes: 204 + 34 of 256): ten of
    // the 22 fragment reads per pair of tiles, and the LDS latency in front of the MFMAs that wait for them,
    // go away.  The middle layer's 48 registers of fragments do not fit and stay in LDS.
    constexpr bool kRegFrags = GNNTRK_BWD_REG_FRAGS && BUF && D == 2 && HT <= 3 && KI == 1 && !BI && OT == 1;
    u32x4 rA1[kRegFrags ? HT : 1];
    u32x2 rD3[kRegFrags ? HT : 1];
    u32x4 rD1[kRegFrags ? GTA : 1][(HT + 1) / 2];
    if constexpr (kRegFrags) {
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            rA1[t] = frag_k32(s_img + F::kA1 + t * 256, lane);
            rD3[t] = frag_k16(s_img + I::kD3 + t * 128, lane);
        }
#pragma unroll
        for (int T = 0; T < GT; ++T)
#pragma unroll
            for (int u = 0; u < (HT + 1) / 2; ++u) rD1[T][u] = frag_k32(s_img + I::kD1 + T * hid_k_dwords(HT) + 256 * u, lane);
    }

    const int out_dim = a.mlp.out_dim, hidden = a.mlp.hidden, in_dim = a.mlp.in_dim;
    const bool out_lane = 4 * g < out_dim;
    // (buffer-addressed shapes: the epilogue is part of the shape class - the tile loop then holds no arm it
    //  never takes; IO::kEpi < 0: read from the arguments)
    const int epi = IO::kEpi >= 0 ? IO::kEpi : a.epilogue;
    const bool need_y = epi == GNNTRK_EPI_RELU || epi == GNNTRK_EPI_SIGMOID;
    const bool want_dw = a.gW[0] != nullptr;
    uint32_t okeep[2];
    {
        const int d = out_dim - 4 * g;
        okeep[0] = (d >= 1 ? 0x0000ffffu : 0u) | (d >= 2 ? 0xffff0000u : 0u);
        okeep[1] = (d >= 3 ? 0x0000ffffu : 0u) | (d >= 4 ? 0xffff0000u : 0u);
    }
    // upstream-gradient terms, branch-free: a missing second term aliases the first (and is
    // discarded), missing row indices read the term's own rows as int32 (discarded), lanes
    // without output features read chunk 0 (masked by okeep)
    const bool two_terms = a.n_gout > 1;
    const int gq = out_lane ? g : 0;
    const void *gp0 = a.gout[0].ptr, *gp1 = two_terms ? a.gout[1].ptr : a.gout[0].ptr;
    const int32_t gs0 = a.gout[0].stride, gs1 = two_terms ? a.gout[1].stride : a.gout[0].stride;
    const bool gi0_on = a.gout[0].idx != nullptr, gi1_on = two_terms && a.gout[1].idx != nullptr;
    const gci_ptr go_idx0 = gi0_on ? (gci_ptr)a.gout[0].idx : (gci_ptr) reinterpret_cast<const int32_t *>(gp0);
    const gci_ptr go_idx1 = gi1_on ? (gci_ptr)a.gout[1].idx : go_idx0;
    int32_t gcol[4];  // fp32 term: column of register r (clamped)
#pragma unroll
    for (int r = 0; r < 4; ++r) gcol[r] = (4 * gq + r < out_dim) ? 4 * gq + r : out_dim - 1;

    uint8_t *stIn[D], *stX[D], *stG[D];  // one set of staging images per 16-row half
#pragma unroll
    for (int d = 0; d < D; ++d) {
        stIn[d] = s_stage + (wv * D + d) * S::kWave;
        stX[d] = stIn[d] + S::kIn;
        stG[d] = stX[d] + S::kX;
    }
    // byte offsets inside the staging images
    const int wr_tile = c * 32 + 8 * (g ^ ((c >> 2) & 3));                  // write [row c][4g..4g+3]
    const int rd_tile = (4 * g + (c >> 2)) * 32 + 8 * ((c & 3) ^ g);        // transpose read (row >> 2 = g)
    const int in_swz = 16 * ((c >> 3) & 1);                                 // unit swizzle of row c
    const int rd_row = 4 * g + (c >> 2);                                    // row this lane addresses in reads

    f32x4 dW1[HT][2 * KI], dW2[THREE ? HT : 1][HT], dW3[HT];
    f32x4 dW3x[OTX][OT > 1 ? HT : 1];   // last-layer weight gradients of the output features 16 ot .. (ot >= 1)
#pragma unroll
    for (int i = 0; i < OTX; ++i)
#pragma unroll
        for (int j = 0; j < (OT > 1 ? HT : 1); ++j) dW3x[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < HT; ++i) {
#pragma unroll
        for (int j = 0; j < 2 * KI; ++j) dW1[i][j] = zero;
        dW3[i] = zero;
    }
#pragma unroll
    for (int i = 0; i < (THREE ? HT : 1); ++i)
#pragma unroll
        for (int j = 0; j < HT; ++j) dW2[i][j] = zero;

    // accumulator-initialised biases: their gradients are sums over the rows of the gradient tiles - one
    // more MFMA per tile against a tile of ones (every column of the result holds the sum)
    f32x4 dbm[BI ? HT : 1], dbl = zero;
#pragma unroll
    for (int i = 0; i < (BI ? HT : 1); ++i) dbm[i] = zero;
    const u32x2 ones_k16 = {0x3f803f80u, 0x3f803f80u};

    const int64_t n_tiles = (a.n_rows + kTileRows - 1) / kTileRows;
    const TileSched sch = make_sched((n_tiles + D - 1) / D, NW);   // in units of D tiles
    const int32_t last_row = (int32_t)(a.n_rows - 1);
    auto clamp_row = [&](int64_t t) {
        const int64_t r = t * kTileRows + c;
        return (int32_t)(r < last_row ? r : last_row);
    };

    RowIds<KI> rid[D];
    int32_t grow[D][2];
    RawTile<KI> cur[D], nxt[D];
    RawGout gcur[D], gnxt[D];
    // buffer form: ids of the load streams (one unit ahead of the raw loads), raw results per access
    uint32_t idv[D][NIA];
    struct RawBuf {
        u32x4 w16[NLA];   // (an 8-byte access uses the first two dwords)
    };
    RawBuf bcur[D], bnxt[BUF ? 1 : D];
    // D = 1: one 16-row tile per iteration.  D = 2: a wave owns SUPER tiles of 32 consecutive rows
    // and walks the two 16-row halves stage by stage (two independent dependency chains in one
    // instruction stream: the LDS round trips and MFMA latencies of one half hide behind the
    // other), and the weight-gradient contractions run over all 32 rows with K = 32 MFMAs.
    auto tile_of = [&](int64_t grp, int d) { return (sch.cur + grp * sch.step) * D + d; };
    // first row of half d of unit grp as a scalar (buffer form: rows past the end fall out in the
    // range check of the descriptors, so nothing is clamped; units past the wave's last one read
    // rows of other waves, or nothing)
    // (32-bit scalar arithmetic: the launcher takes the buffer form only for tensors below 2^31 bytes,
    //  so even two units past the end the byte offsets stay below 2^32)
    const uint32_t u_cur = (uint32_t)sch.cur, u_step = (uint32_t)sch.step;
    auto row0_of = [&](int grp, int d) -> uint32_t {
        return ((u_cur + (uint32_t)grp * u_step) * (uint32_t)D + (uint32_t)d) * (uint32_t)kTileRows;
    };
    auto ids_of = [&](int grp, int d) {
        if constexpr (BUF) {
            const uint32_t r0 = row0_of(grp, d);
#pragma unroll
            for (int i = 0; i < IO::NI; ++i) idv[d][i] = buf_load_u32(r_id[i], v_c4, r0 << 2);
        } else {
            const int32_t row = clamp_row(tile_of(grp, d));
            load_row_ids<KI>(L, row, rid[d]);
            const int32_t i0 = go_idx0[row], i1 = go_idx1[row];
            grow[d][0] = gi0_on ? i0 : row;
            grow[d][1] = gi1_on ? i1 : row;
        }
    };
    // one access of the buffer form: lane offset + scalar offset from the shape
    auto buf_addr = [&](const BufOpShape &sh, const BufOpArgs &ar, uint32_t v_lane, bool use_b, const uint32_t *ids,
                        uint32_t r0, uint32_t &voff, uint32_t &soff) {
        if (sh.gathered) {
            uint32_t id = ids[sh.sa < 0 ? 0 : sh.sa];
            if (sh.sb >= 0) id = use_b ? ids[sh.sb] : id;
            voff = (id << ar.shift) + v_lane;
            soff = 0u;
        } else {
            voff = v_lane;
            soff = r0 << ar.shift;
        }
    };
    auto load_raw_buf = [&](int grp, int d, RawBuf &t) {
        const uint32_t r0 = row0_of(grp, d);
#pragma unroll
        for (int i = 0; i < IO::NL; ++i) {
            uint32_t voff, soff;
            buf_addr(IO::load[i], bp.load[i], v_ld[i], b_ld[i], idv[d], r0, voff, soff);
            if (IO::load[i].w16) {
                t.w16[i] = buf_load_u32x4(r_ld[i], voff, soff);
            } else {
                const u32x2 h = buf_load_u32x2(r_ld[i], voff, soff);
                t.w16[i][0] = h[0];
                t.w16[i][1] = h[1];
            }
        }
    };
    auto load_gout = [&](int grp, int d, RawGout &r) {
        if constexpr (BUF) {
            const uint32_t r0 = row0_of(grp, d);
            r.v = u32x4{0u, 0u, 0u, 0u};
            r.w = u32x2{0u, 0u};
#pragma unroll
            for (int t = 0; t < IO::NG; ++t) {
                uint32_t voff, soff;
                buf_addr(IO::gout[t], bp.gout[t], v_go[t], false, idv[d], r0, voff, soff);
                if constexpr (kBce) {   // the label dword of rows r0 + (c & ~3) .. + 3 (lane group 0; zero past the end)
                    r.v[0] = buf_load_u32(r_lab, v_lab, r0);
                } else if (G32) {   // fp32 upstream gradient of a one-column output (the edge-weight head)
                    r.v[0] = buf_load_u32(r_go[t], voff, soff);
                } else {
                    const u32x2 h = buf_load_u32x2(r_go[t], voff, soff);
                    if (t < 2) {
                        r.v[2 * (t & 1)] = h[0];
                        r.v[2 * (t & 1) + 1] = h[1];
                    } else {
                        r.w = h;
                    }
                }
            }
        } else if (G32) {
            const float GNNTRK_GLOBAL *p = (gcf_ptr) reinterpret_cast<const float *>(gp0) + (int64_t)grow[d][0] * gs0;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) r.v[r4] = __float_as_uint(p[gcol[r4]]);
        } else {
            const u32x2 t0 = *reinterpret_cast<const u32x2 GNNTRK_GLOBAL *>(
                (gch_ptr) reinterpret_cast<const uint16_t *>(gp0) + (int64_t)grow[d][0] * gs0 + 4 * gq);
            const u32x2 t1 = *reinterpret_cast<const u32x2 GNNTRK_GLOBAL *>(
                (gch_ptr) reinterpret_cast<const uint16_t *>(gp1) + (int64_t)grow[d][1] * gs1 + 4 * gq);
            r.v[0] = t0[0];
            r.v[1] = t0[1];
            r.v[2] = two_terms ? t1[0] : 0u;
            r.v[3] = two_terms ? t1[1] : 0u;
        }
    };
    auto load_unit = [&](int grp, int d, RawTile<KI> &t, RawBuf &tb, RawGout &go) {
        if constexpr (BUF)
            load_raw_buf(grp, d, tb);
        else
            load_raw<KI>(L, rid[d], t);
        load_gout(grp, d, go);
    };

    if (sch.cur < sch.end) {
#pragma unroll
        for (int d = 0; d < D; ++d) ids_of(0, d);
#pragma unroll
        for (int d = 0; d < D; ++d) load_unit(0, d, cur[d], bcur[d], gcur[d]);
#pragma unroll
        for (int d = 0; d < D; ++d) ids_of(1, d);
    }

    // transposed reads of the staging images as MFMA operands over the rows: one K = 16
    // operand per half; for D = 2 the halves are joined into one K = 32 operand (k-slot
    // (g, e): e < 4 -> row 4g + e of half 0, e >= 4 -> row 4g + e - 4 of half 1, the same on
    // both operands)
    // (GNNTRK_ABLATE: timing-only builds that leave parts of the tile loop out - wrong results, never shipped:
    //  1 weight-gradient MFMAs + their transposed reads, 2 the staging writes behind them, 4 the first-layer
    //  input-gradient stage, 8 its global stores only (32 / 64: the permuted / the tile's own rows), 16 the middle
    //  layer's dX contraction, 128 the I/O skeleton: loads and stores only)
    constexpr int ABL = GNNTRK_ABLATE | kSkel;   // (kSkel: the I/O-skeleton kernel, mlp_bf16_kernels.h)
    auto dw_acc = [&](const u32x2 (&at)[D], const u32x2 (&bt)[D], f32x4 &acc) {
        if constexpr (ABL & 1) return;
        if constexpr (D == 2)
            acc = mfma_bf16_k32(join(at[0], at[1]), join(bt[0], bt[1]), acc);
        else
            mfma_bf16_k16_acc(at[0], bt[0], acc);
    };

    // counted loop on a scalar trip count: a plain do-while for the compiler, so the
    // loop-carried weight-gradient accumulators are updated in place
    const int64_t span = sch.end - sch.cur, gstep = sch.step;
    const int n_grp = (int)__builtin_amdgcn_readfirstlane((uint32_t)(span > 0 ? (span + gstep - 1) / gstep : 0));
    // Only the LAST unit of the whole range can hold rows past the end (every wave's trip count is
    // exact).  The body is instantiated twice: without the validity masks for the bulk (their
    // selects are a tenth of the loop's VALU work) and with them for that one unit.
    constexpr bool kHot = GNNTRK_BWD_HOT != 0 && BUF && D == 2 && HT == 3 && KI == 1 && THREE && !BI && OT == 1 && !G32 &&
                          GT == 2 && IO::kEpi == GNNTRK_EPI_NONE && ABL == 0;
    // The ReLU-on-load / relu' pattern of the inputs (BufPlan::gate_mode, any_relu) is a launch constant: the
    // bulk loop is instantiated per pattern (gate_tag 0 none, 1 every segment, 2 mixed; -1 = read at run time: the
    // tail unit and the generic I/O), so the first-layer input-gradient stage - a quarter of the kernel by the
    // ablations of round 4 - is straight-line code the scheduler can interleave instead of four uniform branches.
    auto tile_step = [&](auto tail_tag, auto gate_tag, int grp) __attribute__((always_inline)) {
        constexpr bool kTail = decltype(tail_tag)::value;
        constexpr int kGate = decltype(gate_tag)::value;
        // generic form: the next unit's raw data into a second set of registers, rotated at the end of
        // the step.  Buffer form: issued below, as soon as S0 / S1 have consumed the current unit's
        // registers - straight into them (no rotation moves, a dozen registers less).
        if constexpr (!BUF) {
#pragma unroll
            for (int d = 0; d < D; ++d) load_unit(grp + 1, d, nxt[d], bnxt[d], gnxt[d]);
#pragma unroll
            for (int d = 0; d < D; ++d) ids_of(grp + 2, d);
        }

        // (kTail: rows past the end run as invalid rows: zero upstream gradient, stores redirected)
        bool valid[D];
        int32_t srow[D][GTA];  // destination rows of the input-gradient slices
        uint32_t sidv[D][NSIA];  // buffer form: ids of the store streams, this unit's rows
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int64_t tile = tile_of(grp, d);
            valid[d] = !kTail || (tile < n_tiles && tile * kTileRows + c < a.n_rows);
            if constexpr (BUF) {
                const uint32_t r0 = row0_of(grp, d);
#pragma unroll
                for (int i = 0; i < IO::NSI; ++i) sidv[d][i] = buf_load_u32(r_sid[i], v_c4, r0 << 2);
            } else {
                const int32_t rc = clamp_row(tile);
#pragma unroll
                for (int T = 0; T < GT; ++T) {
                    const int32_t v = gidx[T][rc];
                    srow[d][T] = gidx_on[T] ? v : rc;
                }
            }
        }

        // in-kernel target fold (gnntrk_gfold): the sorted ids of this unit's rows (lane c: row c of each half) and, as a
        // wave-uniform broadcast load, the id before the unit.  Issued late (the hot body: beside its seventh slot) -
        // held from the top of the body the registers spilled.
        uint32_t ftg[2] = {0u, 0u}, f_prev = 0u;
        auto fold_ids = [&]() __attribute__((always_inline)) {
            if constexpr (FOLD) {
                const uint32_t r0 = row0_of(grp, 0);
                // (the descriptor of the loads' own id stream: the sorted ids ARE the stream x[tgt] is gathered through)
                ftg[0] = buf_load_u32(r_id[IO::kFoldStream], v_c4, r0 << 2);
                ftg[1] = buf_load_u32(r_id[IO::kFoldStream], v_c4, (r0 + 16u) << 2);
                f_prev = buf_load_u32(r_id[IO::kFoldStream], 0u, (r0 ? r0 - 1u : 0u) << 2);
            }
        };
        if constexpr (FOLD && !(kHot && kGate >= 0 && !kTail)) fold_ids();
        // The fold of one unit, in pieces the hot body places in its slots (the generic body runs them in a row at its
        // end), after the hidden-layer gradient g1 of both halves sits in the staging images stG:
        //   fold_stage(base)   S[row][s] = 1 where id[row] == base + s (16 node ids per window), a 16 x 16 bf16 tile per half;
        //   fold_bs()          S read back transposed like the inputs of the dW1 contraction;
        //   R1[t] = g1_t . S   the dW1 form with S for the inputs: hidden x node sums over the unit's 32 rows (fp32);
        //   fold_store(...)    G = W1'^T . bf16(R1) (the dX1 form: the same fragments, columns = nodes instead of rows),
        //                      one 8-byte store per lane group and node; the run that began in an earlier unit goes to
        //                      the unit's carry row.  The relu' gate and the carries are gnntrk_fold_finish_bf16's.
        // One window unless the unit's ids span more than 16 (isolated nodes in between): fold_rest.
        uint8_t *const sS0 = s_fold + (FOLD ? (wv * 2) * 512 : 0), *const sS1 = sS0 + (FOLD ? 512 : 0);
        auto fold_bounds = [&](uint32_t &first, uint32_t &lastn, bool &cont) __attribute__((always_inline)) {
          if constexpr (FOLD) {
            const uint32_t r0 = row0_of(grp, 0);
            // first / last id of the unit's valid rows (sorted: lane 0 of half 0 / the last valid row's lane)
            const uint32_t nv = (uint32_t)a.n_rows - r0 < 32u ? (uint32_t)a.n_rows - r0 : 32u;
            first = __builtin_amdgcn_readlane(ftg[0], 0);
            lastn = nv > 16u ? __builtin_amdgcn_readlane(ftg[1], (int)(nv - 17u)) : __builtin_amdgcn_readlane(ftg[0], (int)(nv - 1u));
            cont = r0 != 0u && __builtin_amdgcn_readfirstlane(f_prev) == first;   // the unit's first run began in an earlier unit
          }
        };
        auto fold_stage = [&](uint32_t base) __attribute__((always_inline)) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const uint32_t col = ftg[d] - base - 4u * (uint32_t)g;   // this lane's four columns: 4g .. 4g + 3
                u32x2 sv;
                sv[0] = col == 0u ? 0x00003f80u : col == 1u ? 0x3f800000u : 0u;
                sv[1] = col == 2u ? 0x00003f80u : col == 3u ? 0x3f800000u : 0u;
                *reinterpret_cast<u32x2 *>((d ? sS1 : sS0) + c * 32 + 8 * g) = sv;
            }
        };
        auto fold_bs = [&]() __attribute__((always_inline)) -> u32x4 {
            const int rd_s = (4 * g + (c >> 2)) * 32 + 8 * (c & 3);
            return join(lds_read_tr16(reinterpret_cast<const uint16_t *>(sS0 + rd_s)),
                        lds_read_tr16(reinterpret_cast<const uint16_t *>(sS1 + rd_s)));
        };
        auto fold_store = [&](const u32x2 gi, uint32_t base, uint32_t lastn, bool carry0) __attribute__((always_inline)) {
          if constexpr (FOLD) {
            const uint32_t node = base + (uint32_t)c, unit = row0_of(grp, 0) >> 5;
            // ONE store: lane c = 0 of a unit whose first run began earlier goes to the unit's carry row instead
            const bool in = v_fold != kBufOut && node <= lastn;
            const uint32_t row = (carry0 && c == 0) ? bp.fold_nodes + unit : node;
            buf_store_u32x2(gi, r_fout, in ? (row << 4) + v_fold : kBufOut, 0u);
          }
        };
        auto fold_gs = [&](const u32x2 (&rp)[HT]) __attribute__((always_inline)) -> u32x2 {
            return pack_tile(contract_hidden<HT>(s_img + opaque_zero() + I::kD1, rp, lane, zero));
        };
        // windows first_w .. of the unit, each from scratch (own transposed reads of g1)
        auto fold_rest = [&](uint32_t w0, uint32_t first, uint32_t lastn, bool cont) __attribute__((always_inline)) {
          if constexpr (FOLD) {
            const uint32_t nwin = ((lastn - first) >> 4) + 1u;
            for (uint32_t w = w0; w < nwin; ++w) {
                const uint32_t base = first + 16u * w;
                fold_stage(base);
                lds_wave_order();
                const u32x4 bs = fold_bs();
                u32x2 rp[HT];
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    const u32x2 a0 = lds_read_tr16(reinterpret_cast<const uint16_t *>(stG[0] + t * 512 + rd_tile)),
                                a1 = lds_read_tr16(reinterpret_cast<const uint16_t *>(stG[1] + t * 512 + rd_tile));
                    rp[t] = pack_tile(mfma_bf16_k32(join(a0, a1), bs, zero));
                }
                lds_wave_order();   // (the next window / unit overwrites S)
                fold_store(fold_gs(rp), base, lastn, cont && w == 0u);
            }
          }
        };
        // `skel`: the I/O skeleton passes its XOR word instead of computing (loads and stores only)
        auto fold_unit = [&](const u32x2 *skel) __attribute__((always_inline)) {
            if constexpr (FOLD) {
                uint32_t first, lastn;
                bool cont;
                fold_bounds(first, lastn, cont);
                if (skel)
                    fold_store(u32x2{skel[0][0] ^ ftg[0], skel[0][1] ^ ftg[1]}, first, lastn, cont);
                else
                    fold_rest(0u, first, lastn, cont);
            }
        };
        // buffer form: the stores of gradient tile T of half d (one per gradient tensor; other lanes fall out)
        auto store_gi = [&](int T, int d, const u32x2 gi) {
            const uint32_t r0 = row0_of(grp, d);
#pragma unroll
            for (int i = 0; i < IO::NS; ++i)
                if (IO::store[i].slot == T) {
                    uint32_t voff, soff;
                    buf_addr(IO::store[i], bp.store[i], v_st[i], false, sidv[d], r0, voff, soff);
                    if (kTail && !valid[d]) voff = kBufOut;
                    if constexpr (ABL & 8) voff = kBufOut;
                    if constexpr ((ABL & 32) != 0) { if (IO::store[i].gathered) voff = kBufOut; }    // (the permuted rows only)
                    if constexpr ((ABL & 64) != 0) { if (!IO::store[i].gathered) voff = kBufOut; }   // (the tile's own rows only)
                    buf_store_u32x2(gi, r_st[i], voff, soff);
                }
        };
        // ---- HOT FORM: the relational shape (three hidden tiles, two halves, NONE epilogue), hand ordered ----------
        // The generic body below leaves the order of its ~430 instructions to the compiler's scheduler, which
        // clusters the MFMAs of a stage and the pack / ReLU / gate work behind them: the matrix pipe idles while
        // the vector pipe converts and vice versa (both 35-40 % busy, round 4).  Here the two halves A / B run as a
        // SOFTWARE PIPELINE one stage apart - while the MFMAs of a stage of one half occupy the matrix pipe, the
        // conversions of the previous stage of the other half issue in their shadow - and the weight-gradient
        // contractions (which depend on nothing but the staged tiles) fill the slots whose chain MFMAs are few.
        // sched_barrier(0) between the slots keeps the order; inside a slot the compiler interleaves.  Same
        // arithmetic, same operands, same accumulation order as the generic body: bit-identical results.
        if constexpr (kHot && kGate >= 0 && !kTail) {
#define GNNTRK_SB() __builtin_amdgcn_sched_barrier(0)
            const uint32_t *wimg = s_img + opaque_zero();
            const u32x2 z2 = {0u, 0u};
            auto merged = [&](int d) -> u32x4 {
                u32x4 m = IO::load[0].w16 ? bcur[d].w16[0] : u32x4{0u, 0u, 0u, 0u};
                if (!IO::load[0].w16) {
                    m[IO::load[0].slot] = bcur[d].w16[0][0];
                    m[IO::load[0].slot + 1] = bcur[d].w16[0][1];
                }
#pragma unroll
                for (int i = 1; i < IO::NL; ++i) {
                    if (IO::load[i].w16) {
#pragma unroll
                        for (int w = 0; w < 4; ++w) m[w] |= bcur[d].w16[i][w];
                    } else {
                        m[IO::load[i].slot] |= bcur[d].w16[i][0];
                        m[IO::load[i].slot + 1] |= bcur[d].w16[i][1];
                    }
                }
                if (IO::kOnesDword >= 0) m[IO::kOnesDword >= 0 ? IO::kOnesDword : 0] |= ones_v;
                if (kGate != 0) {
                    m[0] = i16x2_max(m[0], rmin_v[0]);
                    m[1] = i16x2_max(m[1], rmin_v[0]);
                    m[2] = i16x2_max(m[2], rmin_v[1]);
                    m[3] = i16x2_max(m[3], rmin_v[1]);
                }
                return m;
            };
            auto upstream = [&](int d) -> u32x2 {
                f32x4 gy;
                gy[0] = bf16_lo(gcur[d].v[0]) + bf16_lo(gcur[d].v[2]);
                gy[1] = bf16_hi(gcur[d].v[0]) + bf16_hi(gcur[d].v[2]);
                gy[2] = bf16_lo(gcur[d].v[1]) + bf16_lo(gcur[d].v[3]);
                gy[3] = bf16_hi(gcur[d].v[1]) + bf16_hi(gcur[d].v[3]);
                if constexpr (IO::NG > 2) {
                    gy[0] += bf16_lo(gcur[d].w[0]);
                    gy[1] += bf16_hi(gcur[d].w[0]);
                    gy[2] += bf16_lo(gcur[d].w[1]);
                    gy[3] += bf16_hi(gcur[d].w[1]);
                }
                return pack_tile(gy);
            };
            auto gated = [&](const f32x4 &acc, const u32x2 &p) -> u32x2 {
                u32x2 r = pack_tile(acc);
                r[0] = gate_bf16x2(r[0], p[0], k_one);
                r[1] = gate_bf16x2(r[1], p[1], k_one);
                return r;
            };
            auto stage_x = [&](int d, int t, const u32x2 &v) { *reinterpret_cast<u32x2 *>(stX[d] + t * 512 + wr_tile) = v; };
            auto stage_g = [&](int d, int t, const u32x2 &v) { *reinterpret_cast<u32x2 *>(stG[d] + t * 512 + wr_tile) = v; };
            auto tr_x = [&](int d, int t) { return lds_read_tr16(reinterpret_cast<const uint16_t *>(stX[d] + t * 512 + rd_tile)); };
            auto tr_g = [&](int d, int t) { return lds_read_tr16(reinterpret_cast<const uint16_t *>(stG[d] + t * 512 + rd_tile)); };

            // -- slot 0: the two B operands, the input image, the next unit's rows
            u32x4 mB[2];
            mB[0] = merged(0);
            mB[1] = merged(1);
#pragma unroll
            for (int d = 0; d < 2; ++d)
                *reinterpret_cast<u32x4 *>(stIn[d] + c * S::kInRow + ((16 * g) ^ in_swz)) = mB[d];
#pragma unroll
            for (int d = 0; d < 2; ++d) load_raw_buf(grp + 1, d, bcur[d]);
            u32x4 fr1[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) fr1[t] = frag_k32(wimg + F::kA1 + t * 256, lane);
            GNNTRK_SB();
            // -- slot 1: L1(A); then L1(B) beside pack(A)
            f32x4 aA[3], aB[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) aA[t] = mfma_bf16_k32(fr1[t], mB[0], zero);
            u32x4 fr2[3][2];   // the middle layer's fragments: read once, used by both halves
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) fr2[t][u] = frag_k32(wimg + F::kA2 + t * 512 + 256 * u, lane);
            u32x2 P1[2][3], P2[2][3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                aB[t] = mfma_bf16_k32(fr1[t], mB[1], zero);
                P1[0][t] = pack_tile_relu(aA[t]);
                GNNTRK_SB();
            }
            // -- slot 2: L2(A) beside pack(B)
            f32x4 cA[3], cB[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                cA[t] = mfma_bf16_k32(fr2[t][0], join(P1[0][0], P1[0][1]), zero);
                P1[1][t] = pack_tile_relu(aB[t]);
                GNNTRK_SB();
            }
            // (the upstream gradients need nothing from the chain: their conversions fill this slot)
            u32x2 g3[2];
            g3[0] = upstream(0);
#pragma unroll
            for (int t = 0; t < 3; ++t) cA[t] = mfma_bf16_k32(fr2[t][1], join(P1[0][2], z2), cA[t]);
            g3[1] = upstream(1);
            GNNTRK_SB();
#pragma unroll
            for (int d = 0; d < 2; ++d) load_gout(grp + 1, d, gcur[d]);
#pragma unroll
            for (int d = 0; d < 2; ++d) ids_of(grp + 2, d);
            // -- slot 3: L2(B) beside pack(A)
#pragma unroll
            for (int t = 0; t < 3; ++t) cB[t] = mfma_bf16_k32(fr2[t][0], join(P1[1][0], P1[1][1]), zero);
            u32x2 fd3[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) fd3[t] = frag_k16(wimg + I::kD3 + t * 128, lane);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                cB[t] = mfma_bf16_k32(fr2[t][1], join(P1[1][2], z2), cB[t]);
                P2[0][t] = pack_tile_relu(cA[t]);
                GNNTRK_SB();
            }
            // -- slot 4: dX3(A) beside pack(B); h2 of A and the upstream gradients go to the staging images
            f32x4 hA[3], hB[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                hA[t] = mfma_bf16_k16(fd3[t], g3[0], zero);
                P2[1][t] = pack_tile_relu(cB[t]);
                stage_x(0, t, P2[0][t]);
                GNNTRK_SB();
            }
            stage_g(0, 0, g3[0]);
            stage_g(1, 0, g3[1]);
            // -- slot 5: dX3(B) beside gate(A)
            u32x2 gh[2][3], g1[2][3];
            u32x4 fd2[3][2];
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) fd2[t][u] = frag_k32(wimg + I::kD2 + t * 512 + 256 * u, lane);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                hB[t] = mfma_bf16_k16(fd3[t], g3[1], zero);
                gh[0][t] = gated(hA[t], P2[0][t]);
                stage_x(1, t, P2[1][t]);
                GNNTRK_SB();
            }
            lds_wave_order();
            // -- slot 6: dX2(A) beside gate(B); dW3 (reads of the staged h2 / g_out, three MFMAs) fills in
            f32x4 eA[3], eB[3];
            u32x2 at3[2];
            at3[0] = tr_g(0, 0);
            at3[1] = tr_g(1, 0);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                eA[t] = mfma_bf16_k32(fd2[t][0], join(gh[0][0], gh[0][1]), zero);
                gh[1][t] = gated(hB[t], P2[1][t]);
                const u32x2 b0 = tr_x(0, t), b1 = tr_x(1, t);
                GNNTRK_SB();
                eA[t] = mfma_bf16_k32(fd2[t][1], join(gh[0][2], z2), eA[t]);
                dW3[t] = mfma_bf16_k32(join(at3[0], at3[1]), join(b0, b1), dW3[t]);
                GNNTRK_SB();
            }
            lds_wave_order();
            // -- slot 7: dX2(B) beside gate(A); h1 and g_h2 replace h2 / g_out in the staging images
            fold_ids();
#pragma unroll
            for (int t = 0; t < 3; ++t) eB[t] = mfma_bf16_k32(fd2[t][0], join(gh[1][0], gh[1][1]), zero);
            u32x4 fd1[2][2];
#pragma unroll
            for (int T = 0; T < 2; ++T)
#pragma unroll
                for (int u = 0; u < 2; ++u) fd1[T][u] = frag_k32(wimg + I::kD1 + T * 512 + 256 * u, lane);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                eB[t] = mfma_bf16_k32(fd2[t][1], join(gh[1][2], z2), eB[t]);
                g1[0][t] = gated(eA[t], P1[0][t]);
                stage_x(0, t, P1[0][t]);
                stage_x(1, t, P1[1][t]);
                stage_g(0, t, gh[0][t]);
                stage_g(1, t, gh[1][t]);
                GNNTRK_SB();
            }
            lds_wave_order();
            // -- slot 8: dX1(A) beside gate(B); dW2 (nine MFMAs over the staged h1 / g_h2) fills in
            f32x4 iA[2], iB[2];
            u32x2 bt2[3][2];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                bt2[t][0] = tr_x(0, t);
                bt2[t][1] = tr_x(1, t);
            }
#pragma unroll
            for (int T = 0; T < 2; ++T) iA[T] = mfma_bf16_k32(fd1[T][0], join(g1[0][0], g1[0][1]), zero);
#pragma unroll
            for (int to = 0; to < 3; ++to) {
                const u32x2 a0 = tr_g(0, to), a1 = tr_g(1, to);
                g1[1][to] = gated(eB[to], P1[1][to]);
                GNNTRK_SB();
#pragma unroll
                for (int t = 0; t < 3; ++t) dW2[to][t] = mfma_bf16_k32(join(a0, a1), join(bt2[t][0], bt2[t][1]), dW2[to][t]);
                GNNTRK_SB();
            }
#pragma unroll
            for (int T = 0; T < 2; ++T) iA[T] = mfma_bf16_k32(fd1[T][1], join(g1[0][2], z2), iA[T]);
            lds_wave_order();
            // -- slot 9: dX1(B) beside the input gradients of A; g_h1 replaces g_h2 in the staging images
            uint32_t f_first = 0u, f_last = 0u;
            bool f_cont = false;
            if constexpr (FOLD) {   // (the fold's segment matrix goes to its image beside this slot)
                fold_bounds(f_first, f_last, f_cont);
                fold_stage(f_first);
            }
#pragma unroll
            for (int T = 0; T < 2; ++T) iB[T] = mfma_bf16_k32(fd1[T][0], join(g1[1][0], g1[1][1]), zero);
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int t = 0; t < 3; ++t) stage_g(d, t, g1[d][t]);
            auto input_grad = [&](int T, int d, const f32x4 &acc) {
                u32x2 gi = pack_tile(acc);
                const u32x2 xin = *reinterpret_cast<const u32x2 *>(stIn[d] + c * S::kInRow + (gin_off[T] ^ in_swz));
                if (kGate == 1) {
                    gi[0] = gate_bf16x2(gi[0], xin[0], k_one);
                    gi[1] = gate_bf16x2(gi[1], xin[1], k_one);
                } else if (kGate == 2) {
                    gi[0] = u16x2_mul(gi[0], (i16x2_min(xin[0], k_one) & gmul_and[T]) | gmul_or[T]);
                    gi[1] = u16x2_mul(gi[1], (i16x2_min(xin[1], k_one) & gmul_and[T]) | gmul_or[T]);
                }
                store_gi(T, d, gi);
            };
#pragma unroll
            for (int T = 0; T < 2; ++T) {
                iB[T] = mfma_bf16_k32(fd1[T][1], join(g1[1][2], z2), iB[T]);
                input_grad(T, 0, iA[T]);
                GNNTRK_SB();
            }
            lds_wave_order();
            // -- slot 10: the input gradients of B; dW1 (six MFMAs over the staged inputs / g_h1)
            u32x2 bt1[2][2];
#pragma unroll
            for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                for (int d = 0; d < 2; ++d)
                    bt1[ts][d] = lds_read_tr16(reinterpret_cast<const uint16_t *>(
                        stIn[d] + rd_row * S::kInRow + ((32 * ts + 8 * (c & 3)) ^ (16 * (g >> 1)))));
            u32x4 f_bs = {0u, 0u, 0u, 0u};
            u32x2 f_rp[3];
            if constexpr (FOLD) f_bs = fold_bs();
#pragma unroll
            for (int to = 0; to < 3; ++to) {
                const u32x2 a0 = tr_g(0, to), a1 = tr_g(1, to);
                if (to < 2) input_grad(to, 1, iB[to]);
                GNNTRK_SB();
#pragma unroll
                for (int ts = 0; ts < 2; ++ts)
                    dW1[to][ts] = mfma_bf16_k32(join(a0, a1), join(bt1[ts][0], bt1[ts][1]), dW1[to][ts]);
                // (the fold's node sums of g1: the dW1 form with the segment matrix for the inputs - the same A operand)
                if constexpr (FOLD) f_rp[to] = pack_tile(mfma_bf16_k32(join(a0, a1), f_bs, zero));
                GNNTRK_SB();
            }
            if constexpr (FOLD) {
                fold_store(fold_gs(f_rp), f_first, f_last, f_cont);
                lds_wave_order();
                if (f_last - f_first >= 16u) fold_rest(1u, f_first, f_last, f_cont);   // (ids more than 16 apart: rare)
            }
            lds_wave_order();  // the next tile overwrites the images
#undef GNNTRK_SB
            return;
        }

        // ABL & 128: the I/O SKELETON of the launch - every load (id streams, gathered and tile rows, upstream
        // terms) and every store of the real kernel, one unit ahead as there, with nothing in between but the XOR
        // that keeps the loads alive: its time is what THIS access pattern costs at this occupancy whatever the
        // arithmetic does (bench.py: roofline.access_floor).
        if constexpr (BUF && (ABL & 128) != 0) {
            u32x2 sk[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                sk[d] = u32x2{gcur[d].v[0] ^ gcur[d].v[2] ^ gcur[d].w[0], gcur[d].v[1] ^ gcur[d].v[3] ^ gcur[d].w[1]};
#pragma unroll
                for (int i = 0; i < IO::NL; ++i) {
                    sk[d][0] ^= bcur[d].w16[i][0] ^ (IO::load[i].w16 ? bcur[d].w16[i][2] : 0u);
                    sk[d][1] ^= bcur[d].w16[i][1] ^ (IO::load[i].w16 ? bcur[d].w16[i][3] : 0u);
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d) load_raw_buf(grp + 1, d, bcur[d]);
#pragma unroll
            for (int d = 0; d < D; ++d) load_gout(grp + 1, d, gcur[d]);
#pragma unroll
            for (int d = 0; d < D; ++d) ids_of(grp + 2, d);
#pragma unroll
            for (int T = 0; T < GT; ++T)
#pragma unroll
                for (int d = 0; d < D; ++d) store_gi(T, d, sk[d]);
            fold_unit(sk);
            return;
        }

        // ---- S0: recompute ----------------------------------------------------------
        const uint32_t *wimg = s_img + opaque_zero();
        u32x2 P1[D][HT], P2[D][HT];
        {
            u32x4 B[D][KI];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if constexpr (BUF) {
                    // the accesses cover disjoint (lane group, dword) positions and return zero
                    // elsewhere: OR them together; pads are stored as zero; ones slot; optional ReLU
                    u32x4 m = IO::load[0].w16 ? bcur[d].w16[0] : u32x4{0u, 0u, 0u, 0u};
                    if (!IO::load[0].w16) {
                        m[IO::load[0].slot] = bcur[d].w16[0][0];
                        m[IO::load[0].slot + 1] = bcur[d].w16[0][1];
                    }
#pragma unroll
                    for (int i = 1; i < IO::NL; ++i) {
                        if (IO::load[i].w16) {
#pragma unroll
                            for (int w = 0; w < 4; ++w) m[w] |= bcur[d].w16[i][w];
                        } else {
                            m[IO::load[i].slot] |= bcur[d].w16[i][0];
                            m[IO::load[i].slot + 1] |= bcur[d].w16[i][1];
                        }
                    }
                    if (IO::kOnesDword >= 0) m[IO::kOnesDword >= 0 ? IO::kOnesDword : 0] |= ones_v;
                    if (kGate >= 0 ? kGate != 0 : any_relu) {
                        m[0] = i16x2_max(m[0], rmin_v[0]);
                        m[1] = i16x2_max(m[1], rmin_v[0]);
                        m[2] = i16x2_max(m[2], rmin_v[1]);
                        m[3] = i16x2_max(m[3], rmin_v[1]);
                    }
                    B[d][0] = m;
                } else {
                    finish_inputs<KI>(L, cur[d], B[d]);
                }
#pragma unroll
                for (int kk = 0; kk < KI; ++kk)
                    *reinterpret_cast<u32x4 *>(stIn[d] + c * S::kInRow + ((64 * kk + 16 * g) ^ in_swz)) = B[d][kk];
            }
            if constexpr (BUF) {   // (the raw input registers are free: the next unit's rows go straight into them)
#pragma unroll
                for (int d = 0; d < D; ++d) load_raw_buf(grp + 1, d, bcur[d]);
            }
            if constexpr (kRegFrags) {
#pragma unroll
                for (int t = 0; t < HT; ++t) {
#pragma unroll
                    for (int d = 0; d < D; ++d) P1[d][t] = pack_tile_relu(mfma_bf16_k32(rA1[t], B[d][0], zero));
                }
                if (THREE) {
#pragma unroll
                    for (int t = 0; t < HT; ++t) {
                        f32x4 acc2[D];
#pragma unroll
                        for (int d = 0; d < D; ++d) acc2[d] = zero;
                        contract_hidden_d<HT, D>(wimg + F::kA2 + t * hid_k_dwords(HT), P1, lane, acc2);
#pragma unroll
                        for (int d = 0; d < D; ++d) P2[d][t] = pack_tile_relu(acc2[d]);
                    }
                }
            } else {
                hidden_chain_d<KI, HT, THREE, D, BI>(wimg, B, lane, P1, P2, s_btab);
            }
        }
        const u32x2(&PLs)[D][HT] = THREE ? P2 : P1;  // input of the last layer
        auto PL = [&](int d) -> const u32x2(&)[HT] { return PLs[d]; };

        // ---- S1: upstream gradient --------------------------------------------------
        u32x2 g3[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            f32x4 gy;
            if (G32) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gy[r] = __uint_as_float(gcur[d].v[r]);
            } else {
                gy[0] = bf16_lo(gcur[d].v[0]) + bf16_lo(gcur[d].v[2]);
                gy[1] = bf16_hi(gcur[d].v[0]) + bf16_hi(gcur[d].v[2]);
                gy[2] = bf16_lo(gcur[d].v[1]) + bf16_lo(gcur[d].v[3]);
                gy[3] = bf16_hi(gcur[d].v[1]) + bf16_hi(gcur[d].v[3]);
                if constexpr (IO::NG > 2) {
                    gy[0] += bf16_lo(gcur[d].w[0]);
                    gy[1] += bf16_hi(gcur[d].w[0]);
                    gy[2] += bf16_lo(gcur[d].w[1]);
                    gy[3] += bf16_hi(gcur[d].w[1]);
                }
            }
            if constexpr (BUF) {   // (lanes without output features loaded zeros)
                if (G32) gy[1] = gy[2] = gy[3] = 0.f;
                if (kTail && !valid[d]) gy = zero;
            } else {
                if (!(out_lane && valid[d])) gy = zero;
            }
            if (need_y) {
                const f32x4 y = contract_hidden<HT>(wimg + F::kA3, PL(d), lane,
                                                    BI ? bias_frag(s_btab + 16 * HT, lane) : zero);
                if constexpr (kBce) {
                    // the head's own output and the BCE gradient of it, in the order of the launches this replaces:
                    // W as mlp16_fwd_kernel stores it, the unit gradient as bce_csr_one, the loss's upstream scalar
                    // as the elementwise product behind it - then the sigmoid's derivative as below
                    const float sg = sigmoidf_(y[0]);
                    const float wq = a.ca + a.cb * sg;
                    uint32_t lab = (gcur[d].v[0] >> (8 * (c & 3))) & 0xffu;
                    if constexpr (kTail) {   // (the last label dword may be cut off by the range check: read the bytes)
                        const int64_t row = (int64_t)row0_of(grp, d) + c;
                        lab = bce.label[row < a.n_rows ? row : a.n_rows - 1];
                    }
                    const float tq = lab ? 1.f : 0.f;
                    float gq = bce_gs * (wq - tq) / fmaxf((1.f - wq) * wq, 1e-12f);
                    gq = gq * bce.gscale;
                    gq = gq * a.cb * sg * (1.f - sg);
                    const bool on = g == 0 && !(kTail && !valid[d]);
                    gy = zero;
                    gy[0] = on ? gq : 0.f;
                    buf_store_u32(__float_as_uint(wq), r_go[0], on ? v_go[0] : kBufOut, row0_of(grp, d) << 2);
                } else if (BUF && G32) {
                    // (buffer form of the fp32-gradient launch = the one-column edge-weight head: the
                    //  sigmoid's derivative for the one feature there is, not for four registers)
                    const float sg = sigmoidf_(y[0]);
                    gy[0] = gy[0] * a.cb * sg * (1.f - sg);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (epi == GNNTRK_EPI_RELU) {
                            gy[r] = y[r] > 0.f ? gy[r] : 0.f;
                        } else {
                            const float sg = sigmoidf_(y[r]);
                            gy[r] = gy[r] * a.cb * sg * (1.f - sg);
                        }
                    }
                }
            } else if (epi == GNNTRK_EPI_RESIDUAL) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gy[r] *= a.cb;
            }
            g3[d] = pack_tile(gy);
            if constexpr (!BUF) {   // (buffer form: lanes / features without data loaded zeros)
                g3[d][0] &= okeep[0];
                g3[d][1] &= okeep[1];
            }
        }

        u32x2 g3x[OTX];   // (D = 1) packed upstream gradient of the output features 16 ot + 4 g .. + 3, ot >= 1
        if constexpr (OT > 1) {
            // loaded here, not a unit ahead: a wide output is not the hot shape.  Epilogues NONE / RESIDUAL only
            // (the launcher refuses the others: no recomputed output for these tiles)
            // (grow[] already holds the rows of the unit after next: the rows of THIS unit once more)
            const int32_t rowc = clamp_row(tile_of(grp, 0));
            const int32_t i0x = go_idx0[rowc], i1x = go_idx1[rowc];
            const int32_t r0x = gi0_on ? i0x : rowc, r1x = gi1_on ? i1x : rowc;
#pragma unroll
            for (int ot = 1; ot < OT; ++ot) {
                const int f0 = 16 * ot + 4 * g, dleft = out_dim - f0;
                const bool on = dleft > 0 && valid[0];
                const int fo = on ? f0 : 0;
                const u32x2 t0 = *reinterpret_cast<const u32x2 GNNTRK_GLOBAL *>(
                    (gch_ptr) reinterpret_cast<const uint16_t *>(gp0) + (int64_t)r0x * gs0 + fo);
                const u32x2 t1 = *reinterpret_cast<const u32x2 GNNTRK_GLOBAL *>(
                    (gch_ptr) reinterpret_cast<const uint16_t *>(gp1) + (int64_t)r1x * gs1 + fo);
                f32x4 gy;
                gy[0] = bf16_lo(t0[0]) + (two_terms ? bf16_lo(t1[0]) : 0.f);
                gy[1] = bf16_hi(t0[0]) + (two_terms ? bf16_hi(t1[0]) : 0.f);
                gy[2] = bf16_lo(t0[1]) + (two_terms ? bf16_lo(t1[1]) : 0.f);
                gy[3] = bf16_hi(t0[1]) + (two_terms ? bf16_hi(t1[1]) : 0.f);
                if (!on) gy = zero;
                if (epi == GNNTRK_EPI_RESIDUAL) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) gy[r] *= a.cb;
                }
                u32x2 gp = pack_tile(gy);
                gp[0] &= (dleft >= 1 ? 0x0000ffffu : 0u) | (dleft >= 2 ? 0xffff0000u : 0u);
                gp[1] &= (dleft >= 3 ? 0x0000ffffu : 0u) | (dleft >= 4 ? 0xffff0000u : 0u);
                g3x[ot - 1] = gp;
            }
        }

        if constexpr (BUF) {   // (the upstream-gradient registers are free: next unit's terms, then the ids after it)
#pragma unroll
            for (int d = 0; d < D; ++d) load_gout(grp + 1, d, gcur[d]);
#pragma unroll
            for (int d = 0; d < D; ++d) ids_of(grp + 2, d);
        }

        // ---- S2 / S3 interleaved: every dW stage reuses the staging images --------------
        // last layer: gradient at its input (hidden, after relu')
        u32x2 gh[D][HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const u32x2 fr = kRegFrags ? rD3[kRegFrags ? t : 0] : frag_k16(wimg + I::kD3 + t * 128, lane);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                f32x4 acc = mfma_bf16_k16(fr, g3[d], zero);
                if constexpr (OT > 1) {
#pragma unroll
                    for (int ot = 1; ot < OT; ++ot)
                        mfma_bf16_k16_acc(frag_k16(wimg + I::kTotal + ((ot - 1) * HT + t) * 128, lane), g3x[ot - 1], acc);
                }
                gh[d][t] = pack_tile(acc);
                gh[d][t][0] = gate_bf16x2(gh[d][t][0], PL(d)[t][0], k_one);
                gh[d][t][1] = gate_bf16x2(gh[d][t][1], PL(d)[t][1], k_one);
            }
        }
        {   // weight gradients are always accumulated (a branch here would turn the
            // loop-carried accumulators into phi copies); only the final write is optional
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if constexpr (!(ABL & 2)) {
#pragma unroll
                    for (int t = 0; t < HT; ++t) *reinterpret_cast<u32x2 *>(stX[d] + t * 512 + wr_tile) = PL(d)[t];
                    *reinterpret_cast<u32x2 *>(stG[d] + wr_tile) = g3[d];
                }
            }
            if constexpr (OT > 1) {   // (the gradient image holds HT >= OT tiles)
#pragma unroll
                for (int ot = 1; ot < OT; ++ot) *reinterpret_cast<u32x2 *>(stG[0] + ot * 512 + wr_tile) = g3x[ot - 1];
            }
            lds_wave_order();
            u32x2 at[D];
#pragma unroll
            for (int d = 0; d < D; ++d) at[d] = lds_read_tr16(reinterpret_cast<const uint16_t *>(stG[d] + rd_tile));
            u32x2 atx[OTX];
            if constexpr (OT > 1) {
#pragma unroll
                for (int ot = 1; ot < OT; ++ot)
                    atx[ot - 1] = lds_read_tr16(reinterpret_cast<const uint16_t *>(stG[0] + ot * 512 + rd_tile));
            }
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                u32x2 bt[D];
#pragma unroll
                for (int d = 0; d < D; ++d)
                    bt[d] = lds_read_tr16(reinterpret_cast<const uint16_t *>(stX[d] + t * 512 + rd_tile));
                dw_acc(at, bt, dW3[t]);
                if constexpr (OT > 1) {
#pragma unroll
                    for (int ot = 1; ot < OT; ++ot) mfma_bf16_k16_acc(atx[ot - 1], bt[0], dW3x[ot - 1][t]);
                }
            }
            if constexpr (BI) mfma_bf16_k16_acc(at[0], ones_k16, dbl);
        }
        // middle layer
        u32x2 g1[D][HT];
        if (THREE) {
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                f32x4 acc[D];
#pragma unroll
                for (int d = 0; d < D; ++d) acc[d] = zero;
                if constexpr (!(ABL & 16)) contract_hidden_d<HT, D>(wimg + I::kD2 + t * hid_k_dwords(HT), gh, lane, acc);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    g1[d][t] = (ABL & 16) ? gh[d][t] : pack_tile(acc[d]);
                    g1[d][t][0] = gate_bf16x2(g1[d][t][0], P1[d][t][0], k_one);
                    g1[d][t][1] = gate_bf16x2(g1[d][t][1], P1[d][t][1], k_one);
                }
            }
            lds_wave_order();
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    if constexpr (ABL & 2) continue;
                    *reinterpret_cast<u32x2 *>(stX[d] + t * 512 + wr_tile) = P1[d][t];
                    *reinterpret_cast<u32x2 *>(stG[d] + t * 512 + wr_tile) = gh[d][t];
                }
            lds_wave_order();
            u32x2 bt[HT][D];
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int d = 0; d < D; ++d)
                    bt[t][d] = lds_read_tr16(reinterpret_cast<const uint16_t *>(stX[d] + t * 512 + rd_tile));
#pragma unroll
            for (int to = 0; to < HT; ++to) {
                u32x2 at[D];
#pragma unroll
                for (int d = 0; d < D; ++d)
                    at[d] = lds_read_tr16(reinterpret_cast<const uint16_t *>(stG[d] + to * 512 + rd_tile));
#pragma unroll
                for (int t = 0; t < HT; ++t) dw_acc(at, bt[t], dW2[to][t]);
                if constexpr (BI) mfma_bf16_k16_acc(at[0], ones_k16, dbm[to]);
            }
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int t = 0; t < HT; ++t) g1[d][t] = gh[d][t];
        }
        // first layer: stage g1, input gradients, dW1
        lds_wave_order();
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                if constexpr (ABL & 2) continue;
                *reinterpret_cast<u32x2 *>(stG[d] + t * 512 + wr_tile) = g1[d][t];
            }
        lds_wave_order();
#pragma unroll
        for (int T = 0; T < ((ABL & 4) ? 0 : GT); ++T) {
            f32x4 accs[D];
#pragma unroll
            for (int d = 0; d < D; ++d) accs[d] = zero;
            if constexpr (kRegFrags) {
#pragma unroll
                for (int u = 0; u < HT / 2; ++u)
#pragma unroll
                    for (int d = 0; d < D; ++d) accs[d] = mfma_bf16_k32(rD1[T][u], join(g1[d][2 * u], g1[d][2 * u + 1]), accs[d]);
                if (HT % 2) {
                    const u32x2 z2 = {0u, 0u};
#pragma unroll
                    for (int d = 0; d < D; ++d) accs[d] = mfma_bf16_k32(rD1[T][HT / 2], join(g1[d][HT - 1], z2), accs[d]);
                }
            } else {
                contract_hidden_d<HT, D>(wimg + I::kD1 + T * hid_k_dwords(HT), g1, lane, accs);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                u32x2 gi = pack_tile(accs[d]);
                const u32x2 xin = *reinterpret_cast<const u32x2 *>(stIn[d] + c * S::kInRow + (gin_off[T] ^ in_swz));
                if constexpr (BUF) {
                    // relu' of the inputs: none / all of the segments (a uniform branch) or mixed; the pad
                    // slots of a gradient row come out as +0 by themselves (zero columns of W1'^T)
                    const int gm = kGate >= 0 ? kGate : gate_mode;
                    if (gm == 1) {
                        gi[0] = gate_bf16x2(gi[0], xin[0], k_one);
                        gi[1] = gate_bf16x2(gi[1], xin[1], k_one);
                    } else if (gm == 2) {
                        gi[0] = u16x2_mul(gi[0], (i16x2_min(xin[0], k_one) & gmul_and[T]) | gmul_or[T]);
                        gi[1] = u16x2_mul(gi[1], (i16x2_min(xin[1], k_one) & gmul_and[T]) | gmul_or[T]);
                    }
                } else {
                    gi[0] = u16x2_mul(gi[0], (i16x2_min(xin[0], k_one) & gmul_and[T]) | gmul_or[T]);
                    gi[1] = u16x2_mul(gi[1], (i16x2_min(xin[1], k_one) & gmul_and[T]) | gmul_or[T]);
                    gi[0] &= gkeep[T][0];
                    gi[1] &= gkeep[T][1];
                }
                if constexpr (BUF) {   // one store per gradient tensor of this tile; other lanes fall out
                    store_gi(T, d, gi);
                } else {
                    // (lanes without a chunk already point at their trash slot with stride 0)
                    const gh_ptr dst = gptr[T] + (int64_t)srow[d][T] * gstride[T];
                    *reinterpret_cast<u32x2 GNNTRK_GLOBAL *>(valid[d] ? dst : my_trash) = gi;
                }
            }
        }
        {
            u32x2 bt[2 * KI][D];
#pragma unroll
            for (int ts = 0; ts < 2 * KI; ++ts)
#pragma unroll
                for (int d = 0; d < D; ++d)
                    bt[ts][d] = lds_read_tr16(reinterpret_cast<const uint16_t *>(
                        stIn[d] + rd_row * S::kInRow + ((32 * ts + 8 * (c & 3)) ^ (16 * (g >> 1)))));
#pragma unroll
            for (int to = 0; to < HT; ++to) {
                u32x2 at[D];
#pragma unroll
                for (int d = 0; d < D; ++d)
                    at[d] = lds_read_tr16(reinterpret_cast<const uint16_t *>(stG[d] + to * 512 + rd_tile));
#pragma unroll
                for (int ts = 0; ts < 2 * KI; ++ts) dw_acc(at, bt[ts], dW1[to][ts]);
            }
        }
        if constexpr (FOLD) {
            lds_wave_order();
            fold_unit(nullptr);
        }
        lds_wave_order();  // the next tile overwrites the images
#if GNNTRK_BWD_SGB
        // experimental: ask the scheduler for an interleaved issue order over the whole (single-block) tile body -
        // per MFMA a few VALU instructions of the other half and a share of the DS / VMEM traffic
        if constexpr (BUF && kGate >= 0 && !kTail && D == 2 && HT == 3 && THREE) {
#pragma unroll
            for (int i = 0; i < GNNTRK_BWD_SGB_N; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                    // MFMA
                __builtin_amdgcn_sched_group_barrier(0x002, GNNTRK_BWD_SGB_V, 0);     // VALU
                __builtin_amdgcn_sched_group_barrier(0x100, GNNTRK_BWD_SGB_R, 0);     // DS read
                if (i % GNNTRK_BWD_SGB_WP == 0) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
                if (i % 3 == 0) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                    // VMEM
            }
        }
#endif
        if constexpr (!BUF) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                cur[d] = nxt[d];
                gcur[d] = gnxt[d];
            }
        }
    };
    const int64_t n_units = (n_tiles + D - 1) / D;
    const bool last_is_partial = n_units * D * kTileRows != a.n_rows;
    const int has_tail = (int)__builtin_amdgcn_readfirstlane(
        (uint32_t)((n_grp > 0 && last_is_partial && sch.cur + (int64_t)(n_grp - 1) * sch.step == n_units - 1) ? 1 : 0));
    const int n_main = n_grp - has_tail;
    if constexpr (BUF && GT > 0 && GNNTRK_BWD_STATIC_GATE) {
        if (gate_mode == 0 && !any_relu) {
            for (int grp = 0; grp < n_main; ++grp) tile_step(std::false_type{}, std::integral_constant<int, 0>{}, grp);
        } else if (gate_mode == 1 && any_relu) {
            for (int grp = 0; grp < n_main; ++grp) tile_step(std::false_type{}, std::integral_constant<int, 1>{}, grp);
        } else if (gate_mode == 2 && any_relu) {
            for (int grp = 0; grp < n_main; ++grp) tile_step(std::false_type{}, std::integral_constant<int, 2>{}, grp);
        } else {
            for (int grp = 0; grp < n_main; ++grp) tile_step(std::false_type{}, std::integral_constant<int, -1>{}, grp);
        }
    } else {
        for (int grp = 0; grp < n_main; ++grp) tile_step(std::false_type{}, std::integral_constant<int, -1>{}, grp);
    }
    if (has_tail) tile_step(std::true_type{}, std::integral_constant<int, -1>{}, n_main);

    // ---- partial block (parameter layout: W1, b1, [W2, b2,] W3, b3) ------------------------
    // The four waves of the workgroup are summed in wave order through LDS (the weight-fragment
    // image is free by now) and ONE block per workgroup goes to the workspace; shapes whose
    // parameter count exceeds the image fall back to one block per wave.
    if (!want_dw) return;
    drain_mfma();
    const int PT = part_total(a.mlp);
    // (five and more hidden tiles: one block per WAVE.  The in-LDS reduction is only instantiated up to four hidden
    //  tiles: for the <1, 7, 0, true> and <1, 8, 0, true> instantiations - 105-120 KB of LDS, 400-500 registers - it
    //  ended in memory-access faults on the MI355X in round 3, at random, while passing the emulator; it was never
    //  reproduced afterwards, and the switch that re-enabled it for diagnostics went in round 5 with the code path:
    //  what ships for the wide shapes is the per-wave form that every stress run has been clean on.
    //  debug_flags & 2048: per-wave blocks everywhere - diagnostics)
    const bool via_lds = PT <= I::kTotal && HT <= 4 && !(a.debug_flags & 2048);
    // (the destination is the workspace in global memory or the LDS image: an address-space-typed pointer in
    //  both cases - through a generic pointer the LDS form became FLAT stores, and those faulted on the MI355X
    //  in the instantiations whose LDS image lies above 64 KB: "write access to a read-only page")
    auto emit = [&](auto pw, bool add) {
        using FP = decltype(pw);
        auto put = [&](FP dst, float v) { *dst = add ? *dst + v : v; };
        int off = 0;
        FP pW1 = pw + off;
        off += hidden * in_dim;
        FP pb1 = pw + off;
        off += hidden;
        FP pW2 = pw + off, pb2 = nullptr;
        if (THREE) {
            off += hidden * hidden;
            pb2 = pw + off;
            off += hidden;
        }
        FP pW3 = pw + off;
        off += out_dim * hidden;
        FP pb3 = pw + off;
#pragma unroll
        for (int to = 0; to < HT; ++to)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * to + 4 * g + r;
                if (o >= hidden) continue;
#pragma unroll
                for (int ts = 0; ts < 2 * KI; ++ts) {
                    if (col1[ts] >= 0)
                        put(pW1 + o * in_dim + col1[ts], dW1[to][ts][r]);
                    else if (col1[ts] == -2)
                        put(pb1 + o, dW1[to][ts][r]);
                }
                if (THREE) {
#pragma unroll
                    for (int t = 0; t < HT; ++t) {
                        const int f = 16 * t + c;
                        if (f < hidden)
                            put(pW2 + o * hidden + f, dW2[THREE ? to : 0][t][r]);
                        else if (f == hid_ones)
                            put(pb2 + o, dW2[THREE ? to : 0][t][r]);
                    }
                }
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = 4 * g + r;
            if (o >= out_dim) continue;
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                const int f = 16 * t + c;
                if (f < hidden)
                    put(pW3 + o * hidden + f, dW3[t][r]);
                else if (f == hid_ones)
                    put(pb3 + o, dW3[t][r]);
            }
        }
        if constexpr (OT > 1) {   // last-layer gradients of the output features 16 ot ..
#pragma unroll
            for (int ot = 1; ot < OT; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = 16 * ot + 4 * g + r;
                    if (o >= out_dim) continue;
#pragma unroll
                    for (int t = 0; t < HT; ++t) {
                        const int f = 16 * t + c;
                        if (f < hidden)
                            put(pW3 + o * hidden + f, dW3x[ot - 1][t][r]);
                        else if (f == hid_ones)
                            put(pb3 + o, dW3x[ot - 1][t][r]);
                    }
                }
        }
        if constexpr (BI) {   // accumulator-initialised biases: column 0 of the ones-operand products
            if (c == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (THREE) {
#pragma unroll
                        for (int to = 0; to < HT; ++to)
                            if (16 * to + 4 * g + r < hidden) put(pb2 + 16 * to + 4 * g + r, dbm[to][r]);
                    }
                    if (4 * g + r < out_dim) put(pb3 + 4 * g + r, dbl[r]);
                }
            }
        }
        if (!add) {  // bias slots without a ones column must still be defined
            if (s_plan.ones_slot < 0)
                for (int o = lane; o < hidden; o += 64) pb1[o] = 0.f;
            if (hid_ones < 0 && !BI) {
                if (THREE)
                    for (int o = lane; o < hidden; o += 64) pb2[o] = 0.f;
                for (int o = lane; o < out_dim; o += 64) pb3[o] = 0.f;
            }
        }
    };
    if (via_lds) {
        GNNTRK_LDS float *buf = (GNNTRK_LDS float *)s_img;
        gf_ptr dst = (gf_ptr)(part + (int64_t)blockIdx.x * PT);
        __syncthreads();  // every wave is done with the fragments and the staging images
        if ((size_t)(NW - 1) * PT * sizeof(float) <= sizeof(s_stage)) {
            // all waves write their blocks AT ONCE, wave 0 over the fragment image, the others into the staging
            // images, and the workgroup adds them in wave order: the same sums as the serial form below (wave
            // after wave into one block: 4 x 6 us of a 16-row launch's 33, round 5), bit for bit
            GNNTRK_LDS float *rest = (GNNTRK_LDS float *)s_stage;
            emit(wv == 0 ? buf : rest + (size_t)(wv - 1) * PT, false);
            __syncthreads();
            for (int i = tid; i < PT; i += NT) {
                float v = buf[i];
                for (int w = 1; w < NW; ++w) v += rest[(size_t)(w - 1) * PT + i];
                dst[i] = v;
            }
        } else {
            for (int i = tid; i < PT; i += NT) buf[i] = 0.f;
            __syncthreads();
            for (int w = 0; w < NW; ++w) {
                if (wv == w) emit(buf, true);
                __syncthreads();
            }
            for (int i = tid; i < PT; i += NT) dst[i] = buf[i];
        }
    } else {
        emit((gf_ptr)(part + (int64_t)(blockIdx.x * NW + wv) * PT), false);
    }
