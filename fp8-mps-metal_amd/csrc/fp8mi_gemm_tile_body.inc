// THE body of one ring tile (or one K slice of it), from the tile map to the fused epilogue: the one source text of every ring-tile kernel.
// fp8mi_gemm.hip expands it at two sites - inside gemm_tile<C, S, Map> (e5m2, MXFP8, MXFP4, MXW4A8, blockwise, grouped) and directly inside
// gemm_kernel (tensorwise e4m3) - because the tensorwise kernels' machine code changes with one more inlined function frame around the
// same text, and does not change with the text itself (DESIGN.md 5.17).  Not a header: no guard, no declarations.
//
// The expansion site provides
//     C                      the Cfg; every `if constexpr (C::...)` below folds at compile time (MXS = 0, FMT = 0 leaves the tensorwise body)
//     BM, BN, WM, WN         the tile's and a wave's extents (compile-time constants)
//     p (MMParams), mx       the problem and the scale carrier (MxArgs, BwScales or an empty type; its type must depend on a template
//                            parameter, or the discarded `if constexpr (C::BW)` branch is still checked against it)
//     smem                   the ring: C::kRingBytes + kFlagBytes of LDS
//     tiles_m, tiles_n, vec_store, nwg, map      the launch constants and the tile map (GridTileMap / GivenTile)
//     FP8MI_TILE_ENTRY_STAMP (optional)          the site's stamp of its kernel entry, ahead of the argument loads: the FP8MI_STAMP build writes
//                                                it to slots 13 / 31 behind the wave's coordinates (gemm_kernel has one, gemm_tile's callers none)

    // ==== part 1: what the first stages' DMA needs - tile map, descriptors, the lane's staging offsets (and scale pieces) ====
    unsigned long long k0_ = 0, k1_ = 0, k2_ = 0, d0_ = 0; (void)k0_; (void)k1_; (void)k2_; (void)d0_;
    STAMP(k0_);
#ifdef FP8MI_STAMP
    const unsigned long long r0_ = __builtin_amdgcn_s_memrealtime();
#endif
    int tile_m, tile_n, kslice, wg;
    map(nwg, tiles_m, tiles_n, tile_m, tile_n, kslice, wg);
    if constexpr (C::XLOCAL) {   // (timing experiment) slice fastest inside an XCD's run: a tile's slices sit on one XCD when the run is a multiple of the split
        const int q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7;
        const int wg_all = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + ((int)blockIdx.x >> 3);
        const int split = max(p.split, 1);
        wg = wg_all / split;
        kslice = wg_all - wg * split;
        tile_m = wg % tiles_m;
        tile_n = wg / tiles_m;
    }
    const int n_tiles = tiles_m * tiles_n;
    const int64_t m0 = (int64_t)tile_m * BM, n0 = (int64_t)tile_n * BN;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm0 = (wave % C::kWavesM) * WM;
    const int wn0 = (wave / C::kWavesM) * WN;
#if defined(FP8MI_STAMP) && defined(FP8MI_TILE_ENTRY_STAMP)
    if (lane == 0 && blockIdx.x < 256 && wave <= 1) g_stamp[blockIdx.x * 32 + (wave ? 13 : 31)] = FP8MI_TILE_ENTRY_STAMP;   // waves 0 and 1: kernel entry
#endif

    // ---- buffer descriptors rebased to this tile's first row ------------
    const int64_t rows_a = min((int64_t)BM, p.M - m0), rows_b = min((int64_t)BN, p.N - n0);
    const int64_t bytes_a = (rows_a - 1) * p.lda + C::kXS * p.K, bytes_b = (rows_b - 1) * p.ldb + p.K;   // (C::W4A8: p.K counts W bytes, an X row has twice as many)
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void *)(p.A + m0 * p.lda), 0,
                                                                   (int)min(bytes_a, (int64_t)0x7FFFFFFF), 0x00020000);
    __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void *)(p.B + n0 * p.ldb), 0,
                                                                   (int)min(bytes_b, (int64_t)0x7FFFFFFF), 0x00020000);

    // ---- per-lane staging plan (loop invariant) --------------------------
    StagePlan<C> pl;
    {
        const int row0 = wave * 8 + (lane >> 3);                           // row of this lane in the wave's first group
        const int chunk = (lane & 7) ^ (((wave & 1) * 4 + (lane >> 4)) & 7);  // = (lane & 7) ^ ((row >> 1) & 7) for every group
        pl.row0 = (uint32_t)row0;
        pl.kpos = (uint32_t)(chunk * 16);
        pl.va0 = (uint32_t)(row0 * p.lda + chunk * 16);
        pl.vb0 = (uint32_t)(row0 * p.ldb + chunk * 16);
        pl.sa = (uint32_t)(C::kLoaders * 8 * p.lda);
        pl.sb = (uint32_t)(C::kLoaders * 8 * p.ldb);
        pl.rows_a = (int)rows_a;
        pl.rows_b = (int)rows_b;
        pl.full = rows_a == BM && rows_b == BN;
        pl.pf_off = kOOB;
        pl.pf_waves = 0;
        pl.bsink = u32x4{0u, 0u, 0u, 0u};
        if constexpr (C::BREG) {   // (timing-only) the B panel's descriptor as plain words for the asm loads; the ring starts out zero: no NaN redo on stale LDS bytes
            static_assert(C::PFD == 0, "BREG borrows the prefetch descriptor");
            pl.pf_rsrc = rsrc_words(p.B + n0 * p.ldb, bytes_b);
            for (int o = (int)threadIdx.x * 16; o < C::kRingBytes; o += C::kThreads * 16) *(u32x4 *)(smem + o) = u32x4{0u, 0u, 0u, 0u};
            __syncthreads();
        }
    }
    if constexpr (C::BW) {
        // descriptors based at the tile's first row block, sized to the scales this tile reads: every in-range lane offset is
        // inside the caller's tensor (the host checked that the whole extent is below 2^31 bytes).  A tile lies inside one
        // 128-row block (BM, BN divide 128), so with 128-row blocks all its rows read the same scale
        const int64_t bx0 = m0 >> mx.sh_a, bw0 = n0 >> mx.sh_b;
        const int64_t nbx = ((m0 + rows_a - 1) >> mx.sh_a) - bx0 + 1, nbw = ((n0 + rows_b - 1) >> mx.sh_b) - bw0 + 1;
        const int64_t ext_x = ((nbx - 1) * mx.sa_sr + (mx.nkb - 1) * mx.sa_sk + 1) * 4, ext_w = ((nbw - 1) * mx.sb_sr + (mx.nkb - 1) * mx.sb_sk + 1) * 4;
        pl.sc.rx = __builtin_amdgcn_make_buffer_rsrc((void *)(mx.sa + bx0 * mx.sa_sr), 0, (int)min(ext_x, (int64_t)0x7FFFFFFF), 0x00020000);
        pl.sc.rw = __builtin_amdgcn_make_buffer_rsrc((void *)(mx.sb + bw0 * mx.sb_sr), 0, (int)min(ext_w, (int64_t)0x7FFFFFFF), 0x00020000);
        pl.sc.kx = (uint32_t)(mx.sa_sk * 4);
        pl.sc.kw = (uint32_t)(mx.sb_sk * 4);
        pl.sc.nkb = (int)mx.nkb;
#pragma unroll
        for (int j = 0; j < C::kScaleLoadsPerWave; ++j) {
            const int idx = wave + j * C::kLoaders, q = idx / C::kScalePieces, part = idx - q * C::kScalePieces;
            const bool is_x = part < C::kScalePiecesA;
            const int row = (is_x ? part : part - C::kScalePiecesA) * 64 + lane;
            const bool ok = idx < C::KS * C::kScalePieces && row < (is_x ? rows_a : rows_b);
            const int64_t rb = is_x ? ((m0 + row) >> mx.sh_a) - bx0 : ((n0 + row) >> mx.sh_b) - bw0;
            pl.sc.voff[j] = ok ? (uint32_t)(rb * (is_x ? mx.sa_sr : mx.sb_sr) * 4 + q * (is_x ? pl.sc.kx : pl.sc.kw)) : kOOB;
            pl.sc.is_x[j] = is_x;
            pl.sc.q[j] = q;
        }
    } else if constexpr (C::MXS) {
        pl.sc.rx = __builtin_amdgcn_make_buffer_rsrc((void *)(mx.sx + m0 * mx.ld_sx), 0, (int)min(rows_a * mx.ld_sx, (int64_t)0x7FFFFFFF), 0x00020000);
        pl.sc.rw = __builtin_amdgcn_make_buffer_rsrc((void *)(mx.sw + n0 * mx.ld_sw), 0, (int)min(rows_b * mx.ld_sw, (int64_t)0x7FFFFFFF), 0x00020000);
#pragma unroll
        for (int j = 0; j < C::kScaleLoadsPerWave; ++j) {
            const int idx = wave + j * C::kLoaders, q = idx / C::kScalePieces, part = idx - q * C::kScalePieces;
            const bool is_x = part < C::kScalePiecesA;
            const int row = (is_x ? part : part - C::kScalePiecesA) * 64 + lane;
            const bool ok = idx < C::KS * C::kScaleHalves * C::kScalePieces && row < (is_x ? rows_a : rows_b);
            pl.sc.voff[j] = ok ? (uint32_t)(row * (is_x ? mx.ld_sx : mx.ld_sw) + q * 4) : kOOB;   // (C::FP4: q counts halves of K-steps, 4 scale bytes each)
            pl.sc.is_x[j] = is_x;
        }
    }
    const int nk_all = (int)((p.K + BK * C::KS - 1) / (BK * C::KS));
    const int nsplit = p.split > 1 ? p.split : 1;
    const int nk_slice = (nk_all + nsplit - 1) / nsplit;           // the host made every slice non-empty
    const int ks0 = kslice * nk_slice, nk = min(nk_slice, nk_all - ks0);
    // K is always walked from 0: every tile kernel then adds the K-steps of an output element in the same order, so the
    // unsplit result does not depend on the tile shape or on where the tile sits (a sharded linear equals the unsharded one
    // bit for bit); a per-m-tile rotated start measured within +-2 % of this
    const int rot = 0;

    // ---- the first stages' DMA goes out here; everything below is computed while it is in flight (issue_prologue) ----
    STAMP(d0_);
    if constexpr (C::FLOOR != 2) issue_prologue<C>(pl, ra, rb, smem, wave, ks0, nk, rot, p.K);
    __builtin_amdgcn_sched_barrier(0);   // nothing of part 2 is scheduled ahead of the issue
#ifdef FP8MI_STAMP
    if (lane == 0 && blockIdx.x < 256 && wave <= 1) g_stamp[blockIdx.x * 32 + (wave ? 14 : 26)] = d0_;   // waves 0 and 1: their first DMA issue
#endif

    // ==== part 2: the rest of the set-up ====
    const EpiScalars es = load_epi_scalars<C::MXS>(p);  // scalar loads, in flight under the K loop
    if (!C::FP4 && !C::OCP && threadIdx.x == 0) *lds_word(smem + C::kRingBytes) = 0;  // NaN verdict word (ordered by the K loop's barriers)
    {   // L2 prefetch plan (prefetch_stage)
        if (C::PFD > 0) {
            // this tile's quarter of its B panel's lines for one stage (B has 4 readers on the XCD: the m-tiles of its group)
            constexpr int kLines = BN * C::KS / 4;
            static_assert(C::PFD == 0 || kLines <= 64, "one prefetch instruction per stage");
            // readers of this B panel on the XCD = the m-tiles of this tile's group (4, fewer in a short last group): with 4 readers
            // wave 0 of each warms one quarter, with 2 readers waves 0-1 of each.  A tile that is its panel's only reader does not
            // prefetch: warming its own lines only adds requests (decode shape M=64 K=14336 N=4096: 18.6 -> 20.5 us, measured)
            const int gm = min(4, tiles_m - (tile_m & ~3)), nshare = gm >= 4 ? 4 : (gm >= 2 ? 2 : 1);
            pl.pf_waves = nshare == 1 ? 0 : 4 / nshare;
            const int quarter = (tile_m % nshare) * (4 / nshare) + wave;
            const int li = (quarter & 3) * kLines + lane, prow = li / C::KS, pk = li % C::KS;
            if (lane < kLines && prow < (int)rows_b && (p.K % (BK * C::KS)) == 0) pl.pf_off = (uint32_t)(prow * p.ldb + pk * BK);
            pl.pf_rsrc = rsrc_words(p.B + n0 * p.ldb, bytes_b);
            if (C::PFA && wave == pl.pf_waves) {
                // the wave behind the B-prefetching ones takes this tile's eighth of its A panel's lines (the 8 n-tiles an XCD runs
                // at one time share the panel; A comes from the Infinity Cache for all but the first XCD to touch it)
                constexpr int kLinesA = BM * C::KS / 8;
                static_assert(!C::PFA || kLinesA <= 64, "one prefetch instruction per stage");
                const int lia = (tile_n & 7) * kLinesA + lane, arow = lia / C::KS, ak = lia % C::KS;
                pl.pf_off = (lane < kLinesA && arow < (int)rows_a && (p.K % (BK * C::KS)) == 0) ? (uint32_t)(arow * p.lda + ak * BK) : kOOB;
                pl.pf_rsrc = rsrc_words(p.A + m0 * p.lda, bytes_a);
            }
        }
    }

    // ---- fragment read offsets (lane constant): row r = lane & 15, lane group g = lane >> 4
    //      reads chunk g and chunk 4 + g of its row, swizzled by (r >> 1) -----
    const int fr = lane & 15, fg = lane >> 4;
    const uint32_t off1 = (uint32_t)(fr * BK + ((fg ^ (fr >> 1)) << 4));
    const uint32_t off2 = (uint32_t)(fr * BK + (((4 + fg) ^ (fr >> 1)) << 4));

    MxLane<C> ml;
    if constexpr (C::BW) {
        ml.xo = (uint32_t)((wm0 + fr) * 4);
        ml.wo = (uint32_t)(C::kScalePiecesA * 256 + (wn0 + fg * 4) * 4);
        ml.rows_ok = 0;
        ml.kend = 0;
    } else if constexpr (C::MXS) {
        // lane (fr, fg) supplies the scale of row fr of each fragment, block fg of the K-step (C::FP4: of each half)
        ml.xo = (uint32_t)((wm0 + fr) * 4 + fg);
        ml.wo = (uint32_t)(C::kScalePiecesA * 256 + (wn0 + fr) * 4 + fg);
        uint32_t ok = 0;
#pragma unroll
        for (int t = 0; t < C::TM; ++t) ok |= (wm0 + t * 16 + fr < rows_a) ? 1u << t : 0u;
#pragma unroll
        for (int t = 0; t < C::TN; ++t) ok |= (wn0 + t * 16 + fr < rows_b) ? 1u << (16 + t) : 0u;
        ml.rows_ok = ok;
        ml.kend = p.K - (C::FP4 || C::W4A8 ? 16 : 32) * fg;
    }

    f32x4 acc[C::TN][C::TM];
    if constexpr (C::FLOOR == 2) {   // timing-only: no K loop (the accumulators are zero: the epilogue stores a tile of zeros)
#pragma unroll
        for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
            for (int tm = 0; tm < C::TM; ++tm) acc[tn][tm] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else
    run_tile_any<C, false, true>(p, smem, pl, ra, rb, wave, wm0, wn0, off1, off2, ks0, nk, rot, ml, acc);

    if constexpr (C::FP4 || C::OCP) {
        // (C::OCP, an e5m2 operand: OCP semantics only - inf and NaN bytes are values, nothing is scrubbed or redone)
        // ---- end of the K loop: one barrier frees the ring.  No NaN check and no scrubbed redo: e2m1 has no NaN encoding (bytes
        // 0x7F / 0xFF are two finite values each), so a NaN accumulator comes from a 0xFF scale or an fp32 overflow, and a redo
        // that zeroed those bytes would change the finite outputs of the tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    } else {
        // ---- end of the K loop: one barrier frees the ring and carries the NaN verdict (fp8mi_gemm_epi.h) ----
        lds_vint *flag = lds_word(smem + C::kRingBytes);
        if (p.nan_zero && acc_has_nan<C>(acc)) *flag = 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (p.nan_zero && *flag) {  // workgroup-uniform: redo the tile with every fragment scrubbed (reference NaN semantics)
            run_tile_any<C, true, false>(p, smem, pl, ra, rb, wave, wm0, wn0, off1, off2, ks0, nk, rot, ml, acc);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }

    // ---- split-K: partial tiles meet in the workspace; only the last-arriving slice runs the epilogue ----
    if (nsplit > 1) {
#ifdef FP8MI_DIAG
        // timing-only bound for a PAIRED exchange (DESIGN.md 6.3): two slices, no exchange at all - each workgroup stores the half of
        // the tile whose rows its slice would own (wrong results: the partner's partial is never added)
        if (p.debug & 1) {
            if ((wave % C::kWavesM) * 2 / C::kWavesM != (kslice & 1)) return;
        } else
#endif
        if (!splitk_combine<C>(p, acc, smem, wg, kslice, nsplit, n_tiles)) return;
    }

    STAMP(k1_);
    // ---- fused epilogue ---------------------------------------------------
    const int rows_m = (int)rows_a, cols_n = (int)rows_b;  // valid extent of this tile
    if (rows_m == BM && cols_n == BN && vec_store) {  // interior tile, 16-byte aligned rows: line-coalesced stores
        if (p.out_dtype == FP8MI_F32) epilogue_staged<C, FP8MI_F32>(p, es, acc, smem, m0, n0, wave, wm0, wn0, lane);
        else if (p.out_dtype == FP8MI_BF16) epilogue_staged<C, FP8MI_BF16>(p, es, acc, smem, m0, n0, wave, wm0, wn0, lane);
        else epilogue_staged<C, FP8MI_F16>(p, es, acc, smem, m0, n0, wave, wm0, wn0, lane);
    } else if (p.out_dtype == FP8MI_F32) epilogue<C, FP8MI_F32>(p, es, acc, m0, n0, wm0, wn0, fr, fg, rows_m, cols_n, vec_store);
    else if (p.out_dtype == FP8MI_BF16) epilogue<C, FP8MI_BF16>(p, es, acc, m0, n0, wm0, wn0, fr, fg, rows_m, cols_n, vec_store);
    else epilogue<C, FP8MI_F16>(p, es, acc, m0, n0, wm0, wn0, fr, fg, rows_m, cols_n, vec_store);
#ifdef FP8MI_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(k2_);
    if (threadIdx.x == 0 && blockIdx.x < 256) {
        g_stamp[blockIdx.x * 32 + 5] = k1_ - k0_;   // entry .. end of K loop (incl. NaN check)
        g_stamp[blockIdx.x * 32 + 6] = k2_ - k1_;   // epilogue incl. store drain
        g_stamp[blockIdx.x * 32 + 7] = __builtin_amdgcn_s_memrealtime() - r0_;  // 100 MHz ticks over the whole tile
        g_stamp[blockIdx.x * 32 + 29] = k0_;
        g_stamp[blockIdx.x * 32 + 30] = k1_;
    }
#endif
