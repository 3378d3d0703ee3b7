// qp_twisted_body.h -- the whole solve of one wave of the register-resident kernel family, as TEXT: included inside the body of
// solve_twisted_kernel and of solve_twisted_group_kernel (qp_twisted.h), and nowhere else.  Each kernel is these statements behind its own
// way of getting the arguments, so the two run the same arithmetic by construction -- and solve_twisted_kernel compiles to exactly the
// instructions it had when the statements stood in it (a shared __device__ function, even one that is always inlined, reaches the
// optimiser in another order and came out with other schedules and operand orders in most instantiations).
// The including scope provides: the template parameters R, M, TILE, LPT, the compile-time bools ONE and EMIT2, and `const TwistedArgs a`.
// EMIT2 (solve_twisted_group8_kernel only: TILE = LPT = 8, ONE): the lane pair emits both segments of a 16-lane step itself.
// The wave's tiles go by blockIdx.x / gridDim.x alone.  No include guard: included once per kernel.
    using C = TwistedCfg<R, M, TILE, LPT>;
    static_assert(!EMIT2 || (ONE && LPT == 8 && TILE == TWMAP8_TILE), "both segments of a step per lane pair: eight trajectories per wave, one whole tile");
    constexpr int NAX = C::NAX;
    constexpr int ND = C::ND, NC = C::NC, NK = C::NK, mL = C::mL, mR = C::mR;
    static_assert(M >= 2, "twisted kernel needs an interior knot");
    static_assert(!ONE || LPT >= 8, "one tile per wave: latency shapes only");
    static_assert((LPT == 2 && (TILE == 32 || TILE == 16)) || (LPT == 8 && TILE == 8) || (LPT == 16 && TILE == 4), "tile shapes: 2 lanes x 32|16, 8 lanes x 8, 16 lanes x 4");

    __shared__ __attribute__((aligned(16))) double s_in[ONE ? 1 : 2][C::IN_D];
    __shared__ __attribute__((aligned(16))) double s_out[EMIT2 ? C::OUT2_D : C::OUT_D];
    (void)s_out;

    const int lane = threadIdx.x;
    const int isR = lane & 1;
    const int tl = lane / LPT;
    const int tlc = tl < TILE ? tl : TILE - 1;  // clamp LDS indexing of idle lanes (TILE == 16)
    const int axl = ((lane % LPT) >> 1) & 3;     // LPT >= 8: axis of this lane pair (3 = idle pair)
    const int sub = LPT == 16 ? (lane >> 3) & 1 : 0;   // LPT == 16: which half of the own segments this lane pair emits
    const int ax0 = LPT == 2 ? 0 : (axl < 3 ? axl : 2);
    const int m = isR ? mR : mL;
    // ONE: this wave's tile is its only one.  The trip count of 1 is hidden from the compiler so that a LOOP remains: everything
    // invariant (lane indices, addresses, the output descriptor) is then hoisted in front of it, i.e. in front of the wait for the loads
    // below, where it costs nothing -- in straight-line code it is scheduled behind the wait, on the wave's critical path.
    int one_trip = 1;
    if constexpr (ONE) asm volatile("" : "+s"(one_trip));
    const int n_tiles = ONE ? (int)blockIdx.x + one_trip : (a.n_traj + TILE - 1) / TILE;

    // A partial last tile is SHIFTED back so that it ends at the batch end (n_traj >= TILE): it stays on the LDS-DMA path and
    // re-solves a few trajectories of its neighbour -- identical values written twice -- instead of sending one wave through the
    // guarded element-wise loads (measured on 4093 trajectories: 6.43 -> 5.03 us: that one wave was the kernel's critical path).
    // Batches smaller than one tile keep the guarded path.
    auto tile_base = [&](int tile) {
        const int b_ = tile * TILE;
        if constexpr (ONE) return b_;
        return (a.n_traj >= TILE && b_ + TILE > a.n_traj) ? a.n_traj - TILE : b_;
    };
    constexpr int DMA_AUX = LPT >= 8 ? 2 : 0;
    auto issue_tile = [&](int tile, int buf) {
        const int base = tile_base(tile);
        const int nv = ONE ? TILE : min(TILE, a.n_traj - base);
        double* s = s_in[buf];
        if (ONE || nv == TILE) {
            dma_tile<C::WP_D, DMA_AUX>(a.waypoints + (size_t)base * NK * 3, s, lane);
            dma_tile<C::T_D, DMA_AUX>(a.times + (size_t)base * M, s + C::T_OFF, lane);
            dma_tile<C::BC_D, DMA_AUX>(a.bc + (size_t)base * 2 * ND * 3, s + C::BC_OFF, lane);
        } else {
            load_tile_guarded<C::WP_D>(a.waypoints + (size_t)base * NK * 3, nv * NK * 3, s, lane, 0.0);
            load_tile_guarded<C::T_D>(a.times + (size_t)base * M, nv * M, s + C::T_OFF, lane, 1.0);
            load_tile_guarded<C::BC_D>(a.bc + (size_t)base * 2 * ND * 3, nv * 2 * ND * 3, s + C::BC_OFF, lane, 0.0);
        }
    };

    int buf = 0;
    UAVQP_STAMP(5);
    if ((int)blockIdx.x < n_tiles) issue_tile(blockIdx.x, 0);
    UAVQP_STAMP(6);

    for (int tile = blockIdx.x; tile < n_tiles; tile += (ONE ? 1 : gridDim.x), buf ^= (ONE ? 0 : 1)) {
        // The wait for the FIRST tile sits inside the loop: everything loop-invariant (lane indices, table constants, addresses --
        // ~130 instructions) lands in the loop pre-header, i.e. between the issue of the first loads and this wait, instead of
        // behind it (measured: load wait 2150 -> 1230 cycles per wave, 5.49 -> 5.05 us on the 4096 batch).
        if (tile == (int)blockIdx.x) {
            wait_vmcnt0();
            wave_lds_sync();
        }
        const int base = tile_base(tile);
        const int nv = ONE ? TILE : min(TILE, a.n_traj - base);
        UAVQP_STAMP(0);
        // prefetch the next tile into the other buffer; it lands while this tile is eliminated
        if constexpr (!ONE) {
            if (tile + (int)gridDim.x < n_tiles) issue_tile(tile + gridDim.x, buf ^ 1);
        }
        UAVQP_STAMP(1);

        const double* __restrict__ s_wp = s_in[buf];
        const double* __restrict__ s_T = s_in[buf] + C::T_OFF;
        const double* __restrict__ s_bc = s_in[buf] + C::BC_OFF;

        // ---------------- validate own half, sanitise so that the arithmetic stays finite ----------------
        bool ok = (tl < nv) && (LPT == 2 || axl < 3);
#pragma unroll
        for (int j = 0; j < mL; ++j)
            if (j < m) {
                const double t = s_T[tlc * M + (isR ? M - 1 - j : j)];
                ok = ok && (t > 0.0) && (t < INFINITY);
            }
        {
            const int oki = ok ? 1 : 0;
            const int other = __builtin_amdgcn_mov_dpp(oki, 0xB1, 0xF, 0xF, true);
            ok = (oki & other) != 0;
        }
        const unsigned long long okmask = __ballot(ok);  // bit LPT*t: trajectory t of this tile is valid

        auto Tof = [&](int j) -> double {
            const double t = s_T[tlc * M + (isR ? M - 1 - j : j)];
            return ok ? t : 1.0;
        };
        auto pos = [&](int j, int ax) -> double { return s_wp[(tlc * NK + (isR ? M - j : j)) * 3 + ax0 + ax]; };

        // ---------------- elimination of own interior knots j = 1..m-1 ----------------
        // index 0 = boundary knot: E_0 = 0, h_0 = y0 (own frame: y'_0 = F y_M for the reversed lane)
        double E[mL][ND][ND], h[mL][ND][NAX];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
#pragma unroll
            for (int c = 0; c < ND; ++c) E[0][i][c] = 0.0;
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) {
                const double v = s_bc[((tlc * 2 + isR) * ND + i) * 3 + ax0 + ax];
                h[0][i][ax] = (isR && ((i & 1) == 0)) ? -v : v;
            }
        }
        // (LPT == 2: the own durations stay in registers for the emission -- the duration tile has a row stride of M doubles, a
        // 4-way bank conflict per read for M = 8)
        // (LPT == 8: also their inverse powers T^-R..T^-(2R-1), which SegBlocks::build computes anyway and the emission needs again)
        // (EMIT2: neither -- its emission is the 16-lane shape's, which reloads the duration and takes its reciprocal)
        constexpr bool KEEP_T = (LPT == 2 || LPT == 8) && !EMIT2, KEEP_IP = LPT == 8 && !EMIT2;
        double Town[KEEP_T ? mL : 1], Tip[KEEP_IP ? mL : 1][R];
#pragma unroll
        for (int j = 0; j < (KEEP_T ? mL : 1); ++j) Town[j] = 1.0;
#pragma unroll
        for (int j = 0; j < (KEEP_IP ? mL : 1); ++j)
#pragma unroll
            for (int k = 0; k < R; ++k) Tip[j][k] = 1.0;
        SegBlocks<R> sa;
        {
            const double t0 = Tof(0);
            Town[0] = t0;
            double ipw[NC];
            sa.build(t0, ipw);
            if constexpr (KEEP_IP) {
#pragma unroll
                for (int k = 0; k < R; ++k) Tip[0][k] = ipw[R + k];
            }
        }
        double pb[NAX], dpa[NAX];
#pragma unroll
        for (int ax = 0; ax < NAX; ++ax) {
            pb[ax] = pos(1, ax);
            dpa[ax] = pb[ax] - pos(0, ax);
        }
#pragma unroll
        for (int j = 1; j < mL; ++j) {
#if defined(UAVQP_TW_SKIP_LAST_ELIM) && !defined(UAVQP_TIMING_BUILD)
#error "UAVQP_TW_SKIP_LAST_ELIM produces WRONG results: timing harness only (tools/ubench/tw, built with -DUAVQP_TIMING_BUILD), never libuavqp.so"
#endif
#ifdef UAVQP_TW_SKIP_LAST_ELIM   // timing-only build (tools/ubench/tw: h_16s): the last elimination step takes its inputs from TWO knots back, so it no
            // longer waits for the step before it -- the same work on a dependent chain one level shorter, i.e. what a cyclic reduction could buy
            // AT MOST (its exchanges not counted); the results are wrong
            constexpr bool tw_short = true;
#else
            constexpr bool tw_short = false;
#endif
            const int jp = (tw_short && j == mL - 1 && j >= 2) ? j - 2 : j - 1;
            if (j < m) {
                SegBlocks<R> sb;
                {
                    const double tj = Tof(j);
                    if constexpr (KEEP_T) Town[j] = tj;
                    double ipw[NC];
                    sb.build(tj, ipw);
                    if constexpr (KEEP_IP) {
#pragma unroll
                        for (int k = 0; k < R; ++k) Tip[j][k] = ipw[R + k];
                    }
                }
                double dpb[NAX];
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) {
                    const double pc = pos(j + 1, ax);
                    dpb[ax] = pc - pb[ax];
                    pb[ax] = pc;
                }
                double S[ND][ND], z[ND][NAX];
#pragma unroll
                for (int i = 0; i < ND; ++i) {
#pragma unroll
                    for (int c = 0; c < ND; ++c) S[i][c] = sa.A11[i][c] + sb.A00(i, c);
#pragma unroll
                    for (int ax = 0; ax < NAX; ++ax) z[i][ax] = sb.gv(i) * dpb[ax] - sa.gw[i] * dpa[ax];
                }
#pragma unroll
                for (int i = 0; i < ND; ++i)
#pragma unroll
                    for (int q = 0; q < ND; ++q) {
                        if (j > 1) {
#pragma unroll
                            for (int c = 0; c <= i; ++c) S[i][c] -= sa.A01[q][i] * E[jp][q][c];
                        }
#pragma unroll
                        for (int ax = 0; ax < NAX; ++ax) z[i][ax] -= sa.A01[q][i] * h[jp][q][ax];
                    }
                typename std::conditional<LPT >= 8, SymInv<ND>, SmallLDL<ND>>::type ldl;
                ldl.factor(S);
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) {
                    double col[ND];
#pragma unroll
                    for (int i = 0; i < ND; ++i) col[i] = z[i][ax];
                    ldl.solve(col);
#pragma unroll
                    for (int i = 0; i < ND; ++i) h[j][i][ax] = col[i];
                }
#pragma unroll
                for (int c = 0; c < ND; ++c) {
                    double col[ND];
#pragma unroll
                    for (int i = 0; i < ND; ++i) col[i] = sb.A01[i][c];
                    ldl.solve(col);
#pragma unroll
                    for (int i = 0; i < ND; ++i) E[j][i][c] = col[i];
                }
                sa = sb;
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) dpa[ax] = dpb[ax];
            }
        }
        UAVQP_STAMP(2);

        // ---------------- meeting knot: own partial Schur complement, exchange, solve ----------------
        // sa = blocks of the last own segment (m-1); E/h index m-1 is the last eliminated knot (or the boundary).
        double P[ND][ND], zp[ND][NAX];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
#pragma unroll
            for (int c = 0; c < ND; ++c) P[i][c] = sa.A11[i][c];
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) zp[i][ax] = -sa.gw[i] * dpa[ax];
        }
        {
            // E/h of knot m-1, selected per lane when the halves differ in length (odd M)
            double El[ND][ND], hl[ND][NAX];
#pragma unroll
            for (int i = 0; i < ND; ++i) {
#pragma unroll
                for (int c = 0; c < ND; ++c) El[i][c] = (mL == mR || !isR) ? E[mL - 1][i][c] : E[mR - 1][i][c];
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) hl[i][ax] = (mL == mR || !isR) ? h[mL - 1][i][ax] : h[mR - 1][i][ax];
            }
#pragma unroll
            for (int i = 0; i < ND; ++i)
#pragma unroll
                for (int q = 0; q < ND; ++q) {
#pragma unroll
                    for (int c = 0; c <= i; ++c) P[i][c] -= sa.A01[q][i] * El[q][c];
#pragma unroll
                    for (int ax = 0; ax < NAX; ++ax) zp[i][ax] -= sa.A01[q][i] * hl[q][ax];
                }
        }
        double ynext[ND][NAX];  // solution at the meeting knot, own frame
        {
            double S[ND][ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) {
#pragma unroll
                for (int c = 0; c <= i; ++c) {
                    const double o = swap_pair(P[i][c]);
                    S[i][c] = P[i][c] + (((i + c) & 1) ? -o : o);  // P_own + F P_other F
                }
#pragma unroll
                for (int c = i + 1; c < ND; ++c) S[i][c] = 0.0;  // upper triangle is never read
            }
            typename std::conditional<LPT >= 8, SymInv<ND>, SmallLDL<ND>>::type ldl;
            ldl.factor(S);
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) {
                double col[ND];
#pragma unroll
                for (int i = 0; i < ND; ++i) {
                    const double o = swap_pair(zp[i][ax]);
                    col[i] = zp[i][ax] + ((i & 1) ? o : -o);  // z_own + F z_other, F_ii = (-1)^(i+1)
                }
                ldl.solve(col);
#pragma unroll
                for (int i = 0; i < ND; ++i) ynext[i][ax] = col[i];
            }
        }
        UAVQP_STAMP(3);

        // The prefetched tile has had the whole elimination to land; this also retires the previous
        // tile's stores (issued before the prefetch) so that the waits below never see them.
        if constexpr (!ONE) wait_vmcnt0();

        // ---------------- back-substitution + emission of own segments j = m-1 .. 0 ----------------
        bool finite = true;
        double* __restrict__ out = a.coeff + (size_t)base * 3 * M * NC;

        if constexpr (LPT >= 8) {
            // one axis per lane pair.  Back-substitution first (in place, h[j] <- y_j), so that the mL segment evaluations below are
            // independent of each other and the scheduler can overlap their dependent FP64 chains.
#pragma unroll
            for (int j = mL - 1; j >= 1; --j) {
                if (j < m) {
#pragma unroll
                    for (int i = 0; i < ND; ++i)
#pragma unroll
                        for (int c = 0; c < ND; ++c) {
                            const double src = (j == mL - 1 || j == m - 1) ? ynext[c][0] : h[j + 1 < mL ? j + 1 : j][c][0];
                            h[j][i][0] -= E[j][i][c] * src;
                        }
                }
            }
            if constexpr (EMIT2) {
            // Eight trajectories per wave, one lane pair per (trajectory, axis, side): in step s the pair evaluates BOTH own segments
            // 2 s and 2 s + 1 -- the NSUB == 2 step below once per `sub`, now a compile-time constant (same candidates, same
            // segment_coeffs on the reloaded duration and its fast_rcp, same `finite` rule), so every segment gets the operations the
            // 16-lane shape gives it.  A sub-step in which no lane has a segment (2 s + 1 == mL) is not evaluated at all; one in which
            // only the reversed lanes have none (odd M) leaves them a chunk that is dropped, as there.  Both chunks go to LDS rows laid
            // out as TWO 16-lane tiles of four trajectories (qp_twisted_map8.h), and the copy-out of a step is six stores of 16 bytes
            // per lane, each the 16-lane kernel's store of one axis of four trajectories: the same lines from the same lane groups,
            // write-through, dropped pieces out of range, interleaved with the next step's arithmetic.
            constexpr int H = (mL + 1) / 2, RS = C::RS8, NIT = TWMAP8_PIECES;
            static_assert(twmap8_steps(M) == H, "the map's steps are the kernel's");
            // (where the rows lie, and why the twelve b128 writes of 16 consecutive lanes start in twelve bank quads: qp_twisted_map8.h)
            auto row_addr = [&](int blk, int rest) -> int { return twmap8_row_addr(blk, rest); };
            static_assert(NC <= TWMAP8_ROW_DOUBLES, "a chunk fits its row");
            const unsigned tile_bytes = (unsigned)TILE * 3u * M * NC * 8u;
            const unsigned long long obase = (unsigned long long)out;
            const unsigned ob_lo = __builtin_amdgcn_readfirstlane((unsigned)obase), ob_hi = __builtin_amdgcn_readfirstlane((unsigned)(obase >> 32));
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)ob_hi << 32) | ob_lo), 0,
                                                                __builtin_amdgcn_readfirstlane(tile_bytes), 0x00020000);
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            // the piece this lane copies: the same row slot of the six blocks (half x axis).  The decode is written out here from the
            // map's building blocks (twmap_rest_*, twmap8_block_*, twmap_own_segment, twmap_global_segment) so that everything that does
            // not depend on the step or the block is computed once in front of the loop; twmap8_piece() is the same composition as ONE
            // function, and it is that function the CPU test walks -- the kernel's own composition (c_off + (axis * M + segment) * NC * 8,
            // keep) is covered by the bitwise GPU tests only (tests/test_gpu_twisted_group8.py).  Keep the two in step.
            // The decode starts from an OPAQUE copy of the lane index.  It depends on the lane alone, so with the hidden trip count
            // (one_trip above) all of it -- a dozen dwords per lane: the keeps, the offsets, the row slot -- was hoisted in front of
            // the load wait and stayed live across the whole elimination, where the register peak is: 182 VGPRs for (4, 8), 226 for
            // (3, 16), two waves per SIMD.  A fused launch fills its SIMDs, so what counts is how many waves fit, not what one wave
            // has in front of its wait: behind the elimination the same values cost ~25 instructions and no register at the peak
            // (156 / 154 VGPRs: three waves; docs/measurement_log.md, 2026-10-21).  The eager kernels keep their hoisted set-up.
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));
            const int c_rest = lane_e >> 2, c_col = lane_e & 3;
            const int c_R = twmap_rest_side<2>(c_rest), c_sub = twmap_rest_sub<2>(c_rest), c_tl4 = twmap_rest_traj<2>(c_rest);
            const int c_m = c_R ? mR : mL;
            bool c_keep[2];
            unsigned c_off[2];   // + axis * M * NC * 8 + segment * NC * 8
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int c_tl = hf * 4 + c_tl4;
                c_keep[hf] = (c_col < NC / 2) && ((okmask >> (LPT * c_tl)) & 1ull);
                c_off[hf] = (unsigned)(((c_tl * 3 * M) * NC + 2 * c_col) * 8);
            }
            const int c_lds = c_rest * RS + 2 * c_col;
            // own rows: one per sub; the idle pairs write behind the blocks (or, where those rows are not allocated, not at all)
            int my_lds[2];
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
                my_lds[sb] = axl < 3 ? row_addr(twmap8_block(tlc, axl), twmap8_rest(tlc, sb, isR))
                                     : (C::IDLE_ROWS2 ? twmap8_idle_addr((lane >> 3) * 2 + isR) : 0);
            auto flush = [&](int sp) {   // copy-out of step sp: NIT LDS reads, NIT stores
                // (every row is read, also one nobody wrote in this step: where 2 sp + 1 == mL the sub-1 rows hold the previous step's
                //  chunks -- or, for M = 2, whatever LDS held at wave start.  Those pieces are never stored: jv < c_m below is false for
                //  them and the store gets the out-of-range offset)
                double2 v[NIT];
#pragma unroll
                for (int it = 0; it < NIT; ++it) v[it] = *reinterpret_cast<const double2*>(s_out + row_addr(it, 0) + c_lds);
                const int jv = twmap_own_segment<2>(sp, c_sub);               // own segment of the producing lane
                const int cseg = twmap_global_segment(M, c_R, jv);
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int hf = twmap8_block_half(it), cax = twmap8_block_axis(it);
                    u32x4 w;
                    w.x = (unsigned)__double2loint(v[it].x); w.y = (unsigned)__double2hiint(v[it].x);
                    w.z = (unsigned)__double2loint(v[it].y); w.w = (unsigned)__double2hiint(v[it].y);
                    const unsigned off = (c_keep[hf] && jv < c_m) ? c_off[hf] + (unsigned)((cax * M + cseg) * NC * 8) : 0xFFFFFFF0u;
                    __builtin_amdgcn_raw_buffer_store_b128(w, rsrc, off, 0, 17 /* sc0 sc1: write-through, nothing left dirty for the kernel boundary */);
                }
            };
#pragma unroll
            for (int s = 0; s < H; ++s) {
                if (s > 0) flush(s - 1);
                double c8[2][NC];
                auto sub_step = [&](auto sub_c) {
                    constexpr int sb = decltype(sub_c)::value;
                    const int j = twmap_own_segment<2>(s, sb);
                    if (j < mL) {
                        const bool act = (j < m);
                        const int jc = act ? j : (m > 0 ? m - 1 : 0);
                        const double pj = pos(jc, 0), pj1 = pos(jc + 1, 0);
                        double ys[ND], ye[ND];
#pragma unroll
                        for (int d = 0; d < ND; ++d) {
                            const double fs = ((d & 1) == 0) ? -1.0 : 1.0;
                            auto Y = [&](int q) -> double { return (q >= mL || q == m) ? ynext[d][0] : h[q < mL ? q : mL - 1][d][0]; };
                            // pair 1's segment lies behind pair 0's: its start is pair 0's end
                            const double yj = sb ? Y(2 * s + 1) : h[2 * s][d][0], yj1 = sb ? Y(2 * s + 2) : Y(2 * s + 1);
                            ys[d] = isR ? fs * yj1 : yj;
                            ye[d] = isR ? fs * yj : yj1;
                        }
                        const double Tj = Tof(jc);
                        segment_coeffs<R>(isR ? pj1 : pj, ys, isR ? pj : pj1, ye, Tj, fast_rcp(Tj), c8[sb]);
                        if (act) finite = finite && (fabs(c8[sb][NC - 1]) < INFINITY) && (fabs(c8[sb][R]) < INFINITY);
                    }
                };
                sub_step(std::integral_constant<int, 0>{});
                sub_step(std::integral_constant<int, 1>{});
                if (s > 0) {
                    // the previous step's copy-out between this step's arithmetic: LDS reads first, then one store per ~20 VALU instructions
                    __builtin_amdgcn_sched_group_barrier(0x100, NIT, 0);
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        __builtin_amdgcn_sched_group_barrier(0x2, 20, 0);
                        __builtin_amdgcn_sched_group_barrier(0x40, 1, 0);
                    }
                }
#pragma unroll
                for (int sb = 0; sb < 2; ++sb) {
                    if (twmap_own_segment<2>(s, sb) < mL && (C::IDLE_ROWS2 || axl < 3)) {
                        // (lanes without a segment in this sub-step write too, and so do the idle pairs where their rows exist
                        //  (C::IDLE_ROWS2) -- rows / chunks that are never copied out; where they do not exist the idle pairs are masked off)
                        double* so = s_out + my_lds[sb];
#pragma unroll
                        for (int k = 0; k < NC; k += 2) *reinterpret_cast<double2*>(so + k) = make_double2(c8[sb][k], c8[sb][k + 1]);
                    }
                }
                // single-wave workgroup: LDS operations execute in issue order; this only pins the compiler's order of the accesses
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (s == H - 1) flush(s);
            }
            } else {
            // LPT == 16: two lane pairs per (trajectory, axis) repeat elimination and back-substitution and split the EMISSION --
            // in step s pair `sub` evaluates the own segment s * NSUB + sub (selects between compile-time candidates, one instruction
            // stream): 4 trajectories per wave, a 4096-trajectory batch fills all 1024 SIMDs.  The two pairs of a side emit ADJACENT
            // segments in the same step, and the staging rows of a trajectory are ordered by address (side 0 sub 0, side 0 sub 1,
            // side 1 sub 1, side 1 sub 0: the reversed lanes' segments descend), so that for r = 4 and even M a step's copy-out writes
            // whole 128-byte lines, each from eight adjacent lanes (M = 8: 16 lines per instruction, no partial line; odd mL leaves the
            // two halves of the middle line to the last step), and for r = 3 96-byte runs.  Before, pair `sub` emitted sub * H + s:
            // every store wrote 64-byte halves of 32 different lines, the other half a step later, and write-through halves are not
            // merged in L2 (tools/ubench/write_patterns.hip patterns 9 / 8).  The map -- (lane, step) -> trajectory, side, segment,
            // column, keep or drop -- is qp_twisted_map.h, shared with tests/cpp/test_twisted_map.cpp.
            //
            // Copy-out, software-pipelined (what the per-wave timelines of tools/ubench/tw asked for: a vector-memory store costs the
            // wave ~100 cycles of issue, sixteen scattered quarter-chunk stores per lane were 1100 of the emission's 3400 cycles and left
            // 6.3 MB dirty in L2 for the kernel boundary to write back):
            //   * the NC-double chunk a lane produces in step s goes to its own LDS row at the end of the step;
            //   * at the START of step s + 1 the wave reads the 48 rows back (16 bytes per lane: whole chunks from adjacent lanes,
            //     one axis per instruction) and its three write-through stores are interleaved with that step's arithmetic (sched_group_barrier): only the
            //     last step's stores are exposed;
            //   * buffer stores through a per-tile descriptor: pieces of an invalid trajectory, of a lane without a segment in that
            //     step (odd M) and -- for batches smaller than a tile -- of trajectories past the end get an out-of-range offset and
            //     are dropped by the hardware: no branch, no sink traffic.
            // 4096 x (M = 8, r = 4), us per launch over rotating buffers: 6.45 (direct stores) -> 5.80 (two-step chunks through LDS,
            // write-through) -> 5.52 (this) for 8 lanes per trajectory, 5.30 for 16.
            constexpr int NSUB = LPT / 8, H = (mL + NSUB - 1) / NSUB;
            // LDS rows: axis-major, 16 rows per axis (one per (trajectory, sub, side) = `rest`), so that copy instruction `it` moves
            // axis `it` and everything else about a piece comes from lane bits: rest = lane >> 2, 16-byte column = lane & 3 (a row
            // is padded to four pieces; r = 3 uses three).  Row stride 10 doubles + 4 doubles per axis: the 12 working lanes of any
            // 16 consecutive lanes start their b128 writes in 12 different bank quads.
            constexpr int RS = C::RS8, NIT = 3;
            auto row_addr = [&](int cax, int rest) -> int { return (cax * 16 + rest) * RS + cax * 4; };
            const unsigned tile_bytes = (unsigned)nv * 3u * M * NC * 8u;
            const unsigned long long obase = (unsigned long long)out;
            const unsigned ob_lo = __builtin_amdgcn_readfirstlane((unsigned)obase), ob_hi = __builtin_amdgcn_readfirstlane((unsigned)(obase >> 32));
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)ob_hi << 32) | ob_lo), 0,
                                                                __builtin_amdgcn_readfirstlane(tile_bytes), 0x00020000);
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            // the piece this lane copies (the same row slot for the three axes)
            const int c_rest = lane >> 2, c_col = lane & 3;
            // (NSUB == 1: the map's decode written out -- the 8-lane shape's instruction stream is left exactly as it was)
            static_assert(twmap_plain_rows(), "one lane pair per axis: rest = trajectory * 2 + side");
            const int c_R = NSUB == 2 ? twmap_rest_side<NSUB>(c_rest) : c_rest & 1, c_sub = NSUB == 2 ? twmap_rest_sub<NSUB>(c_rest) : 0,
                      c_tl = NSUB == 2 ? twmap_rest_traj<NSUB>(c_rest) : c_rest >> 1;
            static_assert(twmap_side_segments(M, 0) == mL && twmap_side_segments(M, 1) == mR, "the map's sides are the kernel's");
            const int c_m = c_R ? mR : mL;
            const bool c_keep = (c_col < NC / 2) && ((okmask >> (LPT * c_tl)) & 1ull);
            const unsigned c_off = (unsigned)(((c_tl * 3 * M) * NC + 2 * c_col) * 8);   // + axis * M * NC * 8 + segment * NC * 8
            const int c_lds = c_rest * RS + 2 * c_col;
            const int my_rest = twmap_rest<NSUB>(tlc, sub, isR);
            const int my_lds = axl < 3 ? row_addr(axl, my_rest) : 48 * RS + 16 + (lane & 15) * RS;
            auto flush = [&](int sp) {   // copy-out of step sp: NIT LDS reads, NIT stores
                double2 v[NIT];
#pragma unroll
                for (int it = 0; it < NIT; ++it) v[it] = *reinterpret_cast<const double2*>(s_out + row_addr(it, 0) + c_lds);
                const int jv = twmap_own_segment<NSUB>(sp, c_sub);               // own segment of the producing lane
                const int cseg = twmap_global_segment(M, c_R, jv);
#if defined(UAVQP_TW_DROP_STORES) && !defined(UAVQP_TIMING_BUILD)
#error "UAVQP_TW_DROP_STORES produces WRONG results: timing harness only (tools/ubench/twisted_phases4_one_nostores, built with -DUAVQP_TIMING_BUILD), never libuavqp.so"
#endif
                unsigned off0 = (c_keep && jv < c_m) ? c_off + (unsigned)(cseg * NC * 8) : 0xFFFFFFF0u;
#ifdef UAVQP_TW_DROP_STORES   // timing-only build: EVERY piece gets the out-of-range offset (offsets are multiples of 16: or-ing the mask in gives exactly
                // 0xFFFFFFF0) -- the same instructions plus one v_or, the hardware drops all stores.  Against the product this bounds what any change
                // to the store path can return; no coefficient is written
                unsigned tw_drop = 0xFFFFFFF0u;
                asm volatile("" : "+s"(tw_drop));   // (opaque: the address arithmetic stays)
                off0 |= tw_drop;
#endif
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    u32x4 w;
                    w.x = (unsigned)__double2loint(v[it].x); w.y = (unsigned)__double2hiint(v[it].x);
                    w.z = (unsigned)__double2loint(v[it].y); w.w = (unsigned)__double2hiint(v[it].y);
                    // (an out-of-range base stays out of range: 0xFFFFFFF0 + it * M * NC * 8 wraps only for absurd M)
                    const unsigned off = off0 == 0xFFFFFFF0u ? off0 : off0 + (unsigned)(it * M * NC * 8);
                    __builtin_amdgcn_raw_buffer_store_b128(w, rsrc, off, 0, 17 /* sc0 sc1: write-through, nothing left dirty for the kernel boundary */);
                }
            };
#pragma unroll
            for (int s = 0; s < H; ++s) {
                if (s > 0) flush(s - 1);
                const int j = twmap_own_segment<NSUB>(s, sub);
                const bool act = (j < m);
                const int jc = act ? j : (m > 0 ? m - 1 : 0);
                const double pj = pos(jc, 0), pj1 = pos(jc + 1, 0);
                double ys[ND], ye[ND], c8[NC];
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const double fs = ((d & 1) == 0) ? -1.0 : 1.0;
                    auto Y = [&](int q) -> double { return (q >= mL || q == m) ? ynext[d][0] : h[q < mL ? q : mL - 1][d][0]; };
                    double yj = h[NSUB * s][d][0], yj1 = Y(NSUB * s + 1);
                    if constexpr (NSUB == 2) {
                        // pair 1 emits the segment behind pair 0's: its start is pair 0's end -- Y(2 s + 1) is h[2 s + 1] wherever pair 1 has
                        // a segment (2 s + 1 < m), and where it has none its chunk is dropped -- so three candidates serve the two selects
                        // (the candidates are pinned as VALUES first: left alone, the optimiser turns a select between two elements of h
                        // into ONE load through a selected pointer before the loops are unrolled -- and h, indexed at run time, goes to
                        // scratch: 32-48 bytes per lane in the M = 3, 4, 5 shapes)
                        double alt1 = Y(2 * s + 2);
                        asm("" : "+v"(yj));
                        asm("" : "+v"(alt1));
                        asm("" : "+v"(yj1));
                        yj = sub ? yj1 : yj;
                        yj1 = sub ? alt1 : yj1;
                    }
                    ys[d] = isR ? fs * yj1 : yj;
                    ye[d] = isR ? fs * yj : yj1;
                }
                if constexpr (LPT == 8) {
                    // the duration and its inverse powers were kept from the elimination (SegBlocks::build): no reciprocal, no power chain
                    double ipj[NC];
#pragma unroll
                    for (int k = 0; k < R; ++k) { ipj[k] = 1.0; ipj[R + k] = Tip[s][k]; }
                    segment_coeffs_ip<R>(isR ? pj1 : pj, ys, isR ? pj : pj1, ye, Town[s], ipj, c8);
                } else {
                    const double Tj = Tof(jc);
                    segment_coeffs<R>(isR ? pj1 : pj, ys, isR ? pj : pj1, ye, Tj, fast_rcp(Tj), c8);
                }
                if (act) finite = finite && (fabs(c8[NC - 1]) < INFINITY) && (fabs(c8[R]) < INFINITY);
                if (s > 0) {
                    // the previous step's copy-out between this step's arithmetic: LDS reads first, then one store per ~24 VALU instructions
                    __builtin_amdgcn_sched_group_barrier(0x100, NIT, 0);
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        __builtin_amdgcn_sched_group_barrier(0x2, 24, 0);
                        __builtin_amdgcn_sched_group_barrier(0x40, 1, 0);
                    }
                }
                {
                    // (idle pairs and lanes without a segment in this step write too -- rows / chunks that are never copied out)
                    double* so = s_out + my_lds;
#pragma unroll
                    for (int k = 0; k < NC; k += 2) *reinterpret_cast<double2*>(so + k) = make_double2(c8[k], c8[k + 1]);
                }
                // single-wave workgroup: LDS operations execute in issue order; this only pins the compiler's order of the accesses
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (s == H - 1) flush(s);
            }
            }   // !EMIT2
        } else {
            // ---------------- chunk mode (LPT == 2): CH own segments x one axis per emission unit ----------------
            // Every lane writes the 2r*CH coefficients of its chunk, in ORIGINAL segment order, to its own LDS
            // row; the wave then copies the 64 rows out linearly, 16 B per lane: a lane row is one contiguous
            // run in HBM (r = 4, CH = 2: exactly one 128-B line; r = 3, CH = 4: 192 B, and when CH covers the
            // whole half the L and R rows of a trajectory are adjacent, i.e. whole (trajectory, axis) rows).
            // Units are axis-major so that the fragments of a line shared by two chunks are written close
            // together.  Measured on the store pattern alone (tools/ubench/write_patterns.hip): 5.3-5.5 TB/s
            // for line-complete runs vs 3.0-3.5 TB/s when half lines / 48-B chunks arrive a segment apart.
            constexpr int CH = C::CH, NQ = (mL + CH - 1) / CH, RS = C::STAGE_STRIDE, PPL = CH * NC / 2;
            // in-place back-substitution: h[j] <- y_j for the own interior knots j = m-1 .. 1
#pragma unroll
            for (int j = mL - 1; j >= 1; --j) {
                if (j < m) {
#pragma unroll
                    for (int i = 0; i < ND; ++i)
#pragma unroll
                        for (int c = 0; c < ND; ++c)
#pragma unroll
                            for (int ax = 0; ax < NAX; ++ax) {
                                const double src = (j == mL - 1 || j == m - 1) ? ynext[c][ax] : h[j + 1 < mL ? j + 1 : j][c][ax];
                                h[j][i][ax] -= E[j][i][c] * src;
                            }
                }
            }
            double* stage = C::ALIAS ? s_in[buf] : s_out;
            // When the staging rows alias the current input buffer, everything emission still needs from it
            // is pulled into registers first.
            double P_[C::ALIAS ? mL + 1 : 1][3], T_[C::ALIAS ? mL : 1];
            if constexpr (C::ALIAS) {
#pragma unroll
                for (int j = 0; j <= mL; ++j)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) P_[j][ax] = pos(j <= m ? j : m, ax);
#pragma unroll
                for (int j = 0; j < mL; ++j) T_[j] = Tof(j < m ? j : m - 1);
                wave_lds_sync();
            }
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
                for (int q = NQ - 1; q >= 0; --q) {
                    const int cnt = max(0, min((q + 1) * CH, m) - q * CH);  // own segments in this chunk (lane-dependent for odd M)
                    double* row = stage + lane * RS;
#pragma unroll
                    for (int s = 0; s < CH; ++s) {
                        const int j = q * CH + s;  // own segment
                        if (j < mL) {
                            const int jc = j < m ? j : (m > 0 ? m - 1 : 0);
                            double ys[ND], ye[ND], c8[NC];
#pragma unroll
                            for (int d = 0; d < ND; ++d) {
                                const double fs = ((d & 1) == 0) ? -1.0 : 1.0;
                                const double yj = h[j][d][ax];
                                const double yj1 = (j + 1 >= mL || j + 1 == m) ? ynext[d][ax] : h[j + 1 < mL ? j + 1 : j][d][ax];
                                ys[d] = isR ? fs * yj1 : yj;
                                ye[d] = isR ? fs * yj : yj1;
                            }
                            double pa, pb, Tj;
                            if constexpr (C::ALIAS) { pa = P_[j][ax]; pb = P_[j + 1][ax]; Tj = T_[j]; }
                            else { pa = pos(jc, ax); pb = pos(jc + 1, ax); Tj = Town[j]; }
                            segment_coeffs<R>(isR ? pb : pa, ys, isR ? pa : pb, ye, Tj, fast_rcp(Tj), c8);
                            if (j < m) finite = finite && (fabs(c8[NC - 1]) < INFINITY) && (fabs(c8[R]) < INFINITY);
                            // slot in original order: L ascending, R descending within the chunk
                            const int slot = isR ? (cnt - 1 - s) : s;
                            if (s < cnt) {
                                double* so = row + slot * NC;
#pragma unroll
                                for (int k = 0; k < NC; k += 2) *reinterpret_cast<double2*>(so + k) = make_double2(c8[k], c8[k + 1]);
                            }
                        }
                    }
                    wave_lds_sync();
#pragma unroll
                    for (int it = 0; it < PPL; ++it) {
                        // which 16-byte piece a lane copies.  Plain order (lane it*64 + l -> piece l of 8 consecutive rows)
                        // is 2-way conflicted for 128-byte rows at the write-friendly stride of 36 dwords: ds_read_b128
                        // serves the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32) over 64 banks, and the four
                        // half rows a group reads must tile them -- which at 9 bank-quads per row only both halves of
                        // rows rho and rho + 8 do.  So instruction `it` takes rows it + 8 k (k = 0..7), quad q of a
                        // 32-lane half reads half (q >> 1) & 1 of row it + 8 * {0, 2, 2, 0, 3, 1, 1, 3}[q]: every row is
                        // still written out as one complete 128-byte line (SQ_LDS_BANK_CONFLICT 34 % -> see profiles/).
                        int pl, col;
                        if constexpr (PPL == 8 && TILE == 32) {
                            const int kq = (lane >> 2) & 7;
                            pl = it + 8 * ((0xD728 >> (2 * kq)) & 3) + (lane & 32);
                            col = ((kq >> 1) & 1) * 4 + (lane & 3);
                        } else if constexpr (PPL == 12 && TILE == 32) {
                            // 192-byte rows at 52 dwords (13 bank-quads): a read group tiles the banks with the same third
                            // of four rows 4 apart -- instruction `it` copies third it % 3 of rows gamma + 16 (it / 3) + 4 i,
                            // gamma = the lane group, i = the quad's place in it
                            const int kq = lane >> 2, k7 = kq & 7;
                            const int gam = (kq >> 3) * 2 + ((0x96 >> k7) & 1), i4 = k7 >> 1;
                            pl = gam + 16 * (it / 3) + 4 * i4;
                            col = 4 * (it % 3) + (lane & 3);
                        } else {
                            const int g = it * 64 + lane;
                            pl = g / PPL;
                            col = g - pl * PPL;
                        }
                        const int ctl = pl >> 1, cR = pl & 1;
                        const int cm = cR ? mR : mL;
                        const int ccnt = max(0, min((q + 1) * CH, cm) - q * CH);
                        const int first = cR ? (M - q * CH - ccnt) : q * CH;
                        const double2 v = *reinterpret_cast<const double2*>(stage + pl * RS + 2 * col);
                        const bool keep = (2 * col < ccnt * NC) && (ctl < TILE) && ((okmask >> (2 * (ctl < TILE ? ctl : 0))) & 1ull);
                        // (the explicit vmcnt(0) above is a builtin, so the compiler knows no LDS-DMA is pending here
                        //  and a predicated store does not make it re-insert waits before the LDS reads)
                        if (keep) store_pair_wt(out + (((size_t)ctl * 3 + ax) * M + first) * NC + 2 * col, v);
                    }
                    wave_lds_sync();  // rows are rewritten by the next unit: keep the reads above it
                }
            }
        }
        {
            const int f = finite ? 1 : 0;
            const int other = __builtin_amdgcn_mov_dpp(f, 0xB1, 0xF, 0xF, true);
            bool fin = (f & other) != 0;
            if constexpr (LPT >= 8) {  // all axis pairs of the trajectory must be finite
                const unsigned long long fm = __ballot(fin || axl == 3);
                constexpr unsigned long long grp = LPT == 8 ? 0xFFull : 0xFFFFull;
                fin = ((fm >> (LPT * tlc)) & grp) == grp;
            }
            bool okt = ok;
            if constexpr (LPT >= 8) okt = (okmask >> (LPT * tlc)) & 1ull;  // lane 0 of the group is a real axis pair
            if ((lane % LPT) == 0 && tl < nv && a.status) a.status[base + tl] = okt ? (fin ? UAVQP_SOLVED : UAVQP_NON_FINITE) : UAVQP_INVALID_INPUT;
        }
        UAVQP_STAMP(4);
        wave_lds_sync();
    }
