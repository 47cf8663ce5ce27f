// Body of the streaming kernel k_stream<NC, DRIFT> (leap.hip), included INSIDE the kernel and inside its problem-group twin k_stream_group.
// The including kernel provides `pb` (const DevProblem&), `ch`, `cfg`, `parity` and the constants KARGS (its kernel-argument bytes) and CARR: the
// block tasks a workgroup runs side by side -- 1, or 3 in a CARRIER workgroup (k_stream_carrier: 3 x ST_WAVES waves, one workgroup per CU; pack.hip
// fills the carriers by bytes).  Sub-group `sub` = threadIdx.x / 256 of a carrier runs its task on its own four waves with the code, the LDS
// layout (a leading [CARR]) and the partial slots a 256-thread workgroup has for that task; what the sub-groups share is theta' (derived once,
// by the first NC waves of the carrier) and the barriers, which stay workgroup-wide: an empty slot of the table (tix < 0) loads and stores
// nothing but reaches every barrier.  With CARR == 1 every carrier term below is a compile-time constant.
// A textual body and not a force-inlined function: the function form changed the register allocation and wait counts of every existing
// instantiation (a different order of the optimisations around the inlined call); included, k_stream compiles to the instructions it had.
// (no include guard: included once per kernel)
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D, P = DR::P, TB = MAGI_TB;
    WG_TRACE(0, 0);
    // (the "all chains idle" flag is fetched here but tested after the other first loads are on the wire: an early return on it
    //  would put one more dependent round trip in front of every workgroup of every slot)
    const int all_done = ch.gctl->all_done;
    kernarg_prefetch<KARGS>();
    const int c0 = blockIdx.y * NC;
    __shared__ double vcol_s[CARR][NC][TB], vrow_s[CARR][NC][TB], rowout_s[CARR][NC][TB], colacc_s[CARR][ST_WAVES][NC][TB];
    __shared__ double th_s[NC][MAGI_MAX_P];
    const int n_dec = (int)gridDim.x - (CARR == 1 ? pb.n_tasks : pb.n_carriers);        // decision workgroups come FIRST in dispatch order: their one round of
    if ((int)blockIdx.x < n_dec) {                         // loads is then on the wire before the stream saturates the memory system
        if (CARR > 1 && threadIdx.x >= 64 * ST_WAVES) return;      // (the decisions are written for, and sum in the order of, MAGI_TAIL_THREADS threads)
        // ---- the decisions of the previous slot, one workgroup per chain, next to this slot's stream (decide.h) ----
        __shared__ double dsh[25 * 16], dshs[24];
        __shared__ ChainCtl s_ctl;
        __shared__ int s_g[2];
        __shared__ double s_par[PAR_COUNT];
        __shared__ double s_ops[OPS_COUNT * OPS_W];
        __shared__ double s_cst[3 * MAGI_MAX_D];
        const int chain = c0 + (int)blockIdx.x;
        if (chain < ch.n_chains) decide_block<DRIFT>(pb, ch, cfg, chain, parity, all_done, dsh, dshs, &s_ctl, s_g, s_par, s_ops, s_cst);
        return;
    }
    const int sub = CARR == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);      // (wave-uniform: the descriptor stays a scalar load)
    const int t = CARR == 1 ? (int)threadIdx.x : ((int)threadIdx.x & (64 * ST_WAVES - 1)), lane = t & 63, wave = t >> 6;
    double (&vcol)[NC][TB] = vcol_s[sub], (&vrow)[NC][TB] = vrow_s[sub], (&rowout)[NC][TB] = rowout_s[sub];
    double (&colacc)[ST_WAVES][NC][TB] = colacc_s[sub];
    MAGI_STAMPS_DECL(stream, 8);
    MAGI_STAMP(stream, 0);
    // (the descriptor table is read-only for the lifetime of the matrices: fetched through the constant address space it is a
    //  scalar load on its own counter, so waiting for it does not wait for the tile loads issued below and vice versa)
    typedef const int __attribute__((address_space(4))) * const_int_ptr;
    const_int_ptr tk = (const_int_ptr)(unsigned long long)(CARR == 1 ? pb.tasks + 4 * (size_t)((int)blockIdx.x - n_dec)
                                                                     : pb.ctasks + 4 * (size_t)(CARR * ((int)blockIdx.x - n_dec) + sub));
    int4 task;
    task.x = tk[0]; task.y = tk[1]; task.z = tk[2]; task.w = tk[3];
    // a carrier's slot: {ctask_word(block index or -1, "a task of this carrier needs theta'", d), kind word, bi, bj} (magi_internal.h)
    const int tix = CARR == 1 ? (int)blockIdx.x - n_dec : ctask_tile(task.x);
    const bool live = CARR == 1 || tix >= 0;
    // the wave's rows in chunks of 8, two chunks in flight (a0 / a1): 16 KB per wave on the wire while one chunk is in the ALUs.
    // tile loads need nothing but the block index: on the wire before the plan-dependent loads (except in the waves that derive theta')
    // A DEMOTED block (pack.hip: the criterion; workgroup-uniform, known from the descriptor alone) is read from its fp32 copy instead: the wave's
    // strip of 32 rows is 16 KB there -- [row pair][lane][2 rows x 2 columns], tile32_index -- which is exactly the two chunks a wave has in flight:
    // the same sixteen 16-B loads into the same registers (a0 = row pairs 0..7, a1 = 8..15, held as raw bits), no refill round and no walk
    // direction.  Only the addresses differ up to the loop; the loop converts to fp64 on use and runs the same butterflies and accumulators.
    const int s32 = task_slot32(task.y);
    static_assert(ST_RW == 32, "tile32_index lays a block out for 32-row wave strips");
    const double2* A = (s32 ? reinterpret_cast<const double2*>(pb.tiles32 + (size_t)(s32 - 1) * TB * TB + (size_t)(wave * ST_RW) * TB)
                            : reinterpret_cast<const double2*>(pb.tiles + (size_t)(CARR == 1 ? tix : max(tix, 0)) * TB * TB + (size_t)(wave * ST_RW) * TB)) + lane;
    constexpr int NCK = ST_RW / 8;
    // Odd slots walk the wave's row chunks backwards: what a slot read LAST is what the next one reads FIRST, so the tail of the
    // block stream is still in the XCD's L2 (4 MB against 9 MB of blocks per XCD; tools/micro/readshape.hip: 5-15 % on the
    // load-only twin).  Chunk ck of the walk is physical chunk pc(ck); results are summed per PHYSICAL chunk so that they do
    // not depend on the direction.  (Only the one- and two-chain instantiations: four chains have no registers for it.)
    static_assert(NC <= 2, "three or more chains per pass run k_stream_mc");
    constexpr bool ALT = true;
    const int pc0 = (ALT && (parity & 1)) ? NCK - 1 : 0, pcs = (ALT && (parity & 1)) ? -1 : 1;
    const int ld0 = s32 ? 0 : pc0 * 8, ld1 = s32 ? 8 : (pc0 + pcs) * 8;      // first 1-KB line of the two chunks in flight (fp32: the whole strip)
    double2 a0[8], a1[8];
    if ((threadIdx.x >> 6) >= NC && live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) a0[r] = A[(size_t)(ld0 + r) * (TB / 2)];
#pragma unroll
        for (int r = 0; r < 8; ++r) a1[r] = A[(size_t)(ld1 + r) * (TB / 2)];
    }
    __builtin_amdgcn_sched_barrier(0);
    const int d = CARR == 1 ? task.x : ctask_d(task.x), kind = task_kind(task.y), bi = task.z, bj = task.w;
    const bool needth = CARR == 1 ? kind != TK_FH : ctask_theta(task.x);       // workgroup-uniform: some task of the workgroup multiplies f
    const int N = pb.N;

    // What to evaluate for each chain, from the plan the point phase executed LAST (the decisions that complete it run
    // concurrently and may not be read): a leaf -> assume the subtree continues: the speculative state in the other
    // buffer, with theta' derived here exactly as the decisions derive it; a skip-type plan -> the buffer as is.
    const bool isrow = t >= TB;
    const int loc = (isrow ? t - TB : t) & (TB - 1);
    const int gi = (isrow ? bi : bj) * TB + loc;
    const bool wantf = isrow ? (kind != TK_FH) : (kind == TK_FK);
    const double mud = MAGI_SEL_D(pb.mu, d);
    const double tm = point_time<DR>(pb, gi);          // (a time-dependent drift: needs the task alone, on the wire in front of everything the plan decides)
    double xin[NC][D];
    bool act[NC];
    // (small loads first, the tile stream behind them: their wait then does not cover the row loads)
    // (blocks of FH multiply xc on both sides: they need no theta and do not wait for it -- their traffic fills the window
    //  in which the other workgroups derive theta')
    if ((int)(threadIdx.x >> 6) < NC && needth) {
        const int c = wave, cc = min(c0 + c, ch.n_chains - 1);
        const LeafPlan* lp = ch.plan + (size_t)(parity ^ 1) * ch.n_chains + cc;
        const bool derive = lp->active && !lp->skip && lp->leaf;
        double thp = 0.0;
        if (derive) {
            const double* vb = ch.vec + vec_off(pb, cc, 0);
            const double* part = ch.part + (size_t)cc * PART_K * ch.n_wg;
            // (every load of the derivation is issued before the first wait)
            const int e = pb.ND + D + min(lane, P - 1);
            const double qv = (vb + (size_t)(V_Q + lp->cur) * pb.dimp)[e], pv = (vb + (size_t)(V_P + lp->cur) * pb.dimp)[e];
            const double msc = metric_scale(ch, pb.dimp, cc, e);          // (diagonal metric: s of this parameter entry)
            const bool hsup = pb.tsup != nullptr;                         // (supports: the entry's (sign, bound), in the same round of loads)
            const double2 se = ThetaSup::load(pb.tsup, min(lane, P - 1));
            double rows[P];
            part_rows_sum<P>(part, ch.n_wg, PK_TP, lane, rows);
            double tpp = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) if (lane == k) tpp = rows[k];
            if (lane < P) {
                const double ex = m_exp(qv);
                const double sg = ThetaSup::dtheta(hsup, se, ex / (1.0 + ex));      // == par[PAR_SGT] of that state (compute_par_entry)
                double gj = theta_entry_grad(pb.beta_inv, tpp, sg);
                if (pb.prior) gj = theta_entry_grad_prior(gj, Prior::load(pb.prior, D, D + lane), hsup, se, qv, ex, sg);      // (priors: wave-uniform)
                const double qnx = next_entry_pre(pv, qv, lp->hs, lp->eps, gj, msc);
                thp = ThetaSup::theta(hsup, se, qnx, m_log(1.0 + m_exp(qnx)));      // == par'[PAR_TH] (compute_par_entry)
            }
        } else if (lane < P) {
            thp = ch.par[(size_t)cc * PAR_COUNT + PAR_TH + lane];
        }
        if (lane < P) th_s[c][lane] = thp;
        MAGI_STAMP(stream, 1);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int cc = min(c0 + c, ch.n_chains - 1);
        const LeafPlan* lp = ch.plan + (size_t)(parity ^ 1) * ch.n_chains + cc;
        act[c] = (c0 + c < ch.n_chains) && lp->active != 0;
        const int buf = (lp->skip || !lp->leaf) ? lp->cur : (lp->cur ^ 1);
        const double* q = ch.vec + vec_off(pb, cc, V_Q + buf);
#pragma unroll
        for (int dd = 0; dd < D; ++dd) xin[c][dd] = q[dd * N + min(gi, N - 1)];
    }

    if (all_done) return;
    MAGI_STAMPS_ON(decide, if (tix == 0 && t == 0) {
        unsigned long long* st = reinterpret_cast<unsigned long long*>(ch.par + (size_t)c0 * PAR_COUNT + 40 + 11);
        st[1] = __builtin_amdgcn_s_memrealtime();      // [12] first stream workgroup's start
        st[0] = 0ull;                                    // [11] latest stream workgroup end (atomicMax below)
    })
    if ((int)(threadIdx.x >> 6) < NC && live) {                 // (the waves that derived theta' issue their first chunks now)
#pragma unroll
        for (int r = 0; r < 8; ++r) a0[r] = A[(size_t)(ld0 + r) * (TB / 2)];
#pragma unroll
        for (int r = 0; r < 8; ++r) a1[r] = A[(size_t)(ld1 + r) * (TB / 2)];
    }
    __builtin_amdgcn_sched_barrier(0);
    double thv[NC][P];
    MAGI_STAMP(stream, 2);
    if (needth) {
        __syncthreads();             // th_s
        MAGI_STAMP(stream, 3);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int k = 0; k < P; ++k) thv[c][k] = th_s[c][k];
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int k = 0; k < P; ++k) thv[c][k] = 0.0;
    }

#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double xd = xin[c][0];
#pragma unroll
        for (int dd = 1; dd < D; ++dd) if (d == dd) xd = xin[c][dd];
        double val = wantf ? drift_f1_at<DR>(d, xin[c], thv[c], tm) : xd - mud;
        if (gi >= N) val = 0.0;
        if (t < 2 * TB) (isrow ? vrow : vcol)[c][loc] = val;
    }
    __syncthreads();
    MAGI_STAMP(stream, 4);

    constexpr int NACC = ALT ? NCK : 1;            // column accumulators per physical chunk (direction-independent sums)
    double2 vc[NC], cacc[NC][NACC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        vc[c] = *reinterpret_cast<const double2*>(&vcol[c][2 * lane]);
#pragma unroll
        for (int k = 0; k < NACC; ++k) { cacc[c][k].x = 0.0; cacc[c][k].y = 0.0; }
    }
    if (!live) {
        // (an empty slot of a carrier: nothing was loaded and nothing is stored; on to the barrier)
    } else if (s32) {
        // the fp32 copy: physical chunk pk = row pairs 4 pk .. 4 pk + 3 of the strip, already in a0 (pk < 2) / a1; each register pair holds
        // (row 2 k: columns 2 l, 2 l + 1 | row 2 k + 1: the same columns) as four floats.  Converted on use; the products, the butterfly and
        // the per-physical-chunk column sums are the fp64 path's, so the result has no slot parity in it at all.
#pragma unroll
        for (int pk = 0; pk < NCK; ++pk) {
            double2 (&a)[8] = pk < NCK / 2 ? a0 : a1;
            const int row0 = wave * ST_RW + pk * 8;
            double p[NC][8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double2 w = a[(pk & 1) * 4 + j];
                const double e0 = (double)__int_as_float(__double2loint(w.x)), e1 = (double)__int_as_float(__double2hiint(w.x));
                const double o0 = (double)__int_as_float(__double2loint(w.y)), o1 = (double)__int_as_float(__double2hiint(w.y));
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    double2& acc = cacc[c][pk];
                    p[c][2 * j] = fma(e1, vc[c].y, e0 * vc[c].x);
                    const double xe = vrow[c][row0 + 2 * j];
                    acc.x = fma(e0, xe, acc.x);
                    acc.y = fma(e1, xe, acc.y);
                    p[c][2 * j + 1] = fma(o1, vc[c].y, o0 * vc[c].x);
                    const double xo = vrow[c][row0 + 2 * j + 1];
                    acc.x = fma(o0, xo, acc.x);
                    acc.y = fma(o1, xo, acc.y);
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) rowout[c][row0 + (lane >> 3)] = tsum8(p[c], lane);        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double2 tot = cacc[c][0];
#pragma unroll
            for (int k = 1; k < NACC; ++k) { tot.x += cacc[c][k].x; tot.y += cacc[c][k].y; }
            *reinterpret_cast<double2*>(&colacc[wave][c][2 * lane]) = tot;
        }
    } else {
#pragma unroll
    for (int ck = 0; ck < NCK; ++ck) {
        double2 (&a)[8] = (ck & 1) ? a1 : a0;
        const int row0 = wave * ST_RW + (pc0 + pcs * ck) * 8;          // first row of this chunk inside the block
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double p[8];
            double2& acc = cacc[c][ALT ? ck : 0];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const double2 ar = a[r];
                p[r] = fma(ar.y, vc[c].y, ar.x * vc[c].x);
                const double xr = vrow[c][row0 + r];
                acc.x = fma(ar.x, xr, acc.x);
                acc.y = fma(ar.y, xr, acc.y);
            }
            const double s = tsum8(p, lane);
            // all 8 lanes of a group hold the same bits (commutative butterflies): an unconditional store keeps the loop
            // free of branches (with them LLVM sinks the column accumulators behind the loop and the tile stays live)
            rowout[c][row0 + (lane >> 3)] = s;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (ck + 2 < NCK) {
#pragma unroll
            for (int r = 0; r < 8; ++r) a[r] = A[(size_t)((pc0 + pcs * (ck + 2)) * 8 + r) * (TB / 2)];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double2 tot = cacc[c][0];
        if (ALT) {
            // physical chunk order 0, 1, .., NCK - 1 whatever the walk was: walk index of physical chunk k is k (even slots) or NCK - 1 - k
            const bool rev = (parity & 1) != 0;
            tot = rev ? cacc[c][NCK - 1] : cacc[c][0];
#pragma unroll
            for (int k = 1; k < NACC; ++k) {
                const double2 nx = rev ? cacc[c][NCK - 1 - k] : cacc[c][k];
                tot.x += nx.x; tot.y += nx.y;
            }
        }
        *reinterpret_cast<double2*>(&colacc[wave][c][2 * lane]) = tot;
    }
    }       // (fp64 blocks)
    MAGI_STAMP(stream, 5);
    __syncthreads();
    MAGI_STAMP(stream, 6);

    // partials: threads [0, TB) the row-type output (block row bi, slot bj), threads [TB, 2 TB) the
    // column-type output (block row bj, slot bi; the diagonal blocks of FH / FK are complete by rows)
    const int rvec = kind == TK_FH ? TV_HX : kind == TK_FK ? TV_KF : TV_EX;
    const int cvec = kind == TK_FH ? TV_HX : kind == TK_FK ? TV_KF : TV_ETF;
    const bool colout = (kind == TK_FE) || (bi != bj);
    const size_t cstride = (size_t)4 * D * pb.nb * pb.Np;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (!act[c] || t >= 2 * TB || !live) continue;
        double* tp = ch.tpart + (size_t)(c0 + c) * cstride;
        if (!isrow) {
            tp[((size_t)(rvec * D + d) * pb.nb + bj) * pb.Np + bi * TB + loc] = rowout[c][loc];
        } else if (colout) {
            double sum = colacc[0][c][loc];
#pragma unroll
            for (int w = 1; w < ST_WAVES; ++w) sum += colacc[w][c][loc];
            tp[((size_t)(cvec * D + d) * pb.nb + bi) * pb.Np + bj * TB + loc] = sum;
        }
    }
    MAGI_STAMP(stream, 7);
    MAGI_STAMPS_FLUSH(stream, tix == MAGI_STAMP_WG && blockIdx.y == 0 && t == 64 * MAGI_STAMP_WAVE, ch.par, 8);
    MAGI_STAMPS_ON(decide, __syncthreads(); if (t == 0)
        atomicMax(reinterpret_cast<unsigned long long*>(ch.par + (size_t)c0 * PAR_COUNT + 40 + 11), (unsigned long long)__builtin_amdgcn_s_memrealtime());)
