// Body of the point kernel k_point<DRIFT> (leap.hip), included INSIDE the kernel and inside its problem-group twin k_point_group, for the
// reason leap_stream_body.h gives.  The including kernel provides `pb` (const DevProblem&), `ch`, `parity` and the constant KARGS.
// (no include guard: included once per kernel)
    __shared__ double res[PointRes<DRIFT>::N];
    __shared__ double redk[64 * PART_K];
    __shared__ double s_mu[MAGI_MAX_D];
    __shared__ double s_x[PT_POINTS * PT_DSLOT];
    WG_TRACE(1, 0);
    // (flag and plan are fetched together and combined arithmetically: `a || b` would fetch b only after a has arrived --
    //  one more dependent round trip at the head of a 5 us kernel)
    const int all_done = ch.gctl->all_done;
    const LeafPlan lp = ch.plan[(size_t)parity * ch.n_chains + blockIdx.y];
    kernarg_prefetch<KARGS>();
    if (all_done != 0) return;
    if (lp.vop != 0) { boundary_block<DRIFT>(pb, ch, lp, blockIdx.y, blockIdx.x, redk, s_mu, s_x, parity ^ 1); return; }     // a subtree / transition end (decide.h)
    const int gate = (lp.active ^ 1) | lp.skip;
    if (gate != 0) return;
    if constexpr (DriftT<DRIFT>::SEP) {
        if (ch.sep) { point_block_sep<DRIFT>(pb, ch, lp, blockIdx.y, blockIdx.x, res, redk, s_mu, s_x, parity ^ 1); return; }
    }
    point_block<DRIFT>(pb, ch, lp, blockIdx.y, blockIdx.x, res, redk, s_mu, parity ^ 1);
