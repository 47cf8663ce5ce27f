// extern "C" entry points of libmagi_hip.so (see include/magi_hip.h for the contract).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "magi_internal.h"

thread_local std::string g_magi_last_error;

int magi_fail(magi_handle* h, int code, const std::string& msg) {
    g_magi_last_error = msg;
    if (h) h->err = msg;
    return code;
}

namespace {

// leapfrog slots per captured graph (even: a graph starts at slot parity 0).  MAGI_GRAPH_SLOTS overrides it for experiments.
int graph_slots() {
    static const int n = [] {
        const char* e = getenv("MAGI_GRAPH_SLOTS");
        int v = e ? atoi(e) : 128;     // 32 / 64 / 128 / 256 slots: 107.7 / 108.9 / 109.7 / 109.9 samples/s at config 2 (graph boundaries + control-block snapshot;
                                       // round 4, one box); a run wastes at most one graph of early-exit slots at its end
        v = std::max(2, std::min(v, 4096));
        return v & ~1;
    }();
    return n;
}
#define kGraphSlots graph_slots()

void free_dev(void* p) { if (p) (void)hipFree(p); }

void free_matrices(magi_handle* h) {
    free_dev(h->dCsym); free_dev(h->dM); free_dev(h->dMt); free_dev(h->dKsym); free_dev(h->dYobs);
    magi_model_default(h->pb, &h->model);          // (frees dObsw)
    free_dev(h->dTimes);
    h->dTimes = nullptr; h->times_N = 0; h->times_cap = 0; h->pb.tgrid = nullptr;
    free_dev(h->dTiles); free_dev(h->dTasks); free_dev(h->dTiles32);
    for (int k = 0; k < 3; ++k) { free_dev(h->dDense[k]); h->dDense[k] = nullptr; }
    h->dense_N = h->dense_D = 0;
    for (int k = 0; k < magi_handle::WS_COUNT; ++k) { free_dev(h->ws[k]); h->ws[k] = nullptr; h->ws_cap[k] = 0; }
    h->dCsym = h->dM = h->dMt = h->dKsym = h->dYobs = nullptr;
    h->dTiles = nullptr; h->dTasks = nullptr; h->dTiles32 = nullptr;
    h->tiles_cap = h->tasks_cap = h->tiles32_cap = 0;
    h->n_demoted = 0; h->pb.tiles32 = nullptr;
    h->pb.ctasks = nullptr; h->pb.n_carriers = 0; h->carrier_units.clear(); h->carrier_slots.clear(); h->carrier_table.clear();
    h->have_matrices = h->have_problem = false;
}

void free_chains(magi_handle* h) {
    DevChains& c = h->ch;
    free_dev(c.vec); free_dev(c.ctl); free_dev(c.par); free_dev(c.plan); free_dev(c.part); free_dev(c.tpart); free_dev(c.xop); free_dev(c.vop); free_dev(c.gctl); free_dev(c.samples);
    free_dev(c.d_step_size); free_dev(c.d_lar); free_dev(c.d_target); free_dev(c.d_energy); free_dev(c.d_beta);
    free_dev(c.d_leapfrogs); free_dev(c.d_depth); free_dev(c.d_flags);
    free_dev(h->d_chain_ids); free_dev(h->d_fin);
    free_dev(h->d_scale); free_dev(h->d_macc); free_dev(h->d_mwork);
    c = DevChains{};
    h->d_chain_ids = nullptr; h->d_fin = nullptr;
    h->d_scale = h->d_macc = h->d_mwork = nullptr;
    h->window_k0.clear();
    h->cap_chains = 0; h->n_chains = 0; h->samples_cap = 0; h->diag_cap = 0; h->tpart_elems = 0; h->vop_elems = 0;
}

// host <-> device state layout: host X[N][D] row-major  <->  device comp-major [D][N] | sig | th
void pack_state(const DevProblem& pb, const double* X, const double* sp, const double* tp, double* q) {
    for (int d = 0; d < pb.D; ++d)
        for (int i = 0; i < pb.N; ++i) q[(size_t)d * pb.N + i] = X[(size_t)i * pb.D + d];
    for (int d = 0; d < pb.D; ++d) q[pb.ND + d] = sp[d];
    for (int p = 0; p < pb.P; ++p) q[pb.ND + pb.D + p] = tp[p];
    for (int e = pb.dim; e < pb.dimp; ++e) q[e] = 0.0;
}

void unpack_state(const DevProblem& pb, const double* q, double scale, double* X, double* sp, double* tp) {
    if (X)
        for (int d = 0; d < pb.D; ++d)
            for (int i = 0; i < pb.N; ++i) X[(size_t)i * pb.D + d] = scale * q[(size_t)d * pb.N + i];
    if (sp) for (int d = 0; d < pb.D; ++d) sp[d] = scale * q[pb.ND + d];
    if (tp) for (int p = 0; p < pb.P; ++p) tp[p] = scale * q[pb.ND + pb.D + p];
}

int upload_states(magi_handle* h, int n, const double* X, const double* sp, const double* tp) {
    const DevProblem& pb = h->pb;
    std::vector<double> q((size_t)pb.dimp);
    for (int c = 0; c < n; ++c) {
        pack_state(pb, X + (size_t)c * pb.ND, sp + (size_t)c * pb.D, tp + (size_t)c * pb.P, q.data());
        for (int e = 0; e < pb.dim; ++e)
            if (std::isnan(q[e])) return magi_fail(h, MAGI_E_NAN, "NaN in the initial state of chain " + std::to_string(c));
        MAGI_HIP_CHECK(h, hipMemcpy(h->ch.vec + vec_off(pb, c, V_Q), q.data(), sizeof(double) * pb.dimp, hipMemcpyHostToDevice));
    }
    return MAGI_OK;
}

int build_graph(magi_handle* h) {
    magi_stale(h, STALE_GRAPH);
    MAGI_HIP_CHECK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    int rc = MAGI_OK;
    for (int s = 0; s < kGraphSlots && rc == MAGI_OK; ++s) {          // kGraphSlots is even: a graph starts at slot parity 0
        rc = magi_launch_stream(h, h->n_chains, s & 1, true, h->stream);
        if (rc == MAGI_OK) rc = magi_launch_point(h, h->n_chains, s & 1, h->stream);
    }
    hipError_t e = hipStreamEndCapture(h->stream, &h->graph);
    if (rc != MAGI_OK) return rc;
    if (e != hipSuccess) return magi_fail(h, MAGI_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    MAGI_HIP_CHECK(h, hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
    h->graph_valid = true;
    h->graph_slots = kGraphSlots;
    return MAGI_OK;
}

// The options of a handle (MagiOptions), one row each: the name magi_set_option takes, the environment variable magi_create reads
// (none for the test hook slot_budget_graphs: it must not be reachable from a job's environment), the rule of a value, the member.
//   RANGE   a number in [lo, hi]: magi_set_option rejects any other value, a variable outside it keeps the default
//   CLAMP   a number, clamped to [lo, hi]
//   ONE     on when the value is 1;  FLAG  on when it is non-zero (a variable: when it is present, whatever its value)
//   FAMILY  as RANGE; the variable: "mc" -> 1, "valu" -> 2, anything else 0
enum OptRule { RANGE, CLAMP, ONE, FLAG, FAMILY };
struct OptRow { const char *name, *env; OptRule rule; int64_t lo, hi; void (*store)(MagiOptions&, int64_t); };
template <auto M> void store(MagiOptions& o, int64_t v) { o.*M = (std::remove_reference_t<decltype(o.*M)>)v; }
const OptRow kOptions[] = {
    {"stream_family",       "MAGI_STREAM_FAMILY",       FAMILY, 0, 2,         store<&MagiOptions::stream_family>},
    {"family_chains",       "MAGI_FAMILY_CHAINS",       RANGE,  0, 4096,      store<&MagiOptions::family_chains>},
    {"sep_pair_min",        "MAGI_SEP_PAIR_MIN",        CLAMP,  0, 1 << 30,   store<&MagiOptions::sep_pair_min>},
    {"fused_parity",        "MAGI_FUSED_PARITY",        ONE,    0, 1,         store<&MagiOptions::fused_parity>},
    {"gemm_remap_min",      "MAGI_GEMM_REMAP_MIN",      CLAMP,  0, 1 << 30,   store<&MagiOptions::gemm_remap_min>},
    {"potrf_panels",        "MAGI_POTRF_PANELS",        RANGE,  1, 16,        store<&MagiOptions::potrf_panels>},
    {"potrf_lookahead_min", "MAGI_POTRF_LOOKAHEAD_MIN", RANGE,  0, INT64_MAX, store<&MagiOptions::potrf_lookahead_min>},
    {"no_graph",            "MAGI_NO_GRAPH",            FLAG,   0, 1,         store<&MagiOptions::no_graph>},
    {"fit_host_loop",       "MAGI_FIT_HOST_LOOP",       FLAG,   0, 1,         store<&MagiOptions::fit_host_loop>},
    {"build_profile",       "MAGI_BUILD_PROFILE",       FLAG,   0, 1,         store<&MagiOptions::build_profile>},
    {"build_serial",        "MAGI_BUILD_SERIAL",        FLAG,   0, 1,         store<&MagiOptions::build_serial>},
    {"slot_budget_graphs",  nullptr,                    CLAMP,  0, INT64_MAX, store<&MagiOptions::slot_budget_graphs>},
};

// false (the option unchanged) for a RANGE / FAMILY value out of bounds
bool set_option(MagiOptions& o, const OptRow& r, int64_t v) {
    if ((r.rule == RANGE || r.rule == FAMILY) && (v < r.lo || v > r.hi)) return false;
    r.store(o, r.rule == CLAMP ? std::clamp(v, r.lo, r.hi) : r.rule == ONE ? v == 1 : r.rule == FLAG ? v != 0 : v);
    return true;
}

// calls that need matrices of their own (magi_hip.h: magi_group_create)
int refuse_group(magi_handle* h, const char* what) {
    return magi_fail(h, MAGI_E_STATE, std::string(what) + " needs a handle with matrices of its own: this handle is a problem group (magi_group_create)");
}

// Operator bytes one launch of streaming kernel k reads: every block as 128 x 128 doubles, except that the VALU kernels read the
// demoted blocks' fp32 copies (pack.hip); the matrix-core kernels read the fp64 entries of every block.
double block_bytes(const magi_handle* h, StreamKernel k) {
    const bool narrow = k == StreamKernel::Valu1 || k == StreamKernel::Valu2;
    return ((double)h->pb.n_tasks * 8.0 - (narrow ? (double)h->n_demoted * 4.0 : 0.0)) * MAGI_TB * MAGI_TB;
}

// "" when handle m can join a group whose shape is `ref`, else why not
std::string member_mismatch(const DevProblem& ref, const magi_handle* m) {
    if (!m->have_matrices || !m->have_problem) return "has no problem set (magi_set_matrices / magi_build_matrices, then magi_set_problem)";
    // (what the caller chose first, then what follows from it)
    const DevProblem& p = m->pb;
    const struct { const char* name; int a, b; } f[] = {
        {"N", p.N, ref.N}, {"D", p.D, ref.D}, {"P", p.P, ref.P}, {"drift", p.drift, ref.drift}, {"band", p.band, ref.band}, {"ld", p.ld, ref.ld},
        {"n_tasks", p.n_tasks, ref.n_tasks}, {"nb", p.nb, ref.nb}, {"Np", p.Np, ref.Np}, {"wb", p.wb, ref.wb}, {"bandf", p.bandf, ref.bandf},
        {"dim", p.dim, ref.dim}, {"dimp", p.dimp, ref.dimp}};
    for (const auto& x : f)
        if (x.a != x.b) return std::string("differs in shape: ") + x.name + " = " + std::to_string(x.a) + ", the first member's is " + std::to_string(x.b);
    return "";
}

// The members as they stand now, for n_chains = G x per: each has a problem of the group's shape and its own rule puts `per` chains on a
// VALU streaming kernel; their problems go to the device table the group kernels read.
int group_refresh(magi_handle* h, int n_chains) {
    const int G = h->group_n;
    if (n_chains <= 0 || n_chains % G != 0)
        return magi_fail(h, MAGI_E_BADARG, "n_chains = " + std::to_string(n_chains) + " is not a positive multiple of the group's " + std::to_string(G) + " members");
    const int per = n_chains / G;
    std::vector<DevProblem> tab(G);
    for (int m = 0; m < G; ++m) {
        const magi_handle* s = h->members[m];
        const std::string why = member_mismatch(h->pb, s);
        if (!why.empty()) return magi_fail(h, MAGI_E_BADARG, "group member " + std::to_string(m) + " " + why);
        const StreamKernel k = magi_stream_kernel(s, per);
        if (k != StreamKernel::Valu1 && k != StreamKernel::Valu2)
            return magi_fail(h, MAGI_E_BADARG, "group member " + std::to_string(m) + " would stream " + std::to_string(per) +
                                               " chains on a matrix-core kernel (its problem size or its option stream_family): a group runs the VALU kernels only");
        tab[m] = s->pb;
        if (s->stream) MAGI_HIP_CHECK(h, hipStreamSynchronize(s->stream));       // (the member's matrices are complete)
    }
    MAGI_HIP_CHECK(h, hipMemcpy(h->d_members, tab.data(), sizeof(DevProblem) * G, hipMemcpyHostToDevice));
    h->group_per = per;
    return MAGI_OK;
}

// The shared tail of magi_set_times and the three model setters, behind their validation: nothing in flight reads the old table; the sampler
// level is raised before anything can fail; then, unless the table is `plain` (the default, which the kernels serve without a table), n entries
// go to dbuf, grown to them first.  cap: dbuf's capacity (the times), or none for a table of one fixed size that is allocated once.
template <typename T>
int model_upload(magi_handle* h, const T* tab, size_t n, T*& dbuf, size_t* cap, bool plain) {
    if (h->stream) MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    magi_stale(h, STALE_SAMPLER);
    if (plain) return MAGI_OK;
    size_t once = dbuf ? n : 0;
    if (int rc = magi_grow(h, dbuf, cap ? *cap : once, n, "model table")) return rc;
    MAGI_HIP_CHECK(h, hipMemcpy(dbuf, tab, n * sizeof(T), hipMemcpyHostToDevice));
    return MAGI_OK;
}

}  // namespace

void magi_options_from_env(MagiOptions& o) {
    for (const OptRow& r : kOptions)
        if (const char* e = r.env ? getenv(r.env) : nullptr)
            (void)set_option(o, r, r.rule == FLAG ? 1 : r.rule == FAMILY ? (!strcmp(e, "mc") ? 1 : !strcmp(e, "valu") ? 2 : 0) : atoll(e));
    // the storage switch of csrc/pack.hip (below, magi_set_option: no row of the table): 0 or 1, any other value keeps the default
    if (const char* e = getenv("MAGI_TILE_DEMOTE"))
        if (!strcmp(e, "0") || !strcmp(e, "1")) o.tile_demote = e[0] - '0';
    // likewise the launch shape of the VALU streaming kernels (csrc/pack.hip: carriers): -1, 0 or 1
    if (const char* e = getenv("MAGI_STREAM_CARRIERS"))
        if (!strcmp(e, "-1") || !strcmp(e, "0") || !strcmp(e, "1")) o.stream_carriers = atoi(e);
}

// What makes which state of a handle stale.  Every level includes the ones before it; the call, the level it raises, and why -- the code's
// counterpart of the sentences of include/magi_hip.h ("forget the problem", "invalidates the sampler state and the captured graph"):
//
//   call                                                    level     why
//   build_graph                                             GRAPH     the old graph goes before the new capture
//   magi_ensure_chains: another chain count / kernel        GRAPH     grid sizes and the kernel are baked into the graph
//   magi_sampler_set_metric / _metric_window / _adapt_metric GRAPH    ch.scale / ch.macc change between null and non-null: kernel arguments
//   magi_logpost_grad*, magi_time_gradient, _debug_wg_trace SAMPLER   they evaluate in the chains' buffers: the sampler's state is clobbered
//   magi_sampler_init (behind magi_ensure_chains)           SAMPLER   cfg and the output buffers are kernel arguments, the chains are set up anew;
//                                                                     sampler_ready is set at the call's end, the only place that sets it
//   magi_sampler_profile (at its end)                       SAMPLER   the chains stand inside a transition
//   magi_sampler_run: slot budget exhausted                 SAMPLER   a corrupted control block
//   magi_set_times / _theta_support / _prior / _obs_model   SAMPLER   "invalidates the sampler state and the captured graph": the problem, pointers
//     (model_upload)                                                  included, is a kernel argument by value
//   magi_pack_matrices at an unchanged (N, D)               SAMPLER   "the sampler state and the captured graph are invalidated either way"; problem
//     (magi_pack_resident, magi_build_matrices)                       and model stay (have_matrices is down while it works)
//   magi_ensure_chains: more chains than there is room for  CHAINS    the block is released and allocated as a whole
//   magi_destroy                                            CHAINS    (then free_matrices)
//   magi_set_problem                                        PROBLEM   the old problem is forgotten first (dimp may change: the chains go), the model
//                                                                     reset; have_problem is set again at the call's end
//   magi_pack_matrices at another (N, D)                    MATRICES  yobs and dim depend on N, D: "so do magi_build_matrices and magi_pack_resident
//                                                                     when N or D change"
//   magi_set_matrices, magi_build_dense                     MATRICES  "forget the problem, whatever the shape"; the packed operands describe the OLD
//                                                                     dense stacks until a pack has succeeded
//   magi_sampler_ppc, magi_ppc                              none      they read the samples, the problem and its model in place; the scratch is
//                                                                     the call's own (MagiScratch) and the noise has a Philox stream of its own
//   magi_sampler_rank_diagnostics, magi_rank_diagnostics    none      they read the samples and the member's bounds, supports and priors in place;
//                                                                     the scratch is the call's own (MagiScratch)
//   magi_sampler_sensitivities, magi_ode_sensitivities      none      the first reads the samples, the problem's observations and the member's
//                                                                     bounds, supports and priors in place; the scratch is the call's own (MagiScratch)
//
// "SAMPLER includes GRAPH" drops a graph that some of these calls could have kept (the log-posterior and timing calls, the end of
// magi_sampler_profile, the budget exit).  That cannot be observed: a graph is replayed by magi_sampler_run alone, which needs sampler_ready,
// which magi_sampler_init alone sets -- behind its own raise of the level.  Likewise the chains and the model go where the problem is
// forgotten, not at the magi_set_problem that has to follow: the chains hold nothing a call accepts without a problem, and magi_set_problem
// releases them and resets the model whatever it finds.  magi_sampler_init raises its level before its first step that can fail: a failed
// initialisation leaves a sampler that is not ready, not the previous run over buffers the failed call has already rewritten.
void magi_stale(magi_handle* h, MagiStale level) {
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->graph) (void)hipGraphDestroy(h->graph);
    h->graph_exec = nullptr; h->graph = nullptr; h->graph_valid = false;
    if (level >= STALE_SAMPLER) h->sampler_ready = false;
    if (level >= STALE_CHAINS) free_chains(h);
    if (level >= STALE_PROBLEM) { h->have_problem = false; magi_model_default(h->pb, &h->model); }
    if (level >= STALE_MATRICES) h->have_matrices = false;
}

double* magi_workspace(magi_handle* h, int k, size_t n) {
    return magi_grow(h, h->ws[k], h->ws_cap[k], n, "work space") == MAGI_OK ? h->ws[k] : nullptr;
}

int magi_ensure_chains(magi_handle* h, int n) {
    if (!h->group_n && (!h->have_matrices || !h->have_problem)) return magi_fail(h, MAGI_E_STATE, "set matrices and problem first");
    if (n <= 0 || n > 4096) return magi_fail(h, MAGI_E_BADARG, "n_chains out of range");
    if (n > h->cap_chains) {
        magi_stale(h, STALE_CHAINS);     // (all null and cap_chains 0 before the first allocation, cap_chains set behind the last: the next call cleans up a failure)
        DevChains& c = h->ch;
        const DevProblem& pb = h->pb;
        auto zeroed = [h](auto*& p, size_t elems) {
            MAGI_HIP_CHECK(h, hipMalloc(reinterpret_cast<void**>(&p), sizeof(*p) * elems));
            MAGI_HIP_CHECK(h, hipMemset(p, 0, sizeof(*p) * elems));
            return (int)MAGI_OK;
        };
        c.n_wg = magi_leap_wgs(pb);
        h->tpart_elems = std::max(magi_sep_tpart_elems(pb, n), (size_t)n * 4 * pb.D * pb.nb * pb.Np);      // the larger of the two streaming paths' layouts
        h->vop_elems = magi_drift_separable(pb.drift) ? magi_sep_vop_elems(pb, n) : 16;
        int rc;
        if ((rc = zeroed(c.vec, (size_t)n * V_COUNT * pb.dimp)) || (rc = zeroed(c.ctl, (size_t)n)) || (rc = zeroed(c.par, (size_t)PAR_COUNT * n)) ||
            (rc = zeroed(c.plan, (size_t)2 * n)) || (rc = zeroed(c.part, (size_t)PART_K * c.n_wg * n)) ||
            (rc = zeroed(c.tpart, h->tpart_elems)) ||                                     // slots outside the block band stay zero
            (rc = zeroed(c.xop, (size_t)2 * ((n + 15) / 16) * pb.D * pb.Np * 16)) || (rc = zeroed(c.vop, h->vop_elems)) || (rc = zeroed(c.gctl, (size_t)1)))
            return rc;
        MAGI_HIP_CHECK(h, hipMalloc(&h->d_chain_ids, sizeof(long long) * n));
        MAGI_HIP_CHECK(h, hipMalloc(&h->d_fin, sizeof(double) * 8 * n));
        h->cap_chains = n;
    }
    const StreamKernel k = magi_stream_kernel(h, n);
    if (h->n_chains != n || k != h->stream_kernel) magi_stale(h, STALE_GRAPH);
    if (h->n_chains != n && h->ch.vop)       // the mirror's layout depends on the chain count: entries the new layout never writes must read zero
        MAGI_HIP_CHECK(h, hipMemsetAsync(h->ch.vop, 0, sizeof(double) * h->vop_elems, h->stream));
    h->n_chains = n;
    h->ch.n_chains = n;
    h->stream_kernel = k;
    const bool sepk = k == StreamKernel::Sep8 || k == StreamKernel::Sep16;
    if ((h->ch.sep != 0) != sepk && h->ch.tpart)      // the two streaming paths lay tpart out differently: slots the new one never writes must read zero
        MAGI_HIP_CHECK(h, hipMemsetAsync(h->ch.tpart, 0, sizeof(double) * h->tpart_elems, h->stream));
    h->ch.sep = sepk ? 1 : 0;
    h->ch.mc = k == StreamKernel::Mc ? 1 : 0;
    return MAGI_OK;
}

// the one place that knows which drift ids this library serves.  hint: the message says where a traced drift's library comes from
int magi_check_drift_id(magi_handle* h, int drift_id, bool hint) {
#ifdef MAGI_USER_DRIFT_HEADER
    if (drift_id != MAGI_DRIFT_USER) return magi_fail(h, MAGI_E_BADARG, "this library is specialised for a traced f_vec: drift id must be MAGI_DRIFT_USER");
#else
    if (drift_id < MAGI_DRIFT_SEIR3 || drift_id > MAGI_DRIFT_SIRW)
        return magi_fail(h, MAGI_E_BADARG, std::string("unknown drift id") + (hint ? " (a traced f_vec needs its own library: magi_v2_amd.jit)" : ""));
#endif
    return MAGI_OK;
}

extern "C" {

const char* magi_version(void) { return "magi_hip 0.1.0 gfx950"; }

int magi_user_drift_info(int* D, int* P) {
#ifdef MAGI_USER_DRIFT_HEADER
    if (D) *D = MAGI_USER_D;
    if (P) *P = MAGI_USER_P;
    return 1;
#else
    (void)D; (void)P;
    return 0;
#endif
}

int magi_user_drift_time_dependent(void) {
#ifdef MAGI_USER_DRIFT_HEADER
    return DriftT<MAGI_DRIFT_USER>::TDEP ? 1 : 0;
#else
    return 0;
#endif
}

const char* magi_last_error(const magi_handle* h) { return h ? h->err.c_str() : g_magi_last_error.c_str(); }

magi_handle* magi_create(int device_id) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_magi_last_error = std::string("no HIP device available: ") + hipGetErrorString(e);
        return nullptr;
    }
    if (device_id < 0 || device_id >= ndev) {
        g_magi_last_error = "device_id out of range";
        return nullptr;
    }
    if ((e = hipSetDevice(device_id)) != hipSuccess) {
        g_magi_last_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return nullptr;
    }
    magi_handle* h = new magi_handle();
    h->device = device_id;
    magi_options_from_env(h->opt);
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipHostMalloc((void**)&h->h_gctl, sizeof(GlobalCtl) * 4, hipHostMallocDefault)) != hipSuccess) {
        g_magi_last_error = std::string("handle setup: ") + hipGetErrorString(e);
        delete h;
        return nullptr;
    }
    for (int i = 0; i < 4; ++i) (void)hipEventCreateWithFlags(&h->ev[i], hipEventDisableTiming);
    (void)hipEventCreate(&h->ev_t0);
    (void)hipEventCreate(&h->ev_t1);
    h->carrier_fits = magi_carrier_one_per_cu();          // (an occupancy query of the carrier kernels, asked once: pack.hip's eligibility)
    return h;
}

void magi_destroy(magi_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    magi_stale(h, STALE_CHAINS);
    free_matrices(h);
    free_dev(h->d_members);          // (a group's members are the caller's)
    free_dev(h->model.dTsup);
    free_dev(h->model.dPrior);
    for (int i = 0; i < 4; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    if (h->ev_t0) (void)hipEventDestroy(h->ev_t0);
    if (h->ev_t1) (void)hipEventDestroy(h->ev_t1);
    if (h->h_gctl) (void)hipHostFree(h->h_gctl);
    if (h->apply_pin) (void)hipHostFree(h->apply_pin);
    for (int i = 0; i < 3; ++i) if (h->ev_la[i]) (void)hipEventDestroy(h->ev_la[i]);
    if (h->stream_chain) (void)hipStreamDestroy(h->stream_chain);
    for (int i = 0; i < 4; ++i) if (h->ev_pw[i]) (void)hipEventDestroy(h->ev_pw[i]);
    if (h->prof.e0) (void)hipEventDestroy(h->prof.e0);
    if (h->prof.e1) (void)hipEventDestroy(h->prof.e1);
    if (h->stream_trail) (void)hipStreamDestroy(h->stream_trail);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int magi_group_create(magi_handle* const* members, int n_members, magi_handle** out) {
    if (out) *out = nullptr;
    if (!members || !out || n_members < 1 || n_members > 4096) return magi_fail(nullptr, MAGI_E_BADARG, "magi_group_create: need 1 to 4096 members and an out pointer");
    for (int m = 0; m < n_members; ++m) {
        const magi_handle* s = members[m];
        if (!s) return magi_fail(nullptr, MAGI_E_BADARG, "group member " + std::to_string(m) + " is NULL");
        if (s->group_n) return magi_fail(nullptr, MAGI_E_BADARG, "group member " + std::to_string(m) + " is itself a group");
        if (s->device != members[0]->device)
            return magi_fail(nullptr, MAGI_E_BADARG, "group member " + std::to_string(m) + " is on device " + std::to_string(s->device) + ", the first member on " +
                                                     std::to_string(members[0]->device));
        const std::string why = member_mismatch(members[0]->pb, s);
        if (!why.empty()) return magi_fail(nullptr, MAGI_E_BADARG, "group member " + std::to_string(m) + " " + why);
    }
    magi_handle* g = magi_create(members[0]->device);
    if (!g) return MAGI_E_HIP;                    // (magi_create has set the message)
    g->group_n = n_members;
    g->members.assign(members, members + n_members);
    g->pb = members[0]->pb;                        // the shape; the data of every member is read from the device table
    g->pb.Csym = g->pb.M = g->pb.Mt = g->pb.Ksym = g->pb.yobs = g->pb.tiles = nullptr;
    g->pb.tasks = g->pb.stasks = nullptr;
    g->pb.tiles32 = nullptr;
    g->pb.tgrid = nullptr;
    magi_model_default(g->pb, nullptr);            // (every member brings its own supports, priors and observation model)
    size_t cap = 0;
    const int rc = magi_grow(g, g->d_members, cap, (size_t)n_members, "group table");      // (the message stays in magi_last_error(NULL))
    if (rc) magi_destroy(g);
    else *out = g;
    return rc;
}

int magi_set_matrices(magi_handle* h, int N, int D, int bandsize, const double* C_inv, const double* m,
                      const double* K_inv) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_set_matrices");
    if (!C_inv || !m || !K_inv) return magi_fail(h, MAGI_E_BADARG, "null matrix pointer");
    if (N < 2 || D < 1 || D > MAGI_MAX_D) return magi_fail(h, MAGI_E_BADARG, "need N >= 2 and 1 <= D <= " + std::to_string(MAGI_MAX_D));
    (void)hipSetDevice(h->device);
    magi_stale(h, STALE_MATRICES);     // the packed operands describe the OLD dense stacks until the pack below has succeeded
    const size_t bytes = (size_t)D * N * N * sizeof(double);
    int rc = magi_ensure_dense(h, N, D);
    if (rc) return rc;
    MAGI_HIP_CHECK(h, hipMemcpy(h->dDense[0], C_inv, bytes, hipMemcpyHostToDevice));
    MAGI_HIP_CHECK(h, hipMemcpy(h->dDense[1], m, bytes, hipMemcpyHostToDevice));
    MAGI_HIP_CHECK(h, hipMemcpy(h->dDense[2], K_inv, bytes, hipMemcpyHostToDevice));
    rc = magi_pack_matrices(h, N, D, bandsize, h->dDense[0], h->dDense[1], h->dDense[2]);
    (void)hipStreamSynchronize(h->stream);
    return rc;
}

int magi_build_dense(magi_handle* h, const double* I, int N, int D, int n_sel, const int32_t* sel, const double* phi1, const double* phi2, double nu) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_build_dense");
    if (!I || !sel || !phi1 || !phi2) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    if (N < 2 || D < 1 || D > MAGI_MAX_D || n_sel < 1 || n_sel > D) return magi_fail(h, MAGI_E_BADARG, "need N >= 2, 1 <= D <= " + std::to_string(MAGI_MAX_D) + " and 1 <= n_sel <= D");
    if (!(nu > 1.0)) return magi_fail(h, MAGI_E_BADARG, "nu must exceed 1 (once-differentiable Matern)");
    (void)hipSetDevice(h->device);
    magi_stale(h, STALE_MATRICES);     // the packed operands no longer match the dense stacks until magi_pack_resident
    std::vector<int> s(sel, sel + n_sel);
    return magi_build_dense_device(h, I, N, D, n_sel, s.data(), phi1, phi2, nu);
}

int magi_pack_resident(magi_handle* h, int bandsize) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_pack_resident");
    if (!h->dDense[0] || h->dense_N <= 0) return magi_fail(h, MAGI_E_STATE, "no resident matrices: build or set them first");
    (void)hipSetDevice(h->device);
    int rc = magi_pack_matrices(h, h->dense_N, h->dense_D, bandsize, h->dDense[0], h->dDense[1], h->dDense[2]);
    (void)hipStreamSynchronize(h->stream);
    return rc;
}

int magi_get_dense(magi_handle* h, int bandsize, double* C_inv, double* m, double* K_inv) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_get_dense");
    if (!h->dDense[0] || h->dense_N <= 0) return magi_fail(h, MAGI_E_STATE, "no resident matrices");
    (void)hipSetDevice(h->device);
    const int N = h->dense_N, D = h->dense_D;
    const size_t nn = (size_t)N * N;
    double* outs[3] = {C_inv, m, K_inv};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        MAGI_HIP_CHECK(h, hipMemcpy(outs[k], h->dDense[k], nn * D * sizeof(double), hipMemcpyDeviceToHost));
        if (bandsize >= 0)           // tf.linalg.band_part(., b, b), magi_v2.py:271-274
            for (int d = 0; d < D; ++d)
                for (int i = 0; i < N; ++i) {
                    double* row = outs[k] + (size_t)d * nn + (size_t)i * N;
                    for (int j = 0; j < std::min(N, i - bandsize); ++j) row[j] = 0.0;
                    for (int j = std::max(0, i + bandsize + 1); j < N; ++j) row[j] = 0.0;
                }
    }
    return MAGI_OK;
}

int magi_dense_apply(magi_handle* h, int which, int transpose, int nv, const double* V, double* Y) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_dense_apply");
    if (!h->dDense[0] || h->dense_N <= 0) return magi_fail(h, MAGI_E_STATE, "no resident matrices");
    if (which < 0 || which > 2 || nv < 1 || nv > 8 || !V || !Y) return magi_fail(h, MAGI_E_BADARG, "which in 0..2, 1 <= nv <= 8, non-null vectors");
    (void)hipSetDevice(h->device);
    // (called 2 x 10 000 times by the theta initialiser's general branch: device scratch and pinned staging are kept in the handle
    //  -- grow-only -- and the copies ride on the handle's stream: one synchronisation per call, no allocation)
    const size_t n = (size_t)h->dense_D * h->dense_N * nv;
    double* dV = magi_workspace(h, magi_handle::WS_APPLY, 2 * n);
    if (!dV) return MAGI_E_HIP;
    double* dY = dV + n;
    if (2 * n > h->apply_pin_cap) {
        if (h->apply_pin) (void)hipHostFree(h->apply_pin);
        h->apply_pin = nullptr; h->apply_pin_cap = 0;
        MAGI_HIP_CHECK(h, hipHostMalloc((void**)&h->apply_pin, 2 * n * sizeof(double), hipHostMallocDefault));
        h->apply_pin_cap = 2 * n;
    }
    std::memcpy(h->apply_pin, V, n * sizeof(double));
    MAGI_HIP_CHECK(h, hipMemcpyAsync(dV, h->apply_pin, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = magi_dense_apply_device(h, which, transpose, nv, dV, dY);
    if (rc) return rc;
    MAGI_HIP_CHECK(h, hipMemcpyAsync(h->apply_pin + n, dY, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    std::memcpy(Y, h->apply_pin + n, n * sizeof(double));
    return MAGI_OK;
}

int magi_theta_init(magi_handle* h, int drift_id, int P, const double* Xhat, const double* mu, int num_iters, double learning_rate,
                    double* theta, double* loss_trace) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_theta_init");
    if (!Xhat || !mu || !theta) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    if (!h->dDense[0] || h->dense_N <= 0) return magi_fail(h, MAGI_E_STATE, "no resident matrices: build or set them first");
    if (num_iters < 0 || !(learning_rate > 0.0)) return magi_fail(h, MAGI_E_BADARG, "num_iters >= 0 and learning_rate > 0");
    if (int rc = magi_check_drift_id(h, drift_id)) return rc;
    for (int i = 0; i < h->dense_N * h->dense_D; ++i)
        if (std::isnan(Xhat[i])) return magi_fail(h, MAGI_E_NAN, "NaN in Xhat");
    (void)hipSetDevice(h->device);
    return magi_theta_init_device(h, drift_id, P, Xhat, mu, num_iters, learning_rate, theta, loss_trace);
}

int magi_build_matrices(magi_handle* h, const double* I, int N, int D, const double* phi1, const double* phi2,
                        double nu, int bandsize, double* C_inv, double* m, double* K_inv) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_build_matrices");
    if (!I || !phi1 || !phi2) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    if (N < 2 || D < 1 || D > MAGI_MAX_D) return magi_fail(h, MAGI_E_BADARG, "need N >= 2 and 1 <= D <= " + std::to_string(MAGI_MAX_D));
    if (!(nu > 1.0)) return magi_fail(h, MAGI_E_BADARG, "nu must exceed 1 (once-differentiable Matern)");
    (void)hipSetDevice(h->device);
    return magi_build_matrices_device(h, I, N, D, phi1, phi2, nu, bandsize, C_inv, m, K_inv);
}

int magi_matern_blocks(magi_handle* h, const double* I, int N, double phi1, double phi2, double nu, double* Kappa,
                       double* p_Kappa, double* Kappa_pp) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_matern_blocks");
    if (!I || N < 2) return magi_fail(h, MAGI_E_BADARG, "bad grid");
    (void)hipSetDevice(h->device);
    return magi_matern_blocks_device(h, I, N, phi1, phi2, nu, Kappa, p_Kappa, Kappa_pp);
}

int magi_set_problem(magi_handle* h, const double* mu, const double* N_ds, const int64_t* obs_idx, const double* y,
                     int64_t n_obs, double beta, const double* LB, int drift_id, int P) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_set_problem");
    if (!h->have_matrices) return magi_fail(h, MAGI_E_STATE, "matrices must be set before the problem");
    if (!mu || !N_ds || !LB || (n_obs > 0 && (!obs_idx || !y))) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    DevProblem& pb = h->pb;
    int needD, needP;
#ifndef MAGI_USER_DRIFT_HEADER
    if (drift_id == MAGI_DRIFT_USER) return magi_fail(h, MAGI_E_BADARG, "no user drift compiled into this library (magi_v2_amd.jit builds one)");
#endif
    if (int rc = magi_check_drift_id(h, drift_id, false)) return rc;
    // (the dispatch below sends every id it does not know to its last arm: it is right only behind the check above)
#define MAGI_CALL(DR) needD = DriftT<DR>::D, needP = DriftT<DR>::P
    MAGI_DRIFT_DISPATCH(drift_id, MAGI_CALL);
#undef MAGI_CALL
    if (pb.D != needD || P != needP)
        return magi_fail(h, MAGI_E_BADARG, "drift expects D=" + std::to_string(needD) + ", P=" + std::to_string(needP));
    if (magi_user_drift_time_dependent() && h->times_N != pb.N)
        return magi_fail(h, MAGI_E_STATE, "this drift depends on time: call magi_set_times with the " + std::to_string(pb.N) +
                                          " times of the grid points before magi_set_problem");
    (void)hipSetDevice(h->device);
    const int N = pb.N, D = pb.D;
    std::vector<double> yobs((size_t)N * D, std::nan(""));
    std::vector<int64_t> obs_e((size_t)n_obs);
    for (int64_t k = 0; k < n_obs; ++k) {
        const int64_t idx = obs_idx[k];
        if (idx < 0 || idx >= (int64_t)N * D) return magi_fail(h, MAGI_E_BADARG, "obs_idx out of range");
        const int i = (int)(idx / D), d = (int)(idx % D);          // flat row-major index into X[N][D]
        yobs[(size_t)d * N + i] = y[k];
        obs_e[(size_t)k] = (int64_t)d * N + i;
    }
    // the old problem is forgotten before the first call that can fail (dimp may change: the chains go); the new one starts from the default model
    for (int d = 0; d < MAGI_MAX_D; ++d) h->model.lb_orig[d] = d < D ? LB[d] : 0.0;
    magi_stale(h, STALE_PROBLEM);                                  // (pb.LB = lb_orig)
    h->model.obs_e.swap(obs_e);
    h->model.obs_y.assign(y, y + n_obs);
    pb.yobs = nullptr;
    size_t cap = 0;                                                // (sized exactly: a new block for every problem)
    if (int rc = magi_grow(h, h->dYobs, cap, (size_t)N * D, "observations")) return rc;
    MAGI_HIP_CHECK(h, hipMemcpy(h->dYobs, yobs.data(), sizeof(double) * N * D, hipMemcpyHostToDevice));
    pb.yobs = h->dYobs;
    pb.P = P;
    pb.drift = drift_id;
    pb.dim = pb.ND + D + P;
    pb.dimp = (pb.dim + 7) & ~7;
    pb.beta_inv = 1.0 / beta;
    for (int d = 0; d < MAGI_MAX_D; ++d) {
        pb.mu[d] = d < D ? mu[d] : 0.0;
        pb.N_ds[d] = d < D ? N_ds[d] : 0.0;
    }
    h->have_problem = true;
    return MAGI_OK;
}

int magi_set_times(magi_handle* h, const double* t, int n) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_set_times");
    if (!t) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    // the handle's N: of the resident dense stacks (magi_build_dense, before they are packed) or of the packed matrices
    const int N = (h->dDense[0] && h->dense_N > 0) ? h->dense_N : (h->have_matrices ? h->pb.N : 0);
    if (N <= 0) return magi_fail(h, MAGI_E_STATE, "matrices must be built or set before the times (they fix N)");
    if (n != N) return magi_fail(h, MAGI_E_BADARG, "magi_set_times: n = " + std::to_string(n) + " times for a grid of N = " + std::to_string(N) + " points");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(t[i])) return magi_fail(h, MAGI_E_BADARG, "magi_set_times: t[" + std::to_string(i) + "] is not finite");
    (void)hipSetDevice(h->device);
    const size_t np_ = ((size_t)n + MAGI_TB - 1) / MAGI_TB * MAGI_TB;        // = pb.Np: padded with the last time, no load needs a bounds test
    std::vector<double> pad(np_, t[n - 1]);
    std::copy(t, t + n, pad.begin());
    h->times_N = 0;
    h->pb.tgrid = nullptr;
    if (int rc = model_upload(h, pad.data(), np_, h->dTimes, &h->times_cap, false)) return rc;
    h->pb.tgrid = h->dTimes;
    h->times_N = n;
    return MAGI_OK;
}

// priors whose density lives on (0, inf), and the supports that keep a parameter there
static bool prior_needs_positive(int k) { return k == MAGI_PRIOR_LOGNORMAL || k == MAGI_PRIOR_GAMMA || k == MAGI_PRIOR_INVGAMMA; }
static bool support_is_positive(int kind, double bound) { return kind == MAGI_THETA_POSITIVE || (kind == MAGI_THETA_LOWER && bound >= 0.0); }

int magi_set_theta_support(magi_handle* h, int P, const int* kind, const double* bound) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_set_theta_support");
    if (!h->have_problem) return magi_fail(h, MAGI_E_STATE, "magi_set_theta_support: set the problem first (magi_set_problem resets the supports)");
    if (P != h->pb.P) return magi_fail(h, MAGI_E_BADARG, "magi_set_theta_support: P = " + std::to_string(P) + ", the problem has " + std::to_string(h->pb.P) + " parameters");
    int kd[MAGI_MAX_P] = {};
    double bd[MAGI_MAX_P] = {};
    double2 tab[MAGI_MAX_P];
    bool plain = true;
    for (int p = 0; p < MAGI_MAX_P; ++p) tab[p] = make_double2(1.0, 0.0);
    for (int p = 0; kind && p < P; ++p) {
        const int k = kind[p];
        if (k != MAGI_THETA_POSITIVE && k != MAGI_THETA_LOWER && k != MAGI_THETA_UPPER && k != MAGI_THETA_REAL)
            return magi_fail(h, MAGI_E_BADARG, "magi_set_theta_support: kind[" + std::to_string(p) + "] = " + std::to_string(k) + " is none of MAGI_THETA_*");
        const bool bounded = k == MAGI_THETA_LOWER || k == MAGI_THETA_UPPER;
        if (bounded && (!bound || !std::isfinite(bound[p])))
            return magi_fail(h, MAGI_E_BADARG, "magi_set_theta_support: the bound of parameter " + std::to_string(p) + " is missing or not finite");
        kd[p] = k;
        bd[p] = bounded ? bound[p] : 0.0;
        if (prior_needs_positive(h->model.pr_kind[h->pb.D + p]) && !support_is_positive(k, bd[p]))
            return magi_fail(h, MAGI_E_BADARG, "magi_set_theta_support: parameter " + std::to_string(p) + " has a lognormal, gamma or inverse-gamma prior (magi_set_prior), "
                                               "which needs a support inside (0, inf): POSITIVE, or LOWER with a bound >= 0");
        tab[p] = make_double2(k == MAGI_THETA_REAL ? 0.0 : k == MAGI_THETA_UPPER ? -1.0 : 1.0, bd[p]);
        plain = plain && k == MAGI_THETA_POSITIVE;
    }
    (void)hipSetDevice(h->device);
    MagiModel& m = h->model;
    if (int rc = model_upload(h, tab, (size_t)MAGI_MAX_P, m.dTsup, nullptr, plain)) return rc;
    for (int p = 0; p < MAGI_MAX_P; ++p) { m.th_kind[p] = kd[p]; m.th_bound[p] = bd[p]; }
    h->pb.tsup = plain ? nullptr : m.dTsup;                                  // all-positive: no table, the kernels' default path
    return MAGI_OK;
}

int magi_get_theta_support(magi_handle* h, int P, int* kind, double* bound) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_get_theta_support");
    if (!h->have_problem) return magi_fail(h, MAGI_E_STATE, "magi_get_theta_support: set the problem first");
    if (P != h->pb.P) return magi_fail(h, MAGI_E_BADARG, "magi_get_theta_support: P = " + std::to_string(P) + ", the problem has " + std::to_string(h->pb.P) + " parameters");
    for (int p = 0; p < P; ++p) {
        if (kind) kind[p] = h->model.th_kind[p];
        if (bound) bound[p] = h->model.th_bound[p];
    }
    return MAGI_OK;
}

int magi_set_prior(magi_handle* h, int n, const int* kind, const double* a, const double* b) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_set_prior");
    if (!h->have_problem) return magi_fail(h, MAGI_E_STATE, "magi_set_prior: set the problem first (magi_set_problem resets the priors)");
    const int D = h->pb.D, P = h->pb.P;
    if (n != D + P) return magi_fail(h, MAGI_E_BADARG, "magi_set_prior: n = " + std::to_string(n) + ", the problem has D + P = " + std::to_string(D + P) + " parameter entries");
    constexpr int NT = MAGI_MAX_D + MAGI_MAX_P;
    int kd[NT] = {};
    double av[NT] = {}, bv[NT] = {};
    double4 tab[NT];
    bool plain = true;
    for (int j = 0; j < NT; ++j) tab[j] = make_double4(0.0, 0.0, 0.0, 0.0);
    for (int e = 0; kind && e < n; ++e) {
        const int k = kind[e];
        const std::string who = e < D ? "sigma^2 entry " + std::to_string(e) : "theta entry " + std::to_string(e - D);
        if (k < MAGI_PRIOR_FLAT || k > MAGI_PRIOR_FIXED)
            return magi_fail(h, MAGI_E_BADARG, "magi_set_prior: kind[" + std::to_string(e) + "] = " + std::to_string(k) + " is none of MAGI_PRIOR_*");
        if (k == MAGI_PRIOR_FLAT) continue;
        if (k == MAGI_PRIOR_FIXED && e >= D)
            return magi_fail(h, MAGI_E_BADARG, "magi_set_prior: " + who + ": FIXED is for sigma^2 entries only (a constant in f_vec states a fixed theta)");
        if (!a || !std::isfinite(a[e]) || (k != MAGI_PRIOR_FIXED && (!b || !std::isfinite(b[e]))))
            return magi_fail(h, MAGI_E_BADARG, "magi_set_prior: " + who + ": a parameter is missing or not finite");
        const bool a_pos = k == MAGI_PRIOR_GAMMA || k == MAGI_PRIOR_INVGAMMA || k == MAGI_PRIOR_FIXED;      // (shape, shape, value; a normal's or lognormal's m is free)
        if ((a_pos && !(a[e] > 0.0)) || (k != MAGI_PRIOR_FIXED && !(b[e] > 0.0)))
            return magi_fail(h, MAGI_E_BADARG, "magi_set_prior: " + who + ": sd, shape, rate, scale and a fixed value must be > 0");
        if (e >= D && prior_needs_positive(k) && !support_is_positive(h->model.th_kind[e - D], h->model.th_bound[e - D]))
            return magi_fail(h, MAGI_E_BADARG, "magi_set_prior: " + who + ": a lognormal, gamma or inverse-gamma prior needs a support inside (0, inf): POSITIVE, or LOWER with a "
                                               "bound >= 0 (magi_set_theta_support comes first)");
        kd[e] = k; av[e] = a[e]; bv[e] = k == MAGI_PRIOR_FIXED ? 0.0 : b[e];
        const bool gauss = k == MAGI_PRIOR_NORMAL || k == MAGI_PRIOR_LOGNORMAL;
        tab[e < D ? e : MAGI_MAX_D + (e - D)] = make_double4((double)k, av[e], bv[e], gauss ? 1.0 / (bv[e] * bv[e]) : 0.0);
        plain = false;
    }
    (void)hipSetDevice(h->device);
    MagiModel& m = h->model;
    if (int rc = model_upload(h, tab, (size_t)NT, m.dPrior, nullptr, plain)) return rc;
    for (int j = 0; j < NT; ++j) { m.pr_kind[j] = kd[j]; m.pr_a[j] = av[j]; m.pr_b[j] = bv[j]; }
    h->pb.prior = plain ? nullptr : m.dPrior;                                // all flat: no table, the kernels' default path
    h->pb.fixed_mask = 0;                                                    // a fixed sigma^2_d: bit d, and its constant in place of LB[d]
    for (int d = 0; d < D; ++d) {
        h->pb.LB[d] = kd[d] == MAGI_PRIOR_FIXED ? av[d] : m.lb_orig[d];
        if (kd[d] == MAGI_PRIOR_FIXED) h->pb.fixed_mask |= 1 << d;
    }
    return MAGI_OK;
}

int magi_get_prior(magi_handle* h, int n, int* kind, double* a, double* b) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_get_prior");
    if (!h->have_problem) return magi_fail(h, MAGI_E_STATE, "magi_get_prior: set the problem first");
    if (n != h->pb.D + h->pb.P) return magi_fail(h, MAGI_E_BADARG, "magi_get_prior: n = " + std::to_string(n) + ", the problem has D + P = " + std::to_string(h->pb.D + h->pb.P) + " parameter entries");
    for (int e = 0; e < n; ++e) {
        if (kind) kind[e] = h->model.pr_kind[e];
        if (a) a[e] = h->model.pr_a[e];
        if (b) b[e] = h->model.pr_b[e];
    }
    return MAGI_OK;
}

int magi_set_obs_model(magi_handle* h, int D, const int* link, int64_t n_obs, const double* weight) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_set_obs_model");
    if (!h->have_problem) return magi_fail(h, MAGI_E_STATE, "magi_set_obs_model: set the problem first (magi_set_problem resets the observation model)");
    const int N = h->pb.N;
    if (D != h->pb.D) return magi_fail(h, MAGI_E_BADARG, "magi_set_obs_model: D = " + std::to_string(D) + ", the problem has " + std::to_string(h->pb.D) + " components");
    if (n_obs != (int64_t)h->model.obs_e.size())
        return magi_fail(h, MAGI_E_BADARG, "magi_set_obs_model: n_obs = " + std::to_string(n_obs) + ", magi_set_problem was given " + std::to_string(h->model.obs_e.size()) + " observations");
    int lk[MAGI_MAX_D] = {};
    int links = 0;
    for (int d = 0; link && d < D; ++d) {
        if (link[d] < MAGI_LINK_IDENTITY || link[d] > MAGI_LINK_SQRT)
            return magi_fail(h, MAGI_E_BADARG, "magi_set_obs_model: link[" + std::to_string(d) + "] = " + std::to_string(link[d]) + " is none of MAGI_LINK_*");
        lk[d] = link[d];
        links |= link[d] << (2 * d);
    }
    for (int64_t k = 0; weight && k < n_obs; ++k)
        if (!std::isfinite(weight[k]) || !(weight[k] > 0.0))
            return magi_fail(h, MAGI_E_BADARG, "magi_set_obs_model: weight[" + std::to_string(k) + "] is not a finite number > 0");
    // g_d(y) laid out like yobs; observations given twice: the last one counts, as in magi_set_problem
    std::vector<double> gy((size_t)N * D, std::nan("")), w;
    if (weight) w.assign((size_t)N * D, 1.0);
    for (int64_t k = 0; k < n_obs; ++k) {
        const int64_t e = h->model.obs_e[(size_t)k];
        const int d = (int)(e / N);
        const double y = h->model.obs_y[(size_t)k];
        if (!std::isnan(y) && ((lk[d] == MAGI_LINK_LOG && !(y > 0.0)) || (lk[d] == MAGI_LINK_SQRT && !(y >= 0.0))))
            return magi_fail(h, MAGI_E_BADARG, "magi_set_obs_model: observation " + std::to_string(k) + " of component " + std::to_string(d) + " is outside the domain of its link (log: y > 0, sqrt: y >= 0)");
        gy[(size_t)e] = lk[d] == MAGI_LINK_LOG ? std::log(y) : lk[d] == MAGI_LINK_SQRT ? std::sqrt(y) : y;
        if (weight) w[(size_t)e] = weight[k];
    }
    (void)hipSetDevice(h->device);
    MagiModel& m = h->model;
    if (int rc = model_upload(h, w.data(), (size_t)N * D, m.dObsw, nullptr, !weight)) return rc;
    MAGI_HIP_CHECK(h, hipMemcpy(h->dYobs, gy.data(), sizeof(double) * N * D, hipMemcpyHostToDevice));
    for (int d = 0; d < MAGI_MAX_D; ++d) m.ob_link[d] = lk[d];
    if (weight) m.obs_w.assign(weight, weight + n_obs); else m.obs_w.clear();
    h->pb.obs_links = links;                                                 // all identity and no weights: the kernels' default path
    h->pb.obsw = weight ? m.dObsw : nullptr;
    return MAGI_OK;
}

int magi_get_obs_model(magi_handle* h, int D, int* link, int64_t n_obs, double* weight) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_get_obs_model");
    if (!h->have_problem) return magi_fail(h, MAGI_E_STATE, "magi_get_obs_model: set the problem first");
    if (D != h->pb.D) return magi_fail(h, MAGI_E_BADARG, "magi_get_obs_model: D = " + std::to_string(D) + ", the problem has " + std::to_string(h->pb.D) + " components");
    if (n_obs != (int64_t)h->model.obs_e.size())
        return magi_fail(h, MAGI_E_BADARG, "magi_get_obs_model: n_obs = " + std::to_string(n_obs) + ", magi_set_problem was given " + std::to_string(h->model.obs_e.size()) + " observations");
    for (int d = 0; link && d < D; ++d) link[d] = h->model.ob_link[d];
    for (int64_t k = 0; weight && k < n_obs; ++k) weight[k] = h->model.obs_w.empty() ? 1.0 : h->model.obs_w[(size_t)k];
    return MAGI_OK;
}

static int logpost_grad_impl(magi_handle* h, bool fused, int n_chains, const double* X, const double* sig_pre, const double* th_pre,
                             double beta_temp, double* logp, double* gX, double* gsig, double* gth, double* terms) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_logpost_grad");
    if (!X || !sig_pre || !th_pre) return magi_fail(h, MAGI_E_BADARG, "null state pointer");
    (void)hipSetDevice(h->device);
    int rc = magi_ensure_chains(h, n_chains);
    if (rc) return rc;
    magi_stale(h, STALE_SAMPLER);
    const DevProblem& pb = h->pb;
    if ((rc = upload_states(h, n_chains, X, sig_pre, th_pre))) return rc;
    MAGI_HIP_CHECK(h, hipMemsetAsync(h->ch.gctl, 0, sizeof(GlobalCtl), h->stream));
    if ((rc = magi_launch_prepare(h, n_chains, h->stream))) return rc;
    if (fused) {
        // (option fused_parity = 1: evaluate as an ODD leapfrog slot does -- the streaming kernels walk their blocks backwards there and
        //  read the other halves of the plan ring and of the operand mirrors; tests compare the two)
        const int par = h->opt.fused_parity ? 1 : 0;
        if ((rc = magi_launch_plan_eval(h, n_chains, h->stream, par))) return rc;
        if ((rc = magi_launch_stream(h, n_chains, par, false, h->stream))) return rc;
        if ((rc = magi_launch_point(h, n_chains, par, h->stream))) return rc;
        if ((rc = magi_launch_leap_finalize(h, n_chains, h->d_fin, h->stream, par))) return rc;
    } else {
        if ((rc = magi_launch_gradient(h, n_chains, h->stream))) return rc;
        if ((rc = magi_launch_finalize(h, n_chains, h->d_fin, h->stream))) return rc;
    }
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    std::vector<double> fin((size_t)8 * n_chains), g((size_t)pb.dimp);
    MAGI_HIP_CHECK(h, hipMemcpy(fin.data(), h->d_fin, sizeof(double) * 8 * n_chains, hipMemcpyDeviceToHost));
    for (int c = 0; c < n_chains; ++c) {
        if (logp) logp[c] = beta_temp * fin[(size_t)c * 8];
        if (terms) for (int k = 0; k < 4; ++k) terms[(size_t)c * 4 + k] = fin[(size_t)c * 8 + 1 + k];
        if (gX || gsig || gth) {
            MAGI_HIP_CHECK(h, hipMemcpy(g.data(), h->ch.vec + vec_off(pb, c, V_G), sizeof(double) * pb.dimp, hipMemcpyDeviceToHost));
            unpack_state(pb, g.data(), beta_temp, gX ? gX + (size_t)c * pb.ND : nullptr,
                         gsig ? gsig + (size_t)c * pb.D : nullptr, gth ? gth + (size_t)c * pb.P : nullptr);
        }
    }
    return MAGI_OK;
}

int magi_logpost_grad(magi_handle* h, int n_chains, const double* X, const double* sig_pre, const double* th_pre,
                      double beta_temp, double* logp, double* gX, double* gsig, double* gth, double* terms) {
    return logpost_grad_impl(h, false, n_chains, X, sig_pre, th_pre, beta_temp, logp, gX, gsig, gth, terms);
}

int magi_logpost_grad_fused(magi_handle* h, int n_chains, const double* X, const double* sig_pre, const double* th_pre,
                            double beta_temp, double* logp, double* gX, double* gsig, double* gth, double* terms) {
    return logpost_grad_impl(h, true, n_chains, X, sig_pre, th_pre, beta_temp, logp, gX, gsig, gth, terms);
}

void magi_sampler_cfg_default(magi_sampler_cfg* cfg) {
    if (!cfg) return;
    cfg->num_results = 1000;
    cfg->num_burnin_steps = 1000;
    cfg->num_adaptation_steps = -1;
    cfg->max_tree_depth = 10;
    cfg->mode = MAGI_MODE_NUTS;
    cfg->hmc_leapfrogs = 32;
    cfg->anneal = 1;
    cfg->stale_cache = 1;
    cfg->step_size = 0.1;
    cfg->target_accept_prob = 0.75;
    cfg->max_energy_diff = 1000.0;
    cfg->min_temp = 0.1;
}

int magi_sampler_init(magi_handle* h, const magi_sampler_cfg* cfg, int n_chains, const double* X0, const double* sig_pre0,
                      const double* th_pre0, uint64_t seed, const int64_t* chain_ids) {
    if (!h) return MAGI_E_BADARG;
    if (!cfg || !X0 || !sig_pre0 || !th_pre0) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    if (cfg->num_results < 0 || cfg->num_burnin_steps < 0 || cfg->num_results + cfg->num_burnin_steps <= 0)
        return magi_fail(h, MAGI_E_BADARG, "need num_results + num_burnin_steps > 0");
    if (cfg->max_tree_depth < 1 || cfg->max_tree_depth > MAGI_MAX_DEPTH)
        return magi_fail(h, MAGI_E_BADARG, "max_tree_depth must be in [1, 12]");
    if (cfg->mode != MAGI_MODE_NUTS && cfg->mode != MAGI_MODE_HMC) return magi_fail(h, MAGI_E_BADARG, "unknown sampler mode");
    if (cfg->mode == MAGI_MODE_HMC && cfg->hmc_leapfrogs < 1) return magi_fail(h, MAGI_E_BADARG, "hmc_leapfrogs must be >= 1");
    if (!(cfg->step_size > 0.0)) return magi_fail(h, MAGI_E_BADARG, "step_size must be positive");
    (void)hipSetDevice(h->device);
    int rc;
    if (h->group_n && (rc = group_refresh(h, n_chains))) return rc;
    if ((rc = magi_ensure_chains(h, n_chains))) return rc;
    magi_stale(h, STALE_SAMPLER);    // cfg and the buffers are baked into the captured graph; the sampler is ready again at the end of this call
    const DevProblem& pb = h->pb;
    SamplerCfgDev& c = h->cfg;
    c.total = cfg->num_results + cfg->num_burnin_steps;
    c.burnin = cfg->num_burnin_steps;
    c.n_adapt = cfg->num_adaptation_steps >= 0 ? cfg->num_adaptation_steps : (int)(0.8 * cfg->num_burnin_steps);
    c.max_depth = cfg->max_tree_depth;
    c.mode = cfg->mode;
    c.hmc_L = cfg->hmc_leapfrogs;
    c.anneal = cfg->anneal;
    c.stale = cfg->stale_cache;
    c.step_size = cfg->step_size;
    c.target_accept = cfg->target_accept_prob;
    c.max_energy_diff = cfg->max_energy_diff;
    c.min_temp = cfg->min_temp;
    c.seed = seed;
    h->num_results = cfg->num_results;

    // output buffers (grow-only); the eight diagnostics arrays share a capacity that is down while they grow: a failure part-way leaves each null or valid
    const size_t need_s = (size_t)n_chains * std::max(1, cfg->num_results) * pb.dimp, need_d = (size_t)n_chains * c.total;
    DevChains& d = h->ch;
    if ((rc = magi_grow(h, d.samples, h->samples_cap, need_s, "sample buffer"))) return rc;
    const size_t had_d = h->diag_cap;
    h->diag_cap = 0;
    auto grow_d = [&](auto*& p) { size_t cap = had_d; return magi_grow(h, p, cap, need_d, "sampler diagnostics"); };
    if ((rc = grow_d(d.d_step_size)) || (rc = grow_d(d.d_lar)) || (rc = grow_d(d.d_target)) || (rc = grow_d(d.d_energy)) || (rc = grow_d(d.d_beta)) ||
        (rc = grow_d(d.d_leapfrogs)) || (rc = grow_d(d.d_depth)) || (rc = grow_d(d.d_flags)))
        return rc;
    h->diag_cap = std::max(had_d, need_d);
    // steps not taken yet read as NaN / -1, not as whatever the allocation held
    MAGI_HIP_CHECK(h, hipMemsetAsync(d.samples, 0xFF, need_s * sizeof(double), h->stream));
    for (double* p : {d.d_step_size, d.d_lar, d.d_target, d.d_energy, d.d_beta}) MAGI_HIP_CHECK(h, hipMemsetAsync(p, 0xFF, need_d * sizeof(double), h->stream));
    for (int* p : {d.d_leapfrogs, d.d_depth, d.d_flags}) MAGI_HIP_CHECK(h, hipMemsetAsync(p, 0xFF, need_d * sizeof(int), h->stream));
    h->ch.scale = nullptr;       // a fresh sampler: identity metric, no metric window
    h->ch.macc = nullptr;
    h->window_k0.clear();

    if ((rc = upload_states(h, n_chains, X0, sig_pre0, th_pre0))) return rc;
    std::vector<long long> ids(n_chains);
    for (int i = 0; i < n_chains; ++i) ids[i] = chain_ids ? (long long)chain_ids[i] : (long long)i;
    MAGI_HIP_CHECK(h, hipMemcpy(h->d_chain_ids, ids.data(), sizeof(long long) * n_chains, hipMemcpyHostToDevice));
    if ((rc = magi_launch_init_chains(h, h->d_chain_ids, h->stream))) return rc;
    // bootstrap_results: one gradient at the initial state.  Slot 0 evaluates it, the decisions riding in slot 1's
    // stream store it as the proposal and leave the chains idle; a graph launch then starts at slot parity 0 again.
    if ((rc = magi_launch_prepare(h, n_chains, h->stream))) return rc;
    for (int sl = 0; sl < 2; ++sl) {
        if ((rc = magi_launch_stream(h, n_chains, sl, true, h->stream))) return rc;
        if ((rc = magi_launch_point(h, n_chains, sl, h->stream))) return rc;
    }
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    h->epoch = 0;
    h->sampler_ready = true;
    return MAGI_OK;
}

int magi_sampler_steps_done(magi_handle* h, int64_t* steps) {
    if (!h || !steps) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    std::vector<ChainCtl> ctl(h->n_chains);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains, hipMemcpyDeviceToHost));
    for (int i = 0; i < h->n_chains; ++i) steps[i] = ctl[i].k;
    return MAGI_OK;
}

int magi_sampler_run(magi_handle* h, int n_steps, int64_t* leapfrogs_done, double* kernel_ms) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    if (n_steps <= 0) return magi_fail(h, MAGI_E_BADARG, "n_steps must be positive");
    (void)hipSetDevice(h->device);
    int rc;
    // option no_graph (MAGI_NO_GRAPH=1 at handle creation): launch the leapfrog slots directly (debugging / rocprofv3 kernel traces of
    // long runs: the profiler's graph-node bookkeeping does not survive ~10^5 replayed nodes)
    const bool use_graph = !h->opt.no_graph;
    if (use_graph && !h->graph_valid && (rc = build_graph(h))) return rc;

    // (copies of this call ride on the handle's own non-blocking stream: a blocking hipMemcpy on the legacy stream is refused by HIP while ANOTHER
    //  handle, driven from another host thread, is capturing its graph -- "would make the legacy stream depend on a capturing stream")
    auto fetch = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
        return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
    };
    std::vector<ChainCtl> ctl(h->n_chains);
    MAGI_HIP_CHECK(h, fetch(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains));
    long long lf0 = 0;
    int kmin = h->cfg.total;
    for (auto& c : ctl) { lf0 += c.total_leapfrogs; kmin = std::min(kmin, c.k); }

    GlobalCtl g{};
    g.done_chains = 0;
    g.n_chains = h->n_chains;
    g.all_done = 0;
    g.stop_k = std::min(h->cfg.total, kmin + n_steps);
    g.epoch = ++h->epoch;
    MAGI_HIP_CHECK(h, hipMemcpyAsync(h->ch.gctl, &g, sizeof(GlobalCtl), hipMemcpyHostToDevice, h->stream));
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));   // &g is pageable stack memory
    MAGI_HIP_CHECK(h, hipEventRecord(h->ev_t0, h->stream));

    // pump: keep two graph launches in flight; after each, snapshot the control block
    const int depth = 2;
    long long issued = 0, retired = 0;
    bool done = false;
    // every slot advances every unfinished chain by a leaf or a set-up step, so a transition takes at most 2^max_depth - 1 leaves
    // + one set-up slot per doubling + start / end: a pump that outlives that budget means a corrupted control block
    // (+ one more set-up slot per doubling and two per transition end when a batch of NUTS chains spreads those passes: decide.h)
    const long long per_transition = (h->cfg.mode == MAGI_MODE_HMC ? (long long)h->cfg.hmc_L : (1ll << (h->cfg.max_depth + 1))) + 2 * h->cfg.max_depth + 8;
    long long max_graphs = ((long long)(g.stop_k - kmin) * per_transition + 8) / kGraphSlots + 4;
    if (h->opt.slot_budget_graphs > 0) max_graphs = std::max(1ll, std::min(max_graphs, h->opt.slot_budget_graphs));    // (test hook, magi_set_option only: force the budget exit)
    while (!done) {
        if (issued >= max_graphs && issued == retired) {
            (void)hipStreamSynchronize(h->stream);
            (void)fetch(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains);
            std::string where;
            for (int i = 0; i < h->n_chains; ++i)
                if (ctl[i].phase != PH_IDLE || ctl[i].k < g.stop_k) { where = " (chain " + std::to_string(i) + ": k=" + std::to_string(ctl[i].k) + ", phase=" + std::to_string(ctl[i].phase) + ", depth=" + std::to_string(ctl[i].depth) + ")"; break; }
            magi_stale(h, STALE_SAMPLER);
            return magi_fail(h, MAGI_E_STATE, "sampler did not finish within its slot budget" + where);
        }
        while (issued - retired < depth && issued < max_graphs) {
            const int slot = (int)(issued % 4);
            if (use_graph) {
                MAGI_HIP_CHECK(h, hipGraphLaunch(h->graph_exec, h->stream));
            } else {
                for (int sl = 0; sl < kGraphSlots; ++sl) {
                    if ((rc = magi_launch_stream(h, h->n_chains, sl & 1, true, h->stream))) return rc;
                    if ((rc = magi_launch_point(h, h->n_chains, sl & 1, h->stream))) return rc;
                }
            }
            MAGI_HIP_CHECK(h, hipMemcpyAsync(&h->h_gctl[slot], h->ch.gctl, sizeof(GlobalCtl), hipMemcpyDeviceToHost, h->stream));
            MAGI_HIP_CHECK(h, hipEventRecord(h->ev[slot], h->stream));
            ++issued;
        }
        if (issued == retired) continue;
        const int slot = (int)(retired % 4);
        MAGI_HIP_CHECK(h, hipEventSynchronize(h->ev[slot]));
        if (h->h_gctl[slot].all_done) done = true;
        ++retired;
    }
    MAGI_HIP_CHECK(h, hipEventRecord(h->ev_t1, h->stream));
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    {
        GlobalCtl gend{};
        MAGI_HIP_CHECK(h, fetch(&gend, h->ch.gctl, sizeof(GlobalCtl)));
        h->last_slots = gend.slots;
        h->last_graphs = issued;
    }
    if (kernel_ms) {
        float ms = 0.f;
        MAGI_HIP_CHECK(h, hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
        *kernel_ms = ms;
    }
    if (leapfrogs_done) {
        MAGI_HIP_CHECK(h, fetch(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains));
        long long lf1 = 0;
        for (auto& c : ctl) lf1 += c.total_leapfrogs;
        *leapfrogs_done = lf1 - lf0;
    }
    return MAGI_OK;
}

int magi_sampler_run_stats(magi_handle* h, int64_t* slots_issued, int64_t* graphs_launched) {
    if (!h) return MAGI_E_BADARG;
    if (slots_issued) *slots_issued = h->last_slots;
    if (graphs_launched) *graphs_launched = h->last_graphs;
    return MAGI_OK;
}

int magi_sampler_profile(magi_handle* h, int n_slots, double* stream_us, double* point_us, int64_t* leapfrogs_done) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    if (n_slots < 2 || n_slots > 65536) return magi_fail(h, MAGI_E_BADARG, "n_slots in [2, 65536]");
    (void)hipSetDevice(h->device);
    n_slots &= ~1;                       // slot parity 0 first, as a graph launch
    std::vector<ChainCtl> ctl(h->n_chains);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains, hipMemcpyDeviceToHost));
    long long lf0 = 0;
    for (auto& c : ctl) lf0 += c.total_leapfrogs;
    GlobalCtl g{};
    g.n_chains = h->n_chains;
    g.stop_k = h->cfg.total;             // run on: the chains are paused again below
    g.epoch = ++h->epoch;
    MAGI_HIP_CHECK(h, hipMemcpy(h->ch.gctl, &g, sizeof(GlobalCtl), hipMemcpyHostToDevice));
    std::vector<hipEvent_t> ev((size_t)4 * n_slots, nullptr);
    int rc = MAGI_OK;
    for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) rc = magi_fail(h, MAGI_E_HIP, "hipEventCreate");
    for (int sl = 0; sl < n_slots && rc == MAGI_OK; ++sl) {
        h->prof_e0 = ev[(size_t)4 * sl]; h->prof_e1 = ev[(size_t)4 * sl + 1];
        rc = magi_launch_stream(h, h->n_chains, sl & 1, true, h->stream);
        h->prof_e0 = ev[(size_t)4 * sl + 2]; h->prof_e1 = ev[(size_t)4 * sl + 3];
        if (rc == MAGI_OK) rc = magi_launch_point(h, h->n_chains, sl & 1, h->stream);
    }
    h->prof_e0 = h->prof_e1 = nullptr;
    (void)hipStreamSynchronize(h->stream);
    double ts = 0.0, tp = 0.0;
    int ns = 0, np_ = 0;
    for (int sl = 0; sl < n_slots && rc == MAGI_OK; ++sl) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, ev[(size_t)4 * sl], ev[(size_t)4 * sl + 1]) == hipSuccess) { ts += a; ++ns; }
        if (hipEventElapsedTime(&b, ev[(size_t)4 * sl + 2], ev[(size_t)4 * sl + 3]) == hipSuccess) { tp += b; ++np_; }
    }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    (void)hipGetLastError();
    if (rc) return rc;
    if (stream_us) *stream_us = ns ? ts / ns * 1e3 : 0.0;
    if (point_us) *point_us = np_ ? tp / np_ * 1e3 : 0.0;
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains, hipMemcpyDeviceToHost));
    long long lf1 = 0;
    for (auto& c : ctl) lf1 += c.total_leapfrogs;
    if (leapfrogs_done) *leapfrogs_done = lf1 - lf0;
    // the chains stand somewhere inside a transition: the sampler state is no longer at a transition boundary a later
    // magi_sampler_run could be compared against anything from -- the handle must be re-initialised
    magi_stale(h, STALE_SAMPLER);
    return MAGI_OK;
}

int magi_sampler_get_samples(magi_handle* h, double* X, double* sig_pre, double* th_pre) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    const DevProblem& pb = h->pb;
    const int R = h->num_results;
    std::vector<double> buf((size_t)R * pb.dimp);
    for (int c = 0; c < h->n_chains; ++c) {
        if (R == 0) break;
        MAGI_HIP_CHECK(h, hipMemcpy(buf.data(), h->ch.samples + (size_t)c * R * pb.dimp, sizeof(double) * R * pb.dimp, hipMemcpyDeviceToHost));
        for (int s = 0; s < R; ++s) {
            const size_t o = (size_t)c * R + s;
            unpack_state(pb, buf.data() + (size_t)s * pb.dimp, 1.0, X ? X + o * pb.ND : nullptr,
                         sig_pre ? sig_pre + o * pb.D : nullptr, th_pre ? th_pre + o * pb.P : nullptr);
        }
    }
    return MAGI_OK;
}

int magi_sampler_get_diag(magi_handle* h, double* step_size, double* log_accept_ratio, int32_t* leapfrogs_taken,
                          int32_t* tree_depth, int32_t* has_divergence, int32_t* reach_max_depth, int32_t* is_accepted,
                          double* target_log_prob, double* energy, double* beta_temp) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    const size_t n = (size_t)h->n_chains * h->cfg.total;
    const DevChains& d = h->ch;
    if (step_size) MAGI_HIP_CHECK(h, hipMemcpy(step_size, d.d_step_size, n * sizeof(double), hipMemcpyDeviceToHost));
    if (log_accept_ratio) MAGI_HIP_CHECK(h, hipMemcpy(log_accept_ratio, d.d_lar, n * sizeof(double), hipMemcpyDeviceToHost));
    if (target_log_prob) MAGI_HIP_CHECK(h, hipMemcpy(target_log_prob, d.d_target, n * sizeof(double), hipMemcpyDeviceToHost));
    if (energy) MAGI_HIP_CHECK(h, hipMemcpy(energy, d.d_energy, n * sizeof(double), hipMemcpyDeviceToHost));
    if (beta_temp) MAGI_HIP_CHECK(h, hipMemcpy(beta_temp, d.d_beta, n * sizeof(double), hipMemcpyDeviceToHost));
    if (leapfrogs_taken) MAGI_HIP_CHECK(h, hipMemcpy(leapfrogs_taken, d.d_leapfrogs, n * sizeof(int), hipMemcpyDeviceToHost));
    if (tree_depth) MAGI_HIP_CHECK(h, hipMemcpy(tree_depth, d.d_depth, n * sizeof(int), hipMemcpyDeviceToHost));
    if (has_divergence || reach_max_depth || is_accepted) {
        std::vector<int> f(n);
        MAGI_HIP_CHECK(h, hipMemcpy(f.data(), d.d_flags, n * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (has_divergence) has_divergence[i] = f[i] & 1;
            if (reach_max_depth) reach_max_depth[i] = (f[i] >> 1) & 1;
            if (is_accepted) is_accepted[i] = (f[i] >> 2) & 1;
        }
    }
    return MAGI_OK;
}

int magi_sampler_get_state(magi_handle* h, double* X, double* sig_pre, double* th_pre, double* step_size, double* beta_cache) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    const DevProblem& pb = h->pb;
    std::vector<double> q((size_t)pb.dimp);
    std::vector<ChainCtl> ctl(h->n_chains);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains, hipMemcpyDeviceToHost));
    for (int c = 0; c < h->n_chains; ++c) {
        MAGI_HIP_CHECK(h, hipMemcpy(q.data(), h->ch.vec + vec_off(pb, c, V_CANDQ), sizeof(double) * pb.dimp, hipMemcpyDeviceToHost));
        unpack_state(pb, q.data(), 1.0, X ? X + (size_t)c * pb.ND : nullptr, sig_pre ? sig_pre + (size_t)c * pb.D : nullptr,
                     th_pre ? th_pre + (size_t)c * pb.P : nullptr);
        if (step_size) step_size[c] = ctl[c].da_step_size;
        if (beta_cache) beta_cache[c] = ctl[c].beta_cache;
    }
    return MAGI_OK;
}

// per-chain scalars of a checkpoint (magi_sampler_get_checkpoint / magi_sampler_set_checkpoint)
enum { CKPT_K = 0, CKPT_DA_STEP, CKPT_STEP_SIZE, CKPT_ERR_SUM, CKPT_LOG_AVG, CKPT_LOG_SHRINK, CKPT_BETA_CACHE, CKPT_TOTAL_LF, CKPT_TAG, CKPT_COUNT };

// What a checkpoint belongs to: the sampler configuration, the seed, the chain's Philox id, the state size and the parameters' supports, folded into 52 bits (exact in a
// double).  A resume promises the uninterrupted run bit for bit, which only holds under the same configuration: set_checkpoint compares.
static double ckpt_tag(const magi_handle* h, long long chain_id) {
    unsigned long long x = 1469598103934665603ull;
    auto mix = [&x](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { x ^= b[i]; x *= 1099511628211ull; } };
    const SamplerCfgDev& c = h->cfg;
    const int ints[9] = {c.total, c.burnin, c.n_adapt, c.max_depth, c.mode, c.mode == MAGI_MODE_HMC ? c.hmc_L : 0, c.anneal, c.stale, h->pb.dimp};
    const double dbl[4] = {c.step_size, c.target_accept, c.max_energy_diff, c.min_temp};
    mix(ints, sizeof(ints)); mix(dbl, sizeof(dbl)); mix(&c.seed, sizeof(c.seed)); mix(&chain_id, sizeof(chain_id));
    magi_model_mix(h->model, h->pb, mix);      // (supports, priors, observation model: each while it is set)
    // (fp32 copies of operator blocks, option tile_demote: while the pack made any -- a resume with the other setting would continue on
    //  operators that differ in rounding; a tag at a shape where nothing is demoted is what it was before the format existed)
    if (h->n_demoted) mix(&h->n_demoted, sizeof(h->n_demoted));
    return (double)(x & ((1ull << 52) - 1));
}

int magi_sampler_get_checkpoint(magi_handle* h, double* scalars) {
    if (!h || !scalars) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_sampler_get_checkpoint");
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    std::vector<ChainCtl> ctl(h->n_chains);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains, hipMemcpyDeviceToHost));
    for (int c = 0; c < h->n_chains; ++c) {
        if (ctl[c].phase != PH_IDLE) return magi_fail(h, MAGI_E_STATE, "chain " + std::to_string(c) + " is inside a transition");
        double* o = scalars + (size_t)c * MAGI_CKPT_SCALARS;
        for (int k = 0; k < MAGI_CKPT_SCALARS; ++k) o[k] = 0.0;
        o[CKPT_K] = ctl[c].k; o[CKPT_DA_STEP] = ctl[c].da_step; o[CKPT_STEP_SIZE] = ctl[c].da_step_size;
        o[CKPT_ERR_SUM] = ctl[c].da_error_sum; o[CKPT_LOG_AVG] = ctl[c].da_log_avg; o[CKPT_LOG_SHRINK] = ctl[c].da_log_shrink;
        o[CKPT_BETA_CACHE] = ctl[c].beta_cache; o[CKPT_TOTAL_LF] = (double)ctl[c].total_leapfrogs;
        o[CKPT_TAG] = ckpt_tag(h, ctl[c].chain_id);
    }
    return MAGI_OK;
}

int magi_sampler_set_checkpoint(magi_handle* h, const double* scalars) {
    if (!h || !scalars) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_sampler_set_checkpoint");
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "call magi_sampler_init with the checkpointed states first");
    (void)hipSetDevice(h->device);
    static_assert(CKPT_COUNT <= MAGI_CKPT_SCALARS, "checkpoint layout");
    std::vector<ChainCtl> ctl(h->n_chains);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains, hipMemcpyDeviceToHost));
    for (int c = 0; c < h->n_chains; ++c) {
        const double* o = scalars + (size_t)c * MAGI_CKPT_SCALARS;
        if (ctl[c].phase != PH_IDLE || ctl[c].k != 0) return magi_fail(h, MAGI_E_STATE, "set the checkpoint right after magi_sampler_init");
        auto whole = [](double v, double hi) { return std::isfinite(v) && v >= 0.0 && v <= hi && v == std::floor(v); };
        const std::string who = "checkpoint of chain " + std::to_string(c);
        if (!whole(o[CKPT_K], (double)h->cfg.total) || !whole(o[CKPT_DA_STEP], 2147483647.0) || !whole(o[CKPT_TOTAL_LF], 9007199254740992.0))
            return magi_fail(h, MAGI_E_BADARG, who + ": transition index / adaptation step / leapfrog count must be whole numbers inside this configuration");
        if (!(o[CKPT_STEP_SIZE] > 0.0) || !std::isfinite(o[CKPT_STEP_SIZE]) || !std::isfinite(o[CKPT_ERR_SUM]) || !std::isfinite(o[CKPT_LOG_AVG]) ||
            !std::isfinite(o[CKPT_LOG_SHRINK]) || !(o[CKPT_BETA_CACHE] > 0.0) || !(o[CKPT_BETA_CACHE] <= 1.4426950408889636))      // (the schedule starts at 1 / ln 2, magi_v2.py:833-835)
            return magi_fail(h, MAGI_E_BADARG, who + ": non-finite dual-averaging state, step size <= 0 or cached temperature outside (0, 1 / ln 2]");
        if (o[CKPT_TAG] != ckpt_tag(h, ctl[c].chain_id))
            return magi_fail(h, MAGI_E_BADARG, who + " was taken under another sampler configuration, seed, chain id, problem size, parameter support, prior or observation model: a resume continues "
                                               "the SAME run (magi_hip.h)");
        ctl[c].k = (int)o[CKPT_K]; ctl[c].da_step = (int)o[CKPT_DA_STEP]; ctl[c].da_step_size = o[CKPT_STEP_SIZE];
        ctl[c].da_error_sum = o[CKPT_ERR_SUM]; ctl[c].da_log_avg = o[CKPT_LOG_AVG]; ctl[c].da_log_shrink = o[CKPT_LOG_SHRINK];
        ctl[c].beta_cache = o[CKPT_BETA_CACHE]; ctl[c].total_leapfrogs = (long long)o[CKPT_TOTAL_LF];
    }
    MAGI_HIP_CHECK(h, hipMemcpy(h->ch.ctl, ctl.data(), sizeof(ChainCtl) * h->n_chains, hipMemcpyHostToDevice));
    return MAGI_OK;
}

// ---- diagonal metric (include/magi_hip.h; kernels: DevChains::scale / macc in leap_point.h, leap_reduce.h, metric.hip) ----
// the three device buffers, sized for the chains the handle has room for (freed with them: free_chains)
static int metric_buffers(magi_handle* h) {
    const size_t n = (size_t)h->cap_chains, dimp = (size_t)h->pb.dimp;
    // (cap_chains and dimp cannot change while the chains live: a buffer that exists has its size)
    auto once = [h](double*& p, size_t need) { size_t cap = p ? need : 0; return magi_grow(h, p, cap, need, "metric buffers"); };
    int rc;
    if ((rc = once(h->d_scale, n * dimp)) || (rc = once(h->d_macc, n * 3 * dimp)) || (rc = once(h->d_mwork, n * (dimp + 4)))) return rc;
    return MAGI_OK;
}

// (copies ride on the handle's own stream, as magi_sampler_run's do)
static hipError_t metric_copy(magi_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

static int metric_idle_ctl(magi_handle* h, const char* who, std::vector<ChainCtl>& ctl) {
    ctl.resize(h->n_chains);
    MAGI_HIP_CHECK(h, metric_copy(h, ctl.data(), h->ch.ctl, sizeof(ChainCtl) * h->n_chains, hipMemcpyDeviceToHost));
    for (int c = 0; c < h->n_chains; ++c)
        if (ctl[c].phase != PH_IDLE) return magi_fail(h, MAGI_E_STATE, std::string(who) + ": chain " + std::to_string(c) + " is inside a transition");
    return MAGI_OK;
}

int magi_sampler_set_metric(magi_handle* h, const double* inv_mass_X, const double* inv_mass_sig, const double* inv_mass_th) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    const int given = (inv_mass_X ? 1 : 0) + (inv_mass_sig ? 1 : 0) + (inv_mass_th ? 1 : 0);
    if (given != 0 && given != 3) return magi_fail(h, MAGI_E_BADARG, "magi_sampler_set_metric: give all three arrays, or none for the identity metric");
    if (given == 0) {
        if (h->ch.scale) { h->ch.scale = nullptr; magi_stale(h, STALE_GRAPH); }
        return MAGI_OK;
    }
    int rc;
    {   // (between two magi_sampler_run calls every chain is idle; after magi_sampler_profile it is not, and the header's promise would not hold)
        std::vector<ChainCtl> ctl;
        if ((rc = metric_idle_ctl(h, "magi_sampler_set_metric", ctl))) return rc;
    }
    const DevProblem& pb = h->pb;
    std::vector<double> s((size_t)h->n_chains * pb.dimp);
    for (int c = 0; c < h->n_chains; ++c) {
        double* q = s.data() + (size_t)c * pb.dimp;
        pack_state(pb, inv_mass_X + (size_t)c * pb.ND, inv_mass_sig + (size_t)c * pb.D, inv_mass_th + (size_t)c * pb.P, q);
        for (int e = 0; e < pb.dim; ++e) {
            if (!(q[e] > 0.0) || !std::isfinite(q[e]))
                return magi_fail(h, MAGI_E_BADARG, "magi_sampler_set_metric: inverse mass of chain " + std::to_string(c) + ", state entry " + std::to_string(e) +
                                                   " is not a finite positive number");
            q[e] = std::sqrt(q[e]);
        }
        for (int e = pb.dim; e < pb.dimp; ++e) q[e] = 1.0;
    }
    if ((rc = metric_buffers(h))) return rc;
    MAGI_HIP_CHECK(h, metric_copy(h, h->d_scale, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice));
    if (!h->ch.scale) { h->ch.scale = h->d_scale; magi_stale(h, STALE_GRAPH); }
    return MAGI_OK;
}

int magi_sampler_get_metric(magi_handle* h, double* inv_mass_X, double* inv_mass_sig, double* inv_mass_th) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    const DevProblem& pb = h->pb;
    std::vector<double> s((size_t)h->n_chains * pb.dimp, 1.0);
    if (h->ch.scale) MAGI_HIP_CHECK(h, metric_copy(h, s.data(), h->d_scale, sizeof(double) * s.size(), hipMemcpyDeviceToHost));
    for (double& v : s) v = v * v;                    // (sqrt(v * v) == v in binary floating point: set_metric(get_metric()) restores s exactly)
    for (int c = 0; c < h->n_chains; ++c)
        unpack_state(pb, s.data() + (size_t)c * pb.dimp, 1.0, inv_mass_X ? inv_mass_X + (size_t)c * pb.ND : nullptr,
                     inv_mass_sig ? inv_mass_sig + (size_t)c * pb.D : nullptr, inv_mass_th ? inv_mass_th + (size_t)c * pb.P : nullptr);
    return MAGI_OK;
}

int magi_sampler_metric_window(magi_handle* h, int on) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    (void)hipSetDevice(h->device);
    if (!on) {
        if (h->ch.macc) { h->ch.macc = nullptr; magi_stale(h, STALE_GRAPH); }
        h->window_k0.clear();
        return MAGI_OK;
    }
    int rc;
    std::vector<ChainCtl> ctl;
    if ((rc = metric_idle_ctl(h, "magi_sampler_metric_window", ctl))) return rc;
    if ((rc = metric_buffers(h))) return rc;
    const DevProblem& pb = h->pb;
    const size_t row = sizeof(double) * pb.dimp;
    // sums := 0, shift := the state every chain holds (its trajectory-level proposal: what magi_sampler_get_state returns)
    MAGI_HIP_CHECK(h, hipMemsetAsync(h->d_macc, 0, row * 3 * h->n_chains, h->stream));
    MAGI_HIP_CHECK(h, hipMemcpy2DAsync(h->d_macc, row * 3, h->ch.vec + vec_off(pb, 0, V_CANDQ), row * V_COUNT, row, h->n_chains, hipMemcpyDeviceToDevice, h->stream));
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    h->window_k0.resize(h->n_chains);
    for (int c = 0; c < h->n_chains; ++c) h->window_k0[c] = ctl[c].k;
    if (!h->ch.macc) { h->ch.macc = h->d_macc; magi_stale(h, STALE_GRAPH); }
    return MAGI_OK;
}

int magi_sampler_adapt_metric(magi_handle* h, int n, double kappa, double rel_floor, int restart_adapt_steps, double* step_size_out) {
    if (!h) return MAGI_E_BADARG;
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    if (!h->ch.macc || (int)h->window_k0.size() != h->n_chains) return magi_fail(h, MAGI_E_STATE, "magi_sampler_adapt_metric: no metric window is open");
    if (n < 2) return magi_fail(h, MAGI_E_BADARG, "magi_sampler_adapt_metric: a variance needs n >= 2 states");
    if (!(kappa >= 0.0) || !std::isfinite(kappa) || !(rel_floor > 0.0) || !std::isfinite(rel_floor))
        return magi_fail(h, MAGI_E_BADARG, "magi_sampler_adapt_metric: need a finite kappa >= 0 and a finite rel_floor > 0");
    (void)hipSetDevice(h->device);
    int rc;
    std::vector<ChainCtl> ctl;
    if ((rc = metric_idle_ctl(h, "magi_sampler_adapt_metric", ctl))) return rc;
    for (int c = 0; c < h->n_chains; ++c)
        if (ctl[c].k - h->window_k0[c] != n)
            return magi_fail(h, MAGI_E_BADARG, "magi_sampler_adapt_metric: n = " + std::to_string(n) + ", but chain " + std::to_string(c) + " has finished " +
                                               std::to_string(ctl[c].k - h->window_k0[c]) + " transitions since the window was opened");
    const DevProblem& pb = h->pb;
    const size_t dimp = (size_t)pb.dimp;
    // min s of the metric in force (1 under the identity metric, whose ones the kernel must find where it leaves a chain alone)
    std::vector<double> s((size_t)h->n_chains * dimp, 1.0), min_old(h->n_chains, 1.0);
    if (h->ch.scale) {
        MAGI_HIP_CHECK(h, metric_copy(h, s.data(), h->d_scale, sizeof(double) * s.size(), hipMemcpyDeviceToHost));
        for (int c = 0; c < h->n_chains; ++c) min_old[c] = *std::min_element(s.begin() + c * dimp, s.begin() + c * dimp + pb.dim);
    } else {
        MAGI_HIP_CHECK(h, metric_copy(h, h->d_scale, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice));
    }
    if ((rc = magi_launch_metric_adapt(h, h->n_chains, n, kappa, rel_floor, h->d_macc, h->d_scale, h->d_mwork, h->stream))) return rc;
    std::vector<double> tail((size_t)h->n_chains * 4);
    MAGI_HIP_CHECK(h, hipMemcpy2DAsync(tail.data(), sizeof(double) * 4, h->d_mwork + dimp, sizeof(double) * (dimp + 4), sizeof(double) * 4, h->n_chains,
                                       hipMemcpyDeviceToHost, h->stream));
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    int kept = 0;
    for (int c = 0; c < h->n_chains; ++c) {
        const bool keep = tail[(size_t)c * 4 + 2] != 0.0;
        kept += keep ? 1 : 0;
        if (restart_adapt_steps >= 0) {
            // the step along the stiffest coordinate is kept: eps min(s) is what bounds a stable leapfrog step
            const double eps = keep ? ctl[c].da_step_size : ctl[c].da_step_size * min_old[c] / tail[(size_t)c * 4 + 1];
            ctl[c].da_step_size = eps;
            ctl[c].da_error_sum = 0.0; ctl[c].da_log_avg = 0.0; ctl[c].da_step = 0;
            ctl[c].da_log_shrink = std::log(10.0 * eps);
        }
        if (step_size_out) step_size_out[c] = ctl[c].da_step_size;
    }
    if (restart_adapt_steps >= 0) {
        MAGI_HIP_CHECK(h, metric_copy(h, h->ch.ctl, ctl.data(), sizeof(ChainCtl) * h->n_chains, hipMemcpyHostToDevice));
        h->cfg.n_adapt = restart_adapt_steps;
    }
    h->ch.scale = h->d_scale;
    h->ch.macc = nullptr;              // the window is closed
    h->window_k0.clear();
    magi_stale(h, STALE_GRAPH);
    return kept;
}

int magi_sample(magi_handle* h, const magi_sampler_cfg* cfg, int n_chains, const double* X0, const double* sig_pre0,
                const double* th_pre0, uint64_t seed, const int64_t* chain_ids, double* X_samps, double* sig_pre_samps,
                double* th_pre_samps) {
    int rc = magi_sampler_init(h, cfg, n_chains, X0, sig_pre0, th_pre0, seed, chain_ids);
    if (rc) return rc;
    if ((rc = magi_sampler_run(h, cfg->num_results + cfg->num_burnin_steps, nullptr, nullptr))) return rc;
    return magi_sampler_get_samples(h, X_samps, sig_pre_samps, th_pre_samps);
}

int magi_fit_hparams(magi_handle* h, const double* I, int N, int D, const double* X_filled, const double* mu, const double* mu_phi2,
                     const double* sd_phi2, const double* sigma_sq_loc, double nu, int num_iters, double learning_rate, double jitter,
                     double* phi1, double* phi2, double* sigma_sq, double* loss_trace) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_fit_hparams");
    if (!I || !X_filled || !mu || !mu_phi2 || !sd_phi2 || !sigma_sq_loc || !phi1 || !phi2 || !sigma_sq)
        return magi_fail(h, MAGI_E_BADARG, "null pointer");
    if (N < 2 || D < 1 || num_iters < 0 || !(nu > 1.0)) return magi_fail(h, MAGI_E_BADARG, "bad N, D, num_iters or nu");
    for (int d = 0; d < D; ++d)
        if (!(phi1[d] > 0.0) || !(phi2[d] > 0.0) || !(sigma_sq[d] > 0.0)) return magi_fail(h, MAGI_E_BADARG, "initial values must be positive");
    (void)hipSetDevice(h->device);
    return magi_fit_hparams_device(h, I, N, D, X_filled, mu, mu_phi2, sd_phi2, sigma_sq_loc, nu, num_iters, learning_rate, jitter,
                                   phi1, phi2, sigma_sq, loss_trace);
}

int magi_set_option(magi_handle* h, const char* name, int64_t value) {
    if (!h || !name) return MAGI_E_BADARG;
    // the test switch of csrc/summary.hip: no tuning option (no result depends on it), so it is no row of the table above
    if (std::strcmp(name, "summary_chunk_cols") == 0) {
        if (value < 0 || value > (1 << 24)) return magi_fail(h, MAGI_E_BADARG, "summary_chunk_cols in [0, 16777216]");
        h->opt.summary_chunk_cols = (int)value;
        return MAGI_OK;
    }
    // likewise the two of csrc/gp.hip: its chunk size (no result depends on it) and its per-stage timing (magi_gp_profile)
    if (std::strcmp(name, "gp_chunk_rows") == 0) {
        if (value < 0 || value > (1 << 16)) return magi_fail(h, MAGI_E_BADARG, "gp_chunk_rows in [0, 65536]");
        h->opt.gp_chunk_rows = (int)value;
        return MAGI_OK;
    }
    // the storage switch of csrc/pack.hip: fp32 copies of the operator blocks the criterion certifies (1, the default) or none (0); read at
    // the next packing.  It changes the storage format of a pack, not how a kernel is tuned: kept beside the table like the switches above
    if (std::strcmp(name, "tile_demote") == 0) {
        if (value < 0 || value > 1) return magi_fail(h, MAGI_E_BADARG, "tile_demote in [0, 1]");
        h->opt.tile_demote = (int)value;
        return MAGI_OK;
    }
    // the launch shape of the VALU streaming kernels (csrc/pack.hip: carriers): 0 a workgroup per block (the default), -1 carrier workgroups where they
    // make one launch round of several, 1 wherever a CU holds exactly one; read at the next packing.  No result depends on it, so it is no part of a checkpoint's tag
    if (std::strcmp(name, "stream_carriers") == 0) {
        if (value < -1 || value > 1) return magi_fail(h, MAGI_E_BADARG, "stream_carriers in [-1, 1]");
        h->opt.stream_carriers = (int)value;
        return MAGI_OK;
    }
    if (std::strcmp(name, "gp_profile") == 0) {
        h->opt.gp_profile = value != 0;
        return MAGI_OK;
    }
    for (const OptRow& r : kOptions) {
        if (std::strcmp(r.name, name) != 0) continue;
        if (set_option(h->opt, r, value)) return MAGI_OK;
        return magi_fail(h, MAGI_E_BADARG, std::string(r.name) + " in [" + std::to_string(r.lo) + ", " + std::to_string(r.hi) + "]");
    }
    return magi_fail(h, MAGI_E_BADARG, std::string("unknown option '") + name + "'");
}

int magi_build_profile(magi_handle* h, double* flops, double* ms, int64_t* calls) {
    if (!h || !flops || !ms || !calls) return MAGI_E_BADARG;
    long c[16];
    const int n = magi_build_profile_get(h, flops, ms, c);
    for (int i = 0; i < n; ++i) calls[i] = c[i];
    return n;
}

int magi_debug_par(magi_handle* h, int chain, double* out64) {
    if (!h || !out64 || chain < 0 || chain >= h->n_chains) return MAGI_E_BADARG;
    (void)hipSetDevice(h->device);
    MAGI_HIP_CHECK(h, hipMemcpy(out64, h->ch.par + (size_t)chain * PAR_COUNT, sizeof(double) * PAR_COUNT, hipMemcpyDeviceToHost));
    return MAGI_OK;
}

int magi_gradient_bytes(magi_handle* h, int n_chains, double* phase_bytes) {
    if (!h || !phase_bytes) return MAGI_E_BADARG;
    if (!h->have_matrices) return magi_fail(h, MAGI_E_STATE, "no matrices");
    const DevProblem& pb = h->pb;
    const double W = pb.band < 0 ? (double)pb.N : (double)(2 * pb.band + 1);
    const double mat = (double)pb.D * pb.N * W * 8.0;      // one matrix stack, algorithmic (unpadded) bytes
    const double vec = (double)n_chains * pb.N * pb.D * 8.0;
    phase_bytes[0] = 2.0 * mat + 3.0 * vec;   // Csym, M ; read X, write Cx, r
    phase_bytes[1] = 1.0 * mat + 2.0 * vec;   // Ksym    ; read r, write Kr
    phase_bytes[2] = 1.0 * mat + 5.0 * vec;   // Mt      ; read Kr, X, Cx, yobs, write gX
    phase_bytes[3] = 5.0 * vec;               // reduce  ; read X, Cx, r, Kr, yobs
    const double nslot = (double)std::min(pb.nb, 2 * pb.wb + 1);
    const StreamKernel k = magi_stream_kernel(h, n_chains);
    const double tiles = block_bytes(h, k);                                 // packed blocks of FH, FK (lower block triangle), FE, at the width this kernel reads them
    phase_bytes[4] = tiles + 2.0 * (double)n_chains * pb.n_tasks * MAGI_TB * 8.0;   // k_stream / k_stream_mc: + 2 TB partials per block and chain
    phase_bytes[5] = (double)n_chains * magi_leap_wgs(pb) * PART_K * 8.0; // tail: the workgroup partials
    phase_bytes[6] = 4.0 * vec * nslot + 10.0 * vec;                       // k_point: block partials of the four products; X, yobs, p, rho, g, p_leaf, p', x'
    if (h->have_problem && (k == StreamKernel::Sep8 || k == StreamKernel::Sep16)) {
        // k_stream_sep writes a block vector per (task, product, matrix-core column in use) and reads its operands from the mirror planes
        // (once per XCD at the fabric); its point kernel re-reads the product slots and writes the next slot's mirror
        double st = 0.0, op = 0.0, pr = 0.0, mw = 0.0;
        magi_sep_traffic(pb, n_chains, &st, &op, &pr, &mw);
        phase_bytes[4] = tiles + op + st;
        phase_bytes[6] = pr + 10.0 * vec + mw;
    }
    phase_bytes[7] = 3.0 * (double)pb.D * pb.N * W * 8.0 + 10.0 * vec;    // SURVEY 8d algorithmic bytes of one gradient evaluation
    return MAGI_OK;
}

int magi_tile_formats(magi_handle* h, int n_chains, int64_t* n_blocks, int64_t* n_demoted, double* bytes) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_tile_formats");
    if (!h->have_matrices) return magi_fail(h, MAGI_E_STATE, "no matrices");
    if (n_blocks) *n_blocks = h->pb.n_tasks;
    if (n_demoted) *n_demoted = h->n_demoted;
    if (bytes) *bytes = block_bytes(h, magi_stream_kernel(h, n_chains));
    return MAGI_OK;
}

int magi_stream_carriers(magi_handle* h, int* on, int* n_carriers, int* units, int cap) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_stream_carriers");
    if (!h->have_matrices) return magi_fail(h, MAGI_E_STATE, "no matrices");
    const int n = (int)h->carrier_units.size();
    if (on) *on = h->pb.n_carriers > 0;
    if (n_carriers) *n_carriers = n;
    if (units) {
        if (cap < n) return magi_fail(h, MAGI_E_BADARG, "magi_stream_carriers: room for " + std::to_string(cap) + " carriers, the pack has " + std::to_string(n));
        std::copy(h->carrier_units.begin(), h->carrier_units.end(), units);
    }
    return MAGI_OK;
}

int magi_stream_carrier_tasks(magi_handle* h, int* tasks, int cap) {
    if (!h || !tasks) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_stream_carrier_tasks");
    if (!h->have_matrices) return magi_fail(h, MAGI_E_STATE, "no matrices");
    const int n = MAGI_CARRIER_TASKS * (int)h->carrier_units.size();
    if (cap < n) return magi_fail(h, MAGI_E_BADARG, "magi_stream_carrier_tasks: room for " + std::to_string(cap) + " slots, the table has " + std::to_string(n));
    std::copy(h->carrier_slots.begin(), h->carrier_slots.end(), tasks);
    return MAGI_OK;
}

int magi_stream_kernel_name(magi_handle* h, int n_chains, char* buf, int cap) {
    if (!h || !buf || cap < 2) return MAGI_E_BADARG;
    if (h->group_n) {                  // (the group twins of k_stream<1> / k_stream<2>)
        if (n_chains <= 0 || n_chains % h->group_n) return magi_fail(h, MAGI_E_BADARG, "n_chains is not a positive multiple of the group's members");
        std::snprintf(buf, (size_t)cap, "%s", magi_stream_kernel(h, n_chains) == StreamKernel::Valu2 ? "k_stream_group<2>" : "k_stream_group<1>");
        return MAGI_OK;
    }
    if (!h->have_matrices || !h->have_problem) return magi_fail(h, MAGI_E_STATE, "set matrices and problem first");
    static const char* const names[] = {"k_stream<1>", "k_stream<2>", "k_stream_mc", "k_stream_sep<CW=8>", "k_stream_sep<CW=16>"};   // (StreamKernel order)
    std::snprintf(buf, (size_t)cap, "%s", names[(int)magi_stream_kernel(h, n_chains)]);
    return MAGI_OK;
}

int magi_time_gradient(magi_handle* h, int n_chains, int reps, double* total_ms_per_eval, double* phase_ms) {
    if (!h) return MAGI_E_BADARG;
    if (h->group_n) return refuse_group(h, "magi_time_gradient");
    if (reps <= 0) return magi_fail(h, MAGI_E_BADARG, "reps must be positive");
    (void)hipSetDevice(h->device);
    int rc = magi_ensure_chains(h, n_chains);
    if (rc) return rc;
    MAGI_HIP_CHECK(h, hipMemsetAsync(h->ch.gctl, 0, sizeof(GlobalCtl), h->stream));
    if ((rc = magi_launch_prepare(h, n_chains, h->stream))) return rc;
    if ((rc = magi_launch_plan_eval(h, n_chains, h->stream))) return rc;
    magi_stale(h, STALE_SAMPLER);          // the chain state is clobbered by the timing launches
    float ms = 0.f;
    // warm
    for (int i = 0; i < 3; ++i) {
        if ((rc = magi_launch_gradient(h, n_chains, h->stream))) return rc;
        if ((rc = magi_launch_finalize(h, n_chains, h->d_fin, h->stream))) return rc;
    }
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    MAGI_HIP_CHECK(h, hipEventRecord(h->ev_t0, h->stream));
    for (int i = 0; i < reps; ++i) {
        if ((rc = magi_launch_gradient(h, n_chains, h->stream))) return rc;
        if ((rc = magi_launch_finalize(h, n_chains, h->d_fin, h->stream))) return rc;
    }
    MAGI_HIP_CHECK(h, hipEventRecord(h->ev_t1, h->stream));
    MAGI_HIP_CHECK(h, hipEventSynchronize(h->ev_t1));
    MAGI_HIP_CHECK(h, hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
    if (total_ms_per_eval) *total_ms_per_eval = ms / reps;
    if (phase_ms) {
        for (int ph = 1; ph <= 8; ++ph) {
            MAGI_HIP_CHECK(h, hipEventRecord(h->ev_t0, h->stream));
            for (int i = 0; i < reps; ++i) {
                if (ph <= 3) rc = magi_launch_phase(h, ph, n_chains, h->stream);
                else if (ph == 4) rc = magi_launch_finalize(h, n_chains, h->d_fin, h->stream);
                else if (ph == 5) rc = magi_launch_stream(h, n_chains, i & 1, false, h->stream);       // slot parity alternates as in the sampler (the block walk reverses)
                else if (ph == 6) rc = magi_launch_leap_finalize(h, n_chains, h->d_fin, h->stream);
                else if (ph == 7) rc = magi_launch_point(h, n_chains, 0, h->stream);
                else rc = magi_launch_read_tiles(h, i & 1, h->stream);
                if (rc) return rc;
            }
            MAGI_HIP_CHECK(h, hipEventRecord(h->ev_t1, h->stream));
            MAGI_HIP_CHECK(h, hipEventSynchronize(h->ev_t1));
            MAGI_HIP_CHECK(h, hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
            phase_ms[ph - 1] = ms / reps;
        }
    }
    return MAGI_OK;
}

}  // extern "C"
