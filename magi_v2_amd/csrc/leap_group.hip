// Problem groups (magi_group_create): one sampler over the chains of G problems of one shape, `per` chains each, problem-major.
// k_stream_group / k_point_group are the twins of k_stream<NC> / k_point (leap.hip): the same bodies (leap_stream_body.h,
// leap_point_body.h), with the problem of a workgroup's chains read from the group's device table instead of the kernel arguments.
// A workgroup's chains (grid.y * NC .. + NC - 1; NC divides `per`, so they belong to one problem) select member grid.y * NC / per
// (group_member: a wave-uniform index, scalar loads through the constant address space).  Everything else -- chain buffers, plan ring,
// partials -- is indexed by the group-wide chain index as in k_stream: the members share every shape field, so the layouts agree, and a
// chain computes what it computes in its own handle's k_stream<1 | 2> (which do not depend on the batch a chain runs in).
// (A translation unit of their own: instantiated next to k_point in leap.hip, k_point_group changed k_point's register allocation.)
#include "magi_internal.h"
#include "leap_reduce.h"
#include "leap_point.h"
#include "decide.h"
#include "stamps.h"

namespace {

#include "leap_stream.h"

template <int NC, int DRIFT>
__global__ __launch_bounds__(64 * ST_WAVES) __attribute__((amdgpu_waves_per_eu(3)))
void k_stream_group(const DevProblem* table, DevChains ch, SamplerCfgDev cfg, int parity, int per) {
    constexpr int KARGS = sizeof(const DevProblem*) + sizeof(DevChains) + sizeof(SamplerCfgDev) + 2 * sizeof(int), CARR = 1;      // (a group keeps single tasks)
    const DevProblem& pb = group_member(table, (int)(blockIdx.y * NC) / per);
#include "leap_stream_body.h"
}

// (the chain on grid.y belongs to member grid.y / per)
template <int DRIFT>
__global__ __launch_bounds__(PT_THREADS) void k_point_group(const DevProblem* table, DevChains ch, int parity, int per) {
    constexpr int KARGS = sizeof(const DevProblem*) + sizeof(DevChains) + 2 * sizeof(int);
    const DevProblem& pb = group_member(table, (int)blockIdx.y / per);
#include "leap_point_body.h"
}

template <int NC, int DRIFT>
int launch_stream_group(magi_handle* h, int n_chains, int parity, bool with_decisions, hipStream_t s) {
    const dim3 grid(h->pb.n_tasks + (with_decisions ? NC : 0), (n_chains + NC - 1) / NC);      // (as k_stream's: + one decision workgroup per chain)
    return magi_launch(h, "stream (group) launch: ", k_stream_group<NC, DRIFT>, grid, dim3(64 * ST_WAVES), s, (const DevProblem*)h->d_members, h->ch,
                       h->cfg, parity, h->group_per);
}

}  // namespace

// (magi_stream_kernel picks Valu2 / Valu1 for a group: chain pairs when every member has an even number of chains)
int magi_launch_stream_group(magi_handle* h, int n_chains, int parity, bool with_decisions, hipStream_t s) {
    if (h->stream_kernel == StreamKernel::Valu2) {
#define MAGI_CALL(DR) return launch_stream_group<2, DR>(h, n_chains, parity, with_decisions, s)
        MAGI_DRIFT_DISPATCH(h->pb.drift, MAGI_CALL);
#undef MAGI_CALL
    }
#define MAGI_CALL(DR) return launch_stream_group<1, DR>(h, n_chains, parity, with_decisions, s)
    MAGI_DRIFT_DISPATCH(h->pb.drift, MAGI_CALL);
#undef MAGI_CALL
    return MAGI_OK;
}

int magi_launch_point_group(magi_handle* h, int n_chains, int parity, hipStream_t s) {
    const dim3 g(magi_leap_wgs(h->pb), n_chains), b(PT_THREADS);
#define MAGI_CALL(DR) return magi_launch(h, "point (group) launch: ", k_point_group<DR>, g, b, s, (const DevProblem*)h->d_members, h->ch, parity, h->group_per)
    MAGI_DRIFT_DISPATCH(h->pb.drift, MAGI_CALL);
#undef MAGI_CALL
    return MAGI_OK;
}
