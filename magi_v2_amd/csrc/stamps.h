// Device-side instruments of dev builds (python -m magi_v2_amd.build --variant NAME -D...).  With neither switch below, every macro
// here expands to nothing: the product library is built without them.
//
// -DMAGI_STAMPS=<kernel> [-DMAGI_STAMP_WG=<task or workgroup>]: phase stamps of ONE workgroup of one kernel, read by tools/stamps.py
//     stream  k_stream<1, *>     task MAGI_STAMP_WG, wave MAGI_STAMP_WAVE (default 1)        8 stamps
//     sep     k_stream_sep       task MAGI_STAMP_WG (matrix-core pass 0, basis plane 0)      16 stamps
//     point   k_point            workgroup MAGI_STAMP_WG of chain 0                          6 stamps
//     decide  the decision workgroup of every chain (decide.h, leap_reduce.h)              11 stamps + 2 of the stream workgroups
//     diag    k_diag_chol_inv    component MAGI_STAMP_WG of the first block row             16 stamps, printed
//   A stamp reads the 100 MHz real-time counter (diag: the shader clock, s_memtime) into a register array indexed by compile-time
//   constants (MAGI_STAMPS_DECL, MAGI_STAMP); the selected thread writes the array once, at the kernel's end (MAGI_STAMPS_FLUSH), as raw
//   64-bit counter values to par[40 ..] of chain 0, which magi_debug_par reads back.  (One store per stamp spilled k_stream: 12 -> 27 us.)
// -DMAGI_WG_TRACE: begin / end / placement of EVERY workgroup of the last launch of the streaming kernel and of k_point (WG_TRACE below,
//   magi_debug_wg_trace in leap.hip, tools/exp_wg_trace.py).
#pragma once

#define MAGI_STAMPS_ID_stream 1
#define MAGI_STAMPS_ID_sep 2
#define MAGI_STAMPS_ID_point 3
#define MAGI_STAMPS_ID_decide 4
#define MAGI_STAMPS_ID_diag 5
#define MAGI_STAMPS_CAT_(a, b) a##b
#define MAGI_STAMPS_CAT(a, b) MAGI_STAMPS_CAT_(a, b)

// MAGI_STAMPS_ON(kernel, code): `code` in a build that stamps `kernel`, nothing otherwise
#define MAGI_STAMPS_ON(k, ...) MAGI_STAMPS_IF_##k(__VA_ARGS__)
#define MAGI_STAMPS_IF_stream(...)
#define MAGI_STAMPS_IF_sep(...)
#define MAGI_STAMPS_IF_point(...)
#define MAGI_STAMPS_IF_decide(...)
#define MAGI_STAMPS_IF_diag(...)

#define MAGI_STAMPS_DECL(k, n) MAGI_STAMPS_ON(k, unsigned long long magi_stamps_[n] = {};)
#define MAGI_STAMP(k, i) do { MAGI_STAMPS_ON(k, MAGI_STAMP_SET(i);) } while (0)
#define MAGI_STAMPS_FLUSH(k, selected, par, n) do { MAGI_STAMPS_ON(k, if (selected) for (int i_ = 0; i_ < (n); ++i_) MAGI_STAMP_PUT(par, i_);) } while (0)

#ifdef MAGI_STAMPS
#ifndef MAGI_STAMP_WG
#define MAGI_STAMP_WG 0
#endif
#ifndef MAGI_STAMP_WAVE
#define MAGI_STAMP_WAVE 1
#endif
#define MAGI_STAMP_SET(i) magi_stamps_[(i)] = __builtin_amdgcn_s_memrealtime()
#define MAGI_STAMP_PUT(par, i) reinterpret_cast<unsigned long long*>((par) + 40)[i] = magi_stamps_[i]

#if MAGI_STAMPS_CAT(MAGI_STAMPS_ID_, MAGI_STAMPS) == MAGI_STAMPS_ID_stream
#undef MAGI_STAMPS_IF_stream
#define MAGI_STAMPS_IF_stream(...) __VA_ARGS__
#elif MAGI_STAMPS_CAT(MAGI_STAMPS_ID_, MAGI_STAMPS) == MAGI_STAMPS_ID_sep
#undef MAGI_STAMPS_IF_sep
#define MAGI_STAMPS_IF_sep(...) __VA_ARGS__
#elif MAGI_STAMPS_CAT(MAGI_STAMPS_ID_, MAGI_STAMPS) == MAGI_STAMPS_ID_point
#undef MAGI_STAMPS_IF_point
#define MAGI_STAMPS_IF_point(...) __VA_ARGS__
#elif MAGI_STAMPS_CAT(MAGI_STAMPS_ID_, MAGI_STAMPS) == MAGI_STAMPS_ID_decide
#undef MAGI_STAMPS_IF_decide
#define MAGI_STAMPS_IF_decide(...) __VA_ARGS__
// The decisions' stamps span functions (decide.h, leap_reduce.h) and slots (a leaf's decisions ride in the NEXT slot's stream kernel),
// so they are staged in LDS, as doubles, by thread 0, and flushed to the chain's par[40 .. 50] only when a HOT leaf ends: a run that ends
// on a slow path still reports the last hot leaf.  par[51] / par[52] of the chain of the first stream workgroup hold raw counter values
// of the stream workgroups (latest end by atomicMax / first start, k_stream).
static __shared__ double magi_stamps_[16];
#undef MAGI_STAMP_SET
#undef MAGI_STAMP_PUT
#define MAGI_STAMP_SET(i) if (threadIdx.x == 0) magi_stamps_[(i)] = (double)__builtin_amdgcn_s_memrealtime()
#define MAGI_STAMP_PUT(par, i) (par)[40 + (i)] = magi_stamps_[i]
#elif MAGI_STAMPS_CAT(MAGI_STAMPS_ID_, MAGI_STAMPS) == MAGI_STAMPS_ID_diag
#undef MAGI_STAMPS_IF_diag
#define MAGI_STAMPS_IF_diag(...) __VA_ARGS__
// k_diag_chol_inv has no par block: its stamps are shader clock cycles, printed as offsets from stamp 0
#undef MAGI_STAMP_SET
#define MAGI_STAMP_SET(i) magi_stamps_[(i)] = __builtin_amdgcn_s_memtime()
#undef MAGI_STAMPS_FLUSH
#define MAGI_STAMPS_FLUSH(k, selected, par, n) do { MAGI_STAMPS_ON(k, if (selected) { printf("diag stamps (cycles from start):"); \
    for (int i_ = 1; i_ < (n); ++i_) printf(" %d:%lld", i_, (long long)(magi_stamps_[i_] - magi_stamps_[0])); printf("\n"); }) } while (0)
#else
#error "MAGI_STAMPS: one of stream, sep, point, decide, diag"
#endif
#endif  // MAGI_STAMPS

#ifdef MAGI_WG_TRACE
// begin / end (100 MHz real-time counter), hardware placement (XCC id, HW_ID) and a tag of every workgroup: [kernel][workgroup][4]
static __device__ unsigned long long g_wg_trace[2][4096][4];
struct WgTrace {
    int kern, wg;
    __device__ __forceinline__ WgTrace(int kern_, int tag) : kern(kern_) {
        wg = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
        if (threadIdx.x == 0 && wg < 4096) {
            g_wg_trace[kern][wg][0] = __builtin_amdgcn_s_memrealtime();
            g_wg_trace[kern][wg][2] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
            g_wg_trace[kern][wg][3] = (unsigned long long)(long long)tag;
        }
    }
    __device__ __forceinline__ ~WgTrace() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (the workgroup's stores have retired)
        if ((threadIdx.x & 63) == 0 && wg < 4096) atomicMax(&g_wg_trace[kern][wg][1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
};
#define WG_TRACE(kern, tag) WgTrace wg_trace_((kern), (tag))
#else
#define WG_TRACE(kern, tag) do { } while (0)
#endif
