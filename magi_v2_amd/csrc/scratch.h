// Call-scoped device scratch of the post-processing calls (ode.hip, ode_adaptive.hip, selftest.hip, summary.hip, elpd.hip, gp.hip):
// one hipMalloc per call, the sub-buffers carved from it, the copies on the handle's stream, and the one epilogue of these calls.
//   MagiScratch s(h, "magi_ode_solve");
//   double* dtrj; int* dstatus;
//   s.take(dtrj, cells); s.take(dstatus, S_pad);   // declares the sub-buffers: nothing else sizes the allocation
//   if (int rc = s.alloc()) return rc;             // ONE hipMalloc of their sum; fills in the pointers, zeroes what asked for it
//   s.up(..); if (s.ok()) s.note(magi_launch(..)); s.down(..);
//   return s.finish();
// The total is the sum of the takes, each at the alignment of its type, so a size formula and a carve cannot disagree.  The first
// failure sticks (a HIP error or a launch's return code): every later copy is a no-op, so nothing is downloaded after a failed
// launch.  finish() waits for the stream also on an error path (nothing may be in flight when the buffer goes), frees, and returns
// the launch's code first, then "who: <hip error>", else MAGI_OK; the destructor does the wait-and-free where finish() was not reached.
// Nothing here outlives the call: no pool, no cache, nothing of the handle's own memory.
#pragma once
#include "magi_internal.h"

#include <cstring>
#include <string>
#include <vector>

struct MagiScratch {
    MagiScratch(magi_handle* h, const char* who) : h(h), who(who) { slots.reserve(32); }      // (one host allocation for the slots of any call)
    MagiScratch(const MagiScratch&) = delete;
    MagiScratch& operator=(const MagiScratch&) = delete;
    ~MagiScratch() { release(); }

    // declares a sub-buffer of n T's (n = 0: a pointer nobody dereferences); p is valid after alloc().  zeroed: alloc() clears it.
    // alloc() writes through the ADDRESS of p: p (and a struct that holds it, such as MagiColStats) must neither move nor be copied
    // nor go out of scope between take and alloc.
    template <class T>
    void take(T*& p, size_t n, bool zeroed = false) {
        p = nullptr;
        if (base) { note(magi_fail(h, MAGI_E_STATE, who + ": scratch taken after its allocation")); return; }
        total = (total + alignof(T) - 1) / alignof(T) * alignof(T);
        slots.push_back(Slot{&p, total, zeroed ? n * sizeof(T) : 0});
        total += n * sizeof(T);
    }

    int alloc() {
        if (rc == MAGI_OK && e == hipSuccess && !base) e = hipMalloc((void**)&base, total ? total : 1);
        if (e != hipSuccess || rc != MAGI_OK) return finish();
        for (const Slot& s : slots) {
            char* q = base + s.off;
            std::memcpy(s.p, &q, sizeof q);                          // (s.p is the caller's T*: every object pointer has one representation)
            if (s.zero_bytes && e == hipSuccess) e = hipMemsetAsync(base + s.off, 0, s.zero_bytes, h->stream);
        }
        return MAGI_OK;
    }

    bool ok() const { return rc == MAGI_OK && e == hipSuccess; }
    void note(int r) { if (rc == MAGI_OK) rc = r; }                 // a launch's return code
    void note(hipError_t r) { if (e == hipSuccess) e = r; }         // any other HIP call on the stream
    void up(void* dst, const void* src, size_t bytes) { if (ok()) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream); }
    void down(void* dst, const void* src, size_t bytes) { if (ok()) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream); }
    void down_opt(void* dst, const void* src, size_t bytes) { if (dst) down(dst, src, bytes); }       // an output the caller may leave out

    int finish() {
        const hipError_t es = hipStreamSynchronize(h->stream);
        if (base) (void)hipFree(base);
        base = nullptr;
        if (rc != MAGI_OK) return rc;
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return magi_fail(h, MAGI_E_HIP, who + ": " + hipGetErrorString(e));
        return MAGI_OK;
    }

    magi_handle* const h;
    const std::string who;

private:
    struct Slot { void* p; size_t off, zero_bytes; };             // p: the address of the caller's pointer
    void release() {
        if (!base) return;
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(base);
        base = nullptr;
    }
    std::vector<Slot> slots;
    char* base = nullptr;
    size_t total = 0;
    hipError_t e = hipSuccess;
    int rc = MAGI_OK;
};
