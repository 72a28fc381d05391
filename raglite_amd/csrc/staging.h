// How an entry point's RL_MEM_HOST / RL_MEM_DEVICE arguments reach the device and come back: the per-thread block cache and pinned
// bounce buffer, the device scratch that recycles itself through them, and the per-call frame (Staging) that owns a call's buffers.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "common.h"

namespace rl {

// RL_HIP for the lifecycle calls, whose HIP errors name the entry point ("rl_index_append: out of memory").
inline int hip_status(hipError_t e, const char* who) {
    if (e == hipSuccess) return RL_OK;
    return fail(e == hipErrorOutOfMemory ? RL_ERR_NOMEM : RL_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

// The two arguments every entry point ends with: `stream` as the C ABI passes it, and `mem`, which is one of the two once an entry
// that takes filters has split RL_MEM_FILTERS_DEVICE off.
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int check_mem(int mem, const char* who) {
    if (mem != RL_MEM_HOST && mem != RL_MEM_DEVICE) return fail(RL_ERR_INVALID, std::string(who) + ": bad mem");
    return RL_OK;
}

// The per-thread state below is `inline thread_local`, so every translation unit that includes this header shares one instance per
// thread, and hidden: the library keeps it to itself, which lets the compiler reach it without a call through the PLT per access
// (host-argument calls are latency-bound and touch it some thirty times).
#define RL_THREAD_STATE inline thread_local __attribute__((visibility("hidden")))

// Per-thread cache of small device blocks: RL_MEM_HOST calls stage a query in and a handful of results out, and a
// hipMalloc + hipFree pair per staging buffer costs more than a 10 k-row search (measured: 121 us per host-argument
// search_chunks against 39 us with device arguments).  Blocks up to 4 MiB are recycled, larger ones are not kept.
struct BlockCache {
    struct Block { void* p; size_t bytes; int device; };
    std::vector<Block> free_blocks;
    static constexpr size_t MAX_BLOCK = size_t(4) << 20;
    static constexpr size_t MAX_BLOCKS = 32;
    void* take(size_t bytes, int device, size_t* got) {
        for (size_t i = 0; i < free_blocks.size(); ++i) {
            Block b = free_blocks[i];
            if (b.device == device && b.bytes >= bytes && b.bytes <= 4 * bytes + 4096) {
                free_blocks.erase(free_blocks.begin() + (long)i);
                *got = b.bytes;
                return b.p;
            }
        }
        return nullptr;
    }
    void give(void* p, size_t bytes, int device) {
        if (bytes > MAX_BLOCK || free_blocks.size() >= MAX_BLOCKS) { (void)hipFree(p); return; }
        free_blocks.push_back({p, bytes, device});
    }
    ~BlockCache() {
        for (const Block& b : free_blocks) (void)hipFree(b.p);  // at thread exit; errors during runtime teardown are moot
    }
};
RL_THREAD_STATE BlockCache g_blocks;

// Per-thread pinned bounce buffer for the small host <-> device copies of RL_MEM_HOST calls (a query in, k results
// out).  A hipMemcpyAsync from / to pageable memory is synchronous and goes through the driver's own staging; through
// pinned memory the copies are truly asynchronous and the call needs ONE synchronisation: results are copied out of
// the pinned buffer after it (drain()).  Entries are keyed by the DevBuf they belong to, so that an early error
// return, which destroys its DevBufs without draining, can never copy stale data into a caller's buffer later.
struct PinnedBounce {
    static constexpr size_t CAP = size_t(1) << 20, SMALL = size_t(256) << 10;
    char* base = nullptr;
    size_t used = 0;
    struct Pending { const void* owner; const void* src; void* dst; size_t bytes; };
    std::vector<Pending> pending;
    void* take(size_t bytes) {
        if (bytes == 0 || bytes > SMALL) return nullptr;
        if (!base && hipHostMalloc(reinterpret_cast<void**>(&base), CAP, hipHostMallocDefault) != hipSuccess) {
            base = nullptr;
            (void)hipGetLastError();
            return nullptr;
        }
        const size_t at = (used + 63) & ~size_t(63);
        if (at + bytes > CAP) return nullptr;
        used = at + bytes;
        return base + at;
    }
    void drain() {  // after the stream has been synchronised
        for (const Pending& p : pending) std::memcpy(p.dst, p.src, p.bytes);
        pending.clear();
        used = 0;
    }
    void drop(const void* owner) {
        for (size_t i = pending.size(); i-- > 0;)
            if (pending[i].owner == owner) pending.erase(pending.begin() + (long)i);
    }
    ~PinnedBounce() { if (base) (void)hipHostFree(base); }
};
RL_THREAD_STATE PinnedBounce g_pinned;

// Device scratch that returns itself to the thread's block cache.  The stream must have been synchronised before the
// buffer goes out of scope whenever the device may still be using it, so a recycled block is never in flight: Staging,
// which owns every DevBuf of a call, sees to that.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int device = 0;
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;  // (never allocated: nothing pending under its name either)
        g_pinned.drop(this);
        g_blocks.give(p, bytes, device);
        p = nullptr;
    }
    int alloc(size_t want) {
        release();
        if (want == 0) want = 16;
        RL_HIP(hipGetDevice(&device));
        size_t got = 0;
        p = g_blocks.take(want, device, &got);
        if (p) { bytes = got; return RL_OK; }
        const size_t rounded = (want + 255) & ~size_t(255);
        RL_HIP(hipMalloc(&p, rounded));
        bytes = rounded;
        return RL_OK;
    }
};

// The staging frame of one call: it owns the call's DevBufs and the list of results to copy back, and knows from them how the call
// has to end.  `mem` is where the caller's pointers live; in() and out() hand back what the kernels take (the caller's own pointer
// with RL_MEM_DEVICE, a staged copy otherwise), temp() a device temporary; finish() issues the copy-backs in the order the outputs were
// registered, then synchronises if it must.  A frame that is destroyed without finish() -- an early error return -- copies nothing
// back, now or later.  Constructing one makes no HIP call.  The buffers sit in the frame (no allocation per call; bounce entries are
// keyed by their address, so the frame does not move).
class Staging {
public:
    static constexpr int MAX_BUFFERS = 16;  // the largest caller, rl_search_rerank_spans_ragged, takes 13
    Staging(int mem, hipStream_t s) : mem_(mem), s_(s) {}
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;

    // Input: copied up unless `mem` says it is on the device already (through the pinned bounce buffer when it fits).  An argument
    // that lives elsewhere than the rest (RL_MEM_FILTERS_DEVICE) names its own `mem`.
    template <class T>
    int in(const T* src, size_t count, const T** out) { return in(src, count, out, mem_); }
    template <class T>
    int in(const T* src, size_t count, const T** out, int mem) {
        if (mem == RL_MEM_DEVICE) { *out = src; return RL_OK; }
        const size_t bytes = count * sizeof(T);
        Slot* t;
        RL_TRY(slot(bytes, &t));
        if (bytes) {
            const void* from = src;
            if (void* pin = g_pinned.take(bytes)) {
                std::memcpy(pin, src, bytes);
                from = pin;
            }
            RL_HIP(hipMemcpyAsync(t->buf.p, from, bytes, hipMemcpyHostToDevice, s_));
        }
        *out = static_cast<const T*>(t->buf.p);
        return RL_OK;
    }
    // Output: a device pointer to write to, copied back to `dst` by finish().  A null `dst` (an output the caller did not ask for)
    // gives a null pointer and is not recorded.
    template <class T>
    int out(T* dst, size_t count, T** out) {
        if (mem_ == RL_MEM_DEVICE || dst == nullptr) { *out = dst; return RL_OK; }
        Slot* t;
        RL_TRY(slot(count * sizeof(T), &t));
        t->dst = dst;
        t->out_bytes = count * sizeof(T);
        *out = static_cast<T*>(t->buf.p);
        return RL_OK;
    }
    // An optional output the kernels write either way: out() when the caller asked for it, a temporary otherwise.
    template <class T>
    int out_or_temp(T* dst, size_t count, T** out) {
        return dst ? this->out(dst, count, out) : temp(count * sizeof(T), out);
    }
    // A device temporary that goes back to the block cache with the frame, which is why finish() then synchronises.
    template <class T>
    int temp(size_t bytes, T** out) {
        Slot* t;
        RL_TRY(slot(bytes, &t));
        *out = static_cast<T*>(t->buf.p);
        return RL_OK;
    }

    // Copy-backs, then the synchronisation the frame needs: host arguments wait for their results; a buffer of the frame (with device
    // arguments: a temporary, or an input staged under its own `mem`) must not be recycled under a running kernel; with device
    // arguments and no buffer the call returns while the stream still runs.
    int finish() {
        RL_TRY(copy_back());
        return (mem_ == RL_MEM_HOST || n_ > 0) ? sync() : RL_OK;
    }
    // ... for the calls that promise their caller a finished stream whatever `mem` is (it synchronises after a failed copy-back too)
    int finish_synced() {
        const int st = copy_back();
        const int sy = sync();
        return st == RL_OK ? sy : st;
    }
    // Synchronise and hand the bounced results to the caller's buffers.
    int sync() {
        RL_HIP(hipStreamSynchronize(s_));
        drain();
        return RL_OK;
    }
    // ... for a call that has synchronised the stream itself (to report the error under its own name)
    void drain() { g_pinned.drain(); }

private:
    struct Slot {
        DevBuf buf;
        void* dst = nullptr;  // outputs: where finish() copies the first out_bytes of buf
        size_t out_bytes = 0;
    };
    int slot(size_t bytes, Slot** t) {
        if (n_ == MAX_BUFFERS) return fail(RL_ERR_UNSUPPORTED, "staging: a call asked for more than 16 buffers (raise Staging::MAX_BUFFERS)");
        RL_TRY(slots_[n_].buf.alloc(bytes));
        *t = &slots_[n_++];
        return RL_OK;
    }
    int copy_back() {
        PinnedBounce& pinned = g_pinned;
        for (int i = 0; i < n_; ++i) {
            const Slot& t = slots_[i];
            if (!t.dst || !t.out_bytes) continue;
            if (void* pin = pinned.take(t.out_bytes)) {
                RL_HIP(hipMemcpyAsync(pin, t.buf.p, t.out_bytes, hipMemcpyDeviceToHost, s_));
                pinned.pending.push_back({&t.buf, pin, t.dst, t.out_bytes});
            } else {
                RL_HIP(hipMemcpyAsync(t.dst, t.buf.p, t.out_bytes, hipMemcpyDeviceToHost, s_));
            }
        }
        return RL_OK;
    }
    int mem_;
    hipStream_t s_;
    int n_ = 0;
    Slot slots_[MAX_BUFFERS];
};

}  // namespace rl
