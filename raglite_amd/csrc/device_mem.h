// Device memory a handle owns: the move-only block (Pool), its typed form (DevArray) and the two ways a store grows one.
#pragma once
#include <utility>

#include "scratch_layout.h"
#include "staging.h"

namespace rl {

// Device memory owned by an index: freed with its owner, move-only (one owner per block).  As scratch it grows: reserve() never
// shrinks, frees the old block before it allocates and does not keep the contents (no allocation in steady state).
struct Pool {
    void* p = nullptr;
    size_t cap = 0;
    Pool() = default;
    Pool(const Pool&) = delete;
    Pool& operator=(const Pool&) = delete;
    Pool(Pool&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Pool& operator=(Pool&& o) noexcept {  // (frees what this held right away)
        if (this != &o) { release(); std::swap(p, o.p); std::swap(cap, o.cap); }
        return *this;
    }
    ~Pool() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return RL_OK;
        release();
        RL_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return RL_OK;
    }
    // A fresh block of exactly `bytes` (the buffers a lifecycle call builds before it commits them to the index); frees what it held.
    int alloc(size_t bytes, const char* who) {
        release();
        RL_TRY(hip_status(hipMalloc(&p, bytes), who));
        cap = bytes;
        return RL_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};
// A Pool that reads as the T* the kernels take: the index' fixed-size device arrays.
template <class T>
struct DevArray : Pool {
    operator T*() const { return as<T>(); }
};

// Size, reserve, lay out (scratch_layout.h): the layout's sizing walk says what to reserve, the same walk over the block fills its pointers.
template <class L, class... A>
int carve(Pool& pool, L& layout, A... sizes) {
    RL_TRY(pool.reserve(layout.lay(Carver(), sizes...)));
    layout.lay(Carver(pool.p), sizes...);
    return RL_OK;
}

// Scratch that grows by a quarter more than asked for, so that the next few inserts fit (Pool::reserve keeps a block that is large enough).
inline int reserve_amortised(Pool& pool, size_t bytes, const char* who) {
    if (bytes <= pool.cap) return RL_OK;
    return pool.alloc(bytes + bytes / 4, who);
}

// Room for `need` items in an array that holds `used`: a fresh block of amortised capacity, the contents copied on the device.
template <class T>
int store_grow(DevArray<T>& arr, int64_t* cap, int64_t used, int64_t need, hipStream_t s, const char* who) {
    if (need <= *cap) return RL_OK;
    const int64_t want = std::max<int64_t>({need, *cap + *cap / 2, 1024});
    DevArray<T> bigger;
    RL_TRY(bigger.alloc((size_t)want * sizeof(T), who));
    if (used > 0) RL_TRY(hip_status(hipMemcpyAsync(bigger.p, arr.p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));  // (the old block goes now)
    arr = std::move(bigger);
    *cap = want;
    return RL_OK;
}

}  // namespace rl
