// One owned device buffer (internal): the staging areas of the detector handles whose size follows the largest call so far (grown on
// demand), and the YOLO handle's fixed-size arrays (reserved once at create).  Move-only; the destructor frees.
#pragma once
#include "common.h"

namespace tstar {

template <class T>
struct DeviceBuf {
    T* p = nullptr;
    size_t cap = 0;          // elements

    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    DeviceBuf(DeviceBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DeviceBuf() { release(); }

    // Room for n elements.  n <= cap does nothing.  Otherwise stream s -- the one whose launches read the buffer -- is drained
    // before a live allocation is freed, and the new one holds exactly n elements (no doubling: the HBM budgets count on it).
    // Contents are not preserved.  After a failure the buffer is empty, never dangling.
    int reserve(size_t n, hipStream_t s) {
        if (n <= cap) return TSTAR_OK;
        if (p) TSTAR_HIP_CHECK(hipStreamSynchronize(s));
        release();
        TSTAR_HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
        cap = n;
        return TSTAR_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

}  // namespace tstar
