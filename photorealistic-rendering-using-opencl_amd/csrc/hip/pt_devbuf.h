// pt_devbuf.h -- DevBuf<T>: the owner of one hipMalloc allocation of T records (internal: not installed).  Move-only; frees in its
// destructor, on whatever device is current there (prt_destroy selects the context's before the context dies).  Every operation that
// allocates returns the hipError_t, and a failed one leaves the buffer empty with capacity 0, never dangling.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace prt {

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { DevBuf old(std::move(o)); swap(old); return *this; }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }       // in records
    void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; cap_ = 0;
    }
    // exactly n records (one for n == 0: an empty table is still a pointer a kernel may be given); what was held goes first
    hipError_t alloc(size_t n) {
        reset();
        if (!n) n = 1;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
        if (e == hipSuccess) cap_ = n; else p_ = nullptr;
        return e;
    }
    hipError_t first_use(size_t n) { return p_ ? hipSuccess : alloc(n); }          // allocated once, with the owner's size
    hipError_t reserve(size_t n) { return cap_ >= n ? hipSuccess : alloc(n); }     // grown on demand, contents not kept
    hipError_t upload(const T* src, size_t n) {                                    // exactly n records, filled from the host
        const hipError_t e = alloc(n);
        return e != hipSuccess || !n ? e : hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T>& src) { return upload(src.data(), src.size()); }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace prt
