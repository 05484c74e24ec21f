// Buf<T, KIND>: the one owner of a device (KIND 0) or pinned-host (KIND 1) allocation.  Standard
// headers only: the two functions below are defined in api.hip over HIP, and by tests over malloc.
#pragma once
#include <cstddef>

void *vh_mem_alloc(int kind, size_t bytes);   // kind 0: device; 1: pinned host.  Throws on failure
void vh_mem_free(int kind, void *p);          // never throws

template <typename T, int KIND = 0>
class Buf {
    T *p_ = nullptr;
    size_t n_ = 0;   // elements

public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    // At least n elements (n == 0: one).  True iff it allocated: the old block is freed first (the
    // peak is the larger of the two, not their sum) and its contents are lost; never shrinks.  When
    // the allocation throws the buffer is empty.
    bool reserve(size_t n) {
        if (n == 0) n = 1;
        if (p_ && n_ >= n) return false;
        reset();
        p_ = static_cast<T *>(vh_mem_alloc(KIND, sizeof(T) * n));
        n_ = n;
        return true;
    }
    void reset() {
        if (p_) vh_mem_free(KIND, p_);
        p_ = nullptr;
        n_ = 0;
    }
    size_t size() const { return n_; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
};
