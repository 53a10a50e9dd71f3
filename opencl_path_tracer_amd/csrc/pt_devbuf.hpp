// pt_devbuf.hpp -- the one owner of a device array.  A pt_context holds its d_* arrays as DevBuf fields (pt_context.hpp names the HIP
// allocator and the alias the rest of the code uses), so destroying the context frees them and no call site frees by hand.
//
// What holds at every point a caller can observe:
//   * the pointer is null exactly when the capacity is 0;
//   * a failed allocation leaves the buffer empty: what it held before is already freed, once;
//   * the held pointer is cleared before it is freed, never after a step that can fail.
// Alloc supplies `static bool alloc(void** p, size_t bytes)` and `static void free(void* p)`.  It is a parameter only so that
// tests/cpp/devbuf_test.cpp can drive the type on the CPU with a counting allocator; this header knows nothing of HIP.
#pragma once

#include <cstddef>

namespace ptamd {
#pragma GCC visibility push(hidden)      // internal to the library: its instantiations stay out of libptamd.so's exported symbols

template <class T, class Alloc>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {      // frees what it held
        if (this != &o) {
            reset();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }            // call sites read a DevBuf field as they read the raw pointer it replaces
    size_t capacity() const { return cap_; }      // elements

    void reset() {
        T* old = p_;
        p_ = nullptr; cap_ = 0;
        if (old) Alloc::free(old);
    }
    // room for n elements in a fresh allocation, whatever was held; false: the allocation failed and the buffer is empty
    bool replace(size_t n) {
        reset();
        void* fresh = nullptr;
        if (n == 0) return true;
        if (!Alloc::alloc(&fresh, n * sizeof(T))) return false;
        p_ = static_cast<T*>(fresh); cap_ = n;
        return true;
    }
    // room for at least n elements: nothing happens when it is there already (the contents are not kept when it is not)
    bool reserve(size_t n) { return n <= cap_ || replace(n); }
    // takes over an allocation of n elements that Alloc's allocator made elsewhere (a device builder's result)
    void adopt(T* p, size_t n) {
        reset();
        if (p && n == 0) { Alloc::free(p); p = nullptr; }
        p_ = p; cap_ = p ? n : 0;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

#pragma GCC visibility pop
}  // namespace ptamd
