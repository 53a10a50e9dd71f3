// devbuf_test.cpp -- ownership of DevBuf (csrc/pt_devbuf.hpp) on the CPU, with an allocator that counts.
//
// Every sequence of up to four operations out of reserve (small, large) / replace / adopt / reset / move-assign / destruction is
// run once with no failure, once for each position of one failing allocation and once for each position of one free that reports an
// error (as hipFree does after an earlier asynchronous error; the address is gone all the same, and DevBuf ignores the report).
// After every sequence: each address handed out was freed exactly once, none twice, none that was never handed out; after a failed
// allocation the buffer is null with capacity 0; a reserve with room made no allocator call.
// Plain C++, built with -fsanitize=address,undefined (make sanitize-host; tests/test_devbuf_host.py).  Prints "devbuf_test: ok ...".
#include "pt_devbuf.hpp"

#include <cstdint>
#include <cstdio>
#include <memory>
#include <set>
#include <utility>

namespace {

struct Counting {
    static std::set<uintptr_t> live, ever;
    static uintptr_t next;
    static int allocs, frees, fail_alloc_at, fail_free_at, errors;
    static bool last_free_failed;
    static void begin(int fail_alloc, int fail_free) {
        live.clear(); ever.clear();
        next = 0x1000; allocs = frees = 0;
        fail_alloc_at = fail_alloc; fail_free_at = fail_free;
        last_free_failed = false;
    }
    static bool alloc(void** p, size_t bytes) {
        *p = nullptr;
        if (bytes == 0) { ++errors; std::printf("  allocation of 0 bytes\n"); }
        if (++allocs == fail_alloc_at) return false;
        next += 0x100;                                   // distinct addresses, never reused: a late second free cannot hide
        live.insert(next); ever.insert(next);
        *p = reinterpret_cast<void*>(next);
        return true;
    }
    static void free(void* p) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        last_free_failed = ++frees == fail_free_at;
        if (!ever.count(a)) { ++errors; std::printf("  free of %#lx, which was never handed out\n", (unsigned long)a); }
        else if (!live.erase(a)) { ++errors; std::printf("  second free of %#lx\n", (unsigned long)a); }
    }
    static int calls() { return allocs + frees; }
};
std::set<uintptr_t> Counting::live, Counting::ever;
uintptr_t Counting::next;
int Counting::allocs, Counting::frees, Counting::fail_alloc_at, Counting::fail_free_at, Counting::errors;
bool Counting::last_free_failed;

constexpr int kOps = 7, kMaxLen = 4;
const char* const kOpName[kOps] = {"reserve(2)", "reserve(8)", "replace(4)", "adopt", "reset", "move-assign", "destroy"};

template <class Buf>
bool consistent(const Buf& b) { return (b.get() == nullptr) == (b.capacity() == 0); }

// one sequence under one injected failure; the number of properties it broke
template <class Buf>
int run_sequence(const int* ops, int len, int fail_alloc, int fail_free) {
    const int before = Counting::errors;
    Counting::begin(fail_alloc, fail_free);
    auto fault = [&](const char* what, int at) {
        ++Counting::errors;
        std::printf("  %s after op %d (%s)\n", what, at, kOpName[ops[at]]);
    };
    {
        std::unique_ptr<Buf> b(new Buf);
        for (int i = 0; i < len; ++i) {
            const int calls = Counting::calls();
            const size_t had = b->capacity();
            switch (ops[i]) {
            case 0: case 1: case 2: {
                const size_t n = ops[i] == 0 ? 2 : ops[i] == 1 ? 8 : 4;
                const bool ok = ops[i] == 2 ? b->replace(n) : b->reserve(n);
                if (!ok && (b->get() || b->capacity())) fault("a failed allocation left the buffer non-empty", i);
                if (ok && b->capacity() < n) fault("success without the room asked for", i);
                if (ops[i] != 2 && had >= n && Counting::calls() != calls) fault("reserve with room called the allocator", i);
                break;
            }
            case 3: {
                void* p = nullptr;
                const bool got = Counting::alloc(&p, 5 * sizeof(int));      // (what a device builder hands back)
                b->adopt(static_cast<int*>(p), got ? 5 : 0);
                if (b->get() != p) fault("adopt does not hold the pointer it was given", i);
                break;
            }
            case 4: b->reset(); break;
            case 5: {
                Buf o;
                (void)o.replace(3);
                int* const held = o.get();
                *b = std::move(o);
                if (b->get() != held || o.get() || o.capacity()) fault("move-assign did not move", i);
                break;
            }
            default: b.reset(new Buf); break;
            }
            if (!consistent(*b)) fault("null and capacity 0 do not go together", i);
        }
    }
    for (uintptr_t a : Counting::live) { ++Counting::errors; std::printf("  %#lx was never freed\n", (unsigned long)a); }
    const int broke = Counting::errors - before;
    if (broke) {
        std::printf("^ sequence:");
        for (int i = 0; i < len; ++i) std::printf(" %s", kOpName[ops[i]]);
        std::printf("  [failing allocation %d, failing free %d]\n", fail_alloc, fail_free);
    }
    return broke;
}

template <class Buf>
int run_all(long* runs) {
    int broke = 0, ops[kMaxLen];
    for (int len = 1; len <= kMaxLen; ++len) {
        int total = 1;
        for (int i = 0; i < len; ++i) total *= kOps;
        for (int code = 0; code < total; ++code) {
            for (int i = 0, c = code; i < len; ++i, c /= kOps) ops[i] = c % kOps;
            broke += run_sequence<Buf>(ops, len, 0, 0);
            const int allocs = Counting::allocs, frees = Counting::frees;      // of the run without a failure: an upper bound on both
            for (int k = 1; k <= allocs; ++k) broke += run_sequence<Buf>(ops, len, k, 0);
            for (int k = 1; k <= frees; ++k) broke += run_sequence<Buf>(ops, len, 0, k);
            *runs += 1 + allocs + frees;
        }
    }
    return broke;
}

}  // namespace

int main() {
    long runs = 0;
    const int broke = run_all<ptamd::DevBuf<int, Counting>>(&runs);
    if (broke) { std::printf("devbuf_test: %d broken properties over %ld runs\n", broke, runs); return 1; }
    std::printf("devbuf_test: ok (%ld runs)\n", runs);
    return 0;
}
