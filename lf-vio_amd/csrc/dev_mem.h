// dev_mem.h — the one ownership rule for the memory an lfvio_ctx / lfvio_group holds: Buf<T, A> owns ONE allocation of the
// allocator policy A (a pointer and its capacity in bytes), grows and never shrinks, and frees in its destructor.  Plain C++ (no
// HIP) above the #ifdef: lfvio_hip.hip uses it with the policies at the end, tests/test_dev_mem.py compiles this file alone
// with a recording allocator and walks growth, failure, moves and teardown on the CPU.
//   reserve(bytes)  nothing when bytes <= capacity(); otherwise the old block is freed FIRST (peak memory does not rise), then exactly
//                   `bytes` are allocated.  false: the allocation failed and the buffer is empty; a later reserve() tries again.
//                   Headroom is the caller's business.
//   reset()         frees; false: the allocator refused the block (the buffer is empty all the same: nothing keeps a freed address)
//   b = Buf(...)    move-assignment frees b's block and takes the other's: "allocate the new block, then replace the old one"
// A policy is two static functions: void *alloc(size_t) (nullptr: failed) and bool free(void *).
#pragma once
#include <cstddef>
#include <utility>

template <class T, class A>
class Buf {
  T *p_ = nullptr;
  size_t cap_ = 0;

 public:
  Buf() = default;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) (void)reset(), p_ = std::exchange(o.p_, nullptr), cap_ = std::exchange(o.cap_, 0);
    return *this;
  }
  ~Buf() { (void)reset(); }
  bool reserve(size_t bytes) {
    if (bytes <= cap_) return true;
    (void)reset();
    p_ = static_cast<T *>(A::alloc(bytes));
    cap_ = p_ ? bytes : 0;
    return p_ != nullptr;
  }
  bool reset() {
    const bool ok = !p_ || A::free(p_);
    p_ = nullptr, cap_ = 0;
    return ok;
  }
  size_t capacity() const { return cap_; }
  T *get() const { return p_; }
  operator T *() const { return p_; }  // `buf + offset`, `if (buf)`, a kernel's or a copy's pointer argument
  T *operator->() const { return p_; }
};

#ifdef __HIP__
template <unsigned FLAGS>
struct PinnedMem {  // hipHostMalloc with these flags (the mailbox: hipHostMallocMapped | hipHostMallocCoherent)
  static void *alloc(size_t bytes) { void *p = nullptr; return hipHostMalloc(&p, bytes, FLAGS) == hipSuccess ? p : nullptr; }
  static bool free(void *p) { return hipHostFree(p) == hipSuccess; }
};
struct DeviceMem {
  static void *alloc(size_t bytes) { void *p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
  static bool free(void *p) { return hipFree(p) == hipSuccess; }
};
template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T, unsigned FLAGS = hipHostMallocDefault>
using PinBuf = Buf<T, PinnedMem<FLAGS>>;
#endif
