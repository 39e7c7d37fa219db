// Who owns GPU memory (host code only).  A DevMem hands out device and pinned
// host buffers and remembers each one, so a host object frees everything it
// holds with one release_all() -- on its destroy path, on every failure path,
// and from the destructor as the backstop.  The structs that carry the
// pointers stay plain data: the owner stores the pointers' values, never the
// addresses of struct members.  One allocation per buffer, no pooling: sizes,
// alignment and the moment of each allocation are the caller's.
// Templated on a backend: HipMem wraps the HIP calls and keeps the process-wide
// counts behind xcg_debug_mem_live; oracle/devmem_harness.cc runs it over malloc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <vector>

namespace xcg {

enum MemKind : uint8_t { MEM_DEV = 0, MEM_PINNED = 1 };

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <class B>
class DevMemT {
 public:
  DevMemT() = default;
  DevMemT(const DevMemT&) = delete;
  DevMemT& operator=(const DevMemT&) = delete;
  ~DevMemT() { release_all(); }

  // Allocate `bytes` into *p (null on failure) and remember it.  coherent: host
  // memory a kernel and the host may read and write at the same time.
  template <class T>
  bool dev(T** p, size_t bytes) { return get((void**)p, bytes, MEM_DEV, false); }
  template <class T>
  bool pinned(T** p, size_t bytes, bool coherent = false) { return get((void**)p, bytes, MEM_PINNED, coherent); }

  // A grow-only buffer of capacity *cap (in the caller's unit): nothing when
  // *cap >= want; else the old buffer is freed first, then `bytes` allocated
  // and *cap = newcap.  On failure *p is null and *cap is 0.  The growth
  // policy (newcap, bytes) is the caller's.
  template <class T, class C>
  bool grow(T** p, C* cap, C want, C newcap, size_t bytes, MemKind kind) {
    if (*cap >= want) return true;
    release(*p);
    *p = nullptr;
    *cap = 0;
    if (!get((void**)p, bytes, kind, false)) return false;
    *cap = newcap;
    return true;
  }
  // grow() of a byte buffer to at least half as much again (the zlib stages' policy).
  template <class T>
  bool grow_bytes(T** p, size_t* cap, size_t want, MemKind kind) {
    const size_t n = std::max(want, *cap * 3 / 2);
    return grow(p, cap, want, n, n, kind);
  }
  // grow() of `want` elements exactly (the pair passes' policy).
  template <class T>
  bool grow_exact(T** p, uint64_t* cap, uint64_t want) {
    return grow(p, cap, want, want, want * sizeof(T), MEM_DEV);
  }

  // Free one buffer this owner handed out (null, or one it does not hold: nothing).
  void release(const void* p) {
    if (!p) return;
    for (size_t i = 0; i < held_.size(); ++i)
      if (held_[i].p == p) {
        B::free(held_[i].p, held_[i].bytes, held_[i].kind);
        held_[i] = held_.back();
        held_.pop_back();
        return;
      }
  }
  // Free everything exactly once (idempotent).
  void release_all() {
    for (const Held& h : held_) B::free(h.p, h.bytes, h.kind);
    held_.clear();
  }
  size_t held() const { return held_.size(); }

 private:
  struct Held {
    void* p;
    size_t bytes;
    MemKind kind;
  };
  bool get(void** p, size_t bytes, MemKind kind, bool coherent) {
    if (!B::alloc(p, bytes, kind, coherent)) {
      *p = nullptr;                  // (a failed allocation leaves it unspecified)
      return false;
    }
    if (*p) held_.push_back(Held{*p, bytes, kind});
    return true;
  }
  std::vector<Held> held_;
};

// One stream-ordered temporary: allocated on a stream, freed on that stream
// when the guard leaves scope, on every path.
template <class B>
class StreamTempT {
 public:
  explicit StreamTempT(typename B::stream_t st) : st_(st) {}
  StreamTempT(const StreamTempT&) = delete;
  StreamTempT& operator=(const StreamTempT&) = delete;
  ~StreamTempT() {
    if (p_) B::free_async(p_, bytes_, st_);
  }
  template <class T>
  bool alloc(T** p, size_t bytes) {
    *p = nullptr;
    if (p_) return false;            // (one block per guard)
    if (!B::alloc_async(&p_, bytes, st_)) {
      p_ = nullptr;
      return false;
    }
    bytes_ = bytes;
    *p = (T*)p_;
    return true;
  }

 private:
  typename B::stream_t st_;
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace xcg

#ifndef XCG_DEVMEM_NO_HIP
#include <hip/hip_runtime.h>

namespace xcg {

// The real backend.  live[]: device bytes, pinned bytes, device allocations,
// pinned allocations now held through it, in the whole process.
struct HipMem {
  using stream_t = hipStream_t;
  static inline std::atomic<uint64_t> live[4];
  static void count(void* p, size_t bytes, MemKind kind, bool add) {
    if (!p) return;
    live[kind] += add ? bytes : 0 - (uint64_t)bytes;
    live[2 + kind] += add ? 1 : ~0ull;
  }
  static bool alloc(void** p, size_t bytes, MemKind kind, bool coherent) {
    const hipError_t e = kind == MEM_DEV ? hipMalloc(p, bytes)
                                         : hipHostMalloc(p, bytes, coherent ? hipHostMallocCoherent : 0u);
    if (e == hipSuccess) count(*p, bytes, kind, true);
    return e == hipSuccess;
  }
  static void free(void* p, size_t bytes, MemKind kind) {
    (void)(kind == MEM_DEV ? hipFree(p) : hipHostFree(p));
    count(p, bytes, kind, false);
  }
  static bool alloc_async(void** p, size_t bytes, hipStream_t st) {
    if (hipMallocAsync(p, bytes, st) != hipSuccess) return false;
    count(*p, bytes, MEM_DEV, true);
    return true;
  }
  static void free_async(void* p, size_t bytes, hipStream_t st) {
    (void)hipFreeAsync(p, st);
    count(p, bytes, MEM_DEV, false);
  }
};

using DevMem = DevMemT<HipMem>;
using StreamTemp = StreamTempT<HipMem>;

}  // namespace xcg
#endif
