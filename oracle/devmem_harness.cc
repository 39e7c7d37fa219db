// CPU test of the memory owner (wanproxy_amd/csrc/xcg_devmem.h): the same
// DevMemT / StreamTempT code the library instantiates over HIP, here over a
// counting malloc backend that aborts on a double or foreign free and can fail
// the k-th allocation.  Stand-alone: prints one "ok <case>" line per case and
// exits 0, or names the check that failed and exits 1.  tests/test_devmem.py
// runs it.  TEST INFRASTRUCTURE ONLY.
#define XCG_DEVMEM_NO_HIP
#include "../wanproxy_amd/csrc/xcg_devmem.h"

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>
#include <type_traits>

namespace {

// What the backend did, in order: "a<kind>:<bytes>" / "f<kind>:<bytes>" per call.
struct MallocMem {
  using stream_t = int;
  struct Live {
    size_t bytes;
    int kind;                        // MEM_DEV, MEM_PINNED, or 2 + stream for a stream-ordered block
  };
  static std::map<void*, Live> live;
  static uint64_t live_bytes[2], live_n[2], allocs, frees;
  static long fail_at;               // fail the allocation whose number (from 1) this is; 0: none
  static std::string log;

  static bool take(void** p, size_t bytes, int kind) {
    ++allocs;
    if (fail_at && (long)allocs == fail_at) {
      *p = (void*)0x1;               // (a failed HIP allocation leaves the pointer unspecified)
      return false;
    }
    *p = ::malloc(bytes ? bytes : 1);
    live[*p] = Live{bytes, kind};
    live_bytes[kind == xcg::MEM_PINNED] += bytes;
    live_n[kind == xcg::MEM_PINNED] += 1;
    log += "a" + std::to_string(kind) + ":" + std::to_string(bytes) + " ";
    return true;
  }
  static void give(void* p, size_t bytes, int kind) {
    auto it = live.find(p);
    if (it == live.end() || it->second.bytes != bytes || it->second.kind != kind) {
      fprintf(stderr, "devmem_harness: double or foreign free of %p (%zu bytes, kind %d)\n", p, bytes, kind);
      abort();
    }
    live.erase(it);
    live_bytes[kind == xcg::MEM_PINNED] -= bytes;
    live_n[kind == xcg::MEM_PINNED] -= 1;
    ++frees;
    log += "f" + std::to_string(kind) + ":" + std::to_string(bytes) + " ";
    ::free(p);
  }
  static bool alloc(void** p, size_t bytes, xcg::MemKind kind, unsigned) { return take(p, bytes, kind); }
  static void free(void* p, size_t bytes, xcg::MemKind kind) { give(p, bytes, kind); }
  static bool alloc_async(void** p, size_t bytes, int st) { return take(p, bytes, 2 + st); }
  static void free_async(void* p, size_t bytes, int st) { give(p, bytes, 2 + st); }

  static void reset(long fail = 0) {
    allocs = frees = 0;
    fail_at = fail;
    log.clear();
  }
  static bool none_live() { return live.empty() && !live_bytes[0] && !live_bytes[1] && !live_n[0] && !live_n[1]; }
};
std::map<void*, MallocMem::Live> MallocMem::live;
uint64_t MallocMem::live_bytes[2], MallocMem::live_n[2], MallocMem::allocs, MallocMem::frees;
long MallocMem::fail_at;
std::string MallocMem::log;

using Mem = xcg::DevMemT<MallocMem>;
using Temp = xcg::StreamTempT<MallocMem>;
using xcg::MEM_DEV;
using xcg::MEM_PINNED;

#define CHECK(x)                                                         \
  do {                                                                   \
    if (!(x)) {                                                          \
      fprintf(stderr, "devmem_harness: %s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

// A plain struct of six buffers, as the library's scratch structs are, and its
// table: four device and two pinned buffers of different sizes.
struct Six {
  uint64_t* keys = nullptr;
  uint64_t* vals = nullptr;
  uint32_t* h_flags = nullptr;       // pinned
  uint8_t* pool = nullptr;
  uint32_t* count = nullptr;
  uint32_t* h_count = nullptr;       // pinned
};
bool alloc_six(Mem& m, Six& s) {
  return m.dev(&s.keys, 8 * 100) && m.dev(&s.vals, 8 * 100) && m.pinned(&s.h_flags, 16) &&
         m.dev(&s.pool, 2048 * 7 + 16) && m.dev(&s.count, 16) && m.pinned(&s.h_count, 16);
}

void case_table() {
  for (long k = 0; k <= 6; ++k) {    // 0: no failure
    MallocMem::reset(k);
    Mem m;
    Six s;
    const bool ok = alloc_six(m, s);
    CHECK(ok == (k == 0));
    CHECK(m.held() == (size_t)(k ? k - 1 : 6));
    CHECK(MallocMem::live.size() == m.held());
    if (k == 0) {
      CHECK(MallocMem::live_bytes[0] == 800 + 800 + 2048 * 7 + 16 + 16 && MallocMem::live_bytes[1] == 32);
      CHECK(MallocMem::live_n[0] == 4 && MallocMem::live_n[1] == 2);
    } else {
      void* const f[6] = {s.keys, s.vals, s.h_flags, s.pool, s.count, s.h_count};
      CHECK(f[k - 1] == nullptr);    // the failed one is null, whatever the backend left there
      for (long i = k; i < 6; ++i) CHECK(f[i] == nullptr);   // and nothing behind it was tried
      CHECK(MallocMem::allocs == (uint64_t)k);
    }
    m.release_all();
    CHECK(m.held() == 0 && MallocMem::none_live());
    CHECK(MallocMem::frees == (uint64_t)(k ? k - 1 : 6));
    s = Six{};                       // (the struct stays plain: the owner kept no address inside it)
  }
  printf("ok table\n");
}

void case_release_twice() {
  MallocMem::reset();
  {
    Mem m;
    Six s;
    CHECK(alloc_six(m, s));
    m.release_all();
    CHECK(MallocMem::frees == 6 && MallocMem::none_live());
    m.release_all();                 // idempotent
    CHECK(MallocMem::frees == 6);
    // the owner is usable again, and the destructor frees what is held then
    CHECK(m.dev(&s.keys, 64) && MallocMem::live.size() == 1);
    m.release_all();
    CHECK(MallocMem::frees == 7);
  }                                  // destructor after release_all: nothing left to free
  CHECK(MallocMem::frees == 7 && MallocMem::none_live());
  {
    Mem m;
    Six s;
    CHECK(alloc_six(m, s));
  }                                  // destructor alone
  CHECK(MallocMem::frees == 13 && MallocMem::none_live());
  printf("ok release_twice\n");
}

void case_release_one() {
  MallocMem::reset();
  Mem m;
  Six s;
  CHECK(alloc_six(m, s));
  m.release(s.pool);
  CHECK(m.held() == 5 && MallocMem::live_bytes[0] == 1616 && MallocMem::frees == 1);
  m.release(s.pool);                 // no longer held: nothing
  m.release(nullptr);
  int foreign = 0;
  m.release(&foreign);               // never held: nothing
  CHECK(m.held() == 5 && MallocMem::frees == 1);
  m.release(s.h_count);
  CHECK(MallocMem::live_bytes[1] == 16 && MallocMem::live_n[1] == 1);
  m.release_all();
  CHECK(MallocMem::frees == 6 && MallocMem::none_live());
  printf("ok release_one\n");
}

void case_grow() {
  MallocMem::reset();
  Mem m;
  uint8_t* p = nullptr;
  size_t cap = 0;
  CHECK(m.grow_bytes(&p, &cap, 1000, MEM_DEV) && p && cap == 1000);
  uint8_t* const first = p;
  // sufficient capacity: nothing happens
  CHECK(m.grow_bytes(&p, &cap, 1000, MEM_DEV) && m.grow_bytes(&p, &cap, 1, MEM_DEV));
  CHECK(p == first && cap == 1000 && MallocMem::allocs == 1 && MallocMem::frees == 0);
  // the zlib stages' policy: at least half as much again; the old block is freed first
  MallocMem::log.clear();
  CHECK(m.grow_bytes(&p, &cap, 1001, MEM_DEV) && cap == 1500);
  CHECK(MallocMem::log == "f0:1000 a0:1500 ");
  CHECK(m.grow_bytes(&p, &cap, 4000, MEM_DEV) && cap == 4000 && m.held() == 1);
  // the pair passes' policy: exactly `want` elements
  uint64_t* q = nullptr;
  uint64_t qcap = 0;
  CHECK(m.grow_exact(&q, &qcap, 10) && qcap == 10 && MallocMem::live_bytes[0] == 4000 + 80);
  CHECK(m.grow_exact(&q, &qcap, 11) && qcap == 11 && MallocMem::live_bytes[0] == 4000 + 88);
  // the pair's position arrays: the caller's capacity and byte count, unrelated units
  uint32_t* r = nullptr;
  uint64_t rcap = 0;
  const uint64_t newcap = std::max<uint64_t>(7 + 1, rcap + rcap / 2);
  CHECK(m.grow(&r, &rcap, (uint64_t)8, newcap, (newcap + 1) * 4, MEM_DEV) && rcap == 8);
  CHECK(MallocMem::live_bytes[0] == 4000 + 88 + 36);
  // pinned buffers keep their kind through a grow
  uint8_t* h = nullptr;
  size_t hcap = 0;
  CHECK(m.grow_bytes(&h, &hcap, 64, MEM_PINNED) && m.grow_bytes(&h, &hcap, 65, MEM_PINNED) && hcap == 96);
  CHECK(MallocMem::live_bytes[1] == 96 && MallocMem::live_n[1] == 1);
  // a failed grow: the old block is gone, the pointer null, the capacity 0
  MallocMem::fail_at = (long)MallocMem::allocs + 1;
  const uint64_t frees0 = MallocMem::frees;
  CHECK(!m.grow_bytes(&p, &cap, 5000, MEM_DEV));
  CHECK(p == nullptr && cap == 0 && MallocMem::frees == frees0 + 1 && m.held() == 3);
  // and the next call starts over from nothing
  CHECK(m.grow_bytes(&p, &cap, 10, MEM_DEV) && cap == 10 && m.held() == 4);
  m.release_all();
  CHECK(MallocMem::none_live());
  printf("ok grow\n");
}

int guarded(int st, int leave_at) {
  Temp a(st), b(st);
  uint8_t* pa = nullptr;
  uint32_t* pb = nullptr;
  if (!a.alloc(&pa, 100)) return -5;
  if (leave_at == 1) return 1;       // early return with one block held
  if (!b.alloc(&pb, 200)) return -5; // (a failure here still frees the first)
  if (leave_at == 2) return 2;
  CHECK(pa && pb && MallocMem::live.size() == 2);
  return 0;
}

void case_guard() {
  for (int leave = 0; leave <= 2; ++leave) {
    MallocMem::reset();
    CHECK(guarded(3, leave) == leave);
    CHECK(MallocMem::allocs == (leave == 1 ? 1u : 2u) && MallocMem::frees == MallocMem::allocs);
    CHECK(MallocMem::none_live());   // (a free on another stream than 3 would have aborted)
  }
  MallocMem::reset(2);               // the second allocation fails
  CHECK(guarded(0, 0) == -5 && MallocMem::frees == 1 && MallocMem::none_live());
  MallocMem::reset(1);               // the first fails: nothing to free
  CHECK(guarded(0, 0) == -5 && MallocMem::frees == 0 && MallocMem::none_live());
  {                                  // a guard never used frees nothing; a second alloc on one guard is refused
    MallocMem::reset();
    Temp t(1), u(1);
    uint8_t* p = nullptr;
    uint8_t* q = nullptr;
    CHECK(u.alloc(&p, 8) && !u.alloc(&q, 8) && q == nullptr && MallocMem::allocs == 1);
  }
  CHECK(MallocMem::frees == 1 && MallocMem::none_live());
  printf("ok guard\n");
}

}  // namespace

int main() {
  static_assert(!std::is_copy_constructible<Mem>::value && !std::is_copy_assignable<Mem>::value, "owner copies");
  static_assert(!std::is_copy_constructible<Temp>::value, "guard copies");
  case_table();
  case_release_twice();
  case_release_one();
  case_grow();
  case_guard();
  CHECK(MallocMem::none_live());
  printf("ok live_zero\n");
  return 0;
}
