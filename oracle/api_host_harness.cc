// CPU test of the ABI layer's host-only helpers
// (wanproxy_amd/csrc/xcg_api_host.h): the same code the library's units
// include, here on its own under AddressSanitizer and
// UndefinedBehaviorSanitizer (oracle/Makefile).  Stand-alone: one
// "ok <case>" line per case and exit 0, or the check that failed and exit 1.
// tests/test_api_host.py runs it.  Any sanitizer report ends the program with
// a non-zero status.
// TEST INFRASTRUCTURE ONLY.
#include "../wanproxy_amd/csrc/xcg_api_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace {

#define CHECK(x)                                                               \
  do {                                                                         \
    if (!(x)) {                                                                \
      fprintf(stderr, "api_host_harness: line %d: CHECK(%s)\n", __LINE__, #x); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

constexpr uint64_t S64 = 0xA5A5A5A5A5A5A5A5ull;
constexpr uint32_t S32 = 0xA5A5A5A5u;

void case_status() {
  CHECK(status_of(0) == XCG_OK);
  CHECK(status_of(XCG_RC_NOENT) == XCG_ENOENT);
  CHECK(status_of(XCG_RC_HIP) == XCG_EHIP);
  CHECK(status_of(XCG_RC_NOMEM) == XCG_ENOMEM);
  CHECK(status_of(XCG_RC_INVAL) == XCG_EINVAL);
  CHECK(status_of(XCG_RC_OVERFLOW) == XCG_EOVERFLOW);
  CHECK(status_of(XCG_RC_NOTSUP) == XCG_ENOTSUP);
  // the names keep the values the ABI's statuses have
  CHECK(XCG_RC_NOENT == -2 && XCG_RC_HIP == -5 && XCG_RC_NOMEM == -12 && XCG_RC_INVAL == -22 &&
        XCG_RC_OVERFLOW == -75 && XCG_RC_NOTSUP == -95);
  CHECK(status_of(-1) == XCG_EHIP && status_of(-71) == XCG_EHIP && status_of(-1000) == XCG_EHIP);   // unknown
  puts("ok status");
}

// The string in a heap buffer of exactly its size: a read past the terminator is a sanitizer report.
struct Exact {
  char* p;
  explicit Exact(const char* s) : p((char*)malloc(strlen(s) + 1)) { memcpy(p, s, strlen(s) + 1); }
  ~Exact() { free(p); }
};

void case_uuid() {
  std::string key;
  Exact mixed("01234567-89aB-CdEf-0123-456789ABCDEF");
  CHECK(uuid_key(mixed.p, &key));
  CHECK(key == "01234567-89ab-cdef-0123-456789abcdef");
  key = "unchanged";
  Exact shorter("01234567-89ab-cdef-0123-456789abcde");     // 35 characters
  CHECK(strlen(shorter.p) == 35 && !uuid_key(shorter.p, &key));
  Exact dash("012345678-9ab-cdef-0123-456789abcdef");        // the first dash one place late
  CHECK(strlen(dash.p) == 36 && !uuid_key(dash.p, &key));
  Exact nonhex("01234567-89ab-cdeg-0123-456789abcdef");
  CHECK(strlen(nonhex.p) == 36 && !uuid_key(nonhex.p, &key));
  Exact empty("");
  CHECK(!uuid_key(empty.p, &key));
  CHECK(!uuid_key(nullptr, &key));
  CHECK(key == "unchanged");                                 // (a refused string writes nothing)
  puts("ok uuid");
}

// row i: hash i + 1 in the high word and ~i in the low one, position 2048 * i, a last word nobody reads
std::vector<uint32_t> decl_rows(uint32_t n) {
  std::vector<uint32_t> r(4 * n);
  for (uint32_t i = 0; i < n; ++i) {
    r[4 * i] = ~i;
    r[4 * i + 1] = i + 1;
    r[4 * i + 2] = 2048 * i;
    r[4 * i + 3] = 0xDEADBEEFu;
  }
  return r;
}

void case_decl_rows() {
  for (uint32_t n : {0u, 1u, 3u}) {
    for (uint32_t cap : {n ? n - 1 : 0u, n, n + 2}) {         // below, at, above the count
      for (int null_one = 0; null_one < 3; ++null_one) {      // none, the hashes, the positions
        // only the rows that fit the cap exist (as in xcg_last_declarations): an exactly sized heap buffer
        const uint32_t k = n < cap ? n : cap;
        const std::vector<uint32_t> all = decl_rows(n);
        const std::vector<uint32_t> rows(all.begin(), all.begin() + 4 * k);
        std::vector<uint64_t> h(cap + 2, S64);
        std::vector<uint32_t> p(cap + 2, S32);
        CHECK(unpack_decl_rows(rows.data(), n, cap, null_one == 1 ? nullptr : h.data(),
                               null_one == 2 ? nullptr : p.data()) == n);
        for (uint32_t i = 0; i < cap + 2; ++i) {
          const bool set = i < k;
          CHECK(h[i] == (set && null_one != 1 ? ((uint64_t)(i + 1) << 32 | (uint32_t)~i) : S64));
          CHECK(p[i] == (set && null_one != 2 ? 2048 * i : S32));
        }
      }
    }
  }
  puts("ok decl_rows");
}

void case_ref_rows() {
  // (hash, time, kind, index) as the waves might record them: out of time
  // order, two rows of time 7 (their row order must survive), every kind, the
  // largest index
  struct Row { uint64_t hash; uint32_t time, kind, ref; };
  const Row in[] = {
      {0x1111111122222222ull, 9, 2, 5},
      {0x3333333344444444ull, 7, 1, 0},
      {0x5555555566666666ull, 3, 0, (1u << 30) - 1u},
      {0x7777777788888888ull, 7, 3, 1},
      {0x99999999AAAAAAAAull, 1, 0, 2},
  };
  const uint32_t n = 5;
  const uint32_t want[] = {4, 2, 1, 3, 0};                    // by time; the two 7s in row order
  std::vector<uint32_t> rows(4 * n);
  for (uint32_t i = 0; i < n; ++i) {
    rows[4 * i] = (uint32_t)in[i].hash;
    rows[4 * i + 1] = (uint32_t)(in[i].hash >> 32);
    rows[4 * i + 2] = in[i].time;
    rows[4 * i + 3] = in[i].kind << 30 | in[i].ref;
  }
  for (uint32_t cap : {0u, 1u, 3u, n, n + 2}) {               // (the cap cuts the sorted list, not the rows)
    for (int null_one = 0; null_one < 4; ++null_one) {
      std::vector<uint64_t> h(cap + 2, S64);
      std::vector<uint32_t> kd(cap + 2, S32), rf(cap + 2, S32);
      CHECK(unpack_ref_rows(rows.data(), n, cap, null_one == 1 ? nullptr : h.data(),
                            null_one == 2 ? nullptr : kd.data(), null_one == 3 ? nullptr : rf.data()) == n);
      for (uint32_t j = 0; j < cap + 2; ++j) {
        const bool set = j < (n < cap ? n : cap);
        const Row& r = in[want[set ? j : 0]];
        CHECK(h[j] == (set && null_one != 1 ? r.hash : S64));
        CHECK(kd[j] == (set && null_one != 2 ? r.kind : S32));
        CHECK(rf[j] == (set && null_one != 3 ? r.ref : S32));
      }
    }
  }
  CHECK(unpack_ref_rows(nullptr, 0, 4, nullptr, nullptr, nullptr) == 0);
  puts("ok ref_rows");
}

void case_fits() {
  CHECK(fresh_cache_fits(true, 16, 16));                      // at the limit
  CHECK(!fresh_cache_fits(true, 16, 17));                     // one above it
  CHECK(fresh_cache_fits(true, 16, 0));
  CHECK(fresh_cache_fits(false, 0, 17) && fresh_cache_fits(false, 16, 0xFFFFFFFFu));   // neither bounded nor a pair
  // the three bounds, at the byte where each steps
  CHECK(chunk_declarations(16 * 2048 + 2047) == 16 && chunk_declarations(17 * 2048) == 17);
  CHECK(group_declarations(16 * 2048 + 2047) == 16 && group_declarations(17 * 2048) == 17);
  CHECK(encoded_extracts(17 * 2050 - 1) == 16 && encoded_extracts(17 * 2050) == 17);
  CHECK(chunk_declarations(0) == 0 && encoded_extracts(2049) == 0);
  // the disk tiers: none or one, no unknown bit
  CHECK(disk_flags_valid(0) && disk_flags_valid(XCG_DISK_HOST) && disk_flags_valid(XCG_DISK_DEVICE));
  CHECK(!disk_flags_valid(XCG_DISK_HOST | XCG_DISK_DEVICE) && !disk_flags_valid(4) && !disk_flags_valid(1u << 31));
  CHECK(pow2_at_least(0) == 1 && pow2_at_least(1) == 1 && pow2_at_least(1024) == 1024 && pow2_at_least(1025) == 2048);
  puts("ok fits");
}

// The result words of one per-call decode launch, as decode_small_kernel
// leaves them: in a heap buffer of exactly SD_RES_WORDS words.
struct Results {
  std::vector<uint64_t> w;
  Results() : w(xcg::SD_RES_WORDS, 0) {}
};
struct CallOut {
  uint64_t count = 100, out_len = S64, consumed = S64;
  int32_t status = (int32_t)S32;
  uint32_t nunknown = S32, nextract = S32;
  std::vector<uint8_t> out;
  std::vector<uint64_t> unknown, extract;
  CallOut(size_t outb, uint32_t ucap, uint32_t ecap) : out(outb, 0xA5), unknown(ucap + 2, S64), extract(ecap + 2, S64) {}
  int run(const Results& r, const std::vector<uint8_t>& h_o, uint32_t ucap, uint32_t ecap) {
    return decode_call_results(&count, r.w.data(), h_o.data(), out.data(), &out_len, &consumed, &status, unknown.data(),
                               ucap, &nunknown, extract.data(), ecap, &nextract);
  }
  bool untouched() const {
    for (uint8_t b : out) if (b != 0xA5) return false;
    for (uint64_t v : unknown) if (v != S64) return false;
    for (uint64_t v : extract) if (v != S64) return false;
    return count == 100 && consumed == S64 && status == (int32_t)S32 && nunknown == S32 && nextract == S32;
  }
};

void case_results() {
  using namespace xcg;
  CHECK(SD_RES_UNKNOWN == 8 && SD_RES_EXTRACT == 8 + 2048 && SD_RES_STICKY == 8 + 2048 + 1024 &&
        SD_RES_WORDS == SD_RES_STICKY + 1);
  const std::vector<uint8_t> h_o = {1, 2, 3, 4, 5};
  {  // fallback 1: the batch path takes it, nothing written
    Results r;
    r.w[SDR_FALLBACK] = SD_FB_BATCH;
    r.w[SDR_OUT_LEN] = 5; r.w[SDR_DECLARES] = 3; r.w[SDR_UNKNOWNS] = 2; r.w[SDR_EXTRACTS] = 1;
    CallOut o(5, 4, 4);
    CHECK(o.run(r, h_o, 4, 4) == XCG_ENOTSUP);
    CHECK(o.untouched() && o.out_len == S64);
  }
  {  // fallback 2: more room needed, the size reported and nothing else
    Results r;
    r.w[SDR_FALLBACK] = SD_FB_ROOM;
    r.w[SDR_NEED] = 4098;
    CallOut o(5, 4, 4);
    CHECK(o.run(r, h_o, 4, 4) == XCG_EOVERFLOW);
    CHECK(o.out_len == 4098 && o.untouched());
  }
  {  // the sticky word set: the cache is full, whatever else the words say
    Results r;
    r.w[SD_RES_STICKY] = 4;
    r.w[SDR_OUT_LEN] = 5;
    CallOut o(5, 4, 4);
    CHECK(o.run(r, h_o, 4, 4) == XCG_EOVERFLOW);
    CHECK(o.untouched() && o.out_len == S64);
    r.w[SD_RES_STICKY] = 1ull << 32;                          // (only the word's low half is the status)
    CHECK(o.run(r, h_o, 4, 4) == XCG_OK);
  }
  // unknown hashes: sorted, cut at the cap -- below, at and above the count
  const uint64_t unk[3] = {0x30, 0x10, 0x20};
  for (uint32_t cap : {2u, 3u, 5u}) {
    Results r;
    r.w[SDR_OUT_LEN] = 5; r.w[SDR_CONSUMED] = 77; r.w[SDR_STATUS] = (uint64_t)(int64_t)-1; r.w[SDR_DECLARES] = 3;
    r.w[SDR_UNKNOWNS] = 3;
    for (int i = 0; i < 3; ++i) r.w[SD_RES_UNKNOWN + i] = unk[i];
    CallOut o(5, cap, 4);
    CHECK(o.run(r, h_o, cap, 4) == XCG_OK);
    CHECK(o.out == h_o && o.out_len == 5 && o.consumed == 77 && o.status == -1 && o.count == 103);
    const uint32_t k = cap < 3 ? cap : 3;
    CHECK(o.nunknown == k);
    for (uint32_t i = 0; i < cap + 2; ++i) CHECK(o.unknown[i] == (i < k ? 0x10u * (i + 1) : S64));
    CHECK(o.nextract == 0);
  }
  // EXTRACT hashes: delivered when the count fits the caller's cap and SD_EMAX
  for (uint32_t ne : {0u, 3u, 4u, SD_EMAX, SD_EMAX + 1}) {
    for (uint32_t cap : {3u, SD_EMAX + 2}) {
      Results r;
      r.w[SDR_EXTRACTS] = ne;
      for (uint32_t i = 0; i < SD_EMAX; ++i) r.w[SD_RES_EXTRACT + i] = 0xE000 + i;
      CallOut o(5, 4, cap);
      o.nextract = XCG_NO_REFERENCES;
      CHECK(o.run(r, h_o, 4, cap) == XCG_OK);
      const bool fits = ne <= cap && ne <= SD_EMAX;
      CHECK(o.nextract == (fits ? ne : XCG_NO_REFERENCES));
      for (uint32_t i = 0; i < cap + 2; ++i) CHECK(o.extract[i] == (fits && i < ne ? 0xE000u + i : S64));
      CHECK(o.out_len == 0 && o.nunknown == 0);
    }
  }
  puts("ok results");
}

}  // namespace

int main() {
  case_status();
  case_uuid();
  case_decl_rows();
  case_ref_rows();
  case_fits();
  case_results();
  return 0;
}
