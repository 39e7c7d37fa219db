// The ABI layer's host-only helpers, each written once: the driver-code map,
// the registry's UUID key, the argument predicates, the unpackers of a
// batch's declaration / reference rows and of the per-call decoder's result
// words.  No HIP here, so the whole file runs
// under sanitizers on the CPU (oracle/api_host_harness.cc).
#pragma once
#include <alloca.h>
#include <ctype.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/xcgpu.h"
#include "xcg_decode_words.h"
#include "xcg_rc.h"

// A driver's return code (0 or an XCG_RC_* value) as an ABI status; anything
// else is a HIP error.
static inline int status_of(int rc) {
  switch (rc) {
    case 0: return XCG_OK;
    case XCG_RC_NOENT: return XCG_ENOENT;
    case XCG_RC_NOMEM: return XCG_ENOMEM;
    case XCG_RC_INVAL: return XCG_EINVAL;
    case XCG_RC_OVERFLOW: return XCG_EOVERFLOW;
    case XCG_RC_NOTSUP: return XCG_ENOTSUP;
    default: return XCG_EHIP;      // XCG_RC_HIP and whatever is not a driver code
  }
}

static inline bool uuid_key(const char* u, std::string* key) {     // the 8-4-4-4-12 form UUID::decode takes
  if (!u) return false;
  std::string k(36, ' ');
  for (int i = 0; i < 36; ++i) {
    const char c = u[i];
    const bool dash = i == 8 || i == 13 || i == 18 || i == 23;
    if (dash ? c != '-' : !isxdigit((unsigned char)c)) return false;
    k[i] = (char)tolower((unsigned char)c);
  }
  *key = k;
  return true;
}

static inline uint32_t pow2_at_least(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return (uint32_t)p;
}

// xcg_disk_create_ex / _open / _open_fd: no unknown tier bit, and not both tiers.
static inline bool disk_flags_valid(uint32_t flags) {
  return !(flags & ~(XCG_DISK_HOST | XCG_DISK_DEVICE)) && flags != (XCG_DISK_HOST | XCG_DISK_DEVICE);
}

// Independent and grouped calls give every chunk / group a fresh cache.  On a
// bounded or pair context (limited: a memory limit of `limit` segments) that
// cache must evict nothing, which holds while everything one fresh cache can
// be asked to enter fits the limit; an unbounded context takes any count.
static inline bool fresh_cache_fits(bool limited, uint32_t limit, uint32_t count) {
  return !limited || count <= limit;
}
// The most one fresh cache can enter: a chunk of max_chunk_len input bytes
// declares at most one segment per 2048 of them, and so does a group of
// max_group_len summed input bytes; of encoded bytes, every EXTRACT that
// enters takes 2 + 2048 (lookups enter nothing).
static inline uint32_t chunk_declarations(uint32_t max_chunk_len) { return max_chunk_len / XCG_SEGMENT_LENGTH; }
static inline uint32_t group_declarations(uint32_t max_group_len) { return max_group_len / XCG_SEGMENT_LENGTH; }
static inline uint32_t encoded_extracts(uint32_t max_encoded_len) {
  return max_encoded_len / (2u + XCG_SEGMENT_LENGTH);
}

// A reference row's last word: kind << 30 | index (EV_* and EV_REF_MASK, xcg_cache.h).
constexpr uint32_t ROW_KIND_SHIFT = 30, ROW_REF_MASK = (1u << ROW_KIND_SHIFT) - 1u;

// A chunk's declaration rows, uint4 (hash lo, hash hi, position, -) as 4 words
// each, to (hash, position): the first min(n, cap) of them -- no more rows are
// read, no other entries written; each output array may be null.  Returns n.
static inline uint32_t unpack_decl_rows(const uint32_t* rows, uint32_t n, uint32_t cap, uint64_t* h_hash,
                                        uint32_t* h_pos) {
  const uint32_t k = n < cap ? n : cap;
  for (uint32_t i = 0; i < k; ++i) {
    if (h_hash) h_hash[i] = ((uint64_t)rows[4 * i + 1] << 32) | rows[4 * i];
    if (h_pos) h_pos[i] = rows[4 * i + 2];
  }
  return n;
}

// A chunk's n reference rows (hash lo, hash hi, time, kind << 30 | index), in
// the order the waves recorded them, to stream order: sorted by time, equal
// times in row order; then the first min(n, cap) as (hash, kind, index).
// kind: EV_ENTER 0, EV_HIT 1, EV_GHIT 2, EV_GMISS 3 (xcg_cache.h).  Returns n.
static inline uint32_t unpack_ref_rows(const uint32_t* rows, uint32_t n, uint32_t cap, uint64_t* h_hash,
                                       uint32_t* h_kind, uint32_t* h_ref) {
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return rows[4ull * a + 2] < rows[4ull * b + 2]; });
  const uint32_t k = n < cap ? n : cap;
  for (uint32_t j = 0; j < k; ++j) {
    const uint32_t* e = rows + 4ull * order[j];
    if (h_hash) h_hash[j] = ((uint64_t)e[1] << 32) | e[0];
    if (h_kind) h_kind[j] = e[3] >> ROW_KIND_SHIFT;
    if (h_ref) h_ref[j] = e[3] & ROW_REF_MASK;
  }
  return n;
}

// The result words of one decode_small_kernel launch (xcg_decode_words.h) ->
// the call's outputs.  XCG_ENOTSUP: the kernel declined (fallback); nothing
// was written.  *win_count: the window's declare count, advanced.
static inline int decode_call_results(uint64_t* win_count, const uint64_t* h_res, const uint8_t* h_o, uint8_t* h_out,
                                      uint64_t* h_out_len, uint64_t* h_consumed, int32_t* h_status,
                                      uint64_t* h_unknown, uint32_t unknown_cap, uint32_t* h_nunknown,
                                      uint64_t* h_extract_hash, uint32_t extract_cap, uint32_t* h_nextract) {
  using namespace xcg;
  if ((uint32_t)h_res[SD_RES_STICKY]) return XCG_EOVERFLOW;   // (cache capacity: the sticky word)
  if (h_res[SDR_FALLBACK] == SD_FB_ROOM) {
    *h_out_len = h_res[SDR_NEED];
    return XCG_EOVERFLOW;
  }
  if (h_res[SDR_FALLBACK] != SD_FB_DONE) return XCG_ENOTSUP;
  const uint64_t ol = h_res[SDR_OUT_LEN];
  if (ol) memcpy(h_out, h_o, ol);
  *h_out_len = ol;
  *h_consumed = h_res[SDR_CONSUMED];
  *h_status = (int32_t)(int64_t)h_res[SDR_STATUS];
  *win_count += h_res[SDR_DECLARES];
  const uint32_t nu = (uint32_t)h_res[SDR_UNKNOWNS];
  uint64_t* u = (uint64_t*)alloca(8ull * (nu ? nu : 1));
  memcpy(u, h_res + SD_RES_UNKNOWN, 8ull * nu);
  std::sort(u, u + nu);
  const uint32_t ku = nu < unknown_cap ? nu : unknown_cap;
  if (h_unknown && ku) memcpy(h_unknown, u, 8ull * ku);
  *h_nunknown = ku;
  const uint32_t ne = (uint32_t)h_res[SDR_EXTRACTS];
  if (ne <= extract_cap && ne <= SD_EMAX) {
    if (ne && h_extract_hash) memcpy(h_extract_hash, h_res + SD_RES_EXTRACT, 8ull * ne);
    *h_nextract = ne;
  }
  return XCG_OK;
}
