// The host plan of a decode batch over several windows
// (wanproxy_amd/csrc/xcg_decode_windows_plan.h) on the CPU, against a naive
// model: the window-major stable order of the chunks, each window's first
// position in it, and every refusal.  Stand-alone; tests/test_decode_windows_plan.py
// builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../wanproxy_amd/csrc/xcg_decode_windows_plan.h"

using namespace xcg;

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

// The plan by definition: for each window in turn, its chunks in batch order.
static void naive(const std::vector<uint32_t>& cw, uint32_t nw, std::vector<uint32_t>& order,
                  std::vector<uint32_t>& first) {
  order.clear();
  first.assign(nw + 1, 0);
  for (uint32_t w = 0; w < nw; ++w) {
    first[w] = (uint32_t)order.size();
    for (uint32_t i = 0; i < cw.size(); ++i)
      if (cw[i] == w) order.push_back(i);
  }
  first[nw] = (uint32_t)order.size();
}

static void same_as_naive(const std::vector<uint32_t>& cw, uint32_t nw) {
  const uint32_t n = (uint32_t)cw.size();
  // (exact-size heap arrays: a write past either end is the sanitizer's to report)
  std::vector<uint32_t> order(n), first(nw + 1, 0xDEADBEEF), o2, f2;
  CHECK(dec_windows_plan(cw.data(), n, nw, order.data(), first.data()) == DEC_PLAN_OK);
  naive(cw, nw, o2, f2);
  CHECK(order == o2);
  CHECK(first == f2);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

int main() {
  // ---- orders and first positions
  same_as_naive({}, 1);                                      // no chunk
  same_as_naive({}, 5);
  same_as_naive({0, 0, 0, 0}, 1);                            // one window
  same_as_naive({0, 0, 0, 0}, 3);                            // windows no chunk names
  same_as_naive({2, 2}, 3);
  same_as_naive({0, 1, 0, 2, 1, 0, 2}, 3);
  {
    std::vector<uint32_t> cw(1000);                          // n windows of one chunk, backwards
    for (uint32_t i = 0; i < 1000; ++i) cw[i] = 999 - i;
    same_as_naive(cw, 1000);
  }
  {
    std::vector<uint32_t> cw(DEC_WINDOWS_MAX);               // the cap itself
    for (uint32_t i = 0; i < DEC_WINDOWS_MAX; ++i) cw[i] = (i * 7919u) % DEC_WINDOWS_MAX;
    std::vector<uint32_t> order(cw.size()), first(DEC_WINDOWS_MAX + 1);
    CHECK(dec_windows_plan(cw.data(), (uint32_t)cw.size(), DEC_WINDOWS_MAX, order.data(), first.data()) == DEC_PLAN_OK);
    for (uint32_t w = 0; w < DEC_WINDOWS_MAX; ++w) CHECK(first[w] == w && cw[order[w]] == w);
  }
  for (int round = 0; round < 300; ++round) {
    const uint32_t nw = 1 + rnd() % 40, n = rnd() % 200;
    std::vector<uint32_t> cw(n);
    for (uint32_t i = 0; i < n; ++i) cw[i] = rnd() % nw;
    same_as_naive(cw, nw);
  }
  if (!g_fail) puts("ok order");

  // ---- refusals: nothing written
  {
    const uint32_t cw[3] = {0, 1, 0};
    uint32_t order[3] = {7, 7, 7}, first[3] = {7, 7, 7};
    CHECK(dec_windows_plan(cw, 3, 0, order, first) == DEC_PLAN_INVAL);                       // no window
    CHECK(dec_windows_plan(cw, 3, DEC_WINDOWS_MAX + 1, order, first) == DEC_PLAN_INVAL);     // above the cap
    CHECK(dec_windows_plan(cw, 3, 1, order, first) == DEC_PLAN_INVAL);                       // chunk 1 names window 1
    CHECK(dec_windows_plan(nullptr, 3, 2, order, first) == DEC_PLAN_INVAL);
    CHECK(dec_windows_plan(cw, 3, 2, nullptr, first) == DEC_PLAN_INVAL);
    CHECK(dec_windows_plan(cw, 3, 2, order, nullptr) == DEC_PLAN_INVAL);
    for (int k = 0; k < 3; ++k) CHECK(order[k] == 7 && first[k] == 7);
    CHECK(dec_windows_plan(nullptr, 0, 2, nullptr, first) == DEC_PLAN_OK);                   // no chunk needs no arrays
    CHECK(first[0] == 0 && first[1] == 0 && first[2] == 0);
    CHECK(dec_windows_plan(cw, 3, 2, order, first) == DEC_PLAN_OK);
  }
  {
    int a, b, c;
    const void* ok[3] = {&a, &b, &c};
    const void* twice[3] = {&a, &b, &a};
    const void* null1[3] = {&a, nullptr, &c};
    CHECK(dec_windows_distinct(ok, 3) == DEC_PLAN_OK);
    CHECK(dec_windows_distinct(ok, 1) == DEC_PLAN_OK);
    CHECK(dec_windows_distinct(twice, 3) == DEC_PLAN_INVAL);
    CHECK(dec_windows_distinct(twice, 2) == DEC_PLAN_OK);
    CHECK(dec_windows_distinct(null1, 3) == DEC_PLAN_INVAL);
    CHECK(dec_windows_distinct(nullptr, 3) == DEC_PLAN_INVAL);
    CHECK(dec_windows_distinct(ok, 0) == DEC_PLAN_INVAL);
    CHECK(dec_windows_distinct(ok, DEC_WINDOWS_MAX + 1) == DEC_PLAN_INVAL);
  }
  if (!g_fail) puts("ok refusals");
  return g_fail ? 1 : 0;
}
