// The host's plan of a batch decode over several BACKREF windows
// (xcg_decode_batch_windows): chunk i is a decode() call on decoder
// chunk_window[i], and each decoder numbers its own declares.  The device
// scans the chunks' declare counts in the window-major stable order built
// here -- every chunk of window 0 in batch order, then window 1's, ... -- so a
// chunk's base is the sum over the earlier chunks of its own window, and a
// window's records lie together.  No HIP and no other header of the library:
// tests/native/decode_windows_plan_harness.cc runs it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace xcg {

// Windows one call takes: 256 tail records (4 KiB) of scratch each.
constexpr uint32_t DEC_WINDOWS_MAX = 65536;

enum : int { DEC_PLAN_OK = 0, DEC_PLAN_INVAL = 1 };

// order[n]: the chunks window-major, batch order kept inside a window;
// first[n_windows + 1]: window w's chunks are order[first[w] .. first[w + 1]),
// first[n_windows] = n.  Refuses (nothing written) a null array, no window or
// more than DEC_WINDOWS_MAX, and a chunk that names a window >= n_windows.
inline int dec_windows_plan(const uint32_t* chunk_window, uint32_t n, uint32_t n_windows, uint32_t* order,
                            uint32_t* first) {
  if (n_windows == 0 || n_windows > DEC_WINDOWS_MAX || !first || (n && (!chunk_window || !order)))
    return DEC_PLAN_INVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (chunk_window[i] >= n_windows) return DEC_PLAN_INVAL;
  for (uint32_t w = 0; w <= n_windows; ++w) first[w] = 0;
  for (uint32_t i = 0; i < n; ++i) ++first[chunk_window[i] + 1];
  for (uint32_t w = 0; w < n_windows; ++w) first[w + 1] += first[w];
  std::vector<uint32_t> next(first, first + n_windows);
  for (uint32_t i = 0; i < n; ++i) order[next[chunk_window[i]]++] = i;
  return DEC_PLAN_OK;
}

// The window list itself: every entry non-null, none listed twice.
inline int dec_windows_distinct(const void* const* windows, uint32_t n_windows) {
  if (!windows || n_windows == 0 || n_windows > DEC_WINDOWS_MAX) return DEC_PLAN_INVAL;
  std::vector<const void*> s(windows, windows + n_windows);
  std::sort(s.begin(), s.end(), std::less<const void*>());
  if (s[0] == nullptr) return DEC_PLAN_INVAL;
  for (uint32_t w = 1; w < n_windows; ++w)
    if (s[w] == s[w - 1]) return DEC_PLAN_INVAL;
  return DEC_PLAN_OK;
}

}  // namespace xcg
