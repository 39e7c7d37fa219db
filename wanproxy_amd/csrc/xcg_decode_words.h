// The batch decoder's scratch words and the per-call decoder's result words,
// by name: the layouts the decode units (xcg_decode*.hip), the context
// (xcg_ctx.hip) and the ABI layer (xcg_api_decode.hip) share.  Several words
// are cleared or copied together with their neighbours; each such range is
// pinned by a static_assert beside its struct, so reordering a member fails to
// compile instead of reading a neighbour's word.  No HIP and no other header:
// xcg_api_host.h includes it for the CPU harness (oracle/api_host_harness.cc).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace xcg {

// ---- the batch decoder (xcg_launch_decode)

// XcgDecodeScratch::scratch, device memory.
struct DecScratch {
  uint64_t total_out;    // exclusive scan of the decoded lengths: the batch's output bytes
  uint64_t block_pos;    // min stream position of an unresolvable REF (~0: none)
  uint64_t berr_pos;     // min stream position of a BACKREF to an empty slot (~0: none); bounded and pair
                         //   contexts: written before the classify passes, which read it as their cap
  uint64_t dup_minus1;   // duplicate EXTRACTs listed, minus one (starts at ~0)
  uint64_t n_decl;       // declares of the batch
  uint64_t n_bref;       // BACKREFs of the batch
  uint64_t t_end;        // declares before the stop point
  uint64_t reserved;
};
// one memset (0xFF) clears the two stop positions and the duplicate counter
constexpr size_t DEC_CLEAR_BYTES = 24;
static_assert(offsetof(DecScratch, berr_pos) == offsetof(DecScratch, block_pos) + 8 &&
                  offsetof(DecScratch, dup_minus1) == offsetof(DecScratch, block_pos) + 16,
              "block_pos, berr_pos, dup_minus1: one memset");

// XcgDecodeScratch::counts, device memory: cleared by one memset of the struct.
struct DecCounts {
  uint32_t unknown;      // distinct unknown hashes (decode_refcheck_kernel)
  uint32_t flagged;      // hashes whose EXTRACTs differ in bytes (dec_dup_kernel)
  uint32_t occurrences;  // EXTRACTs of the flagged hashes (dec_occ_*_kernel)
  uint32_t reserved;
};

// The classify pass's stop position and change count (bounded and pair
// contexts), device memory inside the pass's temporary.
struct DecClassifyWords {
  uint64_t block;        // min stream position of an unknown REF this pass (~0: none)
  uint32_t changes;      // chunks whose classification changed
  uint32_t reserved;
};

// XcgDecodeScratch::h_scratch, pinned host memory: where the words above come back.
struct DecHostWords {
  uint64_t total_out, block_pos, berr_pos;   // one copy of DecScratch's first three (sizing pass)
  uint64_t dup_minus1, n_decl, n_bref;       // one copy of DecScratch's next three (scan)
  uint32_t unknown, flagged;                 // one copy of DecCounts' first two (sizing pass)
  uint64_t t_end;                            // the ABI layer's copy of DecScratch::t_end, after the batch
  DecClassifyWords cls;                      // one copy per classify pass (the pair reads `block` only)
  uint64_t status;                           // the context's sticky word (low 32 bits copied)
  uint64_t status_wb;                        //   and the value written back with bit 9 cleared
  uint64_t reuse[3];                         // xcg_debug_decode_reuse: duplicates, flagged hashes, REUSE path taken
  uint64_t reserved;
};
constexpr size_t DEC_SIZING_BYTES = 24, DEC_SCAN_BYTES = 24, DEC_COUNTS_BYTES = 8;
static_assert(offsetof(DecScratch, total_out) == 0 && offsetof(DecHostWords, total_out) == 0 &&
                  offsetof(DecScratch, berr_pos) == 16 && offsetof(DecHostWords, berr_pos) == 16 &&
                  offsetof(DecScratch, block_pos) == offsetof(DecHostWords, block_pos),
              "total_out, block_pos, berr_pos: one copy");
static_assert(offsetof(DecScratch, n_decl) == offsetof(DecScratch, dup_minus1) + 8 &&
                  offsetof(DecScratch, n_bref) == offsetof(DecScratch, dup_minus1) + 16 &&
                  offsetof(DecHostWords, n_decl) == offsetof(DecHostWords, dup_minus1) + 8 &&
                  offsetof(DecHostWords, n_bref) == offsetof(DecHostWords, dup_minus1) + 16,
              "dup_minus1, n_decl, n_bref: one copy");
static_assert(offsetof(DecCounts, unknown) == 0 && offsetof(DecCounts, flagged) == 4 &&
                  offsetof(DecHostWords, flagged) == offsetof(DecHostWords, unknown) + 4,
              "unknown, flagged: one copy");
static_assert(offsetof(DecClassifyWords, changes) == 8 && sizeof(DecClassifyWords) == 16,
              "block, changes: one copy");
static_assert(sizeof(DecScratch) == 64 && sizeof(DecCounts) == 16 && sizeof(DecHostWords) == 128, "");

// ---- the per-call decoder (decode_small_kernel): its result words, u64 each

// The header, then SD_UMAX unknown hashes, then SD_EMAX EXTRACT hashes (op
// order), then the context's sticky word.
enum : uint32_t {
  SDR_OUT_LEN = 0,    // decoded bytes
  SDR_CONSUMED,       // input bytes parsed
  SDR_STATUS,         // the call's status (int64)
  SDR_DECLARES,       // declares before the stop
  SDR_UNKNOWNS,       // unknown hashes listed
  SDR_FALLBACK,       // SD_FB_*
  SDR_EXTRACTS,       // EXTRACTs before the stop
  SDR_NEED,           // decoded size (SD_FB_ROOM: the room the call needs)
  SDR_HEADER
};
enum : uint64_t { SD_FB_DONE = 0, SD_FB_BATCH = 1, SD_FB_ROOM = 2 };   // done; take the batch path; more room needed
constexpr uint32_t SD_UMAX = 2048, SD_EMAX = 1024;
constexpr uint32_t SD_PHASES = 11;       // clock stamps at the phase boundaries (diagnostics)
// A call's input up to this size is staged in LDS first (with the tables:
// 80 KiB + 78 KiB of the 160 KiB): the op walk is a chain of dependent reads,
// one per op, that would each wait on HBM.
constexpr uint32_t SD_LDS_IN = 76000;
constexpr uint32_t SD_RES_UNKNOWN = SDR_HEADER, SD_RES_EXTRACT = SD_RES_UNKNOWN + SD_UMAX,
                   SD_RES_STICKY = SD_RES_EXTRACT + SD_EMAX, SD_RES_WORDS = SD_RES_STICKY + 1;
constexpr uint64_t SD_SCRATCH_PER_OP = 40;   // device scratch: a uint4 op, a u64 hash and a uint4 declare record
static_assert(SDR_HEADER == 8, "eight header words");

}  // namespace xcg
