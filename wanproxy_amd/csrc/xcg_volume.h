// The on-disk format of an XCodecDisk volume (xcodec/xcodec_cache_disk.{h,cc}):
// the one module that knows what the file looks like.  Host code only, no GPU
// runtime (plain g++ compiles it: oracle/volume_harness.cc runs it under sanitizers).
//
//   blocks of 2048 bytes:  18 registry blocks (56 UUIDs of 36 characters each,
//   xuid = position), nb index blocks (a u64 counter, 0 = unused, then 204
//   entries of u16 xuid + u64 hash, hash 0 = none), nb * 204 data blocks.
#pragma once
#include <stdint.h>
#include <sys/types.h>

#include <functional>
#include <string>
#include <vector>

#include "xcg_rc.h"

namespace xcg {

constexpr uint32_t DISK_ENTRIES = 204;   // XCDFS_ENTRIES_PER_INDEX_BLOCK, xcodec_cache_disk.cc:87
constexpr uint32_t REG_BLOCKS = 18, REG_ENTRIES = 2048 / 36, CHECK_BOUNDARY = 80, XUIDS = 1024;
// The ring's empty values, in a reopened volume's image as in the device arrays it is copied to.
constexpr uint64_t NOENT = ~0ull;        // no disk entry
constexpr uint64_t NOKEY = ~0ull;

// The volume (xcodec_cache_disk.cc:72-101): its size, per index block the
// counter it was last written with, the counter of the block being filled,
// the registry's blocks and the UUID each xuid has there.
struct Volume {
  uint64_t bytes = 0;
  uint64_t nb = 0;                 // index blocks
  uint32_t D = 0;                  // nb * 204 data blocks
  std::vector<uint8_t> reg;
  std::vector<std::string> uuid;
  std::vector<uint64_t> ctr;
  uint64_t ibc = 1;
  uint64_t dclock = 0;             // entries written to the disk (every front)
  // a reopened volume's ring (per data block the hash, the entry number in the
  // engine's clock model, the xuid; the blocks' bytes) while no device holds it
  std::vector<uint64_t> h_key, h_ent;
  std::vector<uint32_t> h_xuid;
  std::vector<uint8_t> h_data;
};

// A fresh volume of disk_bytes.  XCG_RC_INVAL: no room for the registry and one index block, or too many data blocks.
int volume_geometry(Volume* V, uint64_t disk_bytes);
// The reload of a volume file (geometry set).  0, or XCG_RC_NOENT: the file cannot be read.
int volume_load(Volume* V, int fd);
// The file as the reference's stands now, from the ring's key[D], xuid[D] and data[D * 2048].
// 0, XCG_RC_NOENT: the path cannot be opened, XCG_RC_HIP: a write failed.
int volume_write(const Volume& V, const char* path, const uint64_t* key, const uint32_t* xuid, const uint8_t* data);
void volume_advance(Volume* V, uint64_t appends);
void volume_reset(Volume* V);
void volume_head(const Volume& V, uint64_t* index_block, uint64_t* next);

void registry_write(Volume* V, uint32_t xuid, const char* u36);
// Which xuid a new front takes, bound(x) telling the xuids that have a front;
// *name: the UUID to register for it (empty: the one it has).  XCG_RC_INVAL: none,
// XCG_RC_HIP: no UUID could be generated.
int volume_front_xuid(const Volume& V, const char* uuid36, int want_xuid, const std::function<bool(uint32_t)>& bound,
                      std::string* name);
void volume_register(Volume* V, uint32_t xuid, const std::string& name);

bool uuid_ok(const uint8_t* u);
bool gen_uuid(char out[37]);
bool pread_all(int fd, uint8_t* p, size_t n, off_t off);
bool pwrite_all(int fd, const uint8_t* p, size_t n, off_t off);

}  // namespace xcg
