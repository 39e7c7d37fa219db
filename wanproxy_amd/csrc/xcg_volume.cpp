// The XCodecDisk volume file: see xcg_volume.h.
#include "xcg_volume.h"

#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <map>
#include <unordered_map>

#include "xcg_segment.h"

namespace xcg {

int volume_geometry(Volume* V, uint64_t disk_bytes) {
  const uint64_t blocks = disk_bytes / SEG;
  if (blocks <= 18) return XCG_RC_INVAL;
  const uint64_t nb = (blocks - 18) / (1 + DISK_ENTRIES);   // xcodec_cache_disk.cc:110-111
  if (nb == 0 || nb * DISK_ENTRIES >= (1ull << 29)) return XCG_RC_INVAL;
  V->nb = nb;
  V->D = (uint32_t)(nb * DISK_ENTRIES);
  V->bytes = disk_bytes;
  V->ctr.assign(nb, 0);
  V->reg.assign(18 * 2048, 0);
  V->uuid.assign(1024, std::string());
  return 0;
}

// XCodecDisk::registry_write (xcodec_cache_disk.cc:603-627): the xuid's
// registry block with the UUID patched in, written back to block 0 (as the
// reference does).  The 18 registry blocks hold 56 UUIDs each: xuids 1008 to
// 1023 have no slot (the reference would take index block 0 for their
// registry block) and are fronts in memory only.
void registry_write(Volume* V, uint32_t xuid, const char* u36) {
  if (xuid >= REG_BLOCKS * REG_ENTRIES) return;
  uint8_t blk[2048];
  memcpy(blk, &V->reg[(xuid / REG_ENTRIES) * 2048], 2048);
  memcpy(&blk[(xuid % REG_ENTRIES) * 36], u36, 36);
  memcpy(&V->reg[0], blk, 2048);
}

// uuid_parse's format (common/uuid/uuid_libuuid.cc UUID::decode): 8-4-4-4-12 hex.
bool uuid_ok(const uint8_t* u) {
  for (int i = 0; i < 36; ++i) {
    if (i == 8 || i == 13 || i == 18 || i == 23) {
      if (u[i] != '-') return false;
    } else if (!isxdigit(u[i])) {
      return false;
    }
  }
  return true;
}

// Whole-range file I/O: one read()/write() moves at most 0x7ffff000 bytes on
// Linux, so a volume past 2 GiB takes several.  A read that meets the end of
// the file leaves the rest zero (the reference's ftruncate'd volume reads as
// zeros there, xcodec_cache_disk.cc:853-860).
bool pread_all(int fd, uint8_t* p, size_t n, off_t off) {
  while (n > 0) {
    const ssize_t r = pread(fd, p, n, off);
    if (r < 0 && errno == EINTR) continue;
    if (r < 0) return false;
    if (r == 0) {
      memset(p, 0, n);
      return true;
    }
    p += r;
    n -= (size_t)r;
    off += r;
  }
  return true;
}

bool pwrite_all(int fd, const uint8_t* p, size_t n, off_t off) {
  while (n > 0) {
    const ssize_t r = pwrite(fd, p, n, off);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return false;
    p += r;
    n -= (size_t)r;
    off += r;
  }
  return true;
}

// UUID::generate (common/uuid/uuid_libuuid.cc: uuid_generate + uuid_unparse):
// a random (version 4) UUID in its 36-character lower-case form.
bool gen_uuid(char out[37]) {
  uint8_t b[16];
  const int fd = ::open("/dev/urandom", O_RDONLY);
  const bool ok = fd != -1 && pread_all(fd, b, 16, 0);
  if (fd != -1) close(fd);
  if (!ok) return false;
  b[6] = (uint8_t)((b[6] & 0x0F) | 0x40);
  b[8] = (uint8_t)((b[8] & 0x3F) | 0x80);
  snprintf(out, 37, "%02x%02x%02x%02x-%02x%02x-%02x%02x-%02x%02x-%02x%02x%02x%02x%02x%02x", b[0], b[1], b[2], b[3],
           b[4], b[5], b[6], b[7], b[8], b[9], b[10], b[11], b[12], b[13], b[14], b[15]);
  return true;
}

// A reopened volume (XCodecDisk::XCodecDisk, xcodec_cache_disk.cc:107-237):
// the registry gives the fronts; index blocks are scanned in block order up
// to the first free one (counter 0); the lowest counter is the write head and
// is not loaded; the rest load in counter order, a later entry of a hash
// replacing an earlier one, the first and last 80 checked against their data
// blocks (index_load_entries :408-478); fronts left without entries leave the
// registry (registry_collect :496-528).  In the engine's clock model the write
// head's entry 0 is clock 204 * (nb + head), and a block b loaded from the last
// lap holds entries numbered from 204 * (nb + head - ((head - b) mod nb)): each
// dies when the head reaches b again, as the reference invalidates it.
int volume_load(Volume* V, int fd) {
  const uint64_t nb = V->nb, D = V->D;
  // the registry and index blocks; the data blocks go straight to h_data
  std::vector<uint8_t> vol((REG_BLOCKS + nb) * 2048);
  V->h_data.assign((size_t)D * SEG, 0);
  if (!pread_all(fd, vol.data(), vol.size(), 0) ||
      !pread_all(fd, V->h_data.data(), V->h_data.size(), (off_t)vol.size())) {
    std::vector<uint8_t>().swap(V->h_data);
    return XCG_RC_NOENT;
  }
  memcpy(&V->reg[0], &vol[0], V->reg.size());
  std::unordered_map<std::string, uint32_t> seen;
  for (uint32_t x = 0; x < REG_BLOCKS * REG_ENTRIES && x < XUIDS; ++x) {
    const uint8_t* u = &V->reg[(x / REG_ENTRIES) * 2048 + (x % REG_ENTRIES) * 36];
    bool zero = true;
    for (int i = 0; i < 36; ++i) zero &= u[i] == 0;
    if (zero || !uuid_ok(u)) continue;
    const std::string us((const char*)u, 36);
    if (seen.count(us)) continue;
    seen[us] = x;
    V->uuid[x] = us;
  }
  if (seen.empty()) {                                       // registry_load: a local UUID (:575-596)
    char u[37];
    if (!gen_uuid(u)) return XCG_RC_NOENT;
    V->uuid[0] = std::string(u, 36);
    registry_write(V, 0, u);
  }
  std::map<uint64_t, uint64_t> cmap;
  uint64_t ibc = 0;
  for (uint64_t o = 0; o < nb; ++o) {
    uint64_t counter;
    memcpy(&counter, &vol[(REG_BLOCKS + o) * 2048], 8);
    if (counter == 0) {
      cmap[0] = o;
      break;
    }
    if (counter > ibc) ibc = counter + 1;
    cmap[counter] = o;
  }
  uint64_t cib = 0;
  if (!cmap.empty()) {
    cib = cmap.begin()->second;
    cmap.erase(cmap.begin());
  }
  V->h_key.assign(D, NOKEY);
  V->h_ent.assign(D, NOENT);
  V->h_xuid.assign(D, 0xFFFFFFFFu);
  for (uint64_t o = 0; o < nb; ++o) {
    memcpy(&V->ctr[o], &vol[(REG_BLOCKS + o) * 2048], 8);
    const uint8_t* q = &vol[(REG_BLOCKS + o) * 2048 + 8];
    for (uint64_t j = 0; j < DISK_ENTRIES; ++j, q += 10) {
      uint16_t xu;
      uint64_t h;
      memcpy(&xu, q, 2);
      memcpy(&h, q + 2, 8);
      if (h == 0) continue;
      V->h_key[o * DISK_ENTRIES + j] = h;
      V->h_xuid[o * DISK_ENTRIES + j] = xu;
    }
  }
  std::vector<std::unordered_map<uint64_t, uint64_t>> index(XUIDS);   // per xuid: hash -> slot
  auto invalidate = [&](uint64_t b) {
    if (V->ctr[b] == 0) return;
    for (uint64_t i = b * DISK_ENTRIES; i < (b + 1) * DISK_ENTRIES; ++i) {
      const uint32_t xu = V->h_xuid[i];
      if (V->h_key[i] == NOKEY || xu >= XUIDS || V->uuid[xu].empty()) continue;
      auto it = index[xu].find(V->h_key[i]);
      if (it != index[xu].end() && it->second == i) index[xu].erase(it);
    }
  };
  unsigned leading = CHECK_BOUNDARY;
  while (!cmap.empty()) {
    bool check;
    if (leading != 0) {
      check = true;
      --leading;
    } else {
      check = cmap.size() <= CHECK_BOUNDARY;
    }
    const uint64_t b = cmap.begin()->second;
    cmap.erase(cmap.begin());
    for (uint64_t j = 0; j < DISK_ENTRIES; ++j) {
      const uint64_t slot = b * DISK_ENTRIES + j;
      const uint64_t h = V->h_key[slot];
      const uint32_t xu = V->h_xuid[slot];
      if (h == NOKEY || xu >= XUIDS || V->uuid[xu].empty()) continue;
      index[xu].erase(h);                                   // ("Replacing previous cache entry.")
      if (check && host_seg_hash(&V->h_data[slot * SEG]) != h) {
        if (cib > b) {                                      // rewrite the block with errors
          invalidate(b);
          cib = b;
          break;
        }
        continue;
      }
      index[xu][h] = slot;
    }
  }
  for (uint32_t x = 1; x < XUIDS; ++x) {                    // registry_collect
    if (V->uuid[x].empty() || !index[x].empty()) continue;
    static const char zero36[36] = {0};
    registry_write(V, x, zero36);
    V->uuid[x].clear();
  }
  for (uint32_t x = 0; x < XUIDS; ++x)
    for (const auto& kv : index[x]) {
      const uint64_t slot = kv.second, b = slot / DISK_ENTRIES;
      const uint64_t bn = nb + cib - ((cib + nb - b) % nb);
      V->h_ent[slot] = DISK_ENTRIES * bn + slot % DISK_ENTRIES;
    }
  V->ibc = ibc == 0 ? 1 : ibc;
  V->dclock = DISK_ENTRIES * (nb + cib);
  return 0;
}

// Write the volume as the reference's file stands now (registry, every
// written index block with its counter and entries, the data blocks).
int volume_write(const Volume& V, const char* path, const uint64_t* key, const uint32_t* xu, const uint8_t* data) {
  const uint64_t nb = V.nb, D = V.D;
  const int fd = ::open(path, O_RDWR | O_CREAT | O_TRUNC, 0600);
  if (fd == -1) return XCG_RC_NOENT;
  bool ok = ftruncate(fd, (off_t)V.bytes) == 0;
  ok = ok && pwrite_all(fd, V.reg.data(), V.reg.size(), 0);
  std::vector<uint8_t> ib(2048);
  for (uint64_t b = 0; ok && b < nb; ++b) {
    memset(ib.data(), 0, ib.size());
    if (V.ctr[b] != 0) {
      uint8_t* q = ib.data();
      memcpy(q, &V.ctr[b], 8);
      q += 8;
      for (uint64_t j = 0; j < DISK_ENTRIES; ++j, q += 10) {
        const uint64_t i = b * DISK_ENTRIES + j;
        const uint64_t h = key[i] == NOKEY ? 0 : key[i];
        const uint16_t x = h == 0 ? 0 : (uint16_t)xu[i];
        memcpy(q, &x, 2);
        memcpy(q + 2, &h, 8);
      }
    }
    ok = pwrite_all(fd, ib.data(), 2048, (off_t)((REG_BLOCKS + b) * 2048));
  }
  ok = ok && pwrite_all(fd, data, (size_t)D * SEG, (off_t)((REG_BLOCKS + nb) * 2048));
  close(fd);
  return ok ? 0 : XCG_RC_HIP;
}

// `appends` more entries written: index blocks the write head leaves are
// written with the running counter (XCodecDisk::enter,
// xcodec_cache_disk.cc:708-738; 0 means unused)
void volume_advance(Volume* V, uint64_t appends) {
  const uint64_t dend = V->dclock + appends;
  for (uint64_t m = V->dclock / DISK_ENTRIES + 1; m <= dend / DISK_ENTRIES; ++m) {
    V->ctr[(m - 1) % V->nb] = V->ibc;
    if (++V->ibc == 0) V->ibc = 1;
  }
  V->dclock = dend;
}

// A fresh volume (the registry stays).
void volume_reset(Volume* V) {
  V->dclock = 0;
  V->ctr.assign(V->nb, 0);
  V->ibc = 1;
}

// Where the write head is: XCodecDisk's current_index_block_ and
// index_block_next_ (xcodec_cache_disk.cc:701-727).
void volume_head(const Volume& V, uint64_t* index_block, uint64_t* next) {
  *index_block = (V.dclock / DISK_ENTRIES) % V.nb;
  *next = V.dclock % DISK_ENTRIES;
}

// Which front (xuid):
//  * want_xuid >= 0: that one -- a host XCodecDiskCache's own xuid_, so the
//    engine's fronts are the host disk's whatever order they bind in; uuid36,
//    when given, must be registered there or nowhere;
//  * uuid36: XCodecDisk::connect (xcodec_cache_disk.cc:640-690), the uuid's
//    registered xuid, else the lowest xuid nothing holds (no registry entry, no
//    front);
//  * neither: XCodecDisk::local (:635-641), xuid 0 when it is registered and
//    free (a reopened volume's local front), else the lowest free xuid under a
//    generated UUID (registry_load's local UUID on a fresh volume, :575-596).
int volume_front_xuid(const Volume& V, const char* uuid36, int want_xuid, const std::function<bool(uint32_t)>& bound,
                      std::string* name) {
  uint32_t xuid = XUIDS;
  if (uuid36)
    for (uint32_t x = 0; x < XUIDS; ++x)
      if (V.uuid[x] == uuid36) { xuid = x; break; }
  if (want_xuid >= 0) {
    if (xuid < XUIDS && xuid != (uint32_t)want_xuid) return XCG_RC_INVAL;
    xuid = (uint32_t)want_xuid;
  } else if (!uuid36 && !V.uuid[0].empty() && !bound(0)) {
    xuid = 0;
  }
  if (xuid < XUIDS && bound(xuid)) return XCG_RC_INVAL;               // (one engine front per disk front)
  if (xuid >= XUIDS)
    for (xuid = 0; xuid < XUIDS && (bound(xuid) || !V.uuid[xuid].empty()); ++xuid) {
    }
  if (xuid >= XUIDS) return XCG_RC_INVAL;                            // XCDFS_XUID_COUNT
  name->clear();
  if (uuid36) {
    name->assign(uuid36, 36);
  } else if (V.uuid[xuid].empty()) {
    char gen[37];
    if (!gen_uuid(gen)) return XCG_RC_HIP;
    name->assign(gen, 36);
  }
  return (int)xuid;
}

// The registry entry, written once the front exists.
void volume_register(Volume* V, uint32_t xuid, const std::string& name) {
  if (!name.empty() && V->uuid[xuid] != name) {
    V->uuid[xuid] = name;
    registry_write(V, xuid, name.c_str());
  }
}

}  // namespace xcg
