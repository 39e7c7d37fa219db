// CPU test of the volume format (wanproxy_amd/csrc/xcg_volume.{h,cpp}): the
// same code the library links, here on its own under AddressSanitizer and
// UndefinedBehaviorSanitizer (oracle/Makefile).  Stand-alone, two modes:
//
//   volume_harness reopen IN DISK_BYTES OUT
//       what xcg_disk_open(IN) + xcg_disk_save(OUT) do before any front binds:
//       the geometry, the reload of IN when it holds anything, OUT written
//       from the loaded image.  Exit 0, or 3 when the volume is refused.
//   volume_harness cases DIR
//       self-contained cases over volume images built here (real 2 KiB
//       segments and their hashes, fixed seeds; files under DIR): one
//       "ok <case>" line per case and exit 0, or the check that failed and
//       exit 1.  tests/test_volume_harness.py runs it.
//
// Any sanitizer report ends the program with a non-zero status.
// TEST INFRASTRUCTURE ONLY.
#include "../wanproxy_amd/csrc/xcg_volume.h"

#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../wanproxy_amd/csrc/xcg_segment.h"

namespace {

using namespace xcg;

#define CHECK(x)                                                             \
  do {                                                                       \
    if (!(x)) {                                                              \
      fprintf(stderr, "volume_harness: line %d: CHECK(%s)\n", __LINE__, #x); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

constexpr uint64_t BLK = 2048, PER = 204;
std::string g_dir;

std::string path_of(const char* name) { return g_dir + "/" + name; }

uint64_t disk_bytes(uint64_t nb) { return (18 + 205 * nb) * BLK; }   // tests/golden/make_pair_golden.py

uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

std::vector<uint8_t> segment(uint64_t seed) {
  std::vector<uint8_t> s(BLK);
  for (size_t i = 0; i < BLK; i += 8) {
    const uint64_t v = splitmix(&seed);
    memcpy(&s[i], &v, 8);
  }
  return s;
}

std::string uuid_of(uint64_t k) {
  char b[37];
  snprintf(b, sizeof b, "%08x-0000-4000-8000-%012llx", 0xF11Eu, (unsigned long long)k);
  return b;
}

std::vector<uint8_t> read_file(const std::string& p) {
  const int fd = ::open(p.c_str(), O_RDONLY);
  CHECK(fd != -1);
  struct stat st;
  CHECK(fstat(fd, &st) == 0);
  std::vector<uint8_t> b((size_t)st.st_size);
  CHECK(pread_all(fd, b.data(), b.size(), 0));
  close(fd);
  return b;
}

void write_file(const std::string& p, const std::vector<uint8_t>& b) {
  const int fd = ::open(p.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
  CHECK(fd != -1);
  CHECK(pwrite_all(fd, b.data(), b.size(), 0));
  close(fd);
}

// A volume image built from the format's description (xcg_volume.h), not by
// volume_write: registry and index blocks in `meta`, the data blocks that hold
// anything in `data`; the rest of the file reads as zeros.
struct Img {
  uint64_t nb;
  std::vector<uint8_t> meta;
  std::map<uint64_t, std::vector<uint8_t>> data;   // slot -> 2048 bytes

  explicit Img(uint64_t nb_) : nb(nb_), meta((18 + nb_) * BLK, 0) {}
  uint64_t bytes() const { return disk_bytes(nb); }
  void reg(uint32_t xuid, const std::string& u36) {
    CHECK(u36.size() == 36 && xuid < 18 * 56);
    memcpy(&meta[(xuid / 56) * BLK + (xuid % 56) * 36], u36.data(), 36);
  }
  void counter(uint64_t b, uint64_t c) { memcpy(&meta[(18 + b) * BLK], &c, 8); }
  void entry(uint64_t b, uint64_t j, uint16_t xuid, uint64_t hash) {
    uint8_t* q = &meta[(18 + b) * BLK + 8 + 10 * j];
    memcpy(q, &xuid, 2);
    memcpy(q + 2, &hash, 8);
  }
  // a real segment in slot b * 204 + j and its entry; returns the hash
  uint64_t put(uint64_t b, uint64_t j, uint16_t xuid, uint64_t seed) {
    std::vector<uint8_t> s = segment(seed);
    const uint64_t h = host_seg_hash(s.data());
    CHECK(h != 0 && h != NOKEY);
    data[b * PER + j] = s;
    entry(b, j, xuid, h);
    return h;
  }
  void write(const std::string& p) const {
    const int fd = ::open(p.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
    CHECK(fd != -1);
    CHECK(ftruncate(fd, (off_t)bytes()) == 0);
    CHECK(pwrite_all(fd, meta.data(), meta.size(), 0));
    for (const auto& kv : data)
      CHECK(pwrite_all(fd, kv.second.data(), BLK, (off_t)((18 + nb + kv.first) * BLK)));
    close(fd);
  }
  std::vector<uint8_t> whole() const {
    std::vector<uint8_t> b(bytes(), 0);
    memcpy(b.data(), meta.data(), meta.size());
    for (const auto& kv : data) memcpy(&b[(18 + nb + kv.first) * BLK], kv.second.data(), BLK);
    return b;
  }
};

// What xcg_disk_open does with a path: 0 and *loaded, or the refusal's code.
int open_volume(Volume* V, const std::string& p, uint64_t bytes, bool* loaded) {
  *loaded = false;
  const int rc = volume_geometry(V, bytes);
  if (rc) return rc;
  const int fd = ::open(p.c_str(), O_RDONLY);
  if (fd == -1) return errno == ENOENT ? 0 : -2;
  struct stat st;
  int lrc = fstat(fd, &st) == 0 ? 0 : -2;
  if (!lrc && st.st_size > 0) {
    lrc = volume_load(V, fd);
    *loaded = lrc == 0;
  }
  close(fd);
  return lrc;
}

// What xcg_disk_save does before any front binds.
int save_volume(const Volume& V, bool loaded, const std::string& p) {
  if (loaded) return volume_write(V, p.c_str(), V.h_key.data(), V.h_xuid.data(), V.h_data.data());
  const std::vector<uint64_t> key(V.D, NOKEY);
  const std::vector<uint32_t> xu(V.D, 0xFFFFFFFFu);
  const std::vector<uint8_t> data((size_t)V.D * BLK, 0);
  return volume_write(V, p.c_str(), key.data(), xu.data(), data.data());
}

Volume load_img(const Img& img, const char* name) {
  const std::string p = path_of(name);
  img.write(p);
  Volume V;
  bool loaded = false;
  CHECK(open_volume(&V, p, img.bytes(), &loaded) == 0 && loaded);
  CHECK(V.nb == img.nb && V.D == img.nb * PER);
  CHECK(V.h_key.size() == V.D && V.h_ent.size() == V.D && V.h_xuid.size() == V.D && V.h_data.size() == V.D * BLK);
  return V;
}

// The entry number the clock model gives slot (b, j) of a block loaded from
// the last lap, the write head standing at block `head`.
uint64_t ent_of(uint64_t nb, uint64_t head, uint64_t b, uint64_t j) {
  return PER * (nb + head - ((head + nb - b) % nb)) + j;
}

// XCodecDisk's running index-block counter after a reload: in block order, a
// counter above it sets it to that counter + 1 (xcodec_cache_disk.cc:148-149).
uint64_t ibc_of(const std::vector<uint64_t>& counters) {
  uint64_t c = 0;
  for (uint64_t v : counters) {
    if (v == 0) break;
    if (v > c) c = v + 1;
  }
  return c == 0 ? 1 : c;
}

void case_geometry() {
  Volume V;
  CHECK(volume_geometry(&V, 0) == -22);
  CHECK(volume_geometry(&V, 17 * BLK) == -22);
  CHECK(volume_geometry(&V, 18 * BLK) == -22);
  CHECK(volume_geometry(&V, 18 * BLK + BLK - 1) == -22);
  CHECK(volume_geometry(&V, 19 * BLK) == -22);                 // no room for one index block
  CHECK(volume_geometry(&V, (18 + 204) * BLK) == -22);
  CHECK(volume_geometry(&V, disk_bytes(1) - 1) == -22);
  CHECK(volume_geometry(&V, ((1ull << 29) / PER + 1) * 205 * BLK + 18 * BLK) == -22);   // 2^29 data blocks or more
  for (uint64_t nb : {1, 3, 12}) {
    for (uint64_t extra : {(uint64_t)0, (uint64_t)1, BLK - 1, 204 * BLK + BLK - 1}) {
      Volume W;
      CHECK(volume_geometry(&W, disk_bytes(nb) + extra) == 0);
      CHECK(W.nb == nb && W.D == nb * PER && W.bytes == disk_bytes(nb) + extra);
      CHECK(W.ctr == std::vector<uint64_t>(nb, 0) && W.ibc == 1 && W.dclock == 0);
      CHECK(W.reg == std::vector<uint8_t>(18 * BLK, 0) && W.uuid == std::vector<std::string>(1024));
      CHECK(W.h_key.empty() && W.h_ent.empty() && W.h_xuid.empty() && W.h_data.empty());
    }
    Volume W;
    CHECK(volume_geometry(&W, disk_bytes(nb + 1) - 1) == 0 && W.nb == nb);
  }
  puts("ok geometry");
}

void case_fresh() {
  Volume V;
  bool loaded = true;
  const std::string out = path_of("fresh.out");
  CHECK(open_volume(&V, path_of("absent.vol"), disk_bytes(3), &loaded) == 0 && !loaded);
  CHECK(save_volume(V, loaded, out) == 0);
  CHECK(read_file(out) == std::vector<uint8_t>(disk_bytes(3), 0));
  // an empty file is a fresh volume too
  write_file(path_of("empty.vol"), {});
  Volume W;
  CHECK(open_volume(&W, path_of("empty.vol"), disk_bytes(3), &loaded) == 0 && !loaded);
  CHECK(save_volume(W, loaded, out) == 0);
  CHECK(read_file(out) == std::vector<uint8_t>(disk_bytes(3), 0));
  puts("ok fresh");
}

// A volume of nb index blocks, every block written: block b has counter
// base + ((b - head) mod nb), so `head` has the lowest.  Two fronts (xuid 0
// and 5) write alternately; a few slots stay empty.  Fills what a reload must give.
struct Expect {
  std::vector<uint64_t> key, ent;
  std::vector<uint32_t> xuid;
};
Img ring_image(uint64_t nb, uint64_t head, uint64_t base, uint64_t seed, Expect* ex, std::vector<uint64_t>* counters) {
  Img img(nb);
  img.reg(0, uuid_of(1));
  img.reg(5, uuid_of(2));
  ex->key.assign(nb * PER, NOKEY);
  ex->ent.assign(nb * PER, NOENT);
  ex->xuid.assign(nb * PER, 0xFFFFFFFFu);
  counters->assign(nb, 0);
  for (uint64_t b = 0; b < nb; ++b) {
    (*counters)[b] = base + (b + nb - head) % nb;
    img.counter(b, (*counters)[b]);
    for (uint64_t j : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)7, 100 + b, (uint64_t)202, (uint64_t)203}) {
      if ((j + b) % 5 == 3) continue;                           // (an empty slot)
      const uint16_t xu = (j + b) % 2 ? 5 : 0;
      const uint64_t h = img.put(b, j, xu, seed + b * 1000 + j);
      ex->key[b * PER + j] = h;
      ex->xuid[b * PER + j] = xu;
      if (b != head) ex->ent[b * PER + j] = ent_of(nb, head, b, j);   // (the head's block is not loaded)
    }
  }
  return img;
}

void check_ring(const Volume& V, const Expect& ex, uint64_t head, const std::vector<uint64_t>& counters) {
  CHECK(V.h_key == ex.key);
  CHECK(V.h_xuid == ex.xuid);
  CHECK(V.h_ent == ex.ent);
  CHECK(V.ctr == counters);
  CHECK(V.ibc == ibc_of(counters));
  CHECK(V.dclock == PER * (V.nb + head));
  uint64_t ib = ~0ull, next = ~0ull;
  volume_head(V, &ib, &next);
  CHECK(ib == head && next == 0);
}

void case_roundtrip() {
  // every block written, the head in the middle: loaded in the order 6 .. 11, 0 .. 4
  {
    Expect ex;
    std::vector<uint64_t> counters;
    const Img img = ring_image(12, 5, 20, 0xA11CE, &ex, &counters);
    const Volume V = load_img(img, "rt12.vol");
    check_ring(V, ex, 5, counters);
    CHECK(V.uuid[0] == uuid_of(1) && V.uuid[5] == uuid_of(2));
    for (uint32_t x = 0; x < 1024; ++x) CHECK(x == 0 || x == 5 || V.uuid[x].empty());
    CHECK(memcmp(V.reg.data(), img.meta.data(), 18 * BLK) == 0);
    CHECK(memcmp(V.h_data.data(), img.whole().data() + (18 + 12) * BLK, 12 * PER * BLK) == 0);
    const std::string o1 = path_of("rt12.out1"), o2 = path_of("rt12.out2");
    CHECK(save_volume(V, true, o1) == 0);
    CHECK(read_file(o1) == img.whole());                      // (the file it was loaded from)
    Volume W;
    bool loaded = false;
    CHECK(open_volume(&W, o1, img.bytes(), &loaded) == 0 && loaded);
    check_ring(W, ex, 5, counters);
    CHECK(save_volume(W, true, o2) == 0);
    CHECK(read_file(o2) == read_file(o1));
  }
  // nb = 3, counters out of block order: 9, 5 (the head), 8
  {
    Expect ex;
    std::vector<uint64_t> counters;
    Img img = ring_image(3, 1, 5, 0xB0B, &ex, &counters);
    counters = {9, 5, 8};
    for (uint64_t b = 0; b < 3; ++b) img.counter(b, counters[b]);
    const Volume V = load_img(img, "rt3.vol");
    check_ring(V, ex, 1, counters);
    CHECK(save_volume(V, true, path_of("rt3.out")) == 0);
    CHECK(read_file(path_of("rt3.out")) == img.whole());
  }
  // a volume not yet full: blocks 0, 1 written, block 2 free (counter 0) is the head
  {
    Img img(3);
    img.reg(0, uuid_of(1));
    Expect ex;
    ex.key.assign(3 * PER, NOKEY);
    ex.ent.assign(3 * PER, NOENT);
    ex.xuid.assign(3 * PER, 0xFFFFFFFFu);
    for (uint64_t b = 0; b < 2; ++b) {
      img.counter(b, b + 1);
      for (uint64_t j = 0; j < 10; ++j) {
        ex.key[b * PER + j] = img.put(b, j, 0, 0xF00 + b * 100 + j);
        ex.xuid[b * PER + j] = 0;
        ex.ent[b * PER + j] = ent_of(3, 2, b, j);
      }
    }
    const Volume V = load_img(img, "rt3p.vol");
    check_ring(V, ex, 2, {1, 2, 0});
    CHECK(V.ibc == 2);                                         // (1 -> 2; 2 is not above 2)
    CHECK(save_volume(V, true, path_of("rt3p.out")) == 0);
    CHECK(read_file(path_of("rt3p.out")) == img.whole());
  }
  puts("ok roundtrip");
}

void case_dup_hash() {
  // counters 9, 5 (head), 8: block 2 loads before block 0
  Img img(3);
  img.reg(0, uuid_of(1));
  img.reg(5, uuid_of(2));
  img.counter(0, 9);
  img.counter(1, 5);
  img.counter(2, 8);
  const uint64_t h = img.put(0, 4, 0, 77);                     // the later one by counter, in the lower block
  CHECK(img.put(2, 9, 0, 77) == h);
  CHECK(img.put(2, 10, 5, 77) == h);                           // another front's entry of the hash: its own index
  const uint64_t g = img.put(2, 20, 0, 78);                    // twice in one block: the later slot
  CHECK(img.put(2, 30, 0, 78) == g);
  const Volume V = load_img(img, "dup.vol");
  CHECK(V.h_ent[0 * PER + 4] == ent_of(3, 1, 0, 4));
  CHECK(V.h_ent[2 * PER + 9] == NOENT);
  CHECK(V.h_ent[2 * PER + 10] == ent_of(3, 1, 2, 10));
  CHECK(V.h_ent[2 * PER + 20] == NOENT);
  CHECK(V.h_ent[2 * PER + 30] == ent_of(3, 1, 2, 30));
  CHECK(V.h_key[2 * PER + 9] == h && V.h_key[2 * PER + 20] == g);   // (the ring still shows what the file holds)
  uint64_t live = 0;
  for (uint64_t e : V.h_ent) live += e != NOENT;
  CHECK(live == 3);
  puts("ok dup_hash");
}

void case_bad_entry() {
  // the head (block 0) is not above the block with the error: the entry is
  // dropped, the block's other entries stay
  {
    Img img(3);
    img.reg(0, uuid_of(1));
    for (uint64_t b = 0; b < 3; ++b) img.counter(b, 5 + b);
    for (uint64_t j = 0; j < 10; ++j) img.put(1, j, 0, 300 + j), img.put(2, j, 0, 400 + j);
    img.data[1 * PER + 5][17] ^= 0x40;
    const uint64_t good = img.put(2, 50, 0, 999);
    img.put(1, 60, 0, 999);                                    // an earlier entry of the hash ...
    img.put(2, 61, 0, 999);
    img.data[2 * PER + 61][0] ^= 1;                            // ... whose later one is damaged: both leave
    const Volume V = load_img(img, "bad0.vol");
    for (uint64_t j = 0; j < 10; ++j) {
      CHECK(V.h_ent[1 * PER + j] == (j == 5 ? NOENT : ent_of(3, 0, 1, j)));
      CHECK(V.h_ent[2 * PER + j] == ent_of(3, 0, 2, j));
    }
    CHECK(V.h_key[2 * PER + 50] == good);
    CHECK(V.h_ent[1 * PER + 60] == NOENT && V.h_ent[2 * PER + 50] == NOENT && V.h_ent[2 * PER + 61] == NOENT);
    CHECK(V.dclock == PER * 3);
  }
  // the head (block 2) is above it: the block is given up from the error on,
  // what it had loaded leaves and it becomes the head ("rewrite the block
  // with errors"), which renumbers the ring
  {
    Img img(3);
    img.reg(0, uuid_of(1));
    img.counter(0, 6);
    img.counter(1, 7);
    img.counter(2, 5);
    for (uint64_t j = 0; j < 10; ++j) img.put(0, j, 0, 500 + j), img.put(1, j, 0, 600 + j);
    img.data[1 * PER + 5][2047] ^= 0x80;
    const Volume V = load_img(img, "bad2.vol");
    for (uint64_t j = 0; j < 10; ++j) {
      CHECK(V.h_ent[0 * PER + j] == ent_of(3, 1, 0, j));
      CHECK(V.h_ent[1 * PER + j] == NOENT);
    }
    CHECK(V.dclock == PER * (3 + 1));
    uint64_t ib, next;
    volume_head(V, &ib, &next);
    CHECK(ib == 1 && next == 0);
  }
  // 162 index blocks, the head at block 0: blocks 1 .. 161 load in order, the
  // first 80 and the last 80 checked -- block 81 is the one that is not
  {
    const uint64_t nb = 162;
    Img img(nb);
    img.reg(0, uuid_of(1));
    for (uint64_t b = 0; b < nb; ++b) img.counter(b, 10 + b);
    for (uint64_t b : {1, 80, 81, 82, 161}) {
      img.put(b, 3, 0, 7000 + b);
      img.put(b, 4, 0, 8000 + b);
      img.data[b * PER + 4][100] ^= 2;
    }
    const Volume V = load_img(img, "bad162.vol");
    for (uint64_t b : {1, 80, 81, 82, 161}) {
      CHECK(V.h_ent[b * PER + 3] == ent_of(nb, 0, b, 3));
      CHECK(V.h_ent[b * PER + 4] == (b == 81 ? ent_of(nb, 0, b, 4) : NOENT));
    }
    CHECK(V.dclock == PER * nb);
  }
  puts("ok bad_entry");
}

void case_registry() {
  {
    Img img(3);
    img.reg(0, uuid_of(1));
    img.reg(1, "this-is-not-a-uuid-but-36-chars-long");
    img.reg(3, uuid_of(1));                                    // a duplicate of xuid 0's
    img.reg(4, uuid_of(4));
    img.reg(5, uuid_of(5));                                    // no entries: collected
    img.reg(6, "F11E0000-ABCD-4000-8000-00000000000a");       // upper-case hex is a UUID
    img.reg(60, uuid_of(60));                                  // in registry block 1, no entries: collected
    img.reg(61, uuid_of(61));
    img.reg(1007, uuid_of(1007));                              // the last registry block (17)
    img.counter(0, 1);
    img.counter(1, 2);
    for (uint16_t x : {0, 1, 2, 3, 4, 6, 61, 1007}) img.put(1, x % 204, x, 100 + x);
    const Volume V = load_img(img, "reg.vol");
    const std::set<uint32_t> kept = {0, 4, 6, 61, 1007};
    for (uint32_t x = 0; x < 1024; ++x) CHECK(V.uuid[x].empty() == !kept.count(x));
    CHECK(V.uuid[0] == uuid_of(1) && V.uuid[4] == uuid_of(4) && V.uuid[61] == uuid_of(61));
    CHECK(V.uuid[6] == "F11E0000-ABCD-4000-8000-00000000000a" && V.uuid[1007] == uuid_of(1007));
    for (uint16_t x : {0, 1, 2, 3, 4, 6, 61, 1007})
      CHECK((V.h_ent[1 * PER + x % 204] != NOENT) == (kept.count(x) != 0));
    // the registry as XCodecDisk::registry_write leaves it: xuid 5's block
    // (0) with the slot zeroed written to block 0, then xuid 60's block (1)
    // with its slot zeroed written to block 0 as well
    std::vector<uint8_t> reg(img.meta.begin(), img.meta.begin() + 18 * BLK);
    memset(&reg[5 * 36], 0, 36);
    std::vector<uint8_t> blk(reg.begin() + BLK, reg.begin() + 2 * BLK);
    memset(&blk[(60 - 56) * 36], 0, 36);
    memcpy(&reg[0], blk.data(), BLK);
    CHECK(V.reg == reg);
  }
  // an empty registry: a generated local UUID at xuid 0, written to the registry
  {
    Img img(3);
    img.counter(0, 1);
    img.counter(1, 2);
    img.put(0, 0, 0, 1);
    const Volume V = load_img(img, "reg0.vol");
    const std::string& u = V.uuid[0];
    CHECK(u.size() == 36 && uuid_ok((const uint8_t*)u.data()));
    CHECK(u[14] == '4' && (u[19] == '8' || u[19] == '9' || u[19] == 'a' || u[19] == 'b'));
    for (char c : u) CHECK(c == '-' || (c >= '0' && c <= '9') || (c >= 'a' && c <= 'f'));
    CHECK(memcmp(V.reg.data(), u.data(), 36) == 0);
    CHECK(std::vector<uint8_t>(V.reg.begin() + 36, V.reg.end()) == std::vector<uint8_t>(18 * BLK - 36, 0));
    for (uint32_t x = 1; x < 1024; ++x) CHECK(V.uuid[x].empty());
    CHECK(V.h_ent[0] == ent_of(3, 2, 0, 0));                   // (xuid 0 is now a front: its entry loads)
    Volume W = load_img(img, "reg0.vol");
    CHECK(W.uuid[0] != u);                                     // (random)
  }
  CHECK(!uuid_ok((const uint8_t*)"f11e0000-0000-4000-8000-00000000000g"));
  CHECK(!uuid_ok((const uint8_t*)"f11e0000-0000-4000-8000000000000000a"));
  CHECK(!uuid_ok((const uint8_t*)"f11e00000-000-4000-8000-00000000000a"));
  puts("ok registry");
}

void case_front_xuid() {
  Volume V;
  CHECK(volume_geometry(&V, disk_bytes(3)) == 0);
  const std::string A = uuid_of(0xA), B = uuid_of(0xB), Cc = uuid_of(0xC), N = uuid_of(0x99);
  V.uuid[0] = A;
  V.uuid[1] = B;
  V.uuid[9] = Cc;
  std::set<uint32_t> b;
  auto bound = [&](uint32_t x) { return b.count(x) != 0; };
  std::string name = "x";
  auto generated = [&]() { return name.size() == 36 && uuid_ok((const uint8_t*)name.data()) && name[14] == '4'; };
  // want_xuid given
  CHECK(volume_front_xuid(V, nullptr, 7, bound, &name) == 7 && generated());
  CHECK(volume_front_xuid(V, nullptr, 9, bound, &name) == 9 && name.empty());           // (keeps its registered UUID)
  CHECK(volume_front_xuid(V, N.c_str(), 7, bound, &name) == 7 && name == N);
  CHECK(volume_front_xuid(V, Cc.c_str(), 9, bound, &name) == 9 && name == Cc);
  CHECK(volume_front_xuid(V, N.c_str(), 1, bound, &name) == 1 && name == N);            // (renames xuid 1)
  CHECK(volume_front_xuid(V, nullptr, 1023, bound, &name) == 1023 && generated());
  // uuid36 registered
  CHECK(volume_front_xuid(V, Cc.c_str(), -1, bound, &name) == 9 && name == Cc);
  CHECK(volume_front_xuid(V, A.c_str(), -1, bound, &name) == 0 && name == A);
  // uuid36 unknown: the lowest xuid neither bound nor registered
  CHECK(volume_front_xuid(V, N.c_str(), -1, bound, &name) == 2 && name == N);
  b = {2, 3};
  CHECK(volume_front_xuid(V, N.c_str(), -1, bound, &name) == 4 && name == N);
  // neither: xuid 0 when registered and free, else the lowest free
  b.clear();
  CHECK(volume_front_xuid(V, nullptr, -1, bound, &name) == 0 && name.empty());
  b = {0};
  CHECK(volume_front_xuid(V, nullptr, -1, bound, &name) == 2 && generated());
  b = {0, 2};
  CHECK(volume_front_xuid(V, nullptr, -1, bound, &name) == 3 && generated());
  {
    Volume F;                                                  // a fresh volume: xuid 0 under a generated UUID
    CHECK(volume_geometry(&F, disk_bytes(3)) == 0);
    b.clear();
    CHECK(volume_front_xuid(F, nullptr, -1, bound, &name) == 0 && generated());
    b = {0};
    CHECK(volume_front_xuid(F, nullptr, -1, bound, &name) == 1 && generated());
  }
  // refusals
  b.clear();
  CHECK(volume_front_xuid(V, Cc.c_str(), 4, bound, &name) == -22);                      // registered under xuid 9
  b = {4, 9, 0};
  CHECK(volume_front_xuid(V, nullptr, 4, bound, &name) == -22);                         // already bound
  CHECK(volume_front_xuid(V, N.c_str(), 4, bound, &name) == -22);
  CHECK(volume_front_xuid(V, Cc.c_str(), -1, bound, &name) == -22);
  CHECK(volume_front_xuid(V, A.c_str(), -1, bound, &name) == -22);
  b.clear();
  for (uint32_t x = 0; x < 1024; ++x)
    if (x % 3) b.insert(x); else V.uuid[x] = uuid_of(0x1000 + x);
  CHECK(volume_front_xuid(V, N.c_str(), -1, bound, &name) == -22);                      // all 1024 taken
  b.insert(0);
  CHECK(volume_front_xuid(V, nullptr, -1, bound, &name) == -22);
  // the registry update once the front exists
  Volume R;
  CHECK(volume_geometry(&R, disk_bytes(3)) == 0);
  volume_register(&R, 3, "");                                  // (keeps what it has)
  CHECK(R.uuid[3].empty() && R.reg == std::vector<uint8_t>(18 * BLK, 0));
  volume_register(&R, 3, A);
  CHECK(R.uuid[3] == A && memcmp(&R.reg[3 * 36], A.data(), 36) == 0);
  std::vector<uint8_t> before = R.reg;
  volume_register(&R, 3, A);                                   // (already registered: nothing written)
  CHECK(R.reg == before);
  volume_register(&R, 60, B);                                  // block 1's copy goes to block 0, as the reference's
  std::vector<uint8_t> blk(BLK, 0);
  memcpy(&blk[(60 - 56) * 36], B.data(), 36);
  CHECK(R.uuid[60] == B && memcmp(&R.reg[0], blk.data(), BLK) == 0);
  CHECK(std::vector<uint8_t>(R.reg.begin() + BLK, R.reg.end()) == std::vector<uint8_t>(17 * BLK, 0));
  before = R.reg;
  volume_register(&R, 1007, Cc);                               // the registry's last slot
  CHECK(R.uuid[1007] == Cc && memcmp(&R.reg[55 * 36], Cc.data(), 36) == 0);
  before = R.reg;
  for (uint32_t x : {1008u, 1023u}) {                          // 18 blocks of 56 slots: no slot for these
    volume_register(&R, x, N);
    CHECK(R.uuid[x] == N && R.reg == before);
  }
  puts("ok front_xuid");
}

void case_advance() {
  const uint64_t nb = 3;
  // k appends in one call = k calls of one, from several clocks
  for (uint64_t start : {(uint64_t)0, (uint64_t)1, PER - 1, PER, 2 * PER + 200, 3 * PER - 1})
    for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)3, PER - 1, PER, PER + 1, 2 * PER + 5, 3 * PER, 3 * PER + 7,
                       7 * PER + 100}) {
      Volume A, B;
      CHECK(volume_geometry(&A, disk_bytes(nb)) == 0 && volume_geometry(&B, disk_bytes(nb)) == 0);
      volume_advance(&A, start);
      for (uint64_t i = 0; i < start; ++i) volume_advance(&B, 1);
      CHECK(A.ctr == B.ctr && A.ibc == B.ibc && A.dclock == B.dclock);
      volume_advance(&A, k);
      for (uint64_t i = 0; i < k; ++i) volume_advance(&B, 1);
      CHECK(A.ctr == B.ctr && A.ibc == B.ibc && A.dclock == B.dclock);
      // the m-th index block filled (from 1) gets counter m: the last nb of them stand
      const uint64_t filled = (start + k) / PER;
      CHECK(A.dclock == start + k && A.ibc == filled + 1);
      for (uint64_t b = 0; b < nb; ++b) {
        uint64_t want = 0;
        for (uint64_t m = 1; m <= filled; ++m)
          if ((m - 1) % nb == b) want = m;
        CHECK(A.ctr[b] == want);
      }
      uint64_t ib, next;
      volume_head(A, &ib, &next);
      CHECK(ib == filled % nb && next == (start + k) % PER);
    }
  // the running counter skips 0 when it wraps
  Volume W;
  CHECK(volume_geometry(&W, disk_bytes(nb)) == 0);
  W.ibc = ~0ull;
  volume_advance(&W, 2 * PER + 1);
  CHECK(W.ctr[0] == ~0ull && W.ctr[1] == 1 && W.ctr[2] == 0 && W.ibc == 2 && W.dclock == 2 * PER + 1);
  Volume X;
  CHECK(volume_geometry(&X, disk_bytes(nb)) == 0);
  X.ibc = ~0ull;
  volume_advance(&X, PER);
  CHECK(X.ctr[0] == ~0ull && X.ibc == 1);
  // a fresh volume again (the registry stays)
  W.uuid[2] = uuid_of(2);
  registry_write(&W, 2, uuid_of(2).c_str());
  const std::vector<uint8_t> reg = W.reg;
  volume_reset(&W);
  CHECK(W.dclock == 0 && W.ibc == 1 && W.ctr == std::vector<uint64_t>(nb, 0) && W.reg == reg && W.uuid[2] == uuid_of(2));
  puts("ok advance");
}

// Loads or is refused (-2); a following write gives exactly `bytes` bytes.
Volume damaged_one(const std::vector<uint8_t>& file, const char* name, uint64_t bytes) {
  const std::string p = path_of(name), out = p + ".out";
  write_file(p, file);
  Volume V;
  bool loaded = false;
  const int rc = open_volume(&V, p, bytes, &loaded);
  CHECK(rc == 0 || rc == -2);
  if (rc != 0) {                                               // refused: the caller has a fresh volume instead
    Volume F;
    CHECK(volume_geometry(&F, bytes) == 0);
    V = F;
    loaded = false;
  }
  CHECK(save_volume(V, loaded, out) == 0);
  struct stat st;
  CHECK(stat(out.c_str(), &st) == 0 && (uint64_t)st.st_size == bytes);
  // what it wrote reloads to the same file
  Volume W;
  CHECK(open_volume(&W, out, bytes, &loaded) == 0);
  if (loaded && W.uuid == V.uuid) {
    CHECK(save_volume(W, loaded, p + ".out2") == 0);
    CHECK(read_file(p + ".out2") == read_file(out));
  }
  return V;
}

void case_damaged() {
  const uint64_t nb = 3, bytes = disk_bytes(nb);
  Expect ex;
  std::vector<uint64_t> counters;
  const Img img = ring_image(nb, 1, 40, 0xDA7A, &ex, &counters);
  const std::vector<uint8_t> good = img.whole();
  // cut to a third: the index survives, the data blocks read as zeros and fail their check
  {
    const Volume V = damaged_one(std::vector<uint8_t>(good.begin(), good.begin() + bytes / 3), "cut.vol", bytes);
    // (block 2 loads first and loses every entry; block 0 meets its first
    // missing data block at entry 202 with the head at block 1 above it: the
    // block is given up and becomes the head)
    CHECK(V.h_key == ex.key);
    for (uint64_t e : V.h_ent) CHECK(e == NOENT);
    CHECK(V.dclock == PER * (nb + 0));
  }
  {
    const Volume V = damaged_one(std::vector<uint8_t>(good.begin(), good.begin() + 18 * BLK), "cut2.vol", bytes);
    CHECK(V.dclock == PER * (nb + 0));                         // (block 0's counter cut off: it reads as free)
    CHECK(V.h_key == std::vector<uint64_t>(V.D, NOKEY) && V.uuid[0] == uuid_of(1) && V.uuid[5].empty());
  }
  // seeded noise of full length, and of a few other lengths
  for (uint64_t len : {bytes, bytes / 3, (uint64_t)1, (uint64_t)2047, 18 * BLK + 9, bytes + 12345}) {
    uint64_t s = 0x5EED + len;
    std::vector<uint8_t> noise(len);
    for (auto& c : noise) c = (uint8_t)splitmix(&s);
    (void)damaged_one(noise, "noise.vol", bytes);
  }
  // index entries with an xuid of 1024 and above: never a front's
  {
    Img bad = img;
    bad.reg(1007, uuid_of(3));                                 // (the registry's last slot: 18 blocks of 56)
    const uint64_t h1 = bad.put(0, 50, 1024, 1), h2 = bad.put(0, 51, 0xFFFF, 2), h3 = bad.put(2, 52, 1007, 3);
    const uint64_t h4 = bad.put(2, 53, 1023, 4);               // (an xuid the registry has no slot for)
    const Volume V = damaged_one(bad.whole(), "xuid.vol", bytes);
    CHECK(V.h_key[50] == h1 && V.h_xuid[50] == 1024 && V.h_ent[50] == NOENT);
    CHECK(V.h_key[51] == h2 && V.h_xuid[51] == 0xFFFF && V.h_ent[51] == NOENT);
    CHECK(V.h_key[2 * PER + 52] == h3 && V.h_ent[2 * PER + 52] == ent_of(nb, 1, 2, 52));
    CHECK(V.h_key[2 * PER + 53] == h4 && V.h_xuid[2 * PER + 53] == 1023 && V.h_ent[2 * PER + 53] == NOENT);
    for (uint64_t i = 0; i < V.D; ++i)
      if (i != 50 && i != 51 && i != 2 * PER + 52 && i != 2 * PER + 53) CHECK(V.h_ent[i] == ex.ent[i]);
  }
  // counters of ~0: every block has the same one, so one is the head and nothing else loads
  {
    Img bad = img;
    for (uint64_t b = 0; b < nb; ++b) bad.counter(b, ~0ull);
    const Volume V = damaged_one(bad.whole(), "ctr.vol", bytes);
    CHECK(V.ctr == std::vector<uint64_t>(nb, ~0ull) && V.ibc == 1);
    for (uint64_t e : V.h_ent) CHECK(e == NOENT);
    Img one = img;                                             // one such counter among good ones: the last to load
    one.counter(2, ~0ull);
    const Volume U = damaged_one(one.whole(), "ctr1.vol", bytes);
    CHECK(U.ibc == 1 && U.dclock == PER * (nb + 1));
    for (uint64_t i = 0; i < U.D; ++i) CHECK(U.h_ent[i] == ex.ent[i]);
  }
  // a file longer than the volume: what lies past it is not read
  {
    std::vector<uint8_t> longer = good;
    uint64_t s = 9;
    for (int i = 0; i < 70000; ++i) longer.push_back((uint8_t)splitmix(&s));
    const Volume V = damaged_one(longer, "long.vol", bytes);
    check_ring(V, ex, 1, counters);
    CHECK(read_file(path_of("long.vol.out")) == good);
  }
  puts("ok damaged");
}

int run_reopen(const char* in, const char* disk, const char* out) {
  char* end = nullptr;
  const uint64_t bytes = strtoull(disk, &end, 10);
  if (!*disk || *end) return 2;
  Volume V;
  bool loaded = false;
  int rc = open_volume(&V, in, bytes, &loaded);
  if (rc == 0) rc = save_volume(V, loaded, out);
  if (rc) {
    fprintf(stderr, "volume_harness: refused (%d)\n", rc);
    return 3;
  }
  printf("ok reopen loaded=%d nb=%llu clock=%llu\n", (int)loaded, (unsigned long long)V.nb, (unsigned long long)V.dclock);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "reopen")) return run_reopen(argv[2], argv[3], argv[4]);
  if (argc != 3 || strcmp(argv[1], "cases")) {
    fprintf(stderr, "usage: volume_harness reopen IN DISK_BYTES OUT | volume_harness cases DIR\n");
    return 2;
  }
  g_dir = argv[2];
  case_geometry();
  case_fresh();
  case_roundtrip();
  case_dup_hash();
  case_bad_entry();
  case_registry();
  case_front_xuid();
  case_advance();
  case_damaged();
  return 0;
}
