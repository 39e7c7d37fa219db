// The life cycle of the pair's state objects (xcg_pair_state.h): a disk is
// created or reopened from a volume file, bound to the first front's device,
// its blocks mapped behind every front's primary; fronts come and go; the
// volume is saved; both are counted and destroyed.  Host code that calls HIP,
// once per context, never hot.  The replay and the commit that run on these
// objects: xcg_pair.hip; the volume file itself: xcg_volume.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <errno.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "xcg_pair_state.h"

namespace xcg {

// Statistics: this front's live disk entries (xuid) or every live entry (xuid ~0).
__global__ __launch_bounds__(256) void pair_count_live_kernel(const uint64_t* dent, const uint32_t* dxuid, uint32_t D,
                                                              uint32_t nb, uint64_t dclock, uint32_t xuid,
                                                              uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool live = false;
  if (i < D) {
    const uint64_t e = dent[i];
    live = e != NOENT && dclock < death_of(e, nb) && (xuid == NIL || dxuid[i] == xuid);
  }
  const uint64_t m = ballot(live);
  if (lane_id() == 0 && m) atomicAdd(out, (uint32_t)__builtin_popcountll(m));
}

// A front goes away or is cleared: its disk entries leave the index (the
// volume's index blocks keep them unless the whole volume is reset).
__global__ __launch_bounds__(256) void pair_drop_front_kernel(uint64_t* dkey, uint64_t* dent, const uint32_t* dxuid,
                                                              uint32_t D, uint32_t xuid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D && (xuid == NIL || dxuid[i] == xuid)) {
    dent[i] = NOENT;
    if (xuid == NIL) dkey[i] = NOKEY;
  }
}

int ensure_front_arrays(XcgPairState* P) {
  if (P->occ) return 0;
  DevMem& m = P->mem;
  return m.dev(&P->occ, 4ull * P->C) && m.dev(&P->freel, 4ull * P->C) && m.dev(&P->ofl, 4ull * (P->C + 1)) &&
                 m.dev(&P->ofr, 4ull * (P->C + 1))
             ? 0 : XCG_RC_HIP;
}

}  // namespace xcg

namespace {

using namespace xcg;

// The disk's device arrays, on the first front's device.
int disk_bind(XcgDiskState* K, int device) {
  if (K->device >= 0) return K->device == device ? 0 : XCG_RC_INVAL;
  const uint64_t D = K->vol.D;
  if (!(K->mem.dev(&K->dkey, 8 * D) && K->mem.dev(&K->dent, 8 * D) && K->mem.dev(&K->dxuid, 4 * D)) ||
      hipMemset(K->dkey, 0xFF, 8 * D) != hipSuccess ||
      hipMemset(K->dent, 0xFF, 8 * D) != hipSuccess || hipMemset(K->dxuid, 0xFF, 4 * D) != hipSuccess) {
    K->mem.release_all();
    K->dkey = K->dent = nullptr;
    K->dxuid = nullptr;
    return XCG_RC_NOMEM;
  }
  K->device = device;
  return 0;
}

// The front's pool: C primary segments followed by the disk's D blocks at
// pool + (C + i) * 2048.  HIP virtual memory maps the disk's one physical
// allocation behind every front; without it each front allocates its own copy
// (a front reads only the blocks it wrote itself, so that is correct too).
int map_pool(XcgPairState* P, int device) {
  XcgDiskState* K = P->disk;
  if (!getenv("XCG_NO_VMM")) {
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    bool ok = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) == hipSuccess &&
              gran > 0;
    if (ok && !K->vmm && K->pool_bytes == 0) {
      // The disk's blocks: HBM, unless the volume does not fit beside what the
      // device already holds (keep 4 GiB free) or the caller asks for the host
      // tier -- then pinned host memory behind the same addresses, which the
      // kernels read and write over PCIe (a spill level below HBM).
      const size_t sd = align_up((size_t)K->vol.D * SEG + 256, gran);
      size_t fr = 0, tot = 0;
      const bool fits = hipMemGetInfo(&fr, &tot) == hipSuccess && fr > sd + (4ull << 30);
      const bool want_host = (K->flags & 1u) != 0 || (!(K->flags & 2u) && !fits);
      if (!want_host && hipMemCreate(&K->pool_h, sd, &prop, 0) == hipSuccess) {
        K->pool_bytes = sd;
        K->vmm = true;
        K->tier = 0;
      } else if (!(K->flags & 2u)) {
        (void)hipGetLastError();
        hipMemAllocationProp hp{};
        hp.type = hipMemAllocationTypePinned;
        hp.location.type = hipMemLocationTypeHost;
        hp.location.id = 0;
        size_t hg = 0;
        const hipError_t e1 = hipMemGetAllocationGranularity(&hg, &hp, hipMemAllocationGranularityMinimum);
        const hipError_t e2 = e1 == hipSuccess && hg && gran % hg == 0 ? hipMemCreate(&K->pool_h, sd, &hp, 0)
                                                                        : hipErrorInvalidValue;
        if (e2 == hipSuccess) {
          K->pool_bytes = sd;
          K->vmm = true;
          K->tier = 1;
        } else {
          // (host-located VMM needs a runtime that has it: ROCm 7.2's does, the
          // 7.0 runtime PyTorch bundles refuses it) -- stay on the device
          if (pair_debug())
            fprintf(stderr, "pair: host tier not available (granularity %s %zu, create %s)\n", hipGetErrorString(e1),
                    hg, hipGetErrorString(e2));
          (void)hipGetLastError();
          if (hipMemCreate(&K->pool_h, sd, &prop, 0) == hipSuccess) {
            K->pool_bytes = sd;
            K->vmm = true;
            K->tier = 0;
          }
        }
      }
    }
    ok = ok && K->vmm;
    if (ok && !K->dva) {
      // The disk's own mapping of its blocks, held until the disk goes: the
      // volume can be saved after every front is gone, and the allocation
      // always has a mapping until it is released (fronts come and go).
      void* va = nullptr;
      hipMemAccessDesc acc{};
      acc.location = prop.location;
      acc.flags = hipMemAccessFlagsProtReadWrite;
      bool m = false;
      bool dok = hipMemAddressReserve(&va, K->pool_bytes, 0, nullptr, 0) == hipSuccess;
      dok = dok && (m = hipMemMap(va, K->pool_bytes, 0, K->pool_h, 0) == hipSuccess);
      dok = dok && hipMemSetAccess(va, K->pool_bytes, &acc, 1) == hipSuccess;
      if (dok) {
        K->dva = va;
      } else {
        if (m) (void)hipMemUnmap(va, K->pool_bytes);
        if (va) (void)hipMemAddressFree(va, K->pool_bytes);
        (void)hipGetLastError();
      }
    }
    const size_t sp = align_up((size_t)P->C * SEG, gran ? gran : 1);
    bool prim = false, reserved = false, m1 = false, m2 = false;
    if (ok) prim = ok = hipMemCreate(&P->prim_h, sp, &prop, 0) == hipSuccess;
    if (ok) reserved = ok = hipMemAddressReserve(&P->va, sp + K->pool_bytes, 0, nullptr, 0) == hipSuccess;
    if (ok) m1 = ok = hipMemMap(P->va, sp, 0, P->prim_h, 0) == hipSuccess;
    if (ok) m2 = ok = hipMemMap((char*)P->va + sp, K->pool_bytes, 0, K->pool_h, 0) == hipSuccess;
    if (ok) {
      hipMemAccessDesc acc{};
      acc.location = prop.location;
      acc.flags = hipMemAccessFlagsProtReadWrite;
      ok = hipMemSetAccess(P->va, sp + K->pool_bytes, &acc, 1) == hipSuccess;
    }
    if (!ok && pair_debug())
      fprintf(stderr, "pair: pool mapping failed (prim %d reserved %d map %d/%d tier %d): %s\n", (int)prim, (int)reserved,
              (int)m1, (int)m2, K->tier, hipGetErrorString(hipGetLastError()));
    if (ok) {
      P->pool_vmm = true;
      P->prim_bytes = sp;
      P->va_bytes = sp + K->pool_bytes;
      P->pool = (uint8_t*)P->va + sp - (size_t)P->C * SEG;
      return 0;
    }
    if (m2) (void)hipMemUnmap((char*)P->va + sp, K->pool_bytes);
    if (m1) (void)hipMemUnmap(P->va, sp);
    if (reserved) (void)hipMemAddressFree(P->va, sp + K->pool_bytes);
    if (prim) (void)hipMemRelease(P->prim_h);
    P->va = nullptr;
    (void)hipGetLastError();
  }
  if (!P->mem.dev(&P->pool, ((uint64_t)P->C + P->D) * SEG + 256)) return XCG_RC_NOMEM;
  P->pool_vmm = false;
  return 0;
}

void unmap_pool(XcgPairState* P) {
  if (P->pool_vmm) {
    (void)hipDeviceSynchronize();
    (void)hipMemUnmap((char*)P->va + P->prim_bytes, P->va_bytes - P->prim_bytes);
    (void)hipMemUnmap(P->va, P->prim_bytes);
    (void)hipMemAddressFree(P->va, P->va_bytes);
    (void)hipMemRelease(P->prim_h);
  } else {
    P->mem.release(P->pool);
  }
  P->pool = nullptr;
}

struct OnDevice {                 // run on `dev`, restore the caller's device after
  int prev = -1;
  explicit OnDevice(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (dev >= 0 && prev != dev) (void)hipSetDevice(dev);
  }
  ~OnDevice() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// The disk's blocks through its own mapping of the physical allocation: the
// bytes are there whether or not any front still maps them.
int read_disk_blocks(const XcgDiskState* K, uint8_t* dst) {
  const uint8_t* src = (const uint8_t*)K->dva;
  for (const XcgPairState* f : K->fronts)            // (no mapping of its own: a live front's)
    if (!src && f) src = f->pool + (uint64_t)f->C * SEG;
  if (!src) return XCG_RC_HIP;
  return hipMemcpy(dst, src, (size_t)K->vol.D * SEG, hipMemcpyDeviceToHost) == hipSuccess ? 0 : XCG_RC_HIP;
}

}  // namespace

extern "C" {

int xcg_disk_state_create(uint64_t disk_bytes, uint32_t flags, XcgDiskState** out) {
  Volume vol;
  const int rc = volume_geometry(&vol, disk_bytes);
  if (rc) return rc;
  XcgDiskState* K = new XcgDiskState;
  K->vol = std::move(vol);
  K->flags = flags;
  *out = K;
  return 0;
}

void xcg_disk_state_release(XcgDiskState* K) {
  if (!K || --K->refs > 0) return;
  K->mem.release_all();
  if (K->dva) {
    (void)hipDeviceSynchronize();
    (void)hipMemUnmap(K->dva, K->pool_bytes);
    (void)hipMemAddressFree(K->dva, K->pool_bytes);
  }
  if (K->vmm) (void)hipMemRelease(K->pool_h);
  delete K;
}

void xcg_disk_state_stats(const XcgDiskState* K, uint64_t* st) {
  uint64_t live = 0, fronts = 0;
  for (const XcgPairState* f : K->fronts) fronts += f != nullptr;
  if (K->device >= 0) {
    DevMem mem;                    // (the probe word, freed on return)
    uint32_t* d = nullptr;
    uint32_t h = 0;
    if (mem.dev(&d, 4) && hipMemset(d, 0, 4) == hipSuccess) {
      hipLaunchKernelGGL(pair_count_live_kernel, dim3(grid_for(K->vol.D)), dim3(256), 0, nullptr,
                         (const uint64_t*)K->dent, (const uint32_t*)K->dxuid, K->vol.D, (uint32_t)K->vol.nb,
                         K->vol.dclock, NIL, d);
      if (hipMemcpy(&h, d, 4, hipMemcpyDeviceToHost) == hipSuccess) live = h;
    }
  }
  st[0] = live;
  st[1] = K->vol.dclock;
  st[2] = K->vol.nb;
  st[3] = fronts;
}

void xcg_pair_state_set_unbounded(XcgPairState* P) { P->unbounded = true; }
int xcg_pair_state_unbounded(const XcgPairState* P) { return P && P->unbounded ? 1 : 0; }

// A pair front on disk K, on the current device.  Which front (xuid) it is:
// volume_front_xuid.  The registry entry is written once the front exists.
int xcg_pair_state_create(uint32_t C, XcgDiskState* K, const char* uuid36, int want_xuid, XcgPairState** out) {
  if (C == 0 || !K || (uint64_t)K->vol.D + C >= (1ull << 30)) return XCG_RC_INVAL;
  if (uuid36 && (strlen(uuid36) != 36 || !uuid_ok((const uint8_t*)uuid36))) return XCG_RC_INVAL;
  if (want_xuid >= (int)XUIDS) return XCG_RC_INVAL;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return XCG_RC_HIP;
  auto bound = [&](uint32_t x) { return x < K->fronts.size() && K->fronts[x] != nullptr; };
  std::string name;
  const int xrc = volume_front_xuid(K->vol, uuid36, want_xuid, bound, &name);
  if (xrc < 0) return xrc;
  const uint32_t xuid = (uint32_t)xrc;
  const int brc = disk_bind(K, device);
  if (brc) return brc;
  XcgPairState* P = new XcgPairState;
  P->C = C;
  P->nb = (uint32_t)K->vol.nb;
  P->D = K->vol.D;
  P->disk = K;
  P->xuid = (uint16_t)xuid;
  P->gclock = K->vol.dclock;
  const uint64_t ids = (uint64_t)C + P->D;
  auto fail = [&](int rc) {
    unmap_pool(P);
    P->mem.release_all();
    delete P;
    return rc;
  };
  DevMem& m = P->mem;
  if (!(m.dev(&P->pkey, 8ull * C) && m.dev(&P->pdisk, 8ull * C) && m.dev(&P->lru, 4ull * C) &&
        m.dev(&P->lru2, 4ull * C) && m.dev(&P->ptime, 8 * ids) && m.dev(&P->erep, 4 * ids)) ||
      hipMemset(P->pkey, 0xFF, 8ull * C) != hipSuccess || hipMemset(P->pdisk, 0xFF, 8ull * C) != hipSuccess ||
      hipMemset(P->ptime, 0xFF, 8 * ids) != hipSuccess || ensure_front_arrays(P) != 0 || map_pool(P, device) != 0)
    return fail(XCG_RC_NOMEM);
  uint8_t* blocks = P->pool + (uint64_t)C * SEG;
  Volume& V = K->vol;
  const uint64_t D = V.D;
  if (!K->pending && !K->zeroed) {
    if (hipMemset(blocks, 0, D * SEG) != hipSuccess) return fail(XCG_RC_HIP);
    K->zeroed = K->vmm;
  }
  if (K->pending) {                                         // a reopened volume's ring and blocks
    if (!K->ring_loaded &&
        (hipMemcpy(K->dkey, V.h_key.data(), 8 * D, hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(K->dent, V.h_ent.data(), 8 * D, hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(K->dxuid, V.h_xuid.data(), 4 * D, hipMemcpyHostToDevice) != hipSuccess))
      return fail(XCG_RC_HIP);
    K->ring_loaded = true;
    if (hipMemcpy(blocks, V.h_data.data(), D * SEG, hipMemcpyHostToDevice) != hipSuccess) return fail(XCG_RC_HIP);
  }
  if (!P->pool_vmm && !K->shadow_ok.empty()) {               // blocks of fronts that went away
    for (uint64_t i = 0; i < D; ++i)
      if (K->shadow_ok[i] &&
          hipMemcpy(blocks + i * SEG, &K->shadow[i * SEG], SEG, hipMemcpyHostToDevice) != hipSuccess)
        return fail(XCG_RC_HIP);
  }
  if (K->pending && K->vmm) {                                // (one copy serves every front)
    K->pending = false;
    K->zeroed = true;                                        // (the blocks hold the volume's bytes)
    std::vector<uint64_t>().swap(V.h_key);
    std::vector<uint64_t>().swap(V.h_ent);
    std::vector<uint32_t>().swap(V.h_xuid);
    std::vector<uint8_t>().swap(V.h_data);
  }
  volume_register(&V, xuid, name);
  P->gstale = true;                                          // (G from the disk's entries at the first call)
  if (xuid >= K->fronts.size()) K->fronts.resize(xuid + 1, nullptr);
  K->fronts[xuid] = P;
  ++K->refs;
  *out = P;
  return 0;
}

void xcg_disk_state_head(const XcgDiskState* K, uint64_t* index_block, uint64_t* next) {
  volume_head(K->vol, index_block, next);
}

uint32_t xcg_pair_state_xuid(const XcgPairState* P) { return P->xuid; }

// Save the volume: the ring's hashes, xuids and blocks from wherever they are
// now (a reopened file no device holds yet, the device, the fronts' copies),
// then the file (volume_write).
int xcg_disk_state_save(XcgDiskState* K, const char* path) {
  const Volume& V = K->vol;
  const uint64_t D = V.D;
  std::vector<uint64_t> key(D, NOKEY);
  std::vector<uint32_t> xu(D, 0xFFFFFFFFu);
  std::vector<uint8_t> data((size_t)D * SEG, 0);
  if (K->pending && !K->ring_loaded) {
    key = V.h_key;
    xu = V.h_xuid;
    data = V.h_data;
  } else if (K->device >= 0) {
    OnDevice on(K->device);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(key.data(), K->dkey, 8 * D, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(xu.data(), K->dxuid, 4 * D, hipMemcpyDeviceToHost) != hipSuccess)
      return XCG_RC_HIP;
    if (K->vmm) {
      if (read_disk_blocks(K, data.data())) return XCG_RC_HIP;
    } else {
      // per-front copies: a block comes from the live front that wrote it,
      // else from what a front that went away left, else from the volume
      if (!V.h_data.empty()) data = V.h_data;
      for (uint64_t i = 0; i < D && !K->shadow_ok.empty(); ++i)
        if (K->shadow_ok[i]) memcpy(&data[i * SEG], &K->shadow[i * SEG], SEG);
      std::vector<uint8_t> tmp((size_t)D * SEG);
      for (XcgPairState* f : K->fronts) {
        if (!f) continue;
        if (hipMemcpy(tmp.data(), f->pool + (uint64_t)f->C * SEG, D * SEG, hipMemcpyDeviceToHost) != hipSuccess)
          return XCG_RC_HIP;
        for (uint64_t i = 0; i < D; ++i)
          if (xu[i] == f->xuid) memcpy(&data[i * SEG], &tmp[i * SEG], SEG);
      }
    }
  }
  return volume_write(V, path, key.data(), xu.data(), data.data());
}

// A volume read through an open descriptor (the reference's XCodecDisk keeps
// its file open as fd_, xcodec_cache_disk.cc:840-871): reloaded when it holds
// one (a non-empty file), else a fresh disk.
int xcg_disk_state_open_fd(int fd, uint64_t disk_bytes, uint32_t flags, XcgDiskState** out) {
  XcgDiskState* K = nullptr;
  const int rc = xcg_disk_state_create(disk_bytes, flags, &K);
  if (rc) return rc;
  struct stat st;
  if (fstat(fd, &st) != 0) {
    delete K;
    return XCG_RC_NOENT;
  }
  if (st.st_size > 0) {
    if (volume_load(&K->vol, fd) != 0) {
      delete K;
      return XCG_RC_NOENT;
    }
    K->pending = true;
  }
  *out = K;
  return 0;
}

// Open a volume file: reloaded when it holds one, else a fresh disk.
int xcg_disk_state_open(const char* path, uint64_t disk_bytes, uint32_t flags, XcgDiskState** out) {
  const int fd = ::open(path, O_RDONLY);
  if (fd == -1) {
    if (errno == ENOENT) return xcg_disk_state_create(disk_bytes, flags, out);
    return XCG_RC_NOENT;
  }
  const int rc = xcg_disk_state_open_fd(fd, disk_bytes, flags, out);
  close(fd);
  return rc;
}

uint8_t* xcg_pair_state_pool(const XcgPairState* P) { return P->pool; }
int xcg_disk_state_tier(const XcgDiskState* K) { return K->tier; }

// A front goes away (its XCodecCache is deleted): its entries leave the ring's
// index (XCodecDisk::disconnect).
void xcg_pair_state_destroy(XcgPairState* P) {
  if (!P) return;
  XcgDiskState* K = P->disk;
  (void)hipDeviceSynchronize();
  if (K && K->dent && !P->pool_vmm) {                        // keep the blocks this front wrote
    const uint64_t D = K->vol.D;
    std::vector<uint32_t> xu(D);
    std::vector<uint8_t> tmp((size_t)D * SEG);
    if (hipMemcpy(xu.data(), K->dxuid, 4 * D, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(tmp.data(), P->pool + (uint64_t)P->C * SEG, D * SEG, hipMemcpyDeviceToHost) == hipSuccess) {
      if (K->shadow_ok.empty()) {
        K->shadow.assign((size_t)D * SEG, 0);
        K->shadow_ok.assign(D, 0);
      }
      for (uint64_t i = 0; i < D; ++i)
        if (xu[i] == P->xuid) {
          memcpy(&K->shadow[i * SEG], &tmp[i * SEG], SEG);
          K->shadow_ok[i] = 1;
        }
    }
  }
  if (K && K->dent)
    hipLaunchKernelGGL(pair_drop_front_kernel, dim3(grid_for(K->vol.D)), dim3(256), 0, nullptr, K->dkey, K->dent,
                       (const uint32_t*)K->dxuid, K->vol.D, (uint32_t)P->xuid);
  (void)hipDeviceSynchronize();
  unmap_pool(P);
  P->mem.release_all();
  if (K) {
    K->fronts[P->xuid] = nullptr;
    xcg_disk_state_release(K);
  }
  delete P;
}

// Drop everything this front holds (XCodecCache objects have no clear: this is
// a fresh front; on a disk of its own, a fresh volume).  The caller wipes G.
int xcg_pair_state_clear(XcgPairState* P) {
  XcgDiskState* K = P->disk;
  uint64_t others = 0;
  for (const XcgPairState* f : K->fronts) others += f && f != P;
  if (hipMemset(P->pkey, 0xFF, 8ull * P->C) != hipSuccess || hipMemset(P->pdisk, 0xFF, 8ull * P->C) != hipSuccess)
    return XCG_RC_HIP;
  hipLaunchKernelGGL(pair_drop_front_kernel, dim3(grid_for(K->vol.D)), dim3(256), 0, nullptr, K->dkey, K->dent,
                     (const uint32_t*)K->dxuid, K->vol.D, others ? (uint32_t)P->xuid : NIL);
  if (!others) volume_reset(&K->vol);                        // a fresh volume
  P->pcount = 0;
  P->gclock = K->vol.dclock;
  P->gstale = false;
  P->prev_passes = 1;
  return hipDeviceSynchronize() == hipSuccess ? 0 : XCG_RC_HIP;
}

void xcg_pair_state_stats(const XcgPairState* P, uint64_t* st) {
  const XcgDiskState* K = P->disk;
  DevMem mem;                      // (the probe word, freed on return)
  uint32_t h = 0;
  uint32_t* d = nullptr;
  if (mem.dev(&d, 4) && hipMemset(d, 0, 4) == hipSuccess) {
    hipLaunchKernelGGL(pair_count_live_kernel, dim3(grid_for(K->vol.D)), dim3(256), 0, nullptr,
                       (const uint64_t*)K->dent, (const uint32_t*)K->dxuid, K->vol.D, (uint32_t)K->vol.nb,
                       K->vol.dclock, (uint32_t)P->xuid, d);
    (void)hipMemcpy(&h, d, 4, hipMemcpyDeviceToHost);
  }
  st[0] = P->pcount;
  st[1] = h;
  st[2] = K->vol.dclock;
  st[3] = P->nb;
}

uint32_t xcg_pair_state_last_base(const XcgPairState* P) { return P->last_base; }
uint32_t xcg_pair_state_disk_blocks(const XcgPairState* P) { return P->D; }
XcgDiskState* xcg_pair_state_disk(const XcgPairState* P) { return P->disk; }
const uint64_t* xcg_pair_state_ptime(const XcgPairState* P) { return P->ptime; }

}  // extern "C"
