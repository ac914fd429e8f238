// bsgpu_host.cpp — libbsgpu host side: the C ABI declared in include/bsgpu.h. What it drives
// lives in the headers included below, one per concern: host_mem.h (buffers, streams, knobs),
// host_engine.h (the run pipeline; it includes the passes host_tree.h, host_dedup.h,
// host_restore.h, host_walk.h, host_gc.h, host_read.h, host_blobpool.h and host_blobs.h),
// host_stream.h (copy pool, streaming context), host_hasher.h.
//
// A run = one launch sequence over a batch of stream segments (bsgpu_internal.h):
//   k_start (descriptors in, counters zeroed) → k_scan (+ its exact pass) → prefix(strip counts) →
//   k_compact → k_select → prefix(flags) → k_chunks → … → k_sha (→ k_early_fix), with the early
//   chains (k_pick → k_early) on a second stream from k_compact on
// Everything after k_scan sizes itself from device-side counters, so a run never waits on the
// host; bsg_engine_finish() is the only synchronisation (and the place where a too-small
// candidate buffer is grown and the run repeated).
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <emmintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/bsgpu.h"
#include "bsgpu_internal.h"
#include "bsgpu_launch.h"
#include "buzhash32_table.inc"
#include "host_pool.h"
#include "host_sha256.h"

using namespace bsg;

// The two limits the tree tests read from this file (tests/tree_cases.py), so they stay here.
// one hash run takes at most this many of a pass's blobs (bsg_engine_hash's own bound)
constexpr uint32_t kTreeHashBatch = 65535;
// A height with at most this many nodes puts every node on a wave ticket (as bsg_hasher's small
// batches do): the call waits for each height's longest node, and a typical node (10-60 KB) is
// under kLongMinBlocks, where the engine's own choice would hash it per lane, ~4x slower per
// block. More nodes than this keep every wave busy per lane, and the engine's choice stands.
constexpr uint64_t kTreeWaveNodes = 4096;

#include "host_mem.h"
#include "host_engine.h"
#include "host_stream.h"
#include "host_hasher.h"

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int64_t bsg_debug_get(int k) {
  if (k < BSG_KNOB_SEQ_WAIT || k > BSG_KNOB_LAST) return -1;
  return knob(k).load();
}

int bsg_debug_set(int k, int64_t value) {
  if (k < BSG_KNOB_SEQ_WAIT || k > BSG_KNOB_LAST || value < 0) return BSG_EINVAL;
  if (k == BSG_KNOB_LONG_MODE && value > 2) return BSG_EINVAL;
  if ((k == BSG_KNOB_EARLY || k == BSG_KNOB_POLL || k == BSG_KNOB_COPY_NT ||
       k == BSG_KNOB_HOST_TAIL) && value > 1)
    return BSG_EINVAL;
  if (k == BSG_KNOB_SEQ_WAIT && value > (int64_t)UINT32_MAX) return BSG_EINVAL;  // a u32 poll count
  knob(k).store(value);
  return BSG_OK;
}

const char* bsg_errstr(int err) {
  switch (err) {
    case BSG_OK: return "ok";
    case BSG_EINVAL: return "invalid argument";
    case BSG_ENOMEM: return "out of memory";
    case BSG_EDEVICE: return "HIP device error";
    case BSG_ESTATE: return "invalid state (write after close?)";
    case BSG_ENODEV: return "no such HIP device";
    case BSG_ENOTFOUND: return "not found";
    case BSG_ECORRUPT: return "blob does not match its ref";
    case BSG_EIO: return "filesystem error";
    default: return "unknown error";
  }
}

bsg_params bsg_params_default(void) {
  bsg_params p;
  p.split_bits = 16;  // split/split.go:89
  p.min_size = 1024;  // split/split.go:88
  p.fanout = 8;       // split/split.go:48
  p.reserved = 0;
  return p;
}

void bsg_default_table(uint32_t out[256]) { std::memcpy(out, kBuzhash32Seed1, 1024); }

int bsg_init(int device) {
  if (device < 0 || device >= bsg_device_count()) return BSG_ENODEV;
  HCHECK(hipSetDevice(device));
  // streams for the pool. The first four get the process's hardware queues (GPU_MAX_HW_QUEUES,
  // 4); every further one still costs ~2.4 ms to create, and each live split::Writer holds
  // three (its hasher's, its first engine's, its copy stream): a Writer opened while others are
  // alive spent 7.5 of its 13 ms creating them (profiles/r03_fresh_ctx_api_trace.txt). So the
  // pool starts with BSG_INIT_STREAMS of them (default 16: five live Writers' worth).
  static const int kWarmStreams = [] {
    const char* v = std::getenv("BSG_INIT_STREAMS");
    const int n = v ? std::atoi(v) : 16;
    return std::max(1, std::min<int>(n, (int)kStreamPoolMax));
  }();
  hipStream_t s[kStreamPoolMax] = {};
  int got = 0;
  hipError_t e = hipSuccess;
  for (; got < kWarmStreams && e == hipSuccess; ++got) e = stream_acquire(device, &s[got]);
  if (e != hipSuccess) --got;
  // the device context, the copy engines and libbsgpu's code object: one small H2D, kernel and
  // D2H on each warm stream (the process's first DMA copy alone costs tens of ms)
  void* d = nullptr;
  PinBuf h;
  if (e == hipSuccess) e = hipMalloc(&d, 4096);
  if (e == hipSuccess) e = h.ensure(4096);
  for (int i = 0; i < got && e == hipSuccess; ++i) {
    e = hipMemcpyAsync(d, h.p, 2048, hipMemcpyHostToDevice, s[i]);
    if (e == hipSuccess) e = launch_copy_out(d, static_cast<uint8_t*>(d) + 2048, 64, s[i]);
    if (e == hipSuccess) e = hipMemcpyAsync(h.p, d, 64, hipMemcpyDeviceToHost, s[i]);
    if (e == hipSuccess) e = hipStreamSynchronize(s[i]);
  }
  if (d) (void)hipFree(d);
  h.release();
  for (int i = 0; i < got; ++i) stream_release(device, s[i]);
  HCHECK(e);
  // every kernel of the split and hash paths once (HIP loads a kernel at its first launch,
  // ~0.5 ms each, ~20 of them): a 64 KiB split, the same bytes as one blob, one blob per lane
  int rc = BSG_OK;
  bsg_engine* eng = bsg_engine_create(device, nullptr, &rc);
  if (!eng) return rc;
  constexpr uint64_t kWarm = 64 << 10;
  uint8_t* buf = static_cast<uint8_t*>(bsg_device_malloc(device, kWarm + kReadSlack));
  const uint64_t off = 0, len = kWarm;
  uint64_t n = 0;
  if (!buf) rc = BSG_ENOMEM;
  eng->early_min = 0;  // the early-chain kernels too (they pick nothing in 64 KiB)
  (void)bsg_engine::host_sha_rate(false);  // the host tail's cost model: one worker's SHA-256 rate
  if (rc == BSG_OK) rc = bsg_fill_splitmix(device, buf, kWarm, 1, eng->stream);
  if (rc == BSG_OK) rc = bsg_engine_run(eng, buf, &off, &len, 1, nullptr);
  if (rc == BSG_OK) rc = bsg_engine_finish(eng, &n);
  if (rc == BSG_OK) rc = bsg_engine_hash(eng, buf, &off, &len, 1);
  if (rc == BSG_OK) rc = bsg_engine_finish(eng, &n);
  if (rc == BSG_OK) {
    uint8_t ref[32];
    uint8_t blob[64] = {0};
    const uint64_t boff = 0, blen = sizeof blob;
    bsg_hasher* hs = bsg_hasher_new(device);
    rc = hs ? bsg_hasher_sum(hs, blob, &boff, &blen, 1, ref) : BSG_EDEVICE;
    bsg_hasher_free(hs);
  }
  bsg_device_free(device, buf);
  bsg_engine_destroy(eng);
  if (rc) return rc;
  bsg::parallel_for(bsg::copy_threads(), [](size_t) {});  // the host copy pool's threads
  // a ring's worth of full-size pinned stages for the first large stream
  if ((rc = StagePool::get().fill(kStages))) return rc;
  // the streaming path once (registered staging, H2D from it, kernels writing into mapped
  // host memory, events): first uses the process would otherwise pay in its first Writer
  bsg_ctx* c = bsg_open(device, nullptr, nullptr, &rc);
  if (!c) return rc;
  std::vector<uint8_t> bytes(kWarm);
  for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = (uint8_t)(i * 2654435761u >> 24);
  rc = bsg_write(c, bytes.data(), bytes.size());
  if (rc == BSG_OK) rc = bsg_close(c);
  bsg_free(c);
  return rc;
}

int bsg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

bsg_engine* bsg_engine_create(int device, const uint32_t* table, int* err) {
  int dummy;
  if (!err) err = &dummy;
  if (device < 0 || device >= bsg_device_count()) {
    *err = BSG_ENODEV;
    return nullptr;
  }
  bsg_engine* e = new (std::nothrow) bsg_engine();
  if (!e) {
    *err = BSG_ENOMEM;
    return nullptr;
  }
  e->dev = device;
  if (hipSetDevice(device) != hipSuccess ||
      stream_acquire(device, &e->stream) != hipSuccess) {
    delete e;
    *err = BSG_EDEVICE;
    return nullptr;
  }
  e->num_cus = device_cus(device);
  std::memcpy(e->htable, table ? table : kBuzhash32Seed1, sizeof e->htable);
  if (e->table.ensure(1024) != hipSuccess ||
      hipMemcpy(e->table.p, e->htable, 1024, hipMemcpyHostToDevice) != hipSuccess) {
    bsg_engine_destroy(e);
    *err = BSG_EDEVICE;
    return nullptr;
  }
  *err = BSG_OK;
  return e;
}

void bsg_engine_destroy(bsg_engine* e) {
  if (!e) return;
  hipSetDevice(e->dev);
  if (e->stream) hipStreamSynchronize(e->stream);
  if (e->hasher) {  // (it ran on e->stream, synchronised above)
    bsg_engine_destroy(e->hasher);
    e->hasher = nullptr;
  }
  // a failed run may have left early chains (k_pick / k_early on estream) that the engine
  // stream never waited for: they read cand, ctr and the data, so they end before any release
  if (e->estream) hipStreamSynchronize(e->estream);
  // the hash workers leave an unfinished tail and are joined before its pinned buffers go
  e->workers.reset();
  const int dev = e->dev;
  const hipStream_t estream = e->estream, stream = e->borrowed_stream ? nullptr : e->stream;
  delete e;  // every buffer and event of the run and of the passes, now that nothing runs
  stream_release(dev, estream);  // (synchronised above)
  stream_release(dev, stream);
}

// Checks a device-resident batch (a 16-byte aligned base and offsets, streams under 2^40 bytes
// whose ends do not wrap, the read slack inside the allocation) and fills the engine's
// descriptors: fresh, final streams. The streams may lie in any order, apart or on top of each
// other. The argument checks come before the first HIP call: a wrapped off + len would pass the
// allocation check below and hand the kernels a wild address.
static int engine_batch(bsg_engine* e, const uint8_t* d_data, const uint64_t* off,
                        const uint64_t* len, uint32_t nstreams) {
  if (!e || (nstreams && (!d_data || !off || !len)) || nstreams > 65535) return BSG_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_data) % 16 != 0) return BSG_EINVAL;
  uint64_t hi = 0;  // an empty stream's offset counts too: it is still an address in d_data
  for (uint32_t s = 0; s < nstreams; ++s) {
    if (off[s] % 16 != 0 || len[s] >= (1ull << 40)) return BSG_EINVAL;
    if (off[s] > UINT64_MAX - len[s]) return BSG_EINVAL;
    hi = std::max<uint64_t>(hi, off[s] + len[s]);
  }
  int rc;
  if ((rc = e->setdev())) return rc;
  // the SHA-256 loader reads up to kReadSlack bytes past a stream's end (masked): that memory
  // must belong to the same allocation
  if (nstreams) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_data) != hipSuccess) {
      (void)hipGetLastError();
      return BSG_EINVAL;  // not a HIP device allocation
    }
    const uint64_t avail = (uint64_t)((const uint8_t*)base + size - d_data);
    if (avail < kReadSlack || hi > avail - kReadSlack) {  // (hi + kReadSlack could wrap)
      std::fprintf(stderr, "bsgpu: device buffer needs %llu readable bytes after the last "
                           "stream (has %llu)\n", (unsigned long long)kReadSlack,
                   (unsigned long long)(avail > hi ? avail - hi : 0));
      return BSG_EINVAL;
    }
  }
  e->descs.assign(nstreams, StreamDesc{});
  for (uint32_t s = 0; s < nstreams; ++s) {
    StreamDesc& d = e->descs[s];
    d.data_off = off[s];
    d.len = len[s];
    d.finalize = 1;
    std::memcpy(d.mid, kIV, sizeof kIV);
  }
  e->d_data = d_data;
  e->nstreams = nstreams;
  return BSG_OK;
}

int bsg_engine_run(bsg_engine* e, const uint8_t* d_data, const uint64_t* off, const uint64_t* len,
                   uint32_t nstreams, const bsg_params* params) {
  Params p;
  bsg_params norm;
  int rc = normalize(params, &p, &norm);
  if (rc) return rc;
  if (e) e->run_done = false;
  if ((rc = engine_batch(e, d_data, off, len, nstreams))) return rc;
  e->p = p;
  e->fanout = norm.fanout;
  e->hash_mode = false;
  return e->enqueue();
}

int bsg_engine_hash(bsg_engine* e, const uint8_t* d_data, const uint64_t* off, const uint64_t* len,
                    uint32_t nblobs) {
  if (e) e->run_done = false;
  int rc = engine_batch(e, d_data, off, len, nblobs);
  if (rc) return rc;
  normalize(nullptr, &e->p, nullptr);
  e->hash_mode = true;
  return e->enqueue_hash();
}

int bsg_engine_finish(bsg_engine* e, uint64_t* nchunks) {
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->finish(nchunks);
}

const bsg_chunk* bsg_engine_chunks_device(const bsg_engine* e) {
  return e ? static_cast<const bsg_chunk*>(e->out.p) : nullptr;
}

int bsg_engine_copy_chunks(bsg_engine* e, bsg_chunk* out, uint64_t cap) {
  if (!e || (!out && cap)) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  const uint64_t n = std::min<uint64_t>(cap, e->last.nchunks);
  if (n) HCHECK(hipMemcpy(out, e->out.p, sizeof(bsg_chunk) * n, hipMemcpyDeviceToHost));
  return BSG_OK;
}

int bsg_engine_copy_counts(bsg_engine* e, uint64_t* counts, uint32_t nstreams) {
  if (!e || !counts || nstreams > e->nstreams) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if (nstreams)
    HCHECK(hipMemcpy(counts, e->scount.p, sizeof(uint64_t) * nstreams, hipMemcpyDeviceToHost));
  return BSG_OK;
}

void* bsg_engine_stream(bsg_engine* e) { return e ? (void*)e->stream : nullptr; }

int bsg_engine_trees(bsg_engine* e, uint64_t* nnodes, uint64_t* arena_bytes) {
  if (!e || !nnodes || !arena_bytes) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if ((rc = e->tree.run(e->view()))) return rc;
  *nnodes = e->tree.plan.nn;
  *arena_bytes = e->tree.plan.arena;
  return BSG_OK;
}

int bsg_engine_copy_roots(bsg_engine* e, uint8_t* roots, uint64_t* node_counts,
                          uint32_t nstreams) {
  if (!e || !roots) return BSG_EINVAL;
  if (!e->tree.current(e->run_done)) return BSG_ESTATE;
  if (nstreams > e->tree.plan.ns) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if (nstreams) {
    HCHECK(hipMemcpy(roots, e->tree.roots.p, 32ull * nstreams, hipMemcpyDeviceToHost));
    if (node_counts)
      HCHECK(hipMemcpy(node_counts, e->tree.ncount.p, 8ull * nstreams, hipMemcpyDeviceToHost));
  }
  return BSG_OK;
}

int bsg_engine_copy_tree_nodes(bsg_engine* e, bsg_tree_node* out, uint64_t cap, uint8_t* arena,
                               uint64_t arena_cap) {
  if (!e || (!out && cap) || (!arena && arena_cap)) return BSG_EINVAL;
  if (!e->tree.current(e->run_done)) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const uint64_t n = std::min<uint64_t>(cap, e->tree.plan.nn);
  const uint64_t nb = std::min<uint64_t>(arena_cap, e->tree.plan.arena);
  if (n) HCHECK(hipMemcpy(out, e->tree.nodes.p, sizeof(bsg_tree_node) * n, hipMemcpyDeviceToHost));
  if (nb) HCHECK(hipMemcpy(arena, e->tree.arena.p, nb, hipMemcpyDeviceToHost));
  return BSG_OK;
}

const bsg_tree_node* bsg_engine_tree_nodes_device(const bsg_engine* e) {
  return e && e->tree.current(e->run_done) ? e->tree.nodes.as<const bsg_tree_node>() : nullptr;
}

const uint8_t* bsg_engine_tree_arena_device(const bsg_engine* e) {
  return e && e->tree.current(e->run_done) ? e->tree.arena.as<uint8_t>() : nullptr;
}

const uint8_t* bsg_engine_roots_device(const bsg_engine* e) {
  return e && e->tree.current(e->run_done) ? e->tree.roots.as<uint8_t>() : nullptr;
}

int bsg_engine_dedup(bsg_engine* e, bsg_refset* set, uint64_t* nunique, uint64_t* unique_bytes) {
  if (!e || !nunique || !unique_bytes || (set && set->dev != e->dev)) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if ((rc = e->dd.run(e->view(), set))) return rc;
  *nunique = e->dd.nunique;
  *unique_bytes = e->dd.bytes;
  return BSG_OK;
}

int bsg_engine_copy_dedup(bsg_engine* e, uint64_t* first, uint64_t cap_first, uint64_t* uniq,
                          uint64_t* pack_off, uint64_t cap_uniq) {
  if (!e) return BSG_EINVAL;
  if (!e->dd.current(e->run_done)) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const uint64_t nf = std::min<uint64_t>(cap_first, e->dd.n);
  const uint64_t nu = std::min<uint64_t>(cap_uniq, e->dd.nunique);
  if (first && nf) HCHECK(hipMemcpy(first, e->dd.first.p, 8 * nf, hipMemcpyDeviceToHost));
  if (uniq && nu) HCHECK(hipMemcpy(uniq, e->dd.uniq.p, 8 * nu, hipMemcpyDeviceToHost));
  if (pack_off) HCHECK(hipMemcpy(pack_off, e->dd.pack_off.p, 8 * (nu + 1), hipMemcpyDeviceToHost));
  return BSG_OK;
}

const uint64_t* bsg_engine_dedup_first_device(const bsg_engine* e) {
  return e && e->dd.current(e->run_done) ? e->dd.first.as<uint64_t>() : nullptr;
}

const uint64_t* bsg_engine_dedup_uniq_device(const bsg_engine* e) {
  return e && e->dd.current(e->run_done) ? e->dd.uniq.as<uint64_t>() : nullptr;
}

const uint64_t* bsg_engine_dedup_pack_off_device(const bsg_engine* e) {
  return e && e->dd.current(e->run_done) ? e->dd.pack_off.as<uint64_t>() : nullptr;
}

int bsg_engine_pack_unique(bsg_engine* e, uint8_t* d_out, uint64_t cap) {
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->dd.pack(e->view(), d_out, cap);
}

static_assert(sizeof(bsg_pool_blob) == sizeof(PoolBlob), "bsg_pool_blob layout");
static_assert(sizeof(bsg_restore_info) == 32, "bsg_restore_info layout");

int bsg_engine_restore(bsg_engine* e, const uint8_t* d_pool, uint64_t pool_bytes,
                       const bsg_pool_blob* blobs, uint64_t nblobs, const bsg_chunk* recs,
                       uint64_t nrecs, uint8_t* d_out, uint64_t out_cap, const uint64_t* out_off,
                       const uint64_t* out_len, uint32_t nstreams, int flags,
                       bsg_restore_info* info) {
  if (info) *info = bsg_restore_info{UINT64_MAX, UINT64_MAX, 0, 0};
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->restore.run(e->view(), d_pool, pool_bytes, blobs, nblobs, recs, nrecs, nullptr, d_out,
                        out_cap, out_off, out_len, nstreams, flags, info);
}

static_assert(sizeof(bsg_walk_info) == 40, "bsg_walk_info layout");

int bsg_engine_walk(bsg_engine* e, const uint8_t* d_pool, uint64_t pool_bytes,
                    const bsg_pool_blob* blobs, uint64_t nblobs, const uint8_t* roots,
                    uint32_t nstreams, int flags, int32_t* status, bsg_walk_info* info) {
  if (info) *info = bsg_walk_info{UINT64_MAX, 0, 0, 0, 0, 0};
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->walk.run(e->view(), d_pool, pool_bytes, blobs, nblobs, roots, nstreams, flags, status,
                     info);
}

int bsg_engine_copy_walk(bsg_engine* e, bsg_chunk* recs, uint64_t cap, uint64_t* sizes,
                         uint64_t* counts, uint32_t nstreams) {
  if (!e) return BSG_EINVAL;
  if (!e->walk.valid) return BSG_ESTATE;
  if (nstreams > e->walk.ns) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  const uint64_t n = std::min<uint64_t>(cap, e->walk.nrecs);
  if (recs && n) HCHECK(hipMemcpy(recs, e->walk.recs.p, sizeof(bsg_chunk) * n, hipMemcpyDeviceToHost));
  if (sizes && nstreams) std::memcpy(sizes, e->walk.sizes.data(), 8ull * nstreams);
  if (counts && nstreams) std::memcpy(counts, e->walk.counts.data(), 8ull * nstreams);
  return BSG_OK;
}

const bsg_chunk* bsg_engine_walk_records_device(const bsg_engine* e) {
  return e && e->walk.valid ? e->walk.recs.as<const bsg_chunk>() : nullptr;
}

int bsg_engine_restore_walk(bsg_engine* e, const uint8_t* d_pool, uint64_t pool_bytes,
                            const bsg_pool_blob* blobs, uint64_t nblobs, uint8_t* d_out,
                            uint64_t out_cap, const uint64_t* out_off, uint32_t nstreams,
                            int flags, bsg_restore_info* info) {
  if (info) *info = bsg_restore_info{UINT64_MAX, UINT64_MAX, 0, 0};
  if (!e) return BSG_EINVAL;
  if (!e->walk.valid) return BSG_ESTATE;
  if (nstreams != e->walk.ns) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->restore.run(e->view(), d_pool, pool_bytes, blobs, nblobs, nullptr, e->walk.nrecs,
                        e->walk.recs.as<ChunkRec>(), d_out, out_cap, out_off,
                        e->walk.sizes.data(), nstreams, flags, info);
}

static_assert(sizeof(bsg_gc_info) == 72, "bsg_gc_info layout");

int bsg_engine_gc_mark(bsg_engine* e, const uint8_t* d_pool, uint64_t pool_bytes,
                       const bsg_pool_blob* blobs, uint64_t nblobs, const uint8_t* roots,
                       uint64_t nroots, int flags, int32_t* status, bsg_gc_info* info) {
  if (info) *info = bsg_gc_info{UINT64_MAX, UINT64_MAX, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->gc.mark(e->view(), d_pool, pool_bytes, blobs, nblobs, roots, nroots, flags, status,
                    info);
}

int bsg_engine_copy_gc(bsg_engine* e, uint8_t* live, uint64_t cap_live, bsg_pool_blob* table,
                       uint64_t cap_table, int flags) {
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->gc.copy(live, cap_live, table, cap_table, flags);
}

const uint8_t* bsg_engine_gc_live_device(const bsg_engine* e) {
  return e && e->gc.valid ? e->gc.live.as<const uint8_t>() : nullptr;
}

int bsg_engine_gc_compact(bsg_engine* e, const uint8_t* d_pool, uint64_t pool_bytes,
                          uint8_t* d_out, uint64_t cap, int flags, uint64_t* out_bytes) {
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->gc.compact(e->view(), d_pool, pool_bytes, d_out, cap, flags, out_bytes);
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_gc_mark call's stages in ms
// (index + Roots, levels, offsets) and the last bsg_engine_gc_compact, with bsg_engine_profile on.
extern "C" int bsg_engine_gc_ms_debug(const bsg_engine* e, float out[4]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile) return BSG_ESTATE;
  for (int i = 0; i < 3; ++i) out[i] = e->gc.ms[i];
  out[3] = e->gc.compact_ms;
  return BSG_OK;
}

// ---- bsg_pool -----------------------------------------------------------------------------
static_assert(sizeof(bsg_pool_put_info) == 64 && sizeof(bsg_pool_stats) == 40, "bsg_pool layouts");

bsg_pool* bsg_pool_new(int device, uint64_t cap_bytes, uint64_t cap_blobs, int* err) {
  int dummy;
  if (!err) err = &dummy;
  if (device < 0 || device >= bsg_device_count()) {
    *err = BSG_ENODEV;
    return nullptr;
  }
  bsg_pool* p = new (std::nothrow) bsg_pool();
  if (!p) {
    *err = BSG_ENOMEM;
    return nullptr;
  }
  *err = herr(hipSetDevice(device));
  if (*err == BSG_OK) *err = p->create(device, cap_bytes, cap_blobs);
  if (*err == BSG_OK) return p;
  (void)hipGetLastError();
  delete p;
  return nullptr;
}

void bsg_pool_free(bsg_pool* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> g(p->mu);  // a put on another thread ends first
    hipSetDevice(p->dev);
  }
  delete p;
}

int bsg_pool_stat(const bsg_pool* p, bsg_pool_stats* out) {
  if (!p || !out) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(const_cast<bsg_pool*>(p)->mu);
  *out = bsg_pool_stats{p->nblobs, p->used, p->cap_blobs, p->cap_bytes, p->pool_bytes()};
  return BSG_OK;
}

const uint8_t* bsg_pool_bytes_device(const bsg_pool* p) {
  return p ? p->bytes.as<const uint8_t>() : nullptr;
}

const bsg_pool_blob* bsg_pool_table_device(const bsg_pool* p) {
  return p ? p->table.as<const bsg_pool_blob>() : nullptr;
}

int bsg_pool_copy_table(bsg_pool* p, bsg_pool_blob* out, uint64_t first, uint64_t cap) {
  if (!p || (!out && cap)) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->dead) return BSG_ESTATE;
  if (first > p->nblobs) return BSG_EINVAL;
  const uint64_t n = std::min<uint64_t>(cap, p->nblobs - first);
  HCHECK(hipSetDevice(p->dev));
  if (n)
    HCHECK(hipMemcpy(out, p->table.as<PoolBlob>() + first, sizeof(PoolBlob) * n,
                     hipMemcpyDeviceToHost));
  return BSG_OK;
}

int bsg_pool_copy_where(bsg_pool* p, uint64_t* where, uint64_t cap) {
  if (!p || (!where && cap)) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->dead || !p->put_done) return BSG_ESTATE;
  const uint64_t n = std::min<uint64_t>(cap, p->nwhere);
  HCHECK(hipSetDevice(p->dev));
  if (n) HCHECK(hipMemcpy(where, p->where.p, 8 * n, hipMemcpyDeviceToHost));
  return BSG_OK;
}

const uint64_t* bsg_pool_where_device(const bsg_pool* p) {
  return p && p->put_done && !p->dead && p->nwhere ? p->where.as<const uint64_t>() : nullptr;
}

int bsg_engine_pool_put(bsg_engine* e, bsg_pool* p, int flags, bsg_pool_put_info* info) {
  bsg_pool_put_info none{};
  if (info) *info = none;
  if (!e || !p || !flags || (flags & ~(BSG_POOL_CHUNKS | BSG_POOL_NODES)) || p->dev != e->dev)
    return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  // the run's input may not lie in the pool's own allocation: the append writes there
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(e->d_data), s1 = s0 + data_span(e->descs);
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(p->bytes.p), p1 = p0 + p->pool_bytes();
  if (s0 < p1 && p0 < s1) return BSG_EINVAL;
  const RunView v = e->view();
  if (!v.usable || p->dead) return BSG_ESTATE;
  const bool nodes = (flags & BSG_POOL_NODES) != 0;
  if (nodes && !e->tree.current(e->run_done)) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  return p->put(v, nodes ? &e->tree : nullptr, flags, info ? info : &none);
}

// ---- a pool collected into a pool; the walk and the restore on a pool where it lies ---------
static_assert(sizeof(bsg_pool_collect_info) == 88, "bsg_pool_collect_info layout");

int bsg_pool_collect(bsg_engine* e, bsg_pool* src, bsg_pool* dst, const uint8_t* roots,
                     uint64_t nroots, int flags, int32_t* status, bsg_pool_collect_info* info) {
  bsg_pool_collect_info none{};
  if (!info) info = &none;
  *info = bsg_pool_collect_info{bsg_gc_info{UINT64_MAX, UINT64_MAX, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 0};
  if (!e || !src || !dst || src == dst || src->dev != e->dev || dst->dev != e->dev ||
      (flags & ~BSG_GC_MISSING_LEAVES) || nroots > 0xffffffffull || (!roots && nroots))
    return BSG_EINVAL;
  // both pools for the whole call, taken together: A -> B beside B -> A cannot deadlock
  std::unique_lock<std::mutex> gs(src->mu, std::defer_lock), gd(dst->mu, std::defer_lock);
  std::lock(gs, gd);
  if (src->dead || dst->dead || dst->nblobs || e->enqueued) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  return dst->collect(e->view(), e->gc, *src, roots, nroots, flags, status, info);
}

// ---- a pool merged into a pool that holds something; two pools synced --------------------------
static_assert(sizeof(bsg_pool_merge_info) == 144, "bsg_pool_merge_info layout");

static bsg_pool_merge_info merge_clear(bool all) {
  bsg_pool_merge_info i{};
  if (!all) i.gc.bad_root = i.gc.bad_blob = UINT64_MAX;
  i.bad_blob = UINT64_MAX;
  return i;
}

int bsg_pool_merge(bsg_engine* e, bsg_pool* src, bsg_pool* dst, const uint8_t* roots,
                   uint64_t nroots, int flags, int32_t* status, bsg_pool_merge_info* info) {
  bsg_pool_merge_info none{};
  if (!info) info = &none;
  const bool all = (flags & BSG_MERGE_ALL) != 0;
  *info = merge_clear(all);
  if (!e || !src || !dst || src == dst || src->dev != e->dev || dst->dev != e->dev ||
      (flags & ~(BSG_GC_MISSING_LEAVES | BSG_MERGE_ALL | BSG_MERGE_VERIFY)) ||
      (all && (roots || nroots || (flags & BSG_GC_MISSING_LEAVES))) || nroots > 0xffffffffull ||
      (!roots && nroots))
    return BSG_EINVAL;
  // both pools for the whole call, taken together, as bsg_pool_collect
  std::unique_lock<std::mutex> gs(src->mu, std::defer_lock), gd(dst->mu, std::defer_lock);
  std::lock(gs, gd);
  if (src->dead || dst->dead || e->enqueued) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const RunView v = e->view();
  const uint8_t* sel = nullptr;
  if (!all) {
    const PoolSrc ps = src->source();
    rc = e->gc.mark(v, src->bytes.as<const uint8_t>(), src->pool_bytes(), nullptr, src->nblobs,
                    roots, nroots, flags & BSG_GC_MISSING_LEAVES, status, &info->gc, &ps);
    if (rc) return rc;
    sel = e->gc.live.as<const uint8_t>();
  }
  MergeWork& w = e->merge[0];
  if ((rc = w.plan(v, *src, *dst, sel, info))) return rc;
  if ((flags & BSG_MERGE_VERIFY) && (rc = w.verify(v, *src, info))) return rc;
  if (!w.fits(*dst, *info)) return BSG_ENOMEM;
  return w.commit(v, *src, *dst);
}

int bsg_pool_sync(bsg_engine* e, bsg_pool* a, bsg_pool* b, int flags, bsg_pool_merge_info info[2]) {
  bsg_pool_merge_info none[2];
  if (!info) info = none;
  info[0] = info[1] = merge_clear(true);
  if (!e || !a || !b || a == b || a->dev != e->dev || b->dev != e->dev ||
      (flags & ~BSG_MERGE_VERIFY))
    return BSG_EINVAL;
  std::unique_lock<std::mutex> ga(a->mu, std::defer_lock), gb(b->mu, std::defer_lock);
  std::lock(ga, gb);
  if (a->dead || b->dead || e->enqueued) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const RunView v = e->view();
  // What b lacks of a and what a lacks of b, each against the other pool as it stands: a blob the
  // first direction appends to b is one a holds, so the second direction would find it known.
  bsg_pool* src[2] = {a, b};
  bsg_pool* dst[2] = {b, a};
  for (int d = 0; d < 2; ++d)
    if ((rc = e->merge[d].plan(v, *src[d], *dst[d], nullptr, &info[d]))) return rc;
  int corrupt = BSG_OK;  // (both directions are verified, so both infos are filled)
  for (int d = 0; d < 2 && (flags & BSG_MERGE_VERIFY); ++d) {
    if ((rc = e->merge[d].verify(v, *src[d], &info[d])) == BSG_ECORRUPT) corrupt = rc;
    else if (rc) return rc;
  }
  if (corrupt) return corrupt;
  for (int d = 0; d < 2; ++d)
    if (!e->merge[d].fits(*dst[d], info[d])) return BSG_ENOMEM;
  // (the second append reads a's blobs below its old end and writes behind it)
  for (int d = 0; d < 2; ++d)
    if ((rc = e->merge[d].commit(v, *src[d], *dst[d]))) return rc;
  return BSG_OK;
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_pool_merge on e (dir 0), or a
// direction of its last bsg_pool_sync: the probe, the plan, the verification, k_pool_merge_append
// and the gather in ms, timed with HIP events on the engine's stream when bsg_engine_profile is on
// (else zeros).
extern "C" int bsg_pool_merge_ms_debug(const bsg_engine* e, int dir, float out[5]) {
  if (!e || !out || dir < 0 || dir > 1) return BSG_EINVAL;
  for (int i = 0; i < 5; ++i) out[i] = e->merge[dir].ms[i];
  return BSG_OK;
}

// ---- blobs put into a pool and got out of it by ref -------------------------------------------
static_assert(sizeof(bsg_pool_get_info) == 48, "bsg_pool_get_info layout");

int bsg_pool_put_blobs(bsg_engine* e, bsg_pool* p, const uint8_t* d_src, const uint64_t* off,
                       const uint64_t* len, uint64_t nblobs, int flags, uint8_t* refs_out,
                       bsg_pool_put_info* info) {
  bsg_pool_put_info none{};
  if (info) *info = none;
  if (!e || !p || flags || nblobs >= (1ull << 32) || (nblobs && (!d_src || !off || !len)) ||
      p->dev != e->dev || reinterpret_cast<uintptr_t>(d_src) % 16 != 0)
    return BSG_EINVAL;
  uint64_t hi = 0;  // an empty blob's offset counts too: it is still an address in d_src
  for (uint64_t i = 0; i < nblobs; ++i) {
    if (off[i] % 16 != 0 || len[i] >= (1ull << 40) || off[i] > UINT64_MAX - len[i])
      return BSG_EINVAL;
    hi = std::max<uint64_t>(hi, off[i] + len[i]);
  }
  int rc = e->setdev();
  if (rc) return rc;
  if (nblobs) {  // the read slack behind the last blob, as bsg_engine_hash
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_src) != hipSuccess) {
      (void)hipGetLastError();
      return BSG_EINVAL;  // not a HIP device allocation
    }
    const uint64_t avail = (uint64_t)((const uint8_t*)base + size - d_src);
    if (avail < kReadSlack || hi > avail - kReadSlack) return BSG_EINVAL;
  }
  std::lock_guard<std::mutex> g(p->mu);
  // the source may not lie in the pool's own allocation: the append writes there
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), s1 = s0 + hi;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(p->bytes.p), p1 = p0 + p->pool_bytes();
  if (s0 < p1 && p0 < s1) return BSG_EINVAL;
  if (p->dead || e->enqueued) return BSG_ESTATE;
  return e->blobs.put(e->view(), *p, d_src, hi, off, len, nblobs, refs_out, info ? info : &none);
}

int bsg_pool_get(bsg_engine* e, bsg_pool* p, const uint8_t* refs, uint64_t nrefs, uint8_t* d_out,
                 uint64_t out_cap, int flags, uint64_t* idx, uint64_t* out_off,
                 bsg_pool_get_info* info) {
  if (info) *info = bsg_pool_get_info{0, 0, 0, 0, UINT64_MAX, 0};
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + out_cap;
  if (!e || !p || !info || (flags & ~BSG_GET_VERIFY) || nrefs >= (1ull << 32) || (!refs && nrefs) ||
      o0 % 16 != 0 || (!d_out) != (!out_cap) || o1 < o0 || p->dev != e->dev)
    return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(p->bytes.p), p1 = p0 + p->pool_bytes();
  if (d_out && o0 < p1 && p0 < o1) return BSG_EINVAL;  // the output inside the pool
  if (p->dead || e->enqueued) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  return e->blobs.get(e->view(), *p, refs, nrefs, d_out, out_cap, flags, idx, out_off, info);
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_pool_put_blobs on e (the hash runs,
// first occurrence + plan, append + gather) and its last bsg_pool_get (probe + sum, verify,
// gather) in ms, timed with HIP events on the engine's stream when bsg_engine_profile is on (else
// zeros).
extern "C" int bsg_pool_blobs_ms_debug(const bsg_engine* e, float out[6]) {
  if (!e || !out) return BSG_EINVAL;
  for (int i = 0; i < 6; ++i) out[i] = e->blobs.ms[i];
  return BSG_OK;
}

int bsg_pool_copy_remap(bsg_pool* p, uint64_t* remap, uint64_t cap) {
  if (!p || (!remap && cap)) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->dead || !p->collect_done) return BSG_ESTATE;
  const uint64_t n = std::min<uint64_t>(cap, p->nremap);
  HCHECK(hipSetDevice(p->dev));
  if (n) HCHECK(hipMemcpy(remap, p->remap.p, 8 * n, hipMemcpyDeviceToHost));
  return BSG_OK;
}

const uint64_t* bsg_pool_remap_device(const bsg_pool* p) {
  return p && p->collect_done && !p->dead && p->nremap ? p->remap.as<const uint64_t>() : nullptr;
}

int bsg_pool_reset(bsg_pool* p) {
  if (!p) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  HCHECK(hipSetDevice(p->dev));
  return p->reset();
}

int bsg_pool_walk(bsg_engine* e, bsg_pool* p, const uint8_t* roots, uint32_t nstreams, int flags,
                  int32_t* status, bsg_walk_info* info) {
  if (info) *info = bsg_walk_info{UINT64_MAX, 0, 0, 0, 0, 0};
  if (!e || !p || p->dev != e->dev) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->dead) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const PoolSrc ps = p->source();
  return e->walk.run(e->view(), p->bytes.as<const uint8_t>(), p->pool_bytes(), nullptr, p->nblobs,
                     roots, nstreams, flags, status, info, &ps);
}

int bsg_pool_restore_walk(bsg_engine* e, bsg_pool* p, uint8_t* d_out, uint64_t out_cap,
                          const uint64_t* out_off, uint32_t nstreams, int flags,
                          bsg_restore_info* info) {
  if (info) *info = bsg_restore_info{UINT64_MAX, UINT64_MAX, 0, 0};
  if (!e || !p || p->dev != e->dev) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->dead) return BSG_ESTATE;
  if (!e->walk.valid) return BSG_ESTATE;
  if (nstreams != e->walk.ns) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  const PoolSrc ps = p->source();
  return e->restore.run(e->view(), p->bytes.as<const uint8_t>(), p->pool_bytes(), nullptr,
                        p->nblobs, nullptr, e->walk.nrecs, e->walk.recs.as<ChunkRec>(), d_out,
                        out_cap, out_off, e->walk.sizes.data(), nstreams, flags, info, &ps);
}

// ---- byte ranges of streams read out of a pool ----------------------------------------------
static_assert(sizeof(bsg_read_range) == 48 && sizeof(bsg_read_info) == 56, "bsg_read layouts");

static void read_clear(uint32_t nranges, int32_t* status, uint64_t* got, bsg_read_info* info) {
  if (info) *info = bsg_read_info{UINT64_MAX, UINT64_MAX, 0, 0, 0, 0, 0, 0};
  if (nranges > 65535) return;  // (BSG_EINVAL: the arrays' lengths are not known to be that)
  for (uint32_t q = 0; q < nranges; ++q) {
    if (status) status[q] = BSG_OK;
    if (got) got[q] = 0;
  }
}

int bsg_engine_read(bsg_engine* e, const uint8_t* d_pool, uint64_t pool_bytes,
                    const bsg_pool_blob* blobs, uint64_t nblobs, const bsg_read_range* ranges,
                    uint32_t nranges, uint8_t* d_out, uint64_t out_cap, const uint64_t* out_off,
                    int flags, int32_t* status, uint64_t* got, bsg_read_info* info) {
  read_clear(nranges, status, got, info);
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->read.run(e->view(), d_pool, pool_bytes, blobs, nblobs, ranges, nranges, d_out, out_cap,
                     out_off, flags, status, got, info);
}

int bsg_pool_read(bsg_engine* e, bsg_pool* p, const bsg_read_range* ranges, uint32_t nranges,
                  uint8_t* d_out, uint64_t out_cap, const uint64_t* out_off, int flags,
                  int32_t* status, uint64_t* got, bsg_read_info* info) {
  read_clear(nranges, status, got, info);
  if (!e || !p || p->dev != e->dev) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->dead) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const PoolSrc ps = p->source();
  return e->read.run(e->view(), p->bytes.as<const uint8_t>(), p->pool_bytes(), nullptr, p->nblobs,
                     ranges, nranges, d_out, out_cap, out_off, flags, status, got, info, &ps);
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_read / bsg_pool_read call's
// stages in ms (index + Roots, levels, placement, resolve + tiling, verify, scatter), with
// bsg_engine_profile on.
extern "C" int bsg_engine_read_ms_debug(const bsg_engine* e, float out[6]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile) return BSG_ESTATE;
  for (int i = 0; i < 6; ++i) out[i] = e->read.ms[i];
  return BSG_OK;
}

// Test tooling (not in bsgpu.h): the pool as a device error during an append leaves it, without
// one: every later call on it is BSG_ESTATE until bsg_pool_reset.
extern "C" int bsg_pool_kill_debug(bsg_pool* p) {
  if (!p) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  p->dead = true;
  return BSG_OK;
}

// Test and measurement tooling (not in bsgpu.h): the last successful bsg_pool_collect into p: its
// k_pool_adopt in ms, timed with HIP events on the collecting engine's stream when its
// bsg_engine_profile is on (else zero). The mark and the gather are bsg_engine_gc_ms_debug's.
extern "C" int bsg_pool_collect_ms_debug(bsg_pool* p, float* out) {
  if (!p || !out) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  *out = p->adopt_ms;
  return BSG_OK;
}

// Test and measurement tooling (not in bsgpu.h): the last successful bsg_engine_pool_put's parts
// in ms (first occurrence and offsets, table append and index, gather, where[]), timed with HIP
// events on the putting engine's stream when its bsg_engine_profile is on (else zeros).
extern "C" int bsg_pool_put_ms_debug(bsg_pool* p, float out[4]) {
  if (!p || !out) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(p->mu);
  for (int i = 0; i < 4; ++i) out[i] = p->ms[i];
  return BSG_OK;
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_walk call's passes in ms
// (index + Roots, levels, placement), with bsg_engine_profile on.
extern "C" int bsg_engine_walk_ms_debug(const bsg_engine* e, float out[3]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile) return BSG_ESTATE;
  for (int i = 0; i < 3; ++i) out[i] = e->walk.ms[i];
  return BSG_OK;
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_restore call's passes in
// ms (index + resolve + tiling check, verify, scatter), with bsg_engine_profile on.
extern "C" int bsg_engine_restore_ms_debug(const bsg_engine* e, float out[3]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile) return BSG_ESTATE;
  for (int i = 0; i < 3; ++i) out[i] = e->restore.ms[i];
  return BSG_OK;
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_dedup and
// bsg_engine_pack_unique calls in ms, timed with HIP events on the engine stream when
// bsg_engine_profile is on; the pack kernel's load variant (1: aligned loads and a byte funnel);
// one hipMemcpyDtoDAsync of n bytes on the engine stream timed the same way.
extern "C" int bsg_engine_dedup_ms_debug(const bsg_engine* e, float out[2]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile || !e->dd.valid) return BSG_ESTATE;
  out[0] = e->dd.ms[0];
  out[1] = e->dd.ms[1];
  return BSG_OK;
}

extern "C" int bsg_engine_pack_mode_debug(bsg_engine* e, int funnel) {
  if (!e || funnel < 0 || funnel > 1) return BSG_EINVAL;
  e->dd.pack_funnel = funnel != 0;
  return BSG_OK;
}

extern "C" int bsg_engine_d2d_ms_debug(bsg_engine* e, void* dst, const void* src, uint64_t n,
                                       float* ms) {
  if (!e || !dst || !src || !ms) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  hipEvent_t a = nullptr, b = nullptr;
  HCHECK(hipEventCreate(&a));
  if (hipEventCreate(&b) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipEventDestroy(a);
    return BSG_EDEVICE;
  }
  hipError_t err = hipEventRecord(a, e->stream);
  if (err == hipSuccess)
    err = hipMemcpyDtoDAsync((hipDeviceptr_t)dst, (hipDeviceptr_t)src, n, e->stream);
  if (err == hipSuccess) err = hipEventRecord(b, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess) err = hipEventElapsedTime(ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (err != hipSuccess) (void)hipGetLastError();
  return herr(err);
}

// ---- bsg_refset ---------------------------------------------------------------------------
bsg_refset* bsg_refset_new(int device, int* err) {
  int dummy;
  if (!err) err = &dummy;
  if (device < 0 || device >= bsg_device_count()) {
    *err = BSG_ENODEV;
    return nullptr;
  }
  bsg_refset* s = new (std::nothrow) bsg_refset();
  if (!s) {
    *err = BSG_ENOMEM;
    return nullptr;
  }
  s->dev = device;
  *err = BSG_EDEVICE;
  if (hipSetDevice(device) == hipSuccess && stream_acquire(device, &s->stream) == hipSuccess) {
    s->num_cus = device_cus(device);
    s->slots = kRefSetSlots0;
    s->key_cap = kRefSetSlots0;
    *err = BSG_ENOMEM;
    if (s->tab.ensure(8 * s->slots) == hipSuccess && s->keys.ensure(32 * s->key_cap) == hipSuccess) {
      *err = herr(hipMemset(s->tab.p, 0xFF, 8 * s->slots));
      if (*err == BSG_OK) return s;
    }
  }
  (void)hipGetLastError();
  bsg_refset_free(s);
  return nullptr;
}

void bsg_refset_free(bsg_refset* s) {
  if (!s) return;
  hipSetDevice(s->dev);
  if (s->stream) {
    hipStreamSynchronize(s->stream);
    stream_release(s->dev, s->stream);
  }
  delete s;
}

uint64_t bsg_refset_count(const bsg_refset* s) { return s ? s->count.load() : 0; }

int bsg_refset_add(bsg_refset* s, const uint8_t* refs, uint64_t n, uint8_t* added) {
  if (!s || (n && !refs) || n > (1ull << 40)) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->dead) return BSG_ESTATE;
  HCHECK(hipSetDevice(s->dev));
  if (!n) return BSG_OK;
  int rc;
  if ((rc = s->work.reserve(n))) return rc;
  MCHECK(s->staged.ensure(32 * n));
  HCHECK(hipMemcpyAsync(s->staged.p, refs, 32 * n, hipMemcpyHostToDevice, s->stream));
  HCHECK(hipMemsetAsync(s->work.hdr.p, 0, sizeof(DedupHdr), s->stream));
  HCHECK(s->work.tab.clear(s->stream));
  DedupArgs a = s->work.args(s->staged.as<uint8_t>(), 32, nullptr, 0, n);
  s->lookup_args(&a);
  HCHECK(dbg("launch_dedup", s->stream, launch_dedup(a, s->stream, s->num_cus)));
  if ((rc = s->work.readback(s->stream))) {
    if (rc == BSG_EDEVICE) s->dead = true;
    return rc;
  }
  const uint64_t m = s->work.last.nunique;
  if (m > n) {
    s->dead = true;
    return BSG_EDEVICE;
  }
  std::vector<uint64_t> first;
  if (added) {
    try {
      first.resize(n);
    } catch (const std::bad_alloc&) {
      return BSG_ENOMEM;
    }
    HCHECK(hipMemcpy(first.data(), s->work.first.p, 8 * n, hipMemcpyDeviceToHost));
  }
  if ((rc = s->add_new(a, m, &s->work, s->stream))) return rc;
  if (added)
    for (uint64_t i = 0; i < n; ++i) added[i] = first[i] == i ? 1 : 0;
  return BSG_OK;
}

int bsg_engine_profile(bsg_engine* e, int enable) {
  if (!e || enable < 0 || enable > 2) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if (enable) HCHECK(e->marks.create(4));
  e->profile = enable;
  return BSG_OK;
}

int bsg_engine_stage_ms(const bsg_engine* e, float out[3]) {
  if (!e || !out || !e->profile) return BSG_EINVAL;
  for (int i = 0; i < 3; ++i) out[i] = e->stage_ms[i];
  return BSG_OK;
}

uint64_t bsg_engine_candidates(const bsg_engine* e) { return e ? e->last.ncand : 0; }

int bsg_engine_diag(const bsg_engine* e, uint64_t out[16]) {
  if (!e || !out) return BSG_EINVAL;
  out[0] = e->last.nlong;
  out[1] = e->last.long_thresh;
  out[2] = e->last.max_nblocks;
  for (int i = 0; i < 5; ++i) out[3 + i] = e->last.diag[i];
  for (int i = 0; i < 5; ++i) out[8 + i] = e->last.diag2[i];
  out[13] = e->last.nshort;
  out[14] = e->last.ntickets;
  out[15] = e->last.total_blocks;
  return BSG_OK;
}

int bsg_engine_host_tail(const bsg_engine* e, uint64_t out[12]) {
  if (!e || !out) return BSG_EINVAL;
  const bsg_engine::TailStat& t = e->tail_stat;
  out[0] = t.chunks;
  out[1] = t.bytes;
  out[2] = t.cut;
  out[3] = (uint64_t)(t.gather_ms > 0 ? t.gather_ms * 1000.f : 0.f);
  out[4] = (uint64_t)std::max<int64_t>(0, t.host_done_us);
  out[5] = (uint64_t)t.impl;
  out[6] = (uint64_t)t.threads;
  out[7] = (uint64_t)t.host_rate;
  out[8] = t.longest_all;
  out[9] = t.longest_left;
  out[10] = t.blocks;
  out[11] = sha256_have_x86() ? 1 : 0;
  return BSG_OK;
}

// Test tooling (not in include/bsgpu.h), beside bsg_engine_early_min_debug: the run size from
// which this engine's later runs may hand chunks to the host (512 MiB by default), a forced cut
// in SHA-256 blocks (every chunk of at least that many, as far as the ring holds them; 0: the
// cost model), the portable hash in the workers, and the ring's size in bytes (0: by the run's).
extern "C" int bsg_engine_host_tail_debug(bsg_engine* e, uint64_t min_bytes, uint32_t force_cut,
                                          int portable, uint64_t ring_bytes) {
  if (!e || e->enqueued || (ring_bytes && ring_bytes < 4096)) return BSG_EINVAL;
  e->tail_min = min_bytes;
  e->tail_force_cut = force_cut;
  e->tail_portable = portable != 0;
  e->tail_ring_force = ring_bytes;
  return BSG_OK;
}

// Experiment tooling (not in include/bsgpu.h): copies the region queues' state after the last
// run (tools/stress_regions.py).
extern "C" int bsg_engine_regions_debug(bsg_engine* e, void* out, uint64_t nbytes) {
  if (!e || !out || !e->regions.p) return BSG_EINVAL;
  if (e->setdev()) return BSG_EDEVICE;
  const uint64_t n = std::min<uint64_t>(nbytes, sizeof(Regions));
  if (hipStreamSynchronize(e->stream) != hipSuccess) return BSG_EDEVICE;
  return hipMemcpy(out, e->regions.p, n, hipMemcpyDeviceToHost) == hipSuccess ? BSG_OK : BSG_EDEVICE;
}

// The Early record behind the device Counters after the last finished run; *ea is left as it
// is after a hash run or where no run had early chains yet.
static int read_early(bsg_engine* e, Early* ea) {
  if (e->hash_mode || !e->ctr.p || e->ctr.cap < sizeof(Counters) + sizeof(Early)) return BSG_OK;
  if (e->setdev() || hipStreamSynchronize(e->stream) != hipSuccess ||
      hipMemcpy(ea, e->dearly(), sizeof(Early), hipMemcpyDeviceToHost) != hipSuccess)
    return BSG_EDEVICE;
  return BSG_OK;
}

// Test tooling (not in include/bsgpu.h): which SHA-256 path the last finished run's jobs took.
// out[0..3]: jobs on solo / group tickets, those tickets, the solo tickets run with a helper
// wave, all wave tickets (k_bucket_scan); out[4], out[5]: 1 if early chain 0 / 1 hashed a chunk
// (k_pick picked one and k_lens took it out of k_sha's queues), read from the Early record
// behind the device Counters; 0 after a hash run or a run without early chains.
extern "C" int bsg_engine_tiers_debug(bsg_engine* e, uint64_t out[6]) {
  if (!e || !out || e->enqueued) return BSG_EINVAL;
  out[0] = e->last.nlong_grp;
  out[1] = e->last.tickets_grp;
  out[2] = e->last.helped;
  out[3] = e->last.ntickets;
  Early ea{};
  const int rc = read_early(e, &ea);
  for (int k = 0; k < kEarly; ++k) out[4 + k] = (ea.top[k] && ea.idx[k]) ? 1 : 0;
  return rc;
}

// Test tooling (not in include/bsgpu.h): the run size from which this engine's later runs take
// early chains (bsg_engine::early_min; kEarlyMinBytes by default, 0: every run). Nothing else
// changes: BSG_KNOB_EARLY, BSG_KNOB_LIGHT_BYTES, the snapshot and hash-mode gates hold as before.
// With it a planted run of a few hundred KiB goes through k_pick, k_early and k_early_fix.
extern "C" int bsg_engine_early_min_debug(bsg_engine* e, uint64_t bytes) {
  if (!e || e->enqueued) return BSG_EINVAL;
  e->early_min = bytes;
  return BSG_OK;
}

// Test tooling (not in include/bsgpu.h): what k_pick and k_lens left in the last finished run's
// Early record: out[0], out[1] = Early::top[0..1] ((blocks << 32) | candidate index, 0: no
// pick), out[2], out[3] = Early::idx[0..1] (1 + the picked chunk's record index, 0: not
// matched). Zeros after a hash run or a run without early chains (k_start clears the record of
// every split run, and only k_pick writes top).
extern "C" int bsg_engine_early_picks_debug(bsg_engine* e, uint64_t out[4]) {
  if (!e || !out || e->enqueued) return BSG_EINVAL;
  Early ea{};
  const int rc = read_early(e, &ea);
  for (int k = 0; k < kEarly; ++k) {
    out[k] = ea.top[k];
    out[kEarly + k] = ea.idx[k];
  }
  return rc;
}

// Test tooling (not in include/bsgpu.h): Counters::rescan of the last finished run, the strips
// whose candidates outnumbered their kSlotCap slots and went through k_rescan; ~0 while a run is
// in flight or without an engine.
extern "C" uint64_t bsg_engine_rescan_debug(const bsg_engine* e) {
  return e && !e->enqueued ? e->last.rescan : ~0ull;
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_trees call's passes in ms,
// timed with HIP events on the engine stream when bsg_engine_profile is on: [0] counting and
// layout, [1] emit, [2] node hashes, [3] the whole call.
extern "C" int bsg_engine_trees_ms_debug(const bsg_engine* e, float out[4]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile || !e->tree.valid) return BSG_ESTATE;
  for (int i = 0; i < 4; ++i) out[i] = e->tree.ms[i];
  return BSG_OK;
}

int bsg_engine_timeline(const bsg_engine* e, uint64_t out[4]) {
  if (!e || !out) return BSG_EINVAL;
  out[0] = e->last.sha_start_rt;
  out[1] = e->last.diag[2];  // longest wave-mode job: start, end
  out[2] = e->last.diag[3];
  out[3] = e->last.lane_end_rt;
  return BSG_OK;
}

bsg_ctx* bsg_open(int device, const bsg_params* params, const uint32_t* table, int* err) {
  int dummy;
  if (!err) err = &dummy;
  Params p;
  bsg_params norm;
  int rc = normalize(params, &p, &norm);
  if (rc) {
    *err = rc;
    return nullptr;
  }
  if (device < 0 || device >= bsg_device_count()) {
    *err = BSG_ENODEV;
    return nullptr;
  }
  bsg_ctx* c = new (std::nothrow) bsg_ctx();
  if (!c) {
    *err = BSG_ENOMEM;
    return nullptr;
  }
  c->params = norm;
  c->p = p;
  if (hipSetDevice(device) != hipSuccess || (rc = c->init(device, table)) != BSG_OK) {
    delete c;
    *err = rc ? rc : BSG_EDEVICE;
    return nullptr;
  }
  *err = BSG_OK;
  return c;
}

int bsg_set_tile(bsg_ctx* c, size_t tile) {
  if (!c || tile < 4096 || c->fill || c->pos != c->stream0 || c->started) return BSG_EINVAL;
  c->tile = tile;
  return BSG_OK;
}

int bsg_set_carry_cap(bsg_ctx* c, size_t bytes) {
  if (!c || c->fill || c->pos != c->stream0 || c->started || bytes > 0xffffffffull)
    return BSG_EINVAL;
  c->carry_cap = bytes;
  return BSG_OK;
}

int bsg_set_stream_base(bsg_ctx* c, uint64_t base) {
  if (!c || c->fill || c->pos != c->stream0 || c->started || c->closed) return BSG_EINVAL;
  c->stream0 = c->pos = base;
  return BSG_OK;
}

static int ctx_write(bsg_ctx* c, const uint8_t* p, size_t n,
                     int (bsg_ctx::*write)(const uint8_t*, size_t)) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (n && !p) return BSG_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  c->started = true;
  int rc = (c->*write)(p, n);
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_write(bsg_ctx* c, const uint8_t* p, size_t n) { return ctx_write(c, p, n, &bsg_ctx::write); }

int bsg_host_register(void* p, size_t n) {
  if (!p || !n) return BSG_EINVAL;
  HCHECK(hipHostRegister(p, n, hipHostRegisterDefault));
  return BSG_OK;
}

int bsg_host_unregister(void* p) {
  if (!p) return BSG_EINVAL;
  HCHECK(hipHostUnregister(p));
  return BSG_OK;
}

int bsg_write_pinned(bsg_ctx* c, const uint8_t* p, size_t n) {
  return ctx_write(c, p, n, &bsg_ctx::write_pinned);
}

int bsg_write_window(bsg_ctx* c, uint8_t** p, size_t* cap) {
  if (!c || !p || !cap) return BSG_EINVAL;
  if (c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  c->started = true;
  int rc = c->window(p, cap);
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_write_commit(bsg_ctx* c, size_t n) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  int rc = c->commit(n);
  if (rc) c->sticky = rc;
  return rc;
}

static int ctx_close(bsg_ctx* c, int (bsg_ctx::*close)()) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return c->sticky;
  c->closed = true;
  if (c->sticky) return c->sticky;
  if (hipSetDevice(c->dev) != hipSuccess) return c->sticky = BSG_EDEVICE;
  int rc = (c->*close)();
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_close(bsg_ctx* c) { return ctx_close(c, &bsg_ctx::close); }

int bsg_close_begin(bsg_ctx* c) { return ctx_close(c, &bsg_ctx::close_begin); }

int bsg_close_step(bsg_ctx* c, size_t* left) {
  if (!c || !left) return BSG_EINVAL;
  *left = 0;
  if (!c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (c->inflight.empty()) return BSG_OK;
  if (hipSetDevice(c->dev) != hipSuccess) return c->sticky = BSG_EDEVICE;
  int rc = c->close_step(left);
  if (rc) c->sticky = rc;
  return rc;
}

size_t bsg_pending(const bsg_ctx* c) {
  if (!c) return 0;
  bsg_ctx* m = const_cast<bsg_ctx*>(c);  // polling completed tiles is not a visible change
  if (!m->sticky && hipSetDevice(m->dev) == hipSuccess) {
    int rc = m->poll();
    if (rc) m->sticky = rc;
  }
  return m->ready.size();
}

size_t bsg_drain(bsg_ctx* c, bsg_chunk* out, size_t cap) {
  if (!c || !out) return 0;
  if (!c->sticky && hipSetDevice(c->dev) == hipSuccess) {
    int rc = c->poll();
    if (rc) c->sticky = rc;
  }
  size_t k = 0;
  while (k < cap && !c->ready.empty()) {
    out[k++] = c->ready.front();
    c->ready.pop_front();
  }
  return k;
}

int bsg_reset(bsg_ctx* c) {
  if (!c) return BSG_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  return c->reset();
}

void bsg_free(bsg_ctx* c) {
  if (!c) return;
  delete c;
}

int bsg_stream_stats_get(bsg_ctx* c, bsg_stream_stats* out) {
  if (!c || !out) return BSG_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  return c->get_stats(out);
}

// bsg_split_hash_batch's engine: a pooled one (DevicePool) with the call's table, or a new one
static bsg_engine* batch_engine_take(int device, const uint32_t* table, int* rc) {
  bsg_engine* e = DevicePool<bsg_engine>::get().take(device);
  if (!e) return bsg_engine_create(device, table, rc);
  *rc = BSG_OK;
  const uint32_t* t = table ? table : kBuzhash32Seed1;
  if (std::memcmp(e->htable, t, sizeof e->htable) != 0) {
    std::memcpy(e->htable, t, sizeof e->htable);
    if (hipSetDevice(device) != hipSuccess ||
        hipMemcpy(e->table.p, e->htable, 1024, hipMemcpyHostToDevice) != hipSuccess) {
      bsg_engine_destroy(e);
      *rc = BSG_EDEVICE;
      return nullptr;
    }
  }
  return e;
}
static void batch_engine_give(bsg_engine* e, bool ok) {
  if (ok && hipSetDevice(e->dev) == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess) {
    e->retry_cap = 0;
    if (DevicePool<bsg_engine>::get().give(e)) return;
  }
  (void)hipGetLastError();
  bsg_engine_destroy(e);
}

int bsg_split_hash_batch(int device, const uint8_t* host_data, const uint64_t* off,
                         const uint64_t* len, uint32_t nstreams, const bsg_params* params,
                         const uint32_t* table, bsg_chunk* out, uint64_t cap, uint64_t* counts,
                         uint64_t* nchunks) {
  if (nstreams && (!host_data || !off || !len)) return BSG_EINVAL;
  if (!out && cap) return BSG_EINVAL;
  int rc;
  bsg_engine* e = batch_engine_take(device, table, &rc);
  if (!e) return rc;
  // Runs of at most 65,535 streams (the engine's limit) and about 8 GiB of device bytes (a
  // larger stream goes alone); each run's streams are packed 16-byte aligned into one buffer.
  constexpr uint32_t kRunStreams = 65535;
  constexpr uint64_t kRunBytes = 8ull << 30;
  constexpr uint64_t kPackWindow = 64ull << 20;
  DevBuf d;
  PinBuf pack;  // the packing window: a full-size stage from the process's pool when one is free
  pack.dma_only = true;
  std::vector<uint64_t> doff;
  uint64_t n = 0;  // records of all runs so far (written to out while they fit in cap)
  for (uint32_t s0 = 0; s0 < nstreams && rc == BSG_OK;) {
    uint32_t s1 = s0;
    uint64_t total = 0;
    doff.clear();
    while (s1 < nstreams && s1 - s0 < kRunStreams &&
           (s1 == s0 || total + len[s1] <= kRunBytes)) {
      doff.push_back(total);
      total += (len[s1] + 15) & ~15ull;
      ++s1;
    }
    if (d.ensure(total + kReadSlack) != hipSuccess) {
      rc = BSG_ENOMEM;
      break;
    }
    // Streams shorter than the pinned window are packed at their device offsets into it and
    // copied a window at a time (one H2D for many small streams); longer ones directly.
    const uint64_t win = std::min<uint64_t>(total, kPackWindow);
    static_assert(kPackWindow <= kStageMax, "a pooled stage holds the packing window");
    if (win && !pack.p) (void)StagePool::get().take(&pack);
    if (win && pack.ensure(win) != hipSuccess) {
      rc = BSG_ENOMEM;
      break;
    }
    uint64_t wlo = 0, whi = 0;  // device span [wlo, whi) staged in pack
    auto flush = [&]() {
      if (whi > wlo && hipMemcpy(static_cast<uint8_t*>(d.p) + wlo, pack.p, whi - wlo,
                                 hipMemcpyHostToDevice) != hipSuccess)
        rc = BSG_EDEVICE;
      wlo = whi;
    };
    for (uint32_t s = s0; s < s1 && rc == BSG_OK; ++s) {
      const uint64_t at = doff[s - s0];
      if (!len[s]) continue;
      if (len[s] > win / 2) {
        flush();
        if (rc == BSG_OK &&
            hipMemcpy(static_cast<uint8_t*>(d.p) + at, host_data + off[s], len[s],
                      hipMemcpyHostToDevice) != hipSuccess)
          rc = BSG_EDEVICE;
        wlo = whi = at + len[s];
        continue;
      }
      if (at + len[s] - wlo > win) flush();
      if (whi == wlo) wlo = whi = at;
      std::memcpy(pack.as<uint8_t>() + (at - wlo), host_data + off[s], len[s]);
      whi = at + len[s];
    }
    if (rc == BSG_OK) flush();
    uint64_t rn = 0;
    if (rc == BSG_OK) rc = bsg_engine_run(e, d.as<uint8_t>(), doff.data(), len + s0, s1 - s0, params);
    if (rc == BSG_OK) rc = bsg_engine_finish(e, &rn);
    if (rc == BSG_OK && n < cap) {
      rc = bsg_engine_copy_chunks(e, out + n, cap - n);
      // records name their stream within the run: make them batch indices
      for (uint64_t k = n; rc == BSG_OK && s0 && k < std::min(cap, n + rn); ++k) out[k].stream += s0;
    }
    if (rc == BSG_OK && counts) rc = bsg_engine_copy_counts(e, counts + s0, s1 - s0);
    n += rn;
    s0 = s1;
  }
  if (nchunks) *nchunks = n;
  d.release();
  StagePool::get().give(&pack);  // keeps a full-size registered stage, frees anything else
  batch_engine_give(e, rc == BSG_OK);
  return rc;
}

void* bsg_device_malloc(int device, size_t bytes) {
  if (device < 0 || device >= bsg_device_count() || hipSetDevice(device) != hipSuccess)
    return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

int bsg_device_free(int device, void* p) {
  if (!p) return BSG_OK;
  HCHECK(hipSetDevice(device));
  HCHECK(hipFree(p));
  return BSG_OK;
}

int bsg_memcpy(int device, void* dst, const void* src, size_t n, int kind) {
  if (n && (!dst || !src)) return BSG_EINVAL;
  HCHECK(hipSetDevice(device));
  hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice
                  : kind == 1 ? hipMemcpyDeviceToHost
                              : hipMemcpyDeviceToDevice;
  if (n) HCHECK(hipMemcpy(dst, src, n, k));
  return BSG_OK;
}

int bsg_device_synchronize(int device) {
  HCHECK(hipSetDevice(device));
  HCHECK(hipDeviceSynchronize());
  return BSG_OK;
}

int bsg_fill_splitmix(int device, uint8_t* d_ptr, uint64_t nbytes, uint64_t seed, void* stream) {
  if (!d_ptr && nbytes) return BSG_EINVAL;
  if (device < 0 || device >= bsg_device_count()) return BSG_ENODEV;
  HCHECK(hipSetDevice(device));
  const int cus = device_cus(device);
  if (nbytes) HCHECK(launch_fill_splitmix(d_ptr, nbytes, seed, (hipStream_t)stream, cus));
  return BSG_OK;
}

}  // extern "C"

extern "C" {

bsg_hasher* bsg_hasher_new(int device) {
  if (device < 0 || device >= bsg_device_count() || hipSetDevice(device) != hipSuccess)
    return nullptr;
  bsg_hasher* h = new (std::nothrow) bsg_hasher();
  if (!h) return nullptr;
  h->dev = device;
  h->num_cus = device_cus(device);
  if (stream_acquire(device, &h->stream) != hipSuccess) {
    delete h;
    return nullptr;
  }
  return h;
}

int bsg_hasher_sum(bsg_hasher* h, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                   uint32_t n, uint8_t* refs) {
  if (!h || (n && (!base || !off || !len || !refs))) return BSG_EINVAL;
  if (n == 0) return BSG_OK;
  HCHECK(hipSetDevice(h->dev));
  return h->sum(base, off, len, n, refs);
}

int bsg_hasher_sum_ptrs(bsg_hasher* h, const uint8_t* const* ptrs, const uint64_t* len,
                        uint32_t n, uint8_t* refs) {
  if (!h || (n && (!ptrs || !len || !refs))) return BSG_EINVAL;
  if (n == 0) return BSG_OK;
  HCHECK(hipSetDevice(h->dev));
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (len[i] && !ptrs[i]) return BSG_EINVAL;
    total += len[i];
  }
  if (n >= bsg_hasher::kEngineMinBlobs && total >= bsg_hasher::kEngineMinBytes)
    return h->sum_engine(nullptr, nullptr, ptrs, len, n, refs);
  // small batches: packed, then the one-blob-per-lane kernel
  std::vector<uint8_t> packed(total ? total : 1);
  std::vector<uint64_t> off(n);
  uint64_t o = 0;
  for (uint32_t i = 0; i < n; ++i) {
    off[i] = o;
    if (len[i]) std::memcpy(packed.data() + o, ptrs[i], len[i]);
    o += len[i];
  }
  return h->sum(packed.data(), off.data(), len, n, refs);
}

size_t bsg_hasher_pinned_bytes(const bsg_hasher* h) {
  if (!h) return 0;
  return h->h_meta.cap + h->h_small.cap + h->stage.cap + h->h_recs.cap;
}

void bsg_hasher_free(bsg_hasher* h) {
  if (!h) return;
  hipSetDevice(h->dev);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->eng) bsg_engine_destroy(h->eng);
  const int dev = h->dev;
  const hipStream_t stream = h->stream;
  delete h;
  stream_release(dev, stream);
}

// (hashers, with their device buffers, pinned staging and engine, are pooled: DevicePool)
int bsg_sha256_batch(int device, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                     uint32_t n, uint8_t* refs) {
  if (n && (!base || !off || !len || !refs)) return BSG_EINVAL;
  if (n == 0) return BSG_OK;
  if (device < 0 || device >= bsg_device_count()) return BSG_ENODEV;
  bsg_hasher* h = DevicePool<bsg_hasher>::get().take(device);
  if (!h && !(h = bsg_hasher_new(device))) return BSG_EDEVICE;
  if (hipSetDevice(device) != hipSuccess) {
    bsg_hasher_free(h);
    return BSG_EDEVICE;
  }
  const int rc = h->sum(base, off, len, n, refs);
  // (sum() synchronised the hasher's streams)
  if (rc != BSG_OK || !DevicePool<bsg_hasher>::get().give(h)) bsg_hasher_free(h);
  return rc;
}

}  // extern "C"
