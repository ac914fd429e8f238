// host_stream.h — the host copy pool (host_pool.h) and the streaming context bsg_ctx.
#pragma once
// ------------------------------------------------------------------------------------------
// Streaming split.Writer (bsg_open / bsg_write / bsg_close / bsg_drain): a pipeline of tiles.
// Tile i's bytes go through a ring of pinned stages, by H2D on the context's copy stream, into
// data slot i mod ndata; its kernels run on engine slot i mod nslots (HIP stream + work buffers).
//
//   host:    copy Write()s into stage s ... flush s (H2D) ... stage s+1 ... submit tile i ...
//   data:    [carry area kCarryCap | tile bytes | read slack]
//   copies:  H2D(i, stage 0..3) -> copied_ev(i)      (waits for data slot i's previous tile)
//   engine:  wait copied_ev(i) -> scan/select(i) -> sel_ev(i) -> k_sha(i) -> records(i)
//
// Tile i+1 needs from tile i only where its open chunk starts, which is known at sel_ev(i), a
// fraction of a millisecond into tile i: the open chunk's bytes (at most kCarryCap; k_sha
// leaves such a chunk unhashed) are copied device-to-device in front of tile i+1's bytes and
// hashed there from the start. Tile i's k_sha — bound by its longest chunk's serial SHA-256
// chain — therefore runs concurrently with tiles i+1, i+2, ... instead of in front of them.
// A longer open chunk falls back to the midstate carry: tile i hashes its whole blocks, and
// tile i+1 waits for tile i's k_sha and continues from the exported midstate.
// Records complete in tile order; bsg_pending/bsg_drain hand them out in stream order.
// ------------------------------------------------------------------------------------------
namespace bsg {

// Host threads copying a large Write into pinned staging (BSG_COPY_THREADS, default 8).
int copy_threads() {
  static const int v = [] {
    const char* e = std::getenv("BSG_COPY_THREADS");
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    return std::max(1, std::min(hw, e ? std::min(64, std::atoi(e)) : 8));
  }();
  return v;
}

namespace {
// One parallel_for call: workers and the caller take indices from `next` until none are left.
struct PoolJob {
  const std::function<void(size_t)>* fn = nullptr;
  size_t n = 0;
  std::atomic<size_t> next{0}, done{0};
  std::mutex mu;
  std::condition_variable cv;
  void run() {
    for (size_t i; (i = next.fetch_add(1)) < n;) {
      (*fn)(i);
      if (done.fetch_add(1) + 1 == n) {
        std::lock_guard<std::mutex> g(mu);
        cv.notify_all();
      }
    }
  }
};

class CopyPool {
 public:
  explicit CopyPool(int workers) {
    for (int i = 0; i < workers; ++i) th_.emplace_back([this] { Work(); });
  }
  void Run(size_t n, const std::function<void(size_t)>& fn) {
    auto job = std::make_shared<PoolJob>();
    job->fn = &fn;
    job->n = n;
    {
      std::lock_guard<std::mutex> g(mu_);
      q_.push_back(job);
    }
    cv_.notify_all();
    job->run();  // the caller works too
    {
      std::unique_lock<std::mutex> g(job->mu);
      job->cv.wait(g, [&] { return job->done.load() == job->n; });
    }
    std::lock_guard<std::mutex> g(mu_);
    for (auto it = q_.begin(); it != q_.end(); ++it)
      if (*it == job) {
        q_.erase(it);
        break;
      }
  }

 private:
  void Work() {
    for (;;) {
      std::shared_ptr<PoolJob> job;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return !q_.empty(); });
        job = q_.front();
        if (job->next.load() >= job->n) {  // every index taken: nothing left to help with
          q_.pop_front();
          continue;
        }
      }
      job->run();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<PoolJob>> q_;
  std::vector<std::thread> th_;
};

CopyPool* copy_pool() {
  // never destroyed: its workers stay blocked on the queue until the process exits
  static CopyPool* pool = copy_threads() > 1 ? new CopyPool(copy_threads() - 1) : nullptr;
  return pool;
}
}  // namespace

void parallel_for(size_t n, const std::function<void(size_t)>& fn) {
  if (n == 0) return;
  if (n == 1 || copy_threads() <= 1) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  copy_pool()->Run(n, fn);
}

bool copy_nt_enabled() { return knob(BSG_KNOB_COPY_NT).load(std::memory_order_relaxed) != 0; }

namespace {
// 64 bytes (one cache line) per iteration: four unaligned 16-byte loads, four streaming stores
// to a 16-byte aligned destination (SSE2, every x86-64 host)
inline void nt_lines(uint8_t* d, const uint8_t* s, size_t lines) {
  for (size_t i = 0; i < lines; ++i, d += 64, s += 64) {
    const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s));
    const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 16));
    const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 32));
    const __m128i e = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 48));
    _mm_stream_si128(reinterpret_cast<__m128i*>(d), a);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 16), b);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 32), c);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 48), e);
  }
}
// the same into two destinations; d2 streams only if it has d1's alignment mod 16, else it
// takes ordinary stores
inline void nt_lines2(uint8_t* d1, uint8_t* d2, const uint8_t* s, size_t lines, bool d2nt) {
  for (size_t i = 0; i < lines; ++i, d1 += 64, d2 += 64, s += 64) {
    __m128i v[4];
    for (int j = 0; j < 4; ++j) v[j] = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 16 * j));
    for (int j = 0; j < 4; ++j) _mm_stream_si128(reinterpret_cast<__m128i*>(d1 + 16 * j), v[j]);
    if (d2nt) {
      for (int j = 0; j < 4; ++j) _mm_stream_si128(reinterpret_cast<__m128i*>(d2 + 16 * j), v[j]);
    } else {
      for (int j = 0; j < 4; ++j) _mm_storeu_si128(reinterpret_cast<__m128i*>(d2 + 16 * j), v[j]);
    }
  }
}
}  // namespace

// The streaming stores are weakly ordered: each copy ends with an sfence, so the bytes are in
// memory before the caller publishes them (a parallel_for's completion, then an H2D copy).
void copy_nt(uint8_t* dst, const uint8_t* src, size_t n) {
  const size_t head = std::min(n, (size_t)(-(uintptr_t)dst & 63));
  std::memcpy(dst, src, head);
  const size_t lines = (n - head) / 64;
  nt_lines(dst + head, src + head, lines);
  const size_t done = head + lines * 64;
  std::memcpy(dst + done, src + done, n - done);
  _mm_sfence();
}

void copy_nt2(uint8_t* d1, uint8_t* d2, const uint8_t* src, size_t n) {
  const size_t head = std::min(n, (size_t)(-(uintptr_t)d1 & 63));
  std::memcpy(d1, src, head);
  std::memcpy(d2, src, head);
  const size_t lines = (n - head) / 64;
  const bool d2nt = (((uintptr_t)d1 ^ (uintptr_t)d2) & 15) == 0;
  nt_lines2(d1 + head, d2 + head, src + head, lines, d2nt);
  const size_t done = head + lines * 64;
  std::memcpy(d1 + done, src + done, n - done);
  std::memcpy(d2 + done, src + done, n - done);
  _mm_sfence();
}

int cpu_node() {
  unsigned cpu = 0, node = 0;
  if (syscall(SYS_getcpu, &cpu, &node, nullptr) != 0) return -1;
  return (int)node;
}

}  // namespace bsg

constexpr int kMaxSlots = 8;
constexpr uint64_t kDefaultCarryCap = 8ull << 20;
// Tiles in flight. Each has its own HIP stream, and streams beyond the process's hardware
// queues (GPU_MAX_HW_QUEUES, 4 by default) share a queue and serialise behind each other's
// k_sha, so the default stays below that.
static int default_slots() {
  const char* e = std::getenv("BSG_STREAM_SLOTS");
  const int v = e ? std::atoi(e) : 3;
  return std::max(2, std::min(kMaxSlots, v));
}

// Device copies of the tiles' bytes, decoupled from the engines: tile i's bytes go to data slot
// i mod ndata and its kernels run on engine slot i mod nslots. With one more data slot than
// engines, tile i's H2D does not wait for tile i - nslots' k_sha (which still reads that engine's
// previous tile), only for tile i - ndata's: the copies run back to back on their own stream
// while the chains of earlier tiles finish.
constexpr int kMaxData = 8;
static int default_data_slots(int nslots) {
  const char* e = std::getenv("BSG_DATA_SLOTS");
  const int v = e ? std::atoi(e) : nslots + 1;
  return std::max(std::max(2, nslots), std::min(kMaxData, v));
}

struct DataSlot {
  DevBuf dbuf;                  // carry area + tile + slack
  Event free_ev;                // recorded on an engine stream after the last reader of dbuf
  bool free_pending = false;    // free_ev recorded, not yet waited for by the copy stream
};

struct TileSlot {
  bsg_engine* eng = nullptr;  // created at the slot's first tile (a small stream needs one)
  PinBuf recs;            // records, D2H'd after k_sha
  Event h2d_ev, done_ev, copied_ev;
  int dslot = 0;          // data slot of the tile using this engine
  // state of the tile currently using the slot
  bool busy = false;          // submitted, records not yet collected
  bool sel_read = false;      // selection snapshot consumed (open_next / nchunks known)
  bool recs_enq = false;      // D2H of records enqueued (done_ev recorded)
  bool final_seg = false;
  uint64_t seg_base = 0, len = 0, nchunks = 0, open_next = 0;
};

// Host staging of the streaming path: a ring of pinned buffers, independent of the device tiles.
// The host fills one stage; a full stage is copied (hipMemcpyAsync, on the engine stream of the
// tile it belongs to) into that tile's device slot right away, so a tile's H2D runs while the
// host is still filling the rest of it, and the pinned memory a context holds is the ring
// (4 x 64 MiB: as much host-side slack as one whole tile), not three whole tiles (3 x 256 MiB).
constexpr int kStages = 4;
constexpr size_t kStageMax = 64ull << 20;
// Full-size stages (kStageMax) are shared process-wide: a context takes them from this pool as
// its stream grows past a stage and gives them back at bsg_reset / bsg_free, so an idle pooled
// context holds no pinned staging, N concurrent contexts share what they use, and bsg_init can
// pin a ring's worth ahead of the first Writer. (Smaller stages — small tiles, a stream's first
// stage while it grows — stay with their context.)
class StagePool {
 public:
  static StagePool& get() {
    static auto* p = new StagePool();  // never destroyed (its buffers live until exit)
    return *p;
  }
  bool take(PinBuf* out) {  // out: empty
    std::lock_guard<std::mutex> g(mu_);
    if (free_.empty()) return false;
    *out = std::move(free_.back());
    free_.pop_back();
    return true;
  }
  void give(PinBuf* b) {  // takes b's buffer if it is a full-size one; b is empty afterwards
    if (!b->p) return;
    if (b->cap >= kStageMax && b->map_len) {
      std::lock_guard<std::mutex> g(mu_);
      if (free_.size() < kMaxFree) {
        free_.push_back(std::move(*b));  // (b stays a DMA stage, empty)
        b->dma_only = true;
        return;
      }
    }
    b->release();
  }
  int fill(int n) {  // bsg_init: make sure n full-size stages are pinned and waiting
    for (;;) {
      {
        std::lock_guard<std::mutex> g(mu_);
        if ((int)free_.size() >= n) return BSG_OK;
      }
      PinBuf b;
      b.dma_only = true;
      if (b.ensure(kStageMax) != hipSuccess) return BSG_ENOMEM;
      give(&b);
      if (b.p) {  // not taken (not a registered mapping): leave the pool as it is
        b.release();
        return BSG_OK;
      }
    }
  }

 private:
  static constexpr size_t kMaxFree = 16;  // at most 1 GiB of idle pinned staging
  std::mutex mu_;
  std::vector<PinBuf> free_;
};

struct Stage {
  PinBuf buf;                // DMA staging (PinBuf::dma_only)
  Event ev;                  // recorded after the H2D that reads the stage
  bool inflight = false;     // an H2D from it may still be running
  Event t0, t1;              // timing events around that H2D (bsg_stream_stats)
  bool timed = false;        // t0/t1 recorded and not yet read
};

// NUMA node of the page holding p (get_mempolicy MPOL_F_NODE | MPOL_F_ADDR; -1 unknown)
static int page_node(const void* p) {
  int node = -1;
  if (!p || syscall(SYS_get_mempolicy, &node, nullptr, 0UL, p, 3UL) != 0) return -1;
  return node;
}


static uint64_t ns_since(std::chrono::steady_clock::time_point t0) {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now() - t0).count();
}

// hipEventElapsedTime(a, b) in nanoseconds into *out, negatives as 0; *out is left alone when the
// events have no time to give
static bool elapsed_ns(hipEvent_t a, hipEvent_t b, uint64_t* out) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  *out = ms > 0.f ? (uint64_t)((double)ms * 1e6) : 0;
  return true;
}

// Where a context is in its current stream: everything a new stream starts over. bsg_ctx is
// one of these plus the resources that outlive a stream, so reset() assigns a fresh value and a
// field added here needs no second mention.
struct StreamState {
  int dcur = 0;             // data slot of the tile the host is filling
  bool dready = false;      // the copy stream waits for data[dcur]'s previous readers already
  int cur = 0;              // slot of the tile the host is filling
  size_t fill = 0;          // bytes of the current tile (copied to the device or staged)
  int scur = 0;             // stage the host is filling
  size_t sfill = 0;         // bytes in stages[scur] (the current tile's last sfill bytes)
  int prev = -1;            // last submitted slot (its open chunk continues into `cur`)
  uint64_t pos = 0;         // stream offset of slots[cur]'s first byte
  uint64_t stream0 = 0;     // stream offset of the stream's first byte (0; bsg_set_stream_base)
  uint8_t hist[64] = {};    // the 64 stream bytes before pos
  uint8_t tail[64] = {};    // the last 64 stream bytes copied to the device so far
  bool closed = false, started = false;
  int sticky = BSG_OK;
  bsg_stream_stats stats{};  // bsg_stream_stats: counters since open / reset
  bool span_set = false;     // span0 recorded
  bool tail_set = false;     // tail1 recorded
  int slast = -1;            // stage of the latest H2D
  bool sent = false;         // the stream's first H2D is issued (first_flush())
};

struct bsg_ctx : StreamState {
  bsg_params params{};
  Params p{};
  int dev = 0;
  uint32_t table[256];
  size_t tile = 256ull << 20;  // (tile and carry_cap are settings: they survive reset())
  uint64_t carry_cap = kDefaultCarryCap;
  int nslots = default_slots();
  TileSlot slots[kMaxSlots];
  int ndata = default_data_slots(nslots);
  DataSlot data[kMaxData];
  hipStream_t cstream = nullptr;  // H2D copies of every tile (from the process's stream pool)
  Stage stages[kStages];
  std::deque<int> inflight; // submitted slots in stream order
  std::deque<bsg_chunk> ready;
  std::atomic<uint64_t> node_bytes[4] = {};  // bsg_stream_stats::copy_bytes_node
  Event span0;  // recorded before the first H2D of the stream
  Event tail0, tail1;  // the final tile's kernels: start, records out

  size_t stage_size() const { return std::min(tile, kStageMax); }

  int init(int device, const uint32_t* tab) {
    dev = device;
    std::memcpy(table, tab ? tab : kBuzhash32Seed1, sizeof table);
    for (Stage& st : stages) {
      st.buf.dma_only = true;
      HCHECK(st.ev.create(hipEventDisableTiming));
      HCHECK(st.t0.create());
      HCHECK(st.t1.create());
    }
    HCHECK(span0.create());
    HCHECK(tail0.create());
    HCHECK(tail1.create());
    return ensure_slot(0);  // the first tile's engine: errors surface at bsg_open
  }

  int ensure_slot(int i) {
    TileSlot& t = slots[i];
    if (t.eng) return BSG_OK;
    int err = BSG_OK;
    t.eng = bsg_engine_create(dev, table, &err);
    if (!t.eng) return err;
    t.eng->snapshot = true;
    HCHECK(t.h2d_ev.create(hipEventDisableTiming));
    HCHECK(t.done_ev.create(hipEventDisableTiming));
    HCHECK(t.copied_ev.create(hipEventDisableTiming));
    return BSG_OK;
  }

  // data[dcur] ready to receive the current tile's bytes on the copy stream: allocated, and
  // ordered after the kernels of the tile that used it last.
  int copy_prepare() {
    if (!cstream) HCHECK(stream_acquire(dev, &cstream));
    DataSlot& ds = data[dcur];
    HCHECK(ds.dbuf.ensure(carry_cap + tile + kReadSlack));
    HCHECK(ds.free_ev.create(hipEventDisableTiming));
    if (!dready) {
      if (ds.free_pending) HCHECK(hipStreamWaitEvent(cstream, ds.free_ev, 0));
      ds.free_pending = false;
      dready = true;
    }
    return BSG_OK;
  }

  // Everything in flight ends, the engines go, the copy stream and the full-size stages return
  // to their pools; the members then free what is left (after every synchronisation here).
  ~bsg_ctx() {
    (void)hipSetDevice(dev);
    if (cstream) (void)hipStreamSynchronize(cstream);
    for (TileSlot& t : slots) {
      if (t.eng) (void)hipStreamSynchronize(t.eng->stream);
      bsg_engine_destroy(t.eng);
    }
    if (cstream) stream_release(dev, cstream);
    for (Stage& st : stages) {
      if (st.ev) (void)hipEventSynchronize(st.ev);
      StagePool::get().give(&st.buf);
    }
  }

  // the finished H2D of stage st into the busy time
  void harvest(Stage& st) {
    if (!st.timed) return;
    uint64_t ns = 0;
    if (elapsed_ns(st.t0, st.t1, &ns)) stats.h2d_busy_ns += ns;
    st.timed = false;
  }

  int get_stats(bsg_stream_stats* out) {
    if (cstream) HCHECK(hipStreamSynchronize(cstream));
    for (Stage& st : stages) harvest(st);
    bsg_stream_stats s = stats;
    if (span_set && slast >= 0) elapsed_ns(span0, stages[slast].t1, &s.h2d_span_ns);
    if (tail_set) {
      if (hipEventSynchronize(tail1) == hipSuccess)
        elapsed_ns(tail0, tail1, &s.last_tile_ns);
      else
        (void)hipGetLastError();
      if (slast >= 0) elapsed_ns(stages[slast].t1, tail1, &s.tail_ns);
    }
    for (int k = 0; k < 4; ++k) s.copy_bytes_node[k] = node_bytes[k].load();
    s.gpu_node = device_node(dev);
    for (const Stage& st : stages) {
      if (!st.buf.p) continue;
      for (size_t at : {(size_t)0, st.buf.cap / 2}) {
        const int nd = page_node(st.buf.as<uint8_t>() + at);
        if (nd >= 0 && nd < 32) s.stage_nodes |= 1u << nd;
      }
    }
    s.copy_nt = bsg::copy_nt_enabled() ? 1u : 0u;
    *out = s;
    return BSG_OK;
  }

  // Selection of slot i is done: learn its chunk count and where its open chunk starts. A
  // candidate-buffer overflow (degenerate input) is re-run synchronously at exact capacity.
  int read_sel(int i) {
    TileSlot& t = slots[i];
    if (t.sel_read) return BSG_OK;
    HCHECK(hipEventSynchronize(t.eng->sel_ev));
    Counters c = *t.eng->h_snap.as<Counters>();
    uint64_t last_end =
        *reinterpret_cast<const uint64_t*>(t.eng->h_snap.as<uint8_t>() + sizeof(Counters));
    if (c.overflow || c.error) {
      uint64_t n = 0;
      int rc = t.eng->finish(&n);  // synchronous; re-runs after an overflow
      if (rc) return rc;
      c = t.eng->last;
      HCHECK(hipMemcpy(&last_end, t.eng->last_end.p, 8, hipMemcpyDeviceToHost));
    }
    t.nchunks = c.nchunks;
    t.open_next = last_end;
    t.sel_read = true;
    return BSG_OK;
  }

  // Enqueue the D2H of slot i's records behind its k_sha.
  int enqueue_recs(int i) {
    TileSlot& t = slots[i];
    if (t.recs_enq) return BSG_OK;
    int rc = read_sel(i);
    if (rc) return rc;
    // by kernel behind k_sha: a hipMemcpyAsync D2H queued here would wait for k_sha inside the
    // shared copy-engine queue and hold up the next tiles' H2D copies behind it
    HCHECK(t.recs.ensure(sizeof(bsg_chunk) * (t.nchunks ? t.nchunks : 1)));
    void* rd = t.recs.dev();
    void* cd = t.eng->h_ctr.dev();
    if (!rd || !cd) return BSG_EDEVICE;
    if (t.nchunks)
      HCHECK(launch_copy_out(t.eng->out.p, rd, sizeof(bsg_chunk) * t.nchunks, t.eng->stream));
    HCHECK(launch_copy_out(t.eng->ctr.p, cd, sizeof(Counters), t.eng->stream));
    HCHECK(hipEventRecord(t.done_ev, t.eng->stream));
    if (t.final_seg) {
      HCHECK(hipEventRecord(tail1, t.eng->stream));
      tail_set = true;
    }
    t.recs_enq = true;
    return BSG_OK;
  }

  // Wait for the oldest in-flight tile (if `wait`) and move its records to `ready`.
  int collect_front(bool wait, bool* got) {
    *got = false;
    if (inflight.empty()) return BSG_OK;
    const int i = inflight.front();
    TileSlot& t = slots[i];
    if (!t.recs_enq) {
      if (!wait) return BSG_OK;
      int rc = enqueue_recs(i);
      if (rc) return rc;
    }
    if (!wait) {
      hipError_t q = hipEventQuery(t.done_ev);
      if (q == hipErrorNotReady) {
        (void)hipGetLastError();
        return BSG_OK;
      }
      HCHECK(q);
    }
    HCHECK(hipEventSynchronize(t.done_ev));
    const Counters& c = *t.eng->h_ctr.as<Counters>();
    if (c.error) return device_error(c.error);
    const bsg_chunk* r = t.recs.as<bsg_chunk>();
    for (uint64_t k = 0; k < t.nchunks; ++k) ready.push_back(r[k]);
    t.busy = false;
    t.eng->enqueued = false;
    inflight.pop_front();
    *got = true;
    return BSG_OK;
  }

  int poll() {
    bool got = true;
    while (got) {
      int rc = collect_front(false, &got);
      if (rc) return rc;
    }
    return BSG_OK;
  }

  // Make slots[i] free for a new tile: its previous tile's records are collected.
  int reclaim(int i) {
    while (slots[i].busy) {
      bool got = false;
      int rc = collect_front(true, &got);
      if (rc) return rc;
    }
    return BSG_OK;
  }

  // Copy the staged bytes of the current tile to its data slot (on the copy stream) and move to
  // the next stage.
  int flush_stage() {
    if (sfill == 0) return BSG_OK;
    int rc = copy_prepare();
    if (rc) return rc;
    Stage& st = stages[scur];
    tail_append(st.buf.as<uint8_t>(), sfill);  // history for the next tile
    if (!span_set) {
      HCHECK(hipEventRecord(span0, cstream));
      span_set = true;
    }
    HCHECK(hipEventRecord(st.t0, cstream));
    HCHECK(hipMemcpyAsync(data[dcur].dbuf.as<uint8_t>() + carry_cap + (fill - sfill), st.buf.p,
                          sfill, hipMemcpyHostToDevice, cstream));
    HCHECK(hipEventRecord(st.t1, cstream));
    HCHECK(hipEventRecord(st.ev, cstream));
    st.inflight = true;
    st.timed = true;
    sent = true;
    stats.h2d_bytes += sfill;
    stats.h2d_copies++;
    slast = scur;
    scur = (scur + 1) % kStages;
    sfill = 0;
    return BSG_OK;
  }

  // stages[scur] ready to take bytes: its previous H2D has run, and it can hold `need` bytes.
  // A stream's first stage grows (doubling from 4 MiB) so a small stream pins a few MiB; once
  // the stream has passed a stage's worth of bytes, stages are allocated whole.
  static constexpr size_t kMinStaging = 4ull << 20;
  int stage_ready(size_t need) {
    Stage& st = stages[scur];
    if (st.inflight) {
      const auto t0 = std::chrono::steady_clock::now();
      HCHECK(hipEventSynchronize(st.ev));
      stats.stage_wait_ns += ns_since(t0);
      st.inflight = false;
      harvest(st);
    }
    const size_t full = stage_size();
    const bool big = pos - stream0 + fill >= full;  // past a stage's worth: whole stages
    const size_t want = big ? full : std::min(full, std::max(need, kMinStaging));
    const size_t have = std::min(st.buf.cap, full);
    if (have >= want) return BSG_OK;
    const size_t nc = big ? full : std::min(full, std::max(want, 2 * have));
    PinBuf pooled;
    // a full-size stage already pinned in the pool beats pinning a new one of any size
    if (full == kStageMax && StagePool::get().take(&pooled)) {
      if (sfill) std::memcpy(pooled.p, st.buf.p, sfill);
      st.buf = std::move(pooled);
      return BSG_OK;
    }
    HCHECK(st.buf.grow(nc, sfill));
    return BSG_OK;
  }
  size_t stage_room() const {
    return std::min(stages[scur].buf.cap, stage_size()) - sfill;
  }
  // The stream's first kFirstFlush staged bytes go to the device at once instead of when the
  // first stage is full, so the H2D pipeline starts a 32 MiB Write earlier (with a full 64 MiB
  // first stage the copy stream idled until the second Write was copied). Later stages flush
  // full, as before; not the tile's last bytes (a final segment keeps them, see write()).
  static constexpr size_t kFirstFlush = 8ull << 20;
  int first_flush() {
    if (sent || sfill < kFirstFlush || fill >= tile) return BSG_OK;
    return flush_stage();
  }

  int submit(bool final_seg) {
    int rc0 = flush_stage();  // every byte of the tile is on its way to the device slot
    if (rc0) return rc0;
    const int i = cur;
    if ((rc0 = ensure_slot(i))) return rc0;
    TileSlot& t = slots[i];
    bsg_engine* e = t.eng;
    // Two invariants keep a tile's buffers safe. reclaim(i) protects the ENGINE's work buffers:
    // the records of the tile kSlots back on this engine are collected before its buffers are
    // reused. The DATA slot is protected by copy_prepare() and its free_ev: the H2D copies run
    // on the context's copy stream (cstream), which waits for the event recorded after the last
    // kernels (and the carry copy) that read the slot, before refilling it.
    rc0 = reclaim(i);
    if (rc0) return rc0;
    if ((rc0 = copy_prepare())) return rc0;
    // the tile's kernels (and the carry copy into its data slot) run after its H2D copies
    HCHECK(hipEventRecord(t.copied_ev, cstream));
    HCHECK(hipStreamWaitEvent(e->stream, t.copied_ev, 0));
    if (final_seg) HCHECK(hipEventRecord(tail0, e->stream));
    uint8_t* base = data[dcur].dbuf.as<uint8_t>();
    StreamDesc d{};
    d.data_off = carry_cap;
    d.len = fill;
    d.seg_base = pos;
    d.open_start = stream0;  // the first tile; later tiles take the previous tile's open chunk
    d.finalize = final_seg ? 1u : 0u;
    d.carry_cap = final_seg ? 0u : (uint32_t)std::min<uint64_t>(carry_cap, 0xffffffffu);
    std::memcpy(d.hist, hist, 64);
    std::memcpy(d.mid, kIV, sizeof kIV);
    if (prev >= 0) {
      TileSlot& pt = slots[prev];
      int rc = read_sel(prev);
      if (rc) return rc;
      const uint64_t open = pt.open_next;
      const uint64_t carry = pos - open;
      d.open_start = open;
      if (carry <= pt.eng->descs[0].carry_cap) {  // bytes carried on the device
        if (carry) {
          // the open chunk may itself have started in front of pt's tile (carried into it)
          const uint8_t* src = data[pt.dslot].dbuf.as<uint8_t>() + (int64_t)carry_cap +
                               ((int64_t)open - (int64_t)pt.seg_base);
          HCHECK(hipMemcpyAsync(base + carry_cap - carry, src, carry, hipMemcpyDeviceToDevice,
                                e->stream));
          // the previous slot must not be overwritten before this copy has read it
          HCHECK(hipEventRecord(t.h2d_ev, e->stream));
          HCHECK(hipStreamWaitEvent(pt.eng->stream, t.h2d_ev, 0));
          d.flags = kDescOpenInDevice;
        }
      } else {  // midstate carry: wait for the previous tile's k_sha
        rc = enqueue_recs(prev);
        if (rc) return rc;
        HCHECK(hipEventSynchronize(pt.done_ev));
        CarryOut co;
        HCHECK(hipMemcpy(&co, pt.eng->carry.p, sizeof co, hipMemcpyDeviceToHost));
        if (!co.valid || co.open_start != open) return BSG_EDEVICE;
        d.consumed = co.consumed;
        d.prefix_len = co.prefix_len;
        std::memcpy(d.mid, co.mid, sizeof co.mid);
      }
      // the previous tile's records can be fetched as soon as its k_sha is done
      rc = enqueue_recs(prev);
      if (rc) return rc;
      // the previous tile's data slot is free once its kernels (and the carry copy above, which
      // its stream now waits for) are done: the copy stream waits for this before refilling it
      DataSlot& pd = data[pt.dslot];
      HCHECK(hipEventRecord(pd.free_ev, pt.eng->stream));
      pd.free_pending = true;
    }
    e->d_data = base;
    e->descs.assign(1, d);
    e->nstreams = 1;
    e->p = p;
    int rc = e->enqueue();
    if (rc) return rc;
    t.busy = true;
    t.sel_read = false;
    t.recs_enq = false;
    t.final_seg = final_seg;
    t.seg_base = pos;
    t.len = fill;
    t.dslot = dcur;
    dcur = (dcur + 1) % ndata;
    dready = false;
    inflight.push_back(i);
    std::memcpy(hist, tail, 64);  // window history for the next tile
    pos += fill;
    fill = 0;
    prev = i;
    cur = (cur + 1) % nslots;
    if (final_seg) return enqueue_recs(i);
    return BSG_OK;
  }

  // Host side of Write: bytes into the staging ring (large pieces on several threads), each full
  // stage on its way to the device at once, full tiles submitted as more data arrives. A stream
  // has no length limit (split.Writer.Write has none, split/split.go:99-101): stream offsets are
  // u64 everywhere; only candidate positions inside one tile travel in 40-bit fields.
  int write(const uint8_t* p, size_t n) {
    if (n >= (1u << 20)) {
      const int nd = page_node(p);
      if (nd >= 0 && nd < 32) stats.src_nodes |= 1u << nd;
    }
    while (n) {
      if (fill == tile) {  // full tile and more data coming: submit it (never the last one)
        int rc = submit(false);
        if (rc) return rc;
      }
      int rc = stage_ready(sfill + std::min(n, tile - fill));
      if (rc) return rc;
      const size_t k = std::min({n, tile - fill, stage_room()});
      const auto t0 = std::chrono::steady_clock::now();
      par_copy(stages[scur].buf.as<uint8_t>() + sfill, p, k);
      stats.host_copy_ns += ns_since(t0);
      stats.host_bytes += k;
      sfill += k;
      fill += k;
      p += k;
      n -= k;
      // a full stage goes to the device now, except the tile's last one: if the stream ends
      // here, it is submitted as the final segment
      if (stage_room() == 0 && fill < tile && (rc = flush_stage())) return rc;
    }
    if (int rc = first_flush()) return rc;
    return poll();
  }

  // Appends bytes that already went to the device (or are on their way) to the running tail.
  void tail_append(const uint8_t* q, size_t k) {
    if (k >= 64) {
      std::memcpy(tail, q + k - 64, 64);
    } else {
      std::memmove(tail, tail + k, 64 - k);
      std::memcpy(tail + 64 - k, q, k);
    }
  }

  // write() from host memory the caller registered (bsg_host_register): no staging copy, the
  // H2D reads the caller's bytes directly, on the engine stream of the tile they belong to. The
  // last bytes (up to 4 KiB) of a segment that completes a tile are staged instead, so that a
  // full tile always keeps unflushed bytes that window() can hold back for the next tile (a
  // final segment needs at least one byte).
  int write_pinned(const uint8_t* q, size_t n) {
    while (n) {
      if (fill == tile) {
        int rc = submit(false);
        if (rc) return rc;
      }
      int rc = flush_stage();  // staged bytes of this tile go first (offsets stay in order)
      if (rc) return rc;
      if ((rc = copy_prepare())) return rc;
      const size_t k = std::min(n, tile - fill);
      const size_t staged = fill + k == tile ? std::min<size_t>(k, 4096) : 0;
      const size_t direct = k - staged;
      if (direct) {
        HCHECK(hipMemcpyAsync(data[dcur].dbuf.as<uint8_t>() + carry_cap + fill, q, direct,
                              hipMemcpyHostToDevice, cstream));
        tail_append(q, direct);
        fill += direct;
      }
      if (staged) {
        if ((rc = stage_ready(staged))) return rc;
        std::memcpy(stages[scur].buf.as<uint8_t>(), q + direct, staged);
        sfill = staged;
        fill += staged;
      }
      q += k;
      n -= k;
    }
    return poll();
  }

  // Zero-copy form of write(): the caller fills pinned staging directly (an io.Reader reads
  // into it), then commits. The window is the rest of the current stage (within the tile).
  int window(uint8_t** p, size_t* cap) {
    if (fill == tile) {
      // The caller may be at EOF, so this tile cannot be the last one submitted as non-final:
      // hold its last bytes (still in the current stage) back for the next tile. (A final
      // segment must hold at least one byte: the flush of the open chunk is emitted by the scan
      // of the final segment's last strip, and an empty segment has none.)
      constexpr size_t kHold = 4096;
      uint8_t held[kHold];
      const size_t hold = std::min({kHold, tile / 2, sfill});
      std::memcpy(held, stages[scur].buf.as<uint8_t>() + sfill - hold, hold);
      sfill -= hold;
      fill -= hold;
      int rc = submit(false);
      if (rc) return rc;
      if ((rc = stage_ready(hold))) return rc;
      std::memcpy(stages[scur].buf.p, held, hold);
      sfill = fill = hold;
    }
    // the window is the stage's free part (within the tile); a full stage grows or is flushed
    int rc = stage_ready(sfill + 1);
    if (rc) return rc;
    if (stage_room() == 0) {  // a full stage below the tile's end: move on to the next one
      if ((rc = flush_stage()) || (rc = stage_ready(1))) return rc;
    }
    *p = stages[scur].buf.as<uint8_t>() + sfill;
    *cap = std::min(stage_room(), tile - fill);
    return BSG_OK;
  }
  int commit(size_t n) {
    if (n > std::min(stage_room(), tile - fill)) return BSG_EINVAL;
    sfill += n;
    fill += n;
    if (stage_room() == 0 && fill < tile) {
      int rc = flush_stage();
      if (rc) return rc;
    }
    if (int rc = first_flush()) return rc;
    return poll();
  }

  // Bytes into pinned staging on the copy pool; the bytes each thread copied are counted by the
  // NUMA node it ran on (bsg_stream_stats)
  void par_copy(uint8_t* dst, const uint8_t* src, size_t n) {
    constexpr size_t kPiece = 2ull << 20;  // per thread, at least
    const bool nt_ok = bsg::copy_nt_enabled() && n >= kPiece;
    auto one = [this, nt_ok](uint8_t* d, const uint8_t* s, size_t m) {
      if (nt_ok)
        bsg::copy_nt(d, s, m);
      else
        std::memcpy(d, s, m);
      const int nd = bsg::cpu_node();
      if (nd >= 0 && nd < 4) node_bytes[nd].fetch_add(m, std::memory_order_relaxed);
    };
    const size_t nt = std::min<size_t>((size_t)copy_threads(), n / kPiece);
    if (nt <= 1) {
      one(dst, src, n);
      return;
    }
    // 1 MiB slices taken dynamically, so a thread that wakes late or runs slow takes fewer
    // (one slice per thread left the others waiting for it)
    const size_t ns = (n + kCopySlice - 1) / kCopySlice;
    parallel_for(ns, [=](size_t k) {
      const size_t o = k * kCopySlice;
      one(dst + o, src + o, std::min(kCopySlice, n - o));
    });
  }

  // Start a new stream on the same buffers (bsg_reset): everything in flight is waited for and
  // discarded, also after a device error (Counters::error is per run: the buffers stay valid).
  // Only a failing HIP call (a real fault) leaves the context unusable: bsg_free it.
  int reset() {
    if (cstream) HCHECK(hipStreamSynchronize(cstream));
    for (DataSlot& ds : data) ds.free_pending = false;
    for (int k = 0; k < nslots; ++k) {
      TileSlot& t = slots[k];
      if (t.eng) HCHECK(hipStreamSynchronize(t.eng->stream));
      t.busy = false;
      t.sel_read = t.recs_enq = false;
      if (t.eng) t.eng->enqueued = false;
    }
    // Full-size stages go back to the process-wide pool, last stage first: the pool is a stack
    // and the next stream takes stage 0's buffer first, so every stream of the context gets the
    // same buffer in the same stage. In the given order, the buffers came back reversed at every
    // reset, and every other 1 GiB rep ran ~3.5 ms (12 %) longer (profiles/r05_bench_final.log,
    // end_to_end.reps_ms: 28.1 / 32.3 / 28.4 ms).
    for (int k = kStages - 1; k >= 0; --k) {
      Stage& st = stages[k];
      if (st.inflight) HCHECK(hipEventSynchronize(st.ev));
      st.inflight = false;
      st.timed = false;
      StagePool::get().give(&st.buf);
    }
    for (auto& b : node_bytes) b.store(0);
    inflight.clear();
    ready.clear();
    static_cast<StreamState&>(*this) = StreamState{};
    return BSG_OK;
  }

  int close_begin() {
    if (fill == 0 && pos == stream0) return BSG_OK;  // empty stream: no chunks
    // The final segment must hold at least one byte: the open chunk's flush is emitted by the
    // scan of its last strip. write() and window() never submit a tile without leaving bytes
    // behind, so this cannot happen; fail loudly rather than drop the last chunk.
    if (fill == 0) return BSG_ESTATE;
    return submit(true);
  }
  int close_step(size_t* left) {  // the oldest tile on the device: wait, collect its records
    bool got = false;
    int rc = collect_front(true, &got);
    *left = inflight.size();
    return rc;
  }
  int close() {
    int rc = close_begin();
    for (size_t left = inflight.size(); rc == BSG_OK && left;) rc = close_step(&left);
    return rc;
  }
};
