// host_engine.h — the run pipeline: one run's plan, buffers and launch sequence (bsg_engine),
// what its passes see of it (RunView) and the second engine they hash blobs through.
#pragma once

namespace {

int normalize(const bsg_params* in, Params* out, bsg_params* norm) {
  bsg_params p = in ? *in : bsg_params_default();
  // Every value split.Bits / split.MinSize accept (split/split.go:137-152 store them unchecked)
  // is valid: 0 takes hashsplit's default (SplitBits 13, MinSize 64 = the window); MinSize 1..63
  // lets a window span a boundary (the hash still depends only on the last 64 stream bytes, so
  // nothing changes but the greedy rule); Bits > 32 can never be met by TrailingZeros32 (<= 32),
  // so the stream is one final chunk. fanout 0 is our C default (Fanout(0) in Go would divide by
  // zero in split.go:86).
  if (p.split_bits == 0) p.split_bits = 13;  // hashsplit defaultSplitBits
  if (p.min_size == 0) p.min_size = 64;      // hashsplit defaultMinSize (window size)
  if (p.fanout == 0) p.fanout = 8;
  out->split_bits = p.split_bits;
  out->min_size = p.min_size;
  out->mask = p.split_bits >= 32 ? 0xffffffffu : ((1u << p.split_bits) - 1u);
  out->pad_ = 0;
  if (norm) *norm = p;
  return BSG_OK;
}

// The sizes of one run, computed once per enqueue (bsg_engine::plan_split / plan_hash) from the
// run's descriptors and parameters: every buffer reservation and argument block reads them here.
struct RunPlan {
  uint32_t ns = 0;         // streams
  uint64_t strips = 0;     // kStrip-byte strips of all streams
  uint64_t total_len = 0;  // bytes of all streams
  uint64_t data_span = 1;  // bytes from d_data to the end of the last stream (k_sha regions)
  uint64_t cand_cap = 0;   // candidate capacity
  uint64_t chunk_cap = 0;  // record capacity
  uint32_t lists = 0;      // k_scan's refine lists
  uint64_t list_cap = 0;   // entries per list
  uint64_t jobs = 0;       // k_sha's job bound: chunk_cap + ns
  bool scan = false;       // scan and selection stages (a split run; a hash run has neither)
  bool early = false;      // early chains on a second stream
  bool light = false;      // ... in the lightly loaded arrangement (bsg_engine, "Round 5")
  bool tail = false;       // host tail (bsg_engine, "Host tail"); then no early chains
};

// Counters::error after a run
int device_error(uint64_t code) {
  std::fprintf(stderr, "bsgpu: device sanity check failed (code %llu)\n", (unsigned long long)code);
  return BSG_EDEVICE;
}

// bytes from d_data to the end of the last stream
uint64_t data_span(const std::vector<StreamDesc>& descs) {
  uint64_t hi = 0;
  for (const StreamDesc& d : descs) hi = std::max<uint64_t>(hi, d.data_off + d.len);
  return hi;
}

// What a pass over a finished run (trees, dedup and pack, restore, walk, gc, read) takes from its engine: where
// it works, the run's inputs and results; `owner` only to hand on to need_hasher / hash_batches.
struct RunView {
  bsg_engine* owner;
  hipStream_t stream;
  int num_cus, profile;
  bool run_done;   // the last enqueue was a bsg_engine_run that finish() completed
  bool usable;     // ... on an engine that is neither a snapshot nor a hash engine
  bool in_flight;  // a run is enqueued and not finished
  const uint8_t* d_data;
  const std::vector<StreamDesc>* descs;  // host side, and on the device:
  StreamDesc* streams;
  uint32_t ns;
  ChunkRec* rec;
  uint64_t nrec, *scount;
  uint32_t fanout;
};

// The second engine of `owner` (hash mode, on its stream), made at first use; and n device blobs
// (data .. + span) hashed through it in batches of kTreeHashBatch: descs(first, count, d) launches
// what writes a batch's descriptors into d, consume(first, count, records, counters) what reads
// its refs. (Both defined below bsg_engine.)
int need_hasher(bsg_engine* owner);
template <class Descs, class Consume>
int hash_batches(bsg_engine* owner, DevBuf& dbuf, uint64_t n, const uint8_t* data, uint64_t span,
                 int sha_mode, Descs descs, Consume consume);

}  // namespace

#include "host_tree.h"
#include "host_dedup.h"
#include "host_restore.h"
#include "host_walk.h"
#include "host_gc.h"
#include "host_read.h"
#include "host_blobpool.h"
#include "host_blobs.h"

struct bsg_engine {
  int dev = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  DevBuf table, streams, strip0, counts, refine, slots, strip_off, partials_a, partials_b, cand, flags,
      fidx, bnd_end, bnd_info, scount, last_end, out, carry, ctr, long_list, order, buckets, jinfo, jdesc,
      regions, oreg, rorder;
  PinBuf h_streams, h_strip0, h_ctr;
  uint32_t htable[256];  // the table in `table` (a pooled batch engine may get another one)
  // Optional snapshot right after selection (streaming pipeline): the counters and every
  // stream's last chunk end land in pinned memory and sel_ev fires, long before k_sha ends.
  bool snapshot = false;
  PinBuf h_snap;  // Counters, then nstreams x u64 last_end
  Event sel_ev;
  // current run
  const uint8_t* d_data = nullptr;
  std::vector<StreamDesc> descs;
  Params p{};
  uint64_t retry_cap = 0;  // exact candidate capacity after an overflow (one re-run)
  uint32_t nstreams = 0;
  bool enqueued = false;
  bool hash_mode = false;  // bsg_engine_hash: every stream is one blob (enqueue_hash)
  int hash_long_mode = -1;  // >= 0: enqueue_hash's SHA path choice instead of the knob's
  Counters last{};
  // optional per-stage HIP events on the engine stream: [scan, compact..chunks, sha]
  int profile = 0;  // bsg_engine_profile mode
  Marks marks;
  float stage_ms[3] = {0, 0, 0};
  // Early chains (bsgpu_internal.h, Early): the two longest sure chunks hashed on a second
  // stream from right after k_compact. The Early record lives after the Counters in `ctr`, so
  // the run's one memset clears both.
  hipStream_t estream = nullptr;
  Event cand_ev, pick_ev, early_ev;
  bool early_open = false;  // chains launched whose end the engine stream does not wait for yet
  static constexpr uint64_t kEarlyMinBytes = 256ull << 20;  // smaller runs: not worth a stream
  uint64_t early_min = kEarlyMinBytes;  // bsg_init's warm-up run lowers it to load the kernels
  bool early_ok() const {
    return !snapshot && !hash_mode && knob(BSG_KNOB_EARLY) != 0;
  }

  // Host tail (bsgpu_internal.h, TailHdr): a lightly loaded run of at least tail_min bytes hands
  // its longest chunks to host threads. k_offload_pick (after k_lens) takes them out of k_sha's
  // queues, k_offload_gather copies their bytes into a pinned ring on the second stream while
  // k_sha runs, the workers hash each chunk as its flag rises, and finish() (or the next run)
  // copies the refs up and launches k_offload_fix. Such a run has no early chains: they start
  // before the lengths are known and would hold on to the very chunks the host should take, and
  // k_sha's helped solo tickets run what is then the GPU's longest chains at the same rate.
  // The ring, the lists and the workers are made at the engine's first such run and kept, so an
  // engine that never runs one holds neither pinned memory nor threads; that first run pays the
  // pinned allocation (tens of ms, host_mem.h) and the threads' creation. The workers belong to
  // the engine: at most 16 threads each, so several engines with tails at once have 16 each.
  // Runs under 512 MiB keep the early-chain path (256 MiB up) that the parity tests pin there.
  static constexpr uint64_t kTailMinBytes = 512ull << 20;
  static constexpr uint64_t kTailRingMax = 256ull << 20;
  // Cost model constants (k_offload_cut): the solo chain's time per block, profiles/BENCH_r06.json
  // sha_path.long.us_per_block; the gather's rate, the same file's end_to_end.h2d_busy_gbs (the
  // link's other direction, measured by the streaming leg).
  static constexpr float kTailUsPerBlock = 0.95f;
  static constexpr float kTailPcieBytesUs = 56e3f;
  uint64_t tail_min = kTailMinBytes;  // test tooling lowers it (bsg_engine_host_tail_debug)
  uint32_t tail_force_cut = 0;        // ... forces the cut (blocks; 0: the cost model)
  bool tail_portable = false;         // ... and the portable hash
  uint64_t tail_ring_force = 0;       // ... and the ring's size (0: by the run's size)
  std::unique_ptr<HashWorkers> workers;
  DevBuf tail_hdr, tail_list, tail_src, tail_refs;
  PinBuf h_tail, h_ring;  // meta, flags, list, refs | the ring
  Event tail_ev, gather_ev0, gather_ev1;
  bool tail_open = false;  // a run's tail is under way: its refs are not in the records yet
  TailArgs tail_args{};
  int64_t tail_t0_ns = 0;  // when the run was enqueued (steady clock)
  struct TailStat {
    uint64_t chunks = 0, bytes = 0, cut = 0, longest_all = 0, longest_left = 0, blocks = 0;
    float gather_ms = 0.f;
    int64_t host_done_us = 0;  // the last host hash's end after the run's enqueue
    int impl = 0, threads = 0;
    double host_rate = 0;      // one worker's measured bytes per second
  } tail_stat;
  bool tail_ok() const {
    return !snapshot && !hash_mode && knob(BSG_KNOB_HOST_TAIL) != 0;
  }

  uint32_t fanout = 8;        // the last bsg_engine_run's
  bool run_done = false;      // the last enqueue was a bsg_engine_run that finish() completed
  // The passes over a finished split run, each with its own buffers. Trees and restore hash
  // blobs through `hasher`, a second engine in hash mode on this engine's stream.
  bool borrowed_stream = false;  // `stream` belongs to the engine this one hashes for
  bsg_engine* hasher = nullptr;
  TreeWork tree;
  DedupWork dd;
  RestoreWork restore;
  WalkWork walk;
  GcWork gc;
  ReadWork read;
  MergeWork merge[2];  // bsg_pool_merge uses the first, bsg_pool_sync one per direction
  BlobWork blobs;
  RunView view() {
    return RunView{this, stream, num_cus, profile, run_done, run_done && !snapshot && !hash_mode,
                   enqueued, d_data, &descs, streams.as<StreamDesc>(), nstreams,
                   out.as<ChunkRec>(), last.nchunks, scount.as<uint64_t>(), fanout};
  }

  // Round 5: a lightly loaded run (at most BSG_KNOB_LIGHT_BYTES, default 4 GiB, where the
  // longest chunk's chain is the step: configs[1], [3], [4]) keeps its early chains on the
  // engine stream right after k_pick and moves selection and k_sha to the second stream, so the
  // chain pays no cross-stream wait (≈ 10-14 us between k_compact and k_pick,
  // profiles/r04_run_timelines_early.txt) and no dispatch gap; selection, which has slack there,
  // pays it instead. A loaded run (configs[2], where the hash work ends with the chain) keeps
  // selection on the engine stream. The knob lets the tests run one input both ways.

  // profile 1: every stage boundary; 2: the SHA-256 stage's two only (on the stream it runs on)
  void mark(int i, hipStream_t on = nullptr) {
    if (profile == 1 || (profile && i >= 2)) marks.record(i, on ? on : stream);
  }

  int setdev() { return herr(hipSetDevice(dev)); }

  RunPlan plan_split() {
    RunPlan pl;
    pl.scan = true;
    pl.ns = nstreams;
    pl.data_span = std::max<uint64_t>(1, data_span(descs));
    uint64_t chunk_bound = 0;
    for (uint32_t s = 0; s < pl.ns; ++s) {
      descs[s].strip0 = pl.strips;
      pl.strips += (descs[s].len + kStrip - 1) / kStrip;
      pl.total_len += descs[s].len;
      chunk_bound += (descs[s].len + (descs[s].seg_base - descs[s].open_start)) / p.min_size + 2;
    }
    {
      // random input yields ~len/2^bits candidates; degenerate input (e.g. all zeros: one per
      // byte) overflows this estimate and is re-run once at its exact size by finish().
      const uint32_t b = std::min<uint32_t>(p.split_bits, 16);
      pl.cand_cap = std::max<uint64_t>(1u << 16, ((pl.total_len >> b) << 2) + 2ull * pl.ns + 1024);
      if (retry_cap > pl.cand_cap) pl.cand_cap = retry_cap;
    }
    // Every chunk ends at a candidate (the forced final one included), and a run whose
    // candidates overflow cand_cap selects nothing, so cand_cap also bounds the chunk count; it
    // is the tighter bound for small MinSize (len / MinSize records would be ~len for MinSize 1).
    pl.chunk_cap = std::min(chunk_bound, pl.cand_cap);
    // the refine lists: one per k_scan workgroup, scan_list_cap entries each
    pl.lists = pl.strips ? scan_lists(pl.strips, num_cus) : 0;
    pl.list_cap = scan_list_cap(pl.strips, pl.lists);
    pl.jobs = pl.chunk_cap + pl.ns;
    // the host tail: lightly loaded runs only (a loaded run's step is its hash work, which the
    // GPU does faster, not one chain)
    pl.tail = tail_ok() && pl.total_len >= tail_min && pl.strips &&
              pl.total_len <= (uint64_t)knob(BSG_KNOB_LIGHT_BYTES).load();
    pl.early = !pl.tail && early_ok() && pl.total_len >= early_min && pl.strips;
    pl.light = pl.early && pl.total_len <= (uint64_t)knob(BSG_KNOB_LIGHT_BYTES).load();
    return pl;
  }

  // bsg_engine_hash: one final chunk per stream, no candidates
  RunPlan plan_hash() {
    RunPlan pl;
    pl.ns = nstreams;
    pl.data_span = std::max<uint64_t>(1, data_span(descs));
    pl.chunk_cap = pl.ns;
    pl.jobs = pl.chunk_cap + pl.ns;
    return pl;
  }

  // The Early record lives after the Counters in `ctr`, so k_start clears both at once; a hash
  // run has no early chains and keeps (and clears) the Counters alone.
  static size_t ctr_bytes(const RunPlan& pl) {
    return sizeof(Counters) + (pl.scan ? sizeof(Early) : 0);
  }

  // Every work buffer at the size the plan needs (a buffer only ever grows).
  int reserve(const RunPlan& pl) {
    const uint64_t nn = pl.ns ? pl.ns : 1;
    // a hash run sizes its records and jobs for one blob at least (an empty batch)
    const uint64_t recs = pl.scan ? pl.chunk_cap : nn;
    const uint64_t jobs = pl.scan ? pl.jobs : 2 * nn;
    if (pl.scan) {
      const uint64_t st = pl.strips ? pl.strips : 1;
      HCHECK(strip0.ensure(sizeof(uint64_t) * (pl.ns + 1)));
      HCHECK(counts.ensure(sizeof(uint32_t) * st));
      // the refine lists, then their lengths (u32 per list)
      HCHECK(refine.ensure(sizeof(uint64_t) * (pl.lists * pl.list_cap + 1) +
                           sizeof(uint32_t) * (pl.lists + 1)));
      HCHECK(slots.ensure(sizeof(uint32_t) * kSlotCap * st));
      HCHECK(strip_off.ensure(sizeof(uint64_t) * st));
      HCHECK(partials_a.ensure(sizeof(uint64_t) * prefix_partials_needed(pl.strips)));
      HCHECK(partials_b.ensure(sizeof(uint64_t) * prefix_partials_needed(pl.cand_cap)));
      HCHECK(cand.ensure(sizeof(uint64_t) * pl.cand_cap));
      HCHECK(flags.ensure(sizeof(uint32_t) * pl.cand_cap));
      HCHECK(fidx.ensure(sizeof(uint64_t) * pl.cand_cap));
      HCHECK(h_strip0.ensure(sizeof(uint64_t) * (pl.ns + 1)));
    }
    HCHECK(streams.ensure(sizeof(StreamDesc) * nn));
    HCHECK(bnd_end.ensure(sizeof(uint64_t) * recs));
    HCHECK(bnd_info.ensure(sizeof(uint64_t) * recs));
    HCHECK(out.ensure(sizeof(ChunkRec) * recs));
    HCHECK(scount.ensure(sizeof(uint64_t) * nn));
    HCHECK(last_end.ensure(sizeof(uint64_t) * nn));
    HCHECK(carry.ensure(sizeof(CarryOut) * nn));
    HCHECK(ctr.ensure(ctr_bytes(pl)));
    HCHECK(long_list.ensure(sizeof(uint64_t) * jobs));
    HCHECK(order.ensure(sizeof(uint64_t) * jobs));
    HCHECK(jinfo.ensure(sizeof(uint32_t) * jobs));
    HCHECK(jdesc.ensure(sizeof(LaneJob) * jobs));
    HCHECK(regions.ensure(sizeof(Regions)));
    HCHECK(oreg.ensure(jobs));
    HCHECK(rorder.ensure(sizeof(uint64_t) * jobs));
    HCHECK(buckets.ensure(sizeof(uint32_t) * 4 * kLptBuckets));
    HCHECK(h_streams.ensure(sizeof(StreamDesc) * nn));
    HCHECK(h_ctr.ensure(sizeof(Counters)));
    return BSG_OK;
  }

  Counters* dctr() const { return ctr.as<Counters>(); }
  Early* dearly() const { return reinterpret_cast<Early*>(ctr.as<uint8_t>() + sizeof(Counters)); }

  // k_start reads the descriptors (and a split run's first strips) from pinned host memory
  StartArgs start_args(const RunPlan& pl) const {
    StartArgs a{};
    a.src = static_cast<const StreamDesc*>(h_streams.dev());
    a.streams = streams.as<StreamDesc>();
    a.nstreams = pl.ns;
    a.last_end = last_end.as<uint64_t>();
    a.scount = scount.as<uint64_t>();
    a.carry = carry.as<CarryOut>();
    a.zero0 = ctr.as<uint32_t>();
    a.nzero0 = (uint32_t)(ctr_bytes(pl) / 4);
    a.zero1 = buckets.as<uint32_t>();
    a.nzero1 = 2 * kLptBuckets;
    if (pl.scan) {
      a.src_strip0 = static_cast<const uint64_t*>(h_strip0.dev());
      a.strip0 = strip0.as<uint64_t>();
      a.zero2 = partials_a.as<uint32_t>();
      a.nzero2 = (uint32_t)(2 * prefix_partials_needed(pl.strips));
      a.zero3 = partials_b.as<uint32_t>();
      a.nzero3 = (uint32_t)(2 * prefix_partials_needed(pl.cand_cap));
    }
    return a;
  }

  ScanArgs scan_args(const RunPlan& pl) const {
    ScanArgs a{};
    a.data = d_data;
    a.streams = streams.as<StreamDesc>();
    a.strip0 = strip0.as<uint64_t>();
    a.nstreams = pl.ns;
    a.nstrips = pl.strips;
    a.table = table.as<uint32_t>();
    a.p = p;
    a.counts = counts.as<uint32_t>();
    a.refine = refine.as<uint64_t>();
    a.slots = slots.as<uint32_t>();
    a.cand_off = strip_off.as<uint64_t>();
    a.cand = cand.as<uint64_t>();
    a.cand_cap = pl.cand_cap;
    a.ctr = dctr();
    a.lists = pl.lists;
    a.list_cap = pl.list_cap;
    a.list_cnt = reinterpret_cast<uint32_t*>(refine.as<uint64_t>() + pl.lists * pl.list_cap + 1);
    return a;
  }

  // a hash run has no candidates: k_blob_jobs writes one final chunk per stream
  ChunkArgs chunk_args(const RunPlan& pl) const {
    ChunkArgs a{};
    if (pl.scan) {
      a.cand = cand.as<uint64_t>();
      a.flags = flags.as<uint32_t>();
      a.fidx = fidx.as<uint64_t>();
    }
    a.bnd_end = bnd_end.as<uint64_t>();
    a.bnd_info = bnd_info.as<uint64_t>();
    a.scount = scount.as<uint64_t>();
    a.last_end = last_end.as<uint64_t>();
    a.chunk_cap = pl.chunk_cap;
    a.p = p;
    a.ctr = dctr();
    a.streams = streams.as<StreamDesc>();
    return a;
  }

  // k_lens .. k_sha and the early chains; `early`: this run's Early record, or nullptr
  ShaArgs sha_args(const RunPlan& pl, int long_mode, Early* early) const {
    ShaArgs a{};
    a.data = d_data;
    a.streams = streams.as<StreamDesc>();
    a.nstreams = pl.ns;
    a.bnd_end = bnd_end.as<uint64_t>();
    a.bnd_info = bnd_info.as<uint64_t>();
    a.last_end = last_end.as<uint64_t>();
    a.ctr = dctr();
    a.out = out.as<ChunkRec>();
    a.carry = carry.as<CarryOut>();
    a.chunk_cap = pl.chunk_cap;
    a.long_list = long_list.as<uint64_t>();
    a.order = order.as<uint64_t>();
    a.bucket_cnt = buckets.as<uint32_t>();
    a.bucket_elig = buckets.as<uint32_t>() + kLptBuckets;
    a.bucket_off = buckets.as<uint32_t>() + 2 * kLptBuckets;
    a.bucket_loff = buckets.as<uint32_t>() + 3 * kLptBuckets;
    a.jinfo = jinfo.as<uint32_t>();
    a.jdesc = jdesc.as<LaneJob>();
    a.reg = regions.as<Regions>();
    a.oreg = oreg.as<uint8_t>();
    a.rorder = pl.data_span > kRegionBytes ? rorder.as<uint64_t>() : order.as<uint64_t>();
    a.span = pl.data_span;
    a.long_mode = long_mode;
    a.waves = 4u * (uint32_t)num_cus;
    a.seq_wait_limit = seq_wait_limit();
    a.cand = pl.scan ? cand.as<uint64_t>() : nullptr;
    a.early = early;
    return a;
  }

  // descriptors in, counters and bucket counts zeroed, streams initialised: one dispatch
  int run_start(const RunPlan& pl, hipStream_t s) {
    // The pinned staging of the previous run may still be in flight: finish() synchronised.
    std::memcpy(h_streams.p, descs.data(), sizeof(StreamDesc) * pl.ns);
    if (pl.scan) {
      uint64_t* h0 = h_strip0.as<uint64_t>();
      for (uint32_t k = 0; k < pl.ns; ++k) h0[k] = descs[k].strip0;
      h0[pl.ns] = pl.strips;
    }
    const StartArgs st = start_args(pl);
    if (!st.src || (pl.scan && !st.src_strip0)) return BSG_EDEVICE;
    HCHECK(dbg("launch_start", s, launch_start(st, s)));
    return BSG_OK;
  }

  // the second stream and the events of the early chains, at the engine's first run with them
  int early_prepare() {
    if (!estream) HCHECK(stream_acquire(dev, &estream));
    // device-side dependencies only: no system-scope release (an L2 write-back) at record
    const unsigned fl = hipEventDisableTiming | hipEventDisableSystemFence;
    HCHECK(cand_ev.create(fl));
    HCHECK(pick_ev.create(fl));
    HCHECK(early_ev.create(fl));
    return BSG_OK;
  }

  // k_scan, the candidate offsets, k_compact: the sorted candidates of the run
  int run_scan(const RunPlan& pl, hipStream_t s) {
    const ScanArgs sa = scan_args(pl);
    mark(0);
    // k_scan: the fast pass, then each workgroup's exact pass over its own refine list
    if (pl.strips) HCHECK(dbg("launch_scan", s, launch_scan(sa, s, num_cus)));
    mark(1);

    PrefixArgs pa{};
    pa.in = counts.as<uint32_t>();
    pa.out = strip_off.as<uint64_t>();
    pa.partials = partials_a.as<uint64_t>();
    pa.n_bound = pl.strips;
    pa.total = &dctr()->ncand;
    pa.overflow = &dctr()->overflow;
    pa.cap = pl.cand_cap;
    pa.error = &dctr()->error;
    HCHECK(dbg("launch_prefix", s, launch_prefix(pa, s)));

    if (pl.strips) HCHECK(dbg("launch_compact", s, launch_compact(sa, s, num_cus)));
    // (exits at once unless a strip had more candidates than slots; k_pick needs them all)
    if (pl.strips) HCHECK(dbg("launch_rescan", s, launch_rescan(sa, s, num_cus)));
    return BSG_OK;
  }

  // k_pick and k_early on stream s
  int run_pick(const RunPlan& pl, const ShaArgs& sh, hipStream_t s) {
    HCHECK(dbg("launch_pick", s,
               launch_pick(cand.as<uint64_t>(), pl.cand_cap, dctr(), p.min_size, dearly(), s,
                           num_cus)));
    HCHECK(hipEventRecord(pick_ev, s));
    HCHECK(dbg("launch_early", s, launch_early(sh, p.split_bits, s)));
    return BSG_OK;
  }

  // The early chains beside selection; *sel_stream: where selection and k_sha then run.
  int run_early(const RunPlan& pl, const ShaArgs& sh, hipStream_t* sel_stream) {
    int rc;
    if (pl.light) {  // chains on the engine stream, selection beside them
      if ((rc = run_pick(pl, sh, stream))) return rc;
      HCHECK(hipStreamWaitEvent(estream, pick_ev, 0));
      *sel_stream = estream;
      early_open = true;  // until the engine stream waits for the selection stream's end
    } else {  // the sorted candidates are final: pick and start two chains beside selection
      HCHECK(hipEventRecord(cand_ev, stream));
      HCHECK(hipStreamWaitEvent(estream, cand_ev, 0));
      if ((rc = run_pick(pl, sh, estream))) return rc;
      HCHECK(hipEventRecord(early_ev, estream));
      early_open = true;
    }
    return BSG_OK;
  }

  // k_select, the chunk indices, k_chunks (and the streaming pipeline's snapshot)
  int run_select(const RunPlan& pl, hipStream_t s) {
    SelArgs sel{cand.as<uint64_t>(), streams.as<StreamDesc>(), flags.as<uint32_t>(), p, dctr()};
    HCHECK(dbg("launch_select", s, launch_select(sel, pl.cand_cap, s, num_cus)));

    PrefixArgs pf{};
    pf.in = flags.as<uint32_t>();
    pf.out = fidx.as<uint64_t>();
    pf.partials = partials_b.as<uint64_t>();
    pf.n_bound = pl.cand_cap;
    pf.n_dev = &dctr()->ncand;
    pf.total = &dctr()->nchunks;
    pf.skip_if = &dctr()->overflow;
    pf.error = &dctr()->error;
    HCHECK(dbg("launch_prefix", s, launch_prefix(pf, s)));

    HCHECK(dbg("launch_chunks", s, launch_chunks(chunk_args(pl), pl.cand_cap, pl.ns, s, num_cus)));
    if (snapshot) {  // by kernel, not by the copy engine (see launch_copy_out)
      HCHECK(h_snap.ensure(sizeof(Counters) + 8ull * (pl.ns ? pl.ns : 1)));
      HCHECK(sel_ev.create(hipEventDisableTiming));
      uint8_t* hs = static_cast<uint8_t*>(h_snap.dev());
      if (!hs) return BSG_EDEVICE;
      HCHECK(launch_copy_out(ctr.p, hs, sizeof(Counters), stream));
      if (pl.ns) HCHECK(launch_copy_out(last_end.p, hs + sizeof(Counters), 8ull * pl.ns, stream));
      HCHECK(hipEventRecord(sel_ev, stream));
    }
    return BSG_OK;
  }

  // One worker's SHA-256 rate (bytes per second), measured once per process for about a
  // millisecond on a resident buffer: bsg_init's warm-up, or the first run with a host tail.
  static double host_sha_rate(bool portable) {
    static const double best = sha256_measure_rate(sha256_best_impl(), 256 << 10, 1.0);
    if (!portable || sha256_best_impl() == kShaPortable) return best;
    static const double plain = sha256_measure_rate(kShaPortable, 256 << 10, 1.0);
    return plain;
  }

  // the workers, the second stream, the ring and the lists of a run with a host tail
  int tail_prepare(const RunPlan& pl) {
    if (!workers) workers.reset(new (std::nothrow) HashWorkers());
    if (!workers) return BSG_ENOMEM;
    if (!estream) HCHECK(stream_acquire(dev, &estream));
    HCHECK(tail_ev.create(hipEventDisableTiming | hipEventDisableSystemFence));
    HCHECK(gather_ev0.create());
    HCHECK(gather_ev1.create());
    const uint64_t ring =
        tail_ring_force ? tail_ring_force
                        : std::min<uint64_t>(kTailRingMax, std::max<uint64_t>(1 << 20, pl.total_len / 8));
    const uint32_t items = kTailMaxItems;
    HCHECK(h_ring.ensure(ring));
    const size_t meta = 64, flags = 4ull * items, list = sizeof(TailItem) * items;
    HCHECK(h_tail.ensure(meta + flags + list + 32ull * items));
    HCHECK(tail_hdr.ensure(sizeof(TailHdr)));
    HCHECK(tail_list.ensure(sizeof(TailItem) * items));
    HCHECK(tail_src.ensure(8ull * items));
    HCHECK(tail_refs.ensure(32ull * items));
    uint8_t* hd = static_cast<uint8_t*>(h_tail.dev());
    uint8_t* rd = static_cast<uint8_t*>(h_ring.dev());
    if (!hd || !rd) return BSG_EDEVICE;
    TailArgs& a = tail_args;
    a = TailArgs{};
    a.jinfo = jinfo.as<uint32_t>();
    a.jdesc = jdesc.as<LaneJob>();
    a.ctr = dctr();
    a.chunk_cap = pl.chunk_cap;
    a.hdr = tail_hdr.as<TailHdr>();
    a.dlist = tail_list.as<TailItem>();
    a.dsrc = tail_src.as<uint64_t>();
    a.hmeta = reinterpret_cast<uint64_t*>(hd);
    a.hready = reinterpret_cast<uint32_t*>(hd + meta);
    a.hlist = reinterpret_cast<TailItem*>(hd + meta + flags);
    a.ring = rd;
    a.ring_bytes = ring;
    a.max_items = items;
    a.force_cut = tail_force_cut;
    const double r1 = host_sha_rate(tail_portable);
    a.us_per_block = kTailUsPerBlock;
    a.pcie_bytes_us = kTailPcieBytesUs;
    a.host1_bytes_us = (float)(r1 * 1e-6);
    a.host_bytes_us = (float)(r1 * 1e-6 * workers->threads());
    a.d_refs = tail_refs.as<uint8_t>();
    a.out = out.as<ChunkRec>();
    tail_stat = TailStat{};
    tail_stat.host_rate = r1;
    tail_stat.threads = workers->threads();
    tail_stat.impl = tail_portable ? (int)kShaPortable : sha256_best_impl();
    return BSG_OK;
  }

  // after k_lens: the host's chunks out of the queues
  int run_tail_pick(const RunPlan& pl, hipStream_t s) {
    uint8_t* hp = h_tail.as<uint8_t>();
    uint64_t* meta = reinterpret_cast<uint64_t*>(hp);
    std::memset(hp, 0, 64 + 4ull * tail_args.max_items);
    meta[0] = kCountUnknown;
    HCHECK(hipMemsetAsync(tail_hdr.p, 0, sizeof(TailHdr), s));
    HCHECK(dbg("launch_tail_pick", s, launch_tail_pick(tail_args, pl.jobs, s, num_cus)));
    return BSG_OK;
  }

  // After the ordering kernels, beside k_sha: the gather on the second stream, the workers
  // started on the (still empty) list. Beside the ordering kernels instead, the gather's writes,
  // which leave at the link's rate, held up theirs: k_order's scatter pass took 0.94 ms for
  // ~10 us and k_bucket_scan 0.33 ms for 16 us (rocprofv3 kernel trace of that arrangement), all
  // of it in front of k_sha. k_sha writes next to nothing while it hashes.
  int run_tail_gather(hipStream_t s) {
    uint8_t* hp = h_tail.as<uint8_t>();
    uint64_t* meta = reinterpret_cast<uint64_t*>(hp);
    HCHECK(hipEventRecord(tail_ev, s));
    HCHECK(hipStreamWaitEvent(estream, tail_ev, 0));
    HCHECK(hipEventRecord(gather_ev0, estream));
    HCHECK(dbg("launch_tail_gather", estream, launch_tail_gather(tail_args, estream)));
    HCHECK(hipEventRecord(gather_ev1, estream));
    static_assert(sizeof(HashItem) == sizeof(TailItem), "the list is the workers' items");
    HashBatch b;
    b.count = meta;
    b.ready = reinterpret_cast<const uint32_t*>(hp + 64);
    b.items = reinterpret_cast<const HashItem*>(hp + 64 + 4ull * tail_args.max_items);
    b.base = h_ring.as<uint8_t>();
    b.base_len = tail_args.ring_bytes;
    b.max_items = tail_args.max_items;
    b.refs = hp + 64 + (4ull + sizeof(TailItem)) * tail_args.max_items;
    b.impl = tail_stat.impl;
    tail_t0_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(
                     std::chrono::steady_clock::now().time_since_epoch()).count();
    workers->start(b);
    tail_open = true;
    return BSG_OK;
  }

  // The open tail to its end: the gather done, every chunk hashed, the refs on the device and
  // k_offload_fix enqueued on the engine stream (behind the run's k_sha).
  int tail_settle() {
    if (!tail_open) return BSG_OK;
    tail_open = false;
    if (stream_wait(estream) != hipSuccess) {  // the list may never become final
      (void)hipGetLastError();
      workers->cancel();
      (void)workers->wait();
      return BSG_EDEVICE;
    }
    const uint64_t bad = workers->wait();
    const uint64_t* meta = h_tail.as<uint64_t>();
    const uint64_t n = std::min<uint64_t>(meta[0], tail_args.max_items);
    tail_stat.chunks = n;
    tail_stat.cut = n ? meta[1] : 0;
    tail_stat.bytes = n ? meta[2] : 0;
    tail_stat.longest_all = meta[3];
    tail_stat.longest_left = meta[4];
    tail_stat.blocks = n ? meta[5] : 0;
    if (hipEventElapsedTime(&tail_stat.gather_ms, gather_ev0, gather_ev1) != hipSuccess) {
      (void)hipGetLastError();
      tail_stat.gather_ms = -1.f;
    }
    tail_stat.host_done_us = n ? (workers->last_done_ns() - tail_t0_ns) / 1000 : 0;
    if (bad || workers->hashed_items() != n) return device_error(64);
    if (n) {
      const uint8_t* refs = h_tail.as<uint8_t>() + 64 + (4ull + sizeof(TailItem)) * tail_args.max_items;
      HCHECK(hipMemcpyAsync(tail_refs.p, refs, 32 * n, hipMemcpyHostToDevice, stream));
      HCHECK(dbg("launch_tail_fix", stream, launch_tail_fix(tail_args, stream)));
    }
    return BSG_OK;
  }

  // the job lists (k_lens .. k_order), then k_sha
  int run_sha(const RunPlan& pl, const ShaArgs& sh, hipStream_t s) {
    if (pl.tail) {
      HCHECK(dbg("launch_lens", s, launch_lens(sh, pl.jobs, s, num_cus)));
      if (int rc = run_tail_pick(pl, s)) return rc;
      HCHECK(dbg("launch_order", s, launch_order(sh, pl.jobs, s, num_cus)));
      if (int rc = run_tail_gather(s)) return rc;
    } else
    HCHECK(dbg("launch_longlist", s, launch_longlist(sh, pl.jobs, s, num_cus)));
    mark(2, s);
    HCHECK(dbg("launch_sha", s, launch_sha(sh, pl.jobs, s, num_cus)));
    return BSG_OK;
  }

  // the early chains' records into place, once they (and k_sha) are done
  int run_early_fix(const RunPlan& pl) {
    if (pl.light) HCHECK(hipEventRecord(early_ev, estream));  // selection + k_sha done
    HCHECK(hipStreamWaitEvent(stream, early_ev, 0));
    early_open = false;  // the engine stream now orders everything after the chains
    HCHECK(dbg("launch_early_fix", stream,
               launch_early_fix(dearly(), out.as<ChunkRec>(), dctr(), stream)));
    return BSG_OK;
  }

  int enqueue() {
    int rc;
    run_done = false;
    dd.valid = false;  // a dedup result belongs to the run it was made from
    tree.valid = false;  // ... and so does a tree (bsg_engine_pool_put reads both)
    if (early_open) {  // a failed run left second-stream work its engine stream never waited for
      HCHECK(hipStreamSynchronize(estream));
      early_open = false;
    }
    // a run enqueued behind one that was not finished: that one's tail first (its refs go into
    // the records this run is about to overwrite, in stream order)
    if ((rc = tail_settle())) return rc;
    const RunPlan pl = plan_split();
    if ((rc = reserve(pl)) || (rc = run_start(pl, stream))) return rc;
    if (pl.early && (rc = early_prepare())) return rc;
    if (pl.tail && (rc = tail_prepare(pl))) return rc;
    if (!pl.tail) tail_stat = TailStat{};
    const ShaArgs sh = sha_args(pl, long_mode(), pl.early ? dearly() : nullptr);
    if ((rc = run_scan(pl, stream))) return rc;
    hipStream_t sel_stream = stream;  // where selection and k_sha run
    if (pl.early && (rc = run_early(pl, sh, &sel_stream))) return rc;
    if ((rc = run_select(pl, sel_stream))) return rc;
    if (pl.early && !pl.light) HCHECK(hipStreamWaitEvent(stream, pick_ev, 0));  // k_lens reads the picks
    if ((rc = run_sha(pl, sh, sel_stream))) return rc;
    if (pl.early && (rc = run_early_fix(pl))) return rc;
    mark(3);
    enqueued = true;
    return BSG_OK;
  }

  // bsg_engine_hash: every stream is one blob, hashed whole (Blob.Ref of many blobs): no scan or
  // selection, one final chunk per stream, then the same job ordering and k_sha as a split run.
  // (No candidates, so such a run cannot overflow: finish() never re-runs it.)
  int enqueue_hash() {
    int rc;
    run_done = false;
    dd.valid = false;  // a dedup result belongs to the run it was made from
    tree.valid = false;  // ... and so does a tree (bsg_engine_pool_put reads both)
    // behind a split run that was not finished: that run's tail first, while its records and
    // lists still stand (reserve may move them); its fix lands before this run in stream order
    if ((rc = tail_settle())) return rc;
    tail_stat = TailStat{};  // a hash run has no tail
    const RunPlan pl = plan_hash();
    if ((rc = reserve(pl)) || (rc = run_start(pl, stream))) return rc;
    mark(0);
    mark(1);  // no scan / selection stage
    if (pl.ns) HCHECK(dbg("launch_blob_jobs", stream,
                          launch_blob_jobs(chunk_args(pl), streams.as<StreamDesc>(), pl.ns, stream,
                                           num_cus)));
    const ShaArgs sh = sha_args(pl, hash_long_mode >= 0 ? hash_long_mode : long_mode(), nullptr);
    if ((rc = run_sha(pl, sh, stream))) return rc;
    mark(3);
    enqueued = true;
    return BSG_OK;
  }

  int finish(uint64_t* nchunks) {
    if (!enqueued) return BSG_ESTATE;
    for (int attempt = 0; attempt < 3; ++attempt) {
      if (int rc = tail_settle()) {
        enqueued = false;
        return rc;
      }
      HCHECK(hipMemcpyAsync(h_ctr.p, ctr.p, sizeof(Counters), hipMemcpyDeviceToHost, stream));
      HCHECK(stream_wait(stream));
      last = *h_ctr.as<Counters>();
      if (!last.overflow) break;
      retry_cap = last.ncand + 1024;  // exact size for this input, then run again
      int rc = hash_mode ? enqueue_hash() : enqueue();
      if (rc) return rc;
    }
    retry_cap = 0;
    if (last.overflow) return BSG_ENOMEM;
    enqueued = false;
    if (last.error) return device_error(last.error);
    if (profile)
      for (int i = 0; i < 3; ++i)
        stage_ms[i] = profile == 2 && i < 2 ? -1.f : marks.ms(i, i + 1, -1.f);
    if (nchunks) *nchunks = last.nchunks;
    run_done = !hash_mode && !snapshot;
    return BSG_OK;
  }

  // A hash run whose descriptors a kernel wrote (d_src, device memory) instead of the host:
  // blob i = data[desc[i].data_off .. + desc[i].len), record i = its ref. Enqueued on `stream`;
  // the caller reads out / ctr on the same stream.
  int enqueue_hash_device(const uint8_t* data, uint64_t span, const StreamDesc* d_src,
                          uint32_t n, int sha_mode) {
    int rc;
    RunPlan pl;
    pl.ns = n;
    pl.data_span = std::max<uint64_t>(1, span);
    pl.chunk_cap = n;
    pl.jobs = 2ull * n;
    if ((rc = reserve(pl))) return rc;
    d_data = data;
    nstreams = n;
    hash_mode = true;
    normalize(nullptr, &p, nullptr);
    StartArgs st = start_args(pl);
    st.src = d_src;
    HCHECK(dbg("launch_start", stream, launch_start(st, stream)));
    HCHECK(dbg("launch_blob_jobs", stream,
               launch_blob_jobs(chunk_args(pl), streams.as<StreamDesc>(), pl.ns, stream, num_cus)));
    const ShaArgs sh = sha_args(pl, sha_mode, nullptr);
    return run_sha(pl, sh, stream);
  }
};

namespace {

int need_hasher(bsg_engine* owner) {
  if (owner->hasher) return BSG_OK;
  bsg_engine* h = new (std::nothrow) bsg_engine();
  if (!h) return BSG_ENOMEM;
  h->dev = owner->dev;
  h->num_cus = owner->num_cus;
  h->stream = owner->stream;
  h->borrowed_stream = true;
  owner->hasher = h;
  return BSG_OK;
}

template <class Descs, class Consume>
int hash_batches(bsg_engine* owner, DevBuf& dbuf, uint64_t n, const uint8_t* data, uint64_t span,
                 int sha_mode, Descs descs, Consume consume) {
  bsg_engine* hasher = owner->hasher;
  for (uint64_t b = 0; b < n; b += kTreeHashBatch) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(kTreeHashBatch, n - b);
    HCHECK(dbuf.ensure(sizeof(StreamDesc) * nb));
    HCHECK(descs(b, nb, dbuf.as<StreamDesc>()));
    if (int rc = hasher->enqueue_hash_device(data, span, dbuf.as<StreamDesc>(), nb, sha_mode))
      return rc;
    HCHECK(consume(b, nb, hasher->out.as<ChunkRec>(), hasher->dctr()));
  }
  return BSG_OK;
}

}  // namespace
