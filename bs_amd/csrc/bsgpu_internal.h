// bsgpu_internal.h — device data layout shared by the HIP kernels and the host engine.
//
// One launch ("run") processes a batch of stream SEGMENTS. A segment is a contiguous range of
// one byte stream that lives in device memory. Fresh streams (the batch API) have zero history,
// IV hash state and finalize=1. Streaming continuation (split.Writer over many Write calls,
// reference split/split.go:99-126) carries a 64-byte window history, the open chunk's start
// and its SHA-256 midstate from one segment to the next.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsg {

constexpr int kScanWG = 512;       // threads per rolling-scan workgroup (8 waves)
#ifndef BSG_STRIP
#define BSG_STRIP 2048
#endif
constexpr int kStrip = BSG_STRIP;  // bytes per lane-strip in the rolling scan
constexpr int kSlotCap = 4;        // candidates kept per strip in the first scan pass
constexpr int kTabRows = 256;      // buzhash32 table rows
constexpr int kTabRep = 64;        // one replica per lane: LDS address = byte*256 + lane*4

// Candidate record (u64): | stream:16 | pos:40 | force:1 | unused:1 | tz:6 |
constexpr int kCandPosShift = 8;
constexpr uint64_t kCandPosMask = (1ull << 40) - 1;
constexpr uint64_t kCandForce = 1ull << 7;

__host__ __device__ inline uint64_t cand_pack(uint32_t stream, uint64_t pos, bool force,
                                              uint32_t tz) {
  return ((uint64_t)stream << 48) | ((pos & kCandPosMask) << kCandPosShift) |
         (force ? kCandForce : 0ull) | (uint64_t)(tz & 63u);
}
__host__ __device__ inline uint32_t cand_stream(uint64_t c) { return (uint32_t)(c >> 48); }
__host__ __device__ inline uint64_t cand_pos(uint64_t c) {
  return (c >> kCandPosShift) & kCandPosMask;
}
__host__ __device__ inline bool cand_force(uint64_t c) { return (c & kCandForce) != 0; }
__host__ __device__ inline uint32_t cand_tz(uint64_t c) { return (uint32_t)(c & 63u); }

// Per-strip slot record (u32): | local_off:24 | force:1 | unused:1 | tz:6 |
__host__ __device__ inline uint32_t slot_pack(uint32_t local, bool force, uint32_t tz) {
  return (local << 8) | (force ? 0x80u : 0u) | (tz & 63u);
}

struct StreamDesc {            // 160 bytes, 16-byte aligned
  uint64_t data_off;           // device byte offset of the segment's first byte
  uint64_t len;                // segment length (bytes)
  uint64_t strip0;             // first global strip index of this segment
  uint64_t seg_base;           // stream offset of the segment's first byte
  uint64_t open_start;         // stream offset where the open (unfinished) chunk starts
  uint64_t consumed;           // open-chunk bytes already folded into mid[] (multiple of 64)
  uint32_t finalize;           // 1: flush the tail as the final chunk (Splitter.Close)
  uint32_t prefix_len;         // open-chunk bytes held in hist[64-prefix_len..63], < 64
  uint32_t mid[8];             // SHA-256 midstate of the open chunk (IV when consumed == 0)
  uint32_t carry_cap;          // non-final segment: leave an open chunk of <= carry_cap bytes
                               // unhashed (the next segment re-hashes it from device memory)
  uint32_t flags;              // kDescOpenInDevice: the open chunk's bytes [open_start, seg_base)
                               // sit in device memory right before data_off (consumed == 0)
  uint8_t hist[64];            // the 64 stream bytes before seg_base (zeros before offset 0)
};
constexpr uint32_t kDescOpenInDevice = 1;
static_assert(sizeof(StreamDesc) == 160, "StreamDesc layout");

struct CarryOut {              // open chunk state after a non-final segment
  uint32_t mid[8];
  uint64_t consumed;           // bytes folded into mid (multiple of 64)
  uint64_t open_start;         // stream offset of the open chunk
  uint32_t prefix_len;         // trailing open-chunk bytes not yet hashed (< 64)
  uint32_t valid;
};

struct ChunkRec {              // == bsg_chunk (include/bsgpu.h)
  uint64_t offset;
  uint64_t len;
  uint32_t level;
  uint32_t stream;
  uint8_t ref[32];
};
static_assert(sizeof(ChunkRec) == 56, "ChunkRec layout");

struct Params {
  uint32_t split_bits;         // trailing-zero bits for a boundary (>= 1; > 32 never splits)
  uint32_t min_size;           // minimum chunk size (>= 1)
  uint32_t mask;               // (1 << split_bits) - 1, all ones for split_bits >= 32
  uint32_t pad_;
};

// Device counters, zeroed at the start of every run (one hipMemsetAsync).
struct Counters {
  uint64_t ncand;              // total candidates (from the strip-count scan)
  uint64_t nchunks;            // total boundaries = finalized chunks
  uint64_t help_wg;            // k_sha workgroups arrived (the first helped/2 run helped solo pairs)
  uint64_t overflow;           // candidate buffer too small (host grows and re-runs)
  uint64_t error;              // device-side sanity check failed (bug guard; run is invalid)
  uint64_t max_nblocks;        // longest SHA-256 job in blocks (k_lens)
  uint64_t long_thresh;        // jobs with >= this many blocks run on the wave-per-chunk path
  uint64_t nlong;              // number of such jobs (k_longlist)
  uint64_t long_head;          // k_sha_long work queue head
  uint64_t nshort;             // jobs on the per-lane path (k_bucket_scatter)
  uint64_t bucket_width;       // LPT bucket width in blocks
  uint64_t diag[5];            // k_sha_long job 0: memtime0/1, realtime0/1, nblocks (diagnostic)
  uint64_t diag2[5];           // k_sha per-lane job order[0]: same fields
  uint64_t rescan;             // strips with more candidates than slots (k_compact re-scans)
  uint64_t total_blocks;       // SHA-256 blocks over all jobs (k_lens)
  uint64_t long_buckets;       // LPT buckets [0, long_buckets) of wave-eligible jobs -> wave mode
  uint64_t ntickets;           // wave-mode work items: kSolo single jobs, then groups of kGroup
  uint64_t sha_arrivals;       // k_sha waves started (diagnostic)
  uint64_t sha_start_rt;       // s_memrealtime of the first k_sha wave (diagnostic)
  uint64_t lane_end_rt;        // latest s_memrealtime at which a wave left per-lane mode
  uint64_t nlong_grp;          // long jobs on solo / kGroup tickets; the rest of the long list
  uint64_t tickets_grp;        //   runs on pair tickets (kPairGroup jobs, one lane pair each)
  uint64_t nrefine;            // strips k_scan listed for its exact pass
  uint64_t helped;             // solo tickets [0, helped) run with a helper wave (k_sha)
  uint64_t scan_ticket;        // k_scan's strip groups handed out past the first (BSG_SCAN_DYN)
  uint64_t pad[7];
};
static_assert(sizeof(Counters) == 320, "Counters layout");

// Per-lane job descriptor (k_lens writes one per job): per-lane mode prefetches it a few blocks
// before its current job ends, so starting the next job costs no dependent loads.
struct LaneJob {
  uint64_t dptr;               // first data byte of the message (device address)
  uint64_t start;              // stream offset of the chunk (record offset)
  uint64_t len;                // message bytes = chunk length (fast jobs)
  uint32_t stream;
  uint32_t meta;               // level | kLaneJobSlow
};
static_assert(sizeof(LaneJob) == 32, "LaneJob layout");
constexpr uint32_t kLaneJobSlow = 0x80000000u;  // continued or open chunk: full sha_setup path

// Per-lane job queues by address region (k_sha per-lane mode). A lane's loads go to its own
// chunk, so the 64 lanes of a wave touch 64 places in HBM per load. With a CU's lanes spread
// over 16 GiB, 97 % of those loads miss the CU's address-translation cache (UTCL1) and a block
// costs ~60 % more than with the CU's lanes inside 2 GiB (tools/ubench/lanes_mem.hip,
// profiles/r02_lanes_tlb.log). The per-lane jobs are therefore regrouped, longest first within
// each region, into regions of at most kRegionBytes of address span, and all waves of a k_sha
// workgroup (one per CU) take their jobs from the same region until it runs dry.
constexpr uint32_t kMaxRegions = 256;
constexpr uint32_t kRegionSegs = 256;        // segments of the LPT order counted separately
constexpr uint32_t kMinRegionJobs = 4096;    // fewer per-lane jobs per region: fewer regions
constexpr uint64_t kRegionBytes = 1ull << 30;
struct Regions {
  uint64_t nregions;                         // R (k_bucket_scan), 1 .. kMaxRegions
  uint64_t rr;                               // round-robin start region of entering waves
  uint64_t pad_[6];
  uint64_t head[kMaxRegions];                // pop counters (zeroed by k_rtotal)
  uint64_t off[kMaxRegions + 1];             // region r's jobs: rorder[off[r] .. off[r + 1])
  uint64_t pad2_[7];
  uint32_t cnt[kRegionSegs * kMaxRegions];   // per segment and region: count, then offset
};

// Early chains (round 4). A step is bound by its longest chunks' serial SHA-256 chains, and
// in k_sha they start only after the whole selection (k_select .. k_order, ~0.1-0.3 ms of small
// dispatches). The sorted candidates already fix the chunks whose both ends are sync points
// (sure boundaries): on a second stream k_pick takes the kEarly longest of them and k_early
// hashes them (a helped pair: two chains, two ring fillers) while selection runs; k_lens takes the chunks (same stream, start and end) out of
// k_sha's queues and k_early_fix writes their records. A pick k_lens does not match is hashed
// by k_sha as usual.
constexpr int kEarly = 2;
struct Early {
  uint64_t top[kEarly];      // k_pick: (blocks << 32) | i for the chunk (E_i, E_i+1]; 0 = none
  uint64_t idx[kEarly];      // k_lens: 1 + the chunk's job index (0: not matched)
  uint64_t diag[5];          // k_early: timing stamps of top[0]'s chain (as Counters::diag)
  uint64_t pad_;
  ChunkRec rec[kEarly];      // k_early: the chunks' records
};
static_assert(sizeof(Early) % 16 == 0, "Early layout");

// Host tail (bsg_engine, "Host tail"; bsgpu_tail.inc). A lightly loaded run's step is its longest
// chunk's serial chain, so the run's longest chunks leave k_sha's queues the way the early picks
// do (jinfo = kNoJob): their bytes go through a pinned ring to host threads (host_sha256.h), which
// hash them while k_sha hashes the rest, and k_offload_fix writes their records.
constexpr uint32_t kTailBuckets = 256;       // job lengths by bucket of (longest / 256 + 1) blocks
constexpr uint32_t kTailMaxItems = 4096;     // chunks one run hands to the host at most
constexpr uint32_t kTailMinBlocks = 256;     // the cost model never offloads below 16 KiB
constexpr uint32_t kTailSlotAlign = 256;     // a chunk's place in the ring
struct TailItem {              // == HashItem (host_sha256.h)
  uint64_t job;                // the chunk's record index
  uint64_t start;              // its stream offset
  uint64_t len;
  uint64_t off;                // of its first byte in the ring (off % 16 == source address % 16)
  uint32_t stream;
  uint32_t level;
};
static_assert(sizeof(TailItem) == 40, "TailItem layout");
struct TailHdr {               // device side, zeroed before every run with a host tail
  uint64_t count;              // chunks taken (k_offload_cut's plan; k_offload_take fills it)
  uint64_t cutb;               // buckets >= cutb are taken (kTailBuckets: none)
  uint64_t bytes;              // ring bytes of the plan
  uint64_t blocks;             // SHA-256 blocks of the plan
  uint64_t mx_all;             // the run's longest job before the cut
  uint64_t mx_left;            // ... and after it (Counters::max_nblocks from then on)
  uint64_t ring_head;          // k_offload_take: ring bytes handed out
  uint64_t taken;              // k_offload_take: chunks appended
  uint32_t cnt[kTailBuckets];  // k_offload_hist, per bucket: candidate jobs,
  uint32_t maxb[kTailBuckets]; //   the longest of them (blocks),
  uint64_t rbytes[kTailBuckets];  // their ring bytes
  uint64_t nblk[kTailBuckets];    //   and their blocks
  uint32_t base[kTailBuckets]; // k_offload_cut: bucket b's first place in the list (longest first)
  uint32_t fill[kTailBuckets]; // k_offload_take: places handed out
};
static_assert(sizeof(TailHdr) % 16 == 0, "TailHdr layout");
constexpr uint32_t kTailMetaWords = 8;  // pinned: count (kCountUnknown until final), cut blocks,
                                        // ring bytes, longest before, longest left, blocks
__host__ __device__ inline uint64_t tail_slot(uint64_t len) {
  return (len + 16 + kTailSlotAlign - 1) & ~(uint64_t)(kTailSlotAlign - 1);
}

constexpr uint32_t kLongMinBlocks = 1024;  // never use the wave path below 64 KiB
#ifndef BSG_SOLO
#define BSG_SOLO 16  // configs[2]: the 9th-16th longest jobs on group tickets (1.40 us per
#endif           // block against 1.19 solo) ended 0.5 ms after the longest
constexpr uint32_t kSolo = BSG_SOLO;  // wave mode: the kSolo longest jobs run one per wave,
constexpr uint32_t kGroup = 8;   // the next ones kGroup per wave (one skewed octet each)
constexpr uint32_t kPairGroup = 32;  // then (optionally) 32 per wave, one skewed lane pair each
constexpr int kLongRow = 68;               // LDS words per K+W row (64 + pad: conflict-free b128)
constexpr int kRingWords = 65 * kLongRow;  // per wave: 64 K+W rows + one row of ones
constexpr int kLptBuckets = 4096;          // longest-first job order: counting sort on nblocks
constexpr uint64_t kReadSlack = 256;       // readable bytes required after every stream's data

// split.Writer's tree built on the device (bsg_engine_trees; bsgpu_tree.inc). Levels are at most
// 32 (TrailingZeros32 - Bits) and fanout at least 1, so a tree has at most 33 heights.
constexpr uint32_t kTreeMaxHeights = 40;
struct TreeNode {              // == bsg_tree_node (include/bsgpu.h)
  uint64_t blob_off;
  uint32_t blob_len;
  uint32_t stream;
  uint32_t height;
  uint32_t reserved;
  uint8_t ref[32];
};
static_assert(sizeof(TreeNode) == 56, "TreeNode layout");
struct TreeHdr {               // totals of one bsg_engine_trees call, read back by the host
  uint64_t nnodes;             // listed nodes of all streams
  uint64_t arena_bytes;        // blob bytes, every blob 16-byte aligned
  uint64_t max_r;              // the largest Root height
  uint64_t error;              // a consistency check failed (bug guard; the result is invalid)
  uint64_t hoff[kTreeMaxHeights + 1];  // height h's nodes have internal ids [hoff[h], hoff[h+1])
};
struct TreeNodeMeta {          // per internal id (height-major, then stream, then offset)
  uint64_t child0;             // first child: a chunk index (height 0) or an internal id
  uint64_t nchild;
  uint64_t offset, size;       // Node.offset / Node.size
  uint64_t out_idx;            // its place in the listed order
  uint64_t blob_off;
  uint32_t blob_len;
  uint32_t stream;
};

// Chunk dedup on the device (bsg_engine_dedup, bsg_refset; bsgpu_dedup.inc). The tables are open
// addressing with linear probing; a slot holds an index (of a record of the run, or of a key in a
// set's append-only key array), never a key, and kDedupEmpty marks a free slot.
constexpr uint64_t kDedupEmpty = ~0ull;
constexpr uint64_t kDedupInSet = 1ull << 63;  // first[i]: the ref was in the set before the call
constexpr uint64_t kRefSetSlots0 = 1024;      // a new set's table
constexpr uint64_t kRefSetLoadPct = 50;       // a set's table doubles before keys * 100 > slots * this
constexpr uint32_t kPackTile = 32768;         // output bytes per workgroup of bsg_engine_pack_unique
struct DedupHdr {              // totals of one dedup pass, read back by the host
  uint64_t error;              // a probe ran through its whole table (bug guard; result invalid)
  uint64_t nunique;
  uint64_t unique_bytes;
  uint64_t pad_;
};

// Streams restored from a pool of blobs (bsg_engine_restore; bsgpu_restore.inc).
constexpr uint32_t kRestoreTile = 32768;      // output bytes of one stream per scatter workgroup
struct PoolBlob {              // == bsg_pool_blob (include/bsgpu.h)
  uint64_t off;
  uint64_t len;
  uint8_t ref[32];
};
static_assert(sizeof(PoolBlob) == 48, "PoolBlob layout");
struct RestoreHdr {            // one call's verdicts, read back by the host
  DedupHdr dd;                 // dd.error: a device-side bound check failed (bug guard)
  uint64_t invalid;            // the records break a layout rule (BSG_EINVAL)
  uint64_t missing;            // smallest record whose ref the pool lacks, else ~0
  uint64_t mismatch;           // smallest record whose len is not its blob's, else ~0
  uint64_t bad_blob;           // smallest pool blob that does not hash to its ref, else ~0
};
static_assert(sizeof(RestoreHdr) == 64, "RestoreHdr layout");

// Split trees read on the device, from Roots to records (bsg_engine_walk; bsgpu_walk.inc). Breadth
// first: level L's frontier holds every node blob at depth L (Root = 0) of every stream, sorted by
// (stream, offset).
constexpr uint32_t kWalkMaxDepth = 64;        // a node deeper than this is refused
constexpr uint32_t kWalkRuns = 12;            // entry lengths 36 and 38..47: at most 11 runs
constexpr uint64_t kWalkDead = ~0ull;         // WalkItem::blob: no node here (empty stream, miss)
constexpr uint32_t kWalkCorrupt = 1;          // per-stream status words, merged by atomicMax:
constexpr uint32_t kWalkNotFound = 2;         //   not found outranks corrupt outranks 0 (ok)
struct WalkItem {              // one frontier entry
  uint64_t blob;               // pool blob index, or kWalkDead
  uint64_t exp_off;            // the cover its parent gives it: the node's own offset ...
  uint64_t exp_size;           // ... and size must equal it (0: a Root, any size)
  uint64_t parent;             // its parent's index in the level above (a Root: its stream)
  uint32_t stream;
  uint32_t flags;              // kWalkNoCover: held to the node's own rules only (exp_* unused)
};
constexpr uint32_t kWalkNoCover = 1;          // WalkItem::flags (bsg_engine_gc_mark's entries)
static_assert(sizeof(WalkItem) == 40, "WalkItem layout");
struct WalkNode {              // what the count pass learns of a frontier entry
  uint64_t nchild;             // 0: dead, or the node failed
  uint64_t offset, size;       // Node.offset / Node.size
  uint64_t nrec;               // records below it (placement, bottom-up)
  uint64_t rbase;              // its first record's place (placement, top-down)
  uint32_t kind;               // 0 none, 1 nodes, 2 leaves
  uint32_t nruns;              // its entries lie in runs of equal entry length:
  uint64_t run_pos[kWalkRuns]; //   run r starts at this byte of the blob
  uint64_t run_idx[kWalkRuns]; //   with this child
  uint32_t run_len[kWalkRuns]; //   and every entry of it has this many bytes
};
struct WalkHdr {               // one call's verdicts and per-level totals, read back by the host
  DedupHdr dd;                 // dd.error: a device-side bound check failed (bug guard)
  uint64_t nnodes;             // node blobs visited
  uint64_t depth;              // deepest node visited
  uint64_t lvl_all[kWalkMaxDepth + 1];    // children of level L's nodes
  uint64_t lvl_nodes[kWalkMaxDepth + 1];  // ... of which `nodes` children (the next frontier)
};
static_assert(sizeof(WalkHdr) % 16 == 0, "WalkHdr layout");

// Byte ranges of streams read out of a pool (bsg_engine_read; bsgpu_read.inc): the walk with a
// window per range, the restore's checks and scatter clipped to it.
struct ReadHdr {               // one call's verdicts, read back by the host
  WalkHdr w;                   // the pruned walk's header (w.dd.error: its bug guard)
  RestoreHdr r;                // resolve, tiling and verify (r.dd.error: theirs); r.invalid bits
                               //   1 | 2: a range's records do not cover its window (bug guard),
                               //   4: a touched blob breaks the hash path's layout rules
  uint64_t verified;           // the touched blobs' lens, summed
  uint64_t pad_;
};
static_assert(sizeof(ReadHdr) % 16 == 0 && offsetof(ReadHdr, r) % 16 == 0, "ReadHdr layout");

// A pool garbage-collected on the device from its Roots (bsg_engine_gc_mark / _compact;
// bsgpu_gc.inc). The mark is the walk's breadth-first search without covers and with every blob
// expanded once: level L's frontier holds the node blobs whose nearest Root is L edges away.
constexpr uint32_t kGcClaimed = 1;            // GcArgs::state[k]: blob k has a frontier entry
constexpr uint32_t kGcFailed = 2;             //   ... and failed the node rules
constexpr uint32_t kGcTile = 32768;           // output bytes per workgroup of the compaction
struct GcHdr {                 // one mark's verdicts and totals, read back by the host
  WalkHdr w;                   // the count pass's header (w.dd.error: the bug guard)
  uint64_t bad_form;           // smallest blob index of a node that fails its rules, else ~0
  uint64_t bad_miss;           // smallest blob index of a node that names a child the pool lacks
  uint64_t verdict;            // kWalkCorrupt / kWalkNotFound, merged by atomicMax
  uint64_t leaf_miss;          // a forgiven `leaves` miss was seen (BSG_GC_MISSING_LEAVES)
  uint64_t missing_leaves;     // distinct such refs (k_gc_missing)
  uint64_t end, end16;         // the end of the last live blob's bytes, tight and 16-aligned
  uint64_t size0;              // what the count pass writes for its one stream (unused)
  uint32_t status0;            // (unused)
  uint32_t pad_;
  uint64_t pad2_;
  uint8_t zero[16];            // the bytes of ALIGN16's padding
};
static_assert(sizeof(GcHdr) % 16 == 0 && offsetof(GcHdr, zero) % 16 == 0, "GcHdr layout");

// A run's new chunks and tree nodes appended to a pool that lives in device memory (bsg_pool,
// bsg_engine_pool_put; bsgpu_pool.inc). The pool's index is the open-addressing table of blob
// indices by ref that launch_ref_index builds for a caller's pool, kept and grown by inserts.
constexpr uint32_t kPoolTile = 32768;         // output bytes per workgroup of the append's gather
struct PoolHdr {               // one put's totals, read back by the host before the pool is written
  DedupHdr dd;                 // the first-occurrence pass's header (dd.error: the bug guard)
  uint64_t total16;            // the new blobs' lens, each rounded up to 16
  uint64_t last_len;           // the last new blob's len
  uint64_t known;              // items whose ref the pool held
  uint64_t repeats;            // items that repeat an earlier item
  uint8_t zero[16];            // the bytes of the padding
};
static_assert(sizeof(PoolHdr) % 16 == 0 && offsetof(PoolHdr, zero) % 16 == 0, "PoolHdr layout");

// A pool's selected blobs appended to a pool that may hold some of them (bsg_pool_merge,
// bsg_pool_sync; bsgpu_pool.inc). One direction's verdicts and totals, read back by the host
// before anything of the destination is written.
struct MergeHdr {
  GcHdr g;                     // the segment gather's header (g.w.dd.error: the bug guard of the
                               //   probe, the plan, the append and the gather; g.zero: padding)
  RestoreHdr r;                // the verification's (r.dd.error: its bug guard; r.invalid bit 4;
                               //   r.bad_blob: the smallest new blob that does not hash to its ref)
  uint64_t selected;           // selected blobs of the source
  uint64_t known;              // ... whose ref the destination held
  uint64_t added_bytes;        // the new blobs' lens, summed
  uint64_t end;                // the end of the last new blob's bytes, from the base
  uint64_t verified;           // the hashed blobs' lens, summed
  uint64_t pad_;
};
static_assert(sizeof(MergeHdr) % 16 == 0 && offsetof(MergeHdr, r) % 16 == 0, "MergeHdr layout");

// Blobs put into a pool and got out of it by ref (bsg_pool_put_blobs, bsg_pool_get;
// bsgpu_blobs.inc). A put's item i is src[span[i].off .. + span[i].len), its ref the hash runs'.
struct BlobSpan {
  uint64_t off;
  uint64_t len;
};
struct GetHdr {                // one get's verdicts and totals, read back by the host
  RestoreHdr r;                // r.dd.error: the bug guard of the probe, the verification and the
                               //   gather; r.invalid bit 4; r.bad_blob: the smallest found blob
                               //   that does not hash to its ref
  uint64_t found;              // requests whose ref the pool holds
  uint64_t bytes;              // their blobs' lens, summed
  uint64_t verified;           // the hashed blobs' lens, summed
  uint64_t pad_;
  uint8_t zero[16];            // the bytes of the padding
};
static_assert(sizeof(GetHdr) % 16 == 0 && offsetof(GetHdr, zero) % 16 == 0, "GetHdr layout");

}  // namespace bsg
