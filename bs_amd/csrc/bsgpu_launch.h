// bsgpu_launch.h — kernel argument blocks and launchers (host <-> bsgpu_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsgpu_internal.h"

namespace bsg {

struct ScanArgs {
  const uint8_t* data;
  const StreamDesc* streams;
  const uint64_t* strip0;   // nstreams + 1 cumulative strip counts
  uint32_t nstreams;
  uint64_t nstrips;
  const uint32_t* table;    // 256 buzhash32 entries
  Params p;
  uint32_t* counts;         // [nstrips]
  uint64_t* refine;         // [lists * list_cap] strips k_scan's exact pass must scan: strip << 32
                            // | the fast pass's hit mask (one bit per 64-byte block); k_scan
                            // workgroup g appends to refine + g * list_cap
  uint32_t* slots;          // [nstrips * kSlotCap]
  const uint64_t* cand_off; // [nstrips] exclusive candidate offsets (compact)
  uint64_t* cand;           // [cand_cap]
  uint64_t cand_cap;
  Counters* ctr;
  uint32_t lists;           // k_scan's grid = the number of refine lists (scan_lists())
  uint64_t list_cap;        // entries per list: the strips one k_scan workgroup scans, at most
  uint32_t* list_cnt;       // [lists] each list's length, stored by its workgroup at exit
};
// k_scan's grid for nstrips strips (its workgroups take 256-strip groups by ticket) and the length
// bound of each workgroup's refine list; the host sizes ScanArgs::refine with them.
uint32_t scan_lists(uint64_t nstrips, int num_cus);
uint64_t scan_list_cap(uint64_t nstrips, uint32_t lists);

struct PrefixArgs {
  const uint32_t* in;
  uint64_t* out;
  uint64_t* partials;
  uint64_t n_bound;         // host bound on n
  const uint64_t* n_dev;    // optional device-side n (min with n_bound)
  uint64_t* total;          // receives the sum
  uint64_t* overflow;       // optional: set to 1 when total > cap
  uint64_t cap;
  const uint64_t* skip_if;  // optional: skip when *skip_if != 0
  uint64_t* error;          // k_prefix1: Counters::error (|= 32: a look-back poll timed out)
};

struct SelArgs {
  const uint64_t* cand;
  const StreamDesc* streams;
  uint32_t* flags;
  Params p;
  Counters* ctr;
};

struct ChunkArgs {
  const uint64_t* cand;
  const uint32_t* flags;
  const uint64_t* fidx;
  uint64_t* bnd_end;
  uint64_t* bnd_info;
  uint64_t* scount;
  uint64_t* last_end;
  uint64_t chunk_cap;
  Params p;
  Counters* ctr;
  const StreamDesc* streams;  // k_chunks: seg_base turns relative candidates into offsets
};

// k_start: a run's set-up in one dispatch (it was two H2D copies, two memsets and k_init): the
// descriptors (and the streams' first strips) from kernel-visible pinned host memory into
// device memory, the counters and the LPT bucket counts zeroed, each stream's open-chunk start
// and carry state initialised.
struct StartArgs {
  const StreamDesc* src;        // the run's descriptors, pinned host memory (device address)
  const uint64_t* src_strip0;   // nstreams + 1 first strips, pinned host memory; null: none
  StreamDesc* streams;
  uint64_t* strip0;
  uint32_t nstreams;
  uint64_t* last_end;
  uint64_t* scount;
  CarryOut* carry;
  uint32_t* zero0;              // Counters (+ Early), zeroed
  uint32_t nzero0;              // words
  uint32_t* zero1;              // LPT bucket counts, zeroed
  uint32_t nzero1;              // words
  uint32_t* zero2;              // the two prefixes' status words (k_prefix1), zeroed
  uint32_t nzero2;              // words
  uint32_t* zero3;
  uint32_t nzero3;
};

struct ShaArgs {
  const uint8_t* data;
  const StreamDesc* streams;
  uint32_t nstreams;
  const uint64_t* bnd_end;
  const uint64_t* bnd_info;
  const uint64_t* last_end;
  Counters* ctr;
  ChunkRec* out;
  CarryOut* carry;
  uint64_t chunk_cap;
  uint64_t* long_list;      // [chunk_cap + nstreams] job ids for the wave-per-chunk path
  uint64_t* order;          // [chunk_cap + nstreams] per-lane jobs, longest first
  uint32_t* bucket_cnt;     // [kLptBuckets] all jobs per LPT bucket, zeroed per run
  uint32_t* bucket_elig;    // [kLptBuckets] wave-eligible jobs per bucket, zeroed per run
  uint32_t* bucket_off;     // [kLptBuckets] per-lane order offsets
  uint32_t* bucket_loff;    // [kLptBuckets] long-list offsets
  uint32_t* jinfo;          // [chunk_cap + nstreams] per job, from k_lens: nblocks | eligible
                            // << 31, or kNoJob (no job: a short open chunk carried as bytes)
  LaneJob* jdesc;           // [chunk_cap + nstreams] per job, from k_lens: what per-lane mode
                            // needs to start it without sha_setup's dependent loads
  Regions* reg;             // per-lane region queues (see Regions)
  uint8_t* oreg;            // [chunk_cap + nstreams] region of order[i] (k_order)
  uint64_t* rorder;         // [chunk_cap + nstreams] per-lane jobs by region, longest first
  uint64_t span;            // bytes from data to the end of the last stream (regions)
  int long_mode;            // 0 auto, 1 per-lane only, 2 wave mode only (experiments)
  uint32_t waves;           // waves of the k_sha grid (4 per CU)
  uint32_t seq_wait_limit;  // polls before a helper-wave handshake flags a device error
                            // (~1 s; BSG_DEBUG_SEQ_WAIT overrides it, 0: fail at once, tests)
  const uint64_t* cand;     // early chains: the sorted candidates (k_lens decodes the picks)
  Early* early;             // early chains of this run, or nullptr
};

struct BlobShaArgs {
  const uint8_t* base;
  const uint64_t* off;
  const uint64_t* len;
  uint64_t n;
  uint8_t* refs;            // [n * 32]
};

hipError_t launch_scan(const ScanArgs& a, hipStream_t s, int num_cus);
hipError_t launch_compact(const ScanArgs& a, hipStream_t s, int num_cus);
hipError_t launch_rescan(const ScanArgs& a, hipStream_t s, int num_cus);
uint64_t prefix_partials_needed(uint64_t n_bound);
hipError_t launch_prefix(const PrefixArgs& a, hipStream_t s);
hipError_t launch_select(const SelArgs& a, uint64_t cand_bound, hipStream_t s, int num_cus);
hipError_t launch_chunks(const ChunkArgs& a, uint64_t cand_bound, uint32_t nstreams, hipStream_t s,
                         int num_cus);
hipError_t launch_start(const StartArgs& a, hipStream_t s);
hipError_t launch_blob_jobs(const ChunkArgs& a, const StreamDesc* streams, uint32_t nstreams,
                            hipStream_t s, int num_cus);
hipError_t launch_sha(const ShaArgs& a, uint64_t job_bound, hipStream_t s, int num_cus);
hipError_t launch_longlist(const ShaArgs& a, uint64_t job_bound, hipStream_t s, int num_cus);
// launch_longlist in two parts for a run with a host tail: k_lens, then (after launch_tail_pick
// took the host's chunks out of jinfo) the ordering kernels
hipError_t launch_lens(const ShaArgs& a, uint64_t job_bound, hipStream_t s, int num_cus);
hipError_t launch_order(const ShaArgs& a, uint64_t job_bound, hipStream_t s, int num_cus);

// Host tail (see TailHdr). launch_tail_pick on the run's stream after k_lens; launch_tail_gather
// on a second stream after it; launch_tail_fix on the run's stream once d_refs holds the host's
// refs.
struct TailArgs {
  uint32_t* jinfo;
  const LaneJob* jdesc;
  Counters* ctr;
  uint64_t chunk_cap;
  TailHdr* hdr;
  TailItem* dlist;          // [max_items] device copy of the list
  uint64_t* dsrc;           // [max_items] the chunks' device addresses
  uint64_t* hmeta;          // pinned [kTailMetaWords]
  TailItem* hlist;          // pinned [max_items]
  uint32_t* hready;         // pinned [max_items]
  uint8_t* ring;            // pinned
  uint64_t ring_bytes;
  uint32_t max_items;
  uint32_t force_cut;       // > 0: take every job of at least this many blocks that fits
  float us_per_block;       // cost model: the GPU chain,
  float pcie_bytes_us;      //   the gather,
  float host_bytes_us;      //   all hash workers together
  float host1_bytes_us;     //   and one of them
  const uint8_t* d_refs;    // [32 * max_items]
  ChunkRec* out;
};
hipError_t launch_tail_pick(const TailArgs& a, uint64_t job_bound, hipStream_t s, int num_cus);
hipError_t launch_tail_gather(const TailArgs& a, hipStream_t s);
hipError_t launch_tail_fix(const TailArgs& a, hipStream_t s);
hipError_t launch_sha_blobs(const BlobShaArgs& a, hipStream_t s, int num_cus);
// Early chains (see Early): picked and hashed on a second stream from k_compact on (k_lens waits
// for the picks), the records' fix-up on the engine stream after k_sha (it waits for the chains).
hipError_t launch_pick(const uint64_t* cand, uint64_t cand_cap, Counters* ctr, uint32_t min_size,
                       Early* e, hipStream_t s, int num_cus);
hipError_t launch_early(const ShaArgs& a, uint32_t split_bits, hipStream_t s);
hipError_t launch_early_fix(Early* e, ChunkRec* out, Counters* ctr, hipStream_t s);
// Device -> pinned host bytes by a kernel on stream s (dst: the device alias of a hipHostMalloc
// buffer). Unlike hipMemcpyAsync D2H, a kernel waiting in its own stream for the work before
// it holds no place in the shared copy-engine queue, so it cannot stall other streams' H2D.
hipError_t launch_copy_out(const void* src, void* dst, uint64_t bytes, hipStream_t s);
hipError_t launch_fill_splitmix(uint8_t* p, uint64_t n, uint64_t seed, hipStream_t s,
                                int num_cus);

// What the engine's passes share (bsgpu_engine_common.inc). sum_parts: the u64s of `part` a
// prefix sum over n items needs. launch_ref_index: the blobs of a pool into a table of blob
// indices by ref (kDedupEmpty-filled, mask + 1 >= 2 * nblobs slots); a ref's slot ends at its
// smallest index.
uint64_t sum_parts(uint64_t n);
hipError_t launch_ref_index(const PoolBlob* blobs, uint64_t nblobs, uint64_t* tab, uint64_t mask,
                            DedupHdr* hdr, hipStream_t s, int num_cus);

// bsg_engine_trees (bsgpu_tree.inc): the records of a finished run in, the listed nodes, their
// blobs and the Roots out. Every buffer but rec / scount belongs to the tree work.
struct TreeArgs {
  const ChunkRec* rec;      // [M] the run's records, stream-major
  uint64_t M;
  const uint64_t* scount;   // [ns] chunks per stream
  uint32_t ns;
  uint32_t fanout;
  uint32_t H;               // heights of the tallest tree (after the first readback)
  uint32_t h;               // the height a per-height pass works on
  uint64_t nn;              // nodes of all streams (after the first readback)
  uint64_t arena_bytes;     // (after the second readback)
  TreeHdr* hdr;
  uint64_t* cstart;         // [ns + 1] first chunk of each stream
  uint32_t* rmax;           // [ns] Root height R, zeroed per call
  uint8_t* kcnt;            // [M] nodes chunk i closes
  uint64_t* tmp;            // [M + 1] a height's compaction ranks
  uint64_t* close;          // [nn] closing chunk by internal id
  uint64_t* shbase;         // [ns * H + 1] listed index of (stream, height)'s first node
  TreeNodeMeta* meta;       // [nn]
  uint64_t* pc;             // [M + 1] prefix of the leaf entries' bytes
  uint64_t* pn;             // [nn + 1] prefix of the node entries' bytes
  uint64_t* aoff;           // [nn + 1] arena offsets
  uint64_t* part;           // [sum_parts(n)] workgroup sums of a prefix pass
  uint8_t* arena;
  TreeNode* nodes;          // [nn] listed order
  uint8_t* roots;           // [ns * 32]
  uint64_t* ncount;         // [ns] listed nodes per stream
};
hipError_t launch_tree_count(const TreeArgs& a, hipStream_t s, int num_cus);
hipError_t launch_tree_layout(TreeArgs a, hipStream_t s, int num_cus);
hipError_t launch_tree_emit(const TreeArgs& a, uint64_t children, hipStream_t s, int num_cus);
hipError_t launch_tree_descs(const TreeArgs& a, uint64_t u0, uint32_t n, StreamDesc* d,
                             hipStream_t s, int num_cus);
hipError_t launch_tree_refs(const TreeArgs& a, uint64_t u0, uint32_t n, const ChunkRec* hashed,
                            const Counters* hctr, hipStream_t s, int num_cus);
hipError_t launch_tree_roots(const TreeArgs& a, hipStream_t s, int num_cus);

// bsg_engine_dedup / bsg_refset_add (bsgpu_dedup.inc): the first occurrence of every 32-byte ref
// among n items (a run's records, or refs a caller handed in) and in a set. Item i's ref is the
// 32 bytes at refs + i * stride (8-byte aligned); its length the u64 at lens + i * len_stride
// (null: 0). With refs2, items [n1, n) lie in a second array with the same strides, item i at
// index i - n1, its length the u32 at lens2 (bsg_engine_pool_put: the run's records, then its
// tree nodes). Nothing here writes the items.
struct DedupArgs {
  const uint8_t* refs;
  uint64_t stride;
  const uint8_t* lens;
  uint64_t len_stride;
  uint64_t n;
  const uint8_t* refs2;      // (null: one array)
  const uint8_t* lens2;
  uint64_t n1;
  uint64_t* tab;             // [tab_mask + 1] the call's own table of item indices, kDedupEmpty-filled
  uint64_t tab_mask;
  const uint8_t* set_keys;   // the set before the call (null: none): its keys, the 32 bytes at
  uint64_t set_stride;       //   set_keys + k * set_stride,
  const uint64_t* set_tab;   // and its table of key indices
  uint64_t set_mask;
  uint64_t set_count;
  uint64_t* first;           // [n] smallest index with the same ref | kDedupInSet
  uint64_t* rank;            // [n + 1] exclusive prefix of "item i is new"
  uint64_t* bpre;            // [n + 1] exclusive prefix of the new items' lengths
  uint64_t* uniq;            // [nunique] the new items, ascending
  uint64_t* pack_off;        // [nunique + 1] exclusive prefix of their lengths
  uint64_t* part;            // [sum_parts(n)] workgroup sums of a prefix pass
  DedupHdr* hdr;
};
hipError_t launch_dedup(const DedupArgs& a, hipStream_t s, int num_cus);

// A set's table and key array. launch_set_rehash: every key index [0, count) into the
// (kDedupEmpty-filled) table. launch_set_add: the m new items uniq[0 .. m) of `d` become keys
// [count, count + m) and enter the table; they are distinct from each other and from every key
// of the set (launch_dedup's result), so no key is compared.
struct SetArgs {
  uint8_t* keys;
  uint64_t* tab;
  uint64_t mask;
  uint64_t count;
  DedupHdr* hdr;
};
hipError_t launch_set_rehash(const SetArgs& a, hipStream_t s, int num_cus);
hipError_t launch_set_add(const SetArgs& a, const DedupArgs& d, uint64_t m, hipStream_t s,
                          int num_cus);

// bsg_engine_pack_unique: out[pack_off[k] .. pack_off[k + 1]) = the bytes of record uniq[k],
// data + streams[rec.stream].data_off + rec.offset. out is 16-byte aligned; nothing outside
// [out, out + total) is written. funnel: aligned 16-byte loads and a byte shift instead of
// unaligned 16-byte loads.
struct PackArgs {
  const uint8_t* data;
  const StreamDesc* streams;
  uint32_t nstreams;
  const ChunkRec* rec;
  uint64_t nrec;
  const uint64_t* uniq;
  const uint64_t* pack_off;
  uint64_t nunique;
  uint64_t total;
  uint8_t* out;
  DedupHdr* hdr;
};
hipError_t launch_pack(const PackArgs& a, bool funnel, hipStream_t s);

// bsg_engine_restore (bsgpu_restore.inc): records name pool blobs by ref; every stream's bytes
// are written to out + out_off[stream]. blobs .. tpre are one upload; tab, seg, sfirst and slast
// belong to the call (tab, sfirst and slast 0xFF-filled, hdr initialised by the caller).
struct RestoreArgs {
  const uint8_t* pool;
  uint64_t pool_bytes;
  const PoolBlob* blobs;
  uint64_t nblobs;
  const ChunkRec* rec;
  uint64_t nrec;
  const uint64_t* out_off;   // [ns]
  const uint64_t* out_len;   // [ns]
  const uint64_t* tpre;      // [ns + 1] exclusive prefix of the streams' output tiles
  uint32_t ns;
  uint64_t* tab;             // [tab_mask + 1] blob indices by ref
  uint64_t tab_mask;
  uint64_t* seg;             // [nrec] pool offset of each record's blob
  uint64_t* sfirst;          // [ns] a stream's first record (~0: none)
  uint64_t* slast;           // [ns] and its last
  uint8_t* out;
  RestoreHdr* hdr;
  // bsg_engine_read (null: none): stream s's output is bytes [win0[s], win0[s] + out_len[s]) of
  // the stream, and its records are the chunks under them, with their own offsets and whole lens
  const uint64_t* win0;      // [ns]
  uint8_t* touched;          // [nblobs] set for every blob a record resolves to
};
// the index of the pool's refs (index: built here into a.tab; else a.tab holds it already), every
// record resolved against it, the records' tiling checked
hipError_t launch_restore_resolve(const RestoreArgs& a, bool index, hipStream_t s, int num_cus);
// blobs [b0, b0 + n) as the descriptors of a hash run, and that run's records against their refs
hipError_t launch_restore_descs(const RestoreArgs& a, uint64_t b0, uint32_t n, StreamDesc* d,
                                hipStream_t s, int num_cus);
hipError_t launch_restore_compare(const RestoreArgs& a, uint64_t b0, uint32_t n,
                                  const ChunkRec* hashed, const Counters* hctr, hipStream_t s,
                                  int num_cus);
// tiles: tpre[ns] (one workgroup per tile)
hipError_t launch_restore_scatter(const RestoreArgs& a, uint64_t tiles, hipStream_t s);

// bsg_engine_walk (bsgpu_walk.inc): from one Root per stream down a pool's node blobs to the
// streams' sizes and records. pool .. status describe the call; level .. nnext the level a pass
// works on; the rest the placement passes. Everything but the pool belongs to the call.
struct WalkArgs {
  const uint8_t* pool;
  uint64_t pool_bytes;
  const PoolBlob* blobs;
  uint64_t nblobs;
  const uint8_t* roots;      // [ns * 32]
  uint32_t ns;
  uint64_t* tab;             // [tab_mask + 1] blob indices by ref
  uint64_t tab_mask;
  WalkHdr* hdr;
  uint64_t* sizes;           // [ns] the Root node's size, zeroed per call
  uint32_t* status;          // [ns] kWalkCorrupt / kWalkNotFound, zeroed per call
  uint32_t level;
  uint32_t last;             // 1: the level's `nodes` children would be deeper than kWalkMaxDepth
  uint64_t n;                // the level's frontier entries
  WalkItem* items;           // [n]
  WalkNode* nodes;           // [n]
  uint64_t* call;            // [n + 1] exclusive prefix of the nodes' children
  uint64_t* cnode;           // [n + 1] ... of their `nodes` children: places in the next frontier
  uint64_t* prec;            // [n + 1] ... of the records below them
  uint64_t nchild;           // k_wk_emit: the level's children; k_wk_records: its `leaves` children
  WalkItem* next;            // [nnext] the next level's frontier
  uint64_t nnext;
  const uint64_t* down_prec; // [down_n + 1] prec of the level below (null: none)
  uint64_t down_n;
  const WalkNode* up_nodes;  // [up_n] the level above
  const uint64_t* up_cnode;
  uint64_t up_n;
  uint64_t* part;            // [sum_parts(n)] workgroup sums of a prefix pass
  ChunkRec* rec;             // [nrec] the result
  uint64_t nrec;
  // bsg_engine_read (null: none): per-stream windows, and what the pruned walk keeps of them
  const uint64_t* win;       // [2 * ns] stream s follows a child iff its cover has a byte in
                             //   [win[2s], win[2s + 1])
  uint8_t* touched;          // [nblobs] set for every Root and followed `nodes` child found
  uint64_t* lfirst;          // [n] a leaf node's first followed child
  uint64_t* lpre;            // [n + 1] exclusive prefix of the leaf nodes' followed children
};
hipError_t launch_walk_roots(const WalkArgs& a, hipStream_t s, int num_cus);
// validate and count the level's nodes, then call and cnode
hipError_t launch_walk_count(const WalkArgs& a, hipStream_t s, int num_cus);
// one thread per child: the next frontier, the leaves held to their covers
hipError_t launch_walk_emit(const WalkArgs& a, hipStream_t s, int num_cus);
// placement: the records below each node (bottom-up), then each node's first record and the
// level's records (top-down)
hipError_t launch_walk_nrec(const WalkArgs& a, hipStream_t s, int num_cus);
hipError_t launch_walk_place(const WalkArgs& a, hipStream_t s, int num_cus);

// bsg_engine_gc_mark / bsg_engine_gc_compact (bsgpu_gc.inc). w is the walk's block for the pool,
// its index, the level at hand and the count pass (w.hdr = &g->w, w.ns = 1 with w.sizes and
// w.status at g's spare words; every frontier entry is kWalkNoCover). Everything but the pool and
// the compaction's output belongs to the mark.
struct GcArgs {
  WalkArgs w;
  GcHdr* g;
  const uint8_t* roots;      // [nroots * 32]
  uint64_t nroots;
  uint64_t* rblob;           // [nroots] a Root's blob, or kWalkDead
  uint32_t* rstatus;         // [nroots] kWalkCorrupt / kWalkNotFound
  uint32_t forgive;          // BSG_GC_MISSING_LEAVES
  uint8_t* live;             // [nblobs] zeroed per mark
  uint32_t* state;           // [nblobs] kGcClaimed | kGcFailed, zeroed per mark
  uint64_t* rank;            // [nblobs + 1] exclusive prefix of live
  uint64_t* noff;            // [nblobs + 1] ... of the live blobs' lens: the new offsets
  uint64_t* noff16;          // [nblobs + 1] ... each len rounded up to 16
  uint64_t* part;            // [sum_parts(nblobs)] workgroup sums of a prefix pass
  uint64_t* mtab;            // k_gc_missing: pool offsets of missing `leaves` refs, by ref
  uint64_t mmask;
  const uint64_t* coff;      // k_gc_compact: noff or noff16
  uint64_t total;            //   the output's bytes
  uint8_t* out;
};
hipError_t launch_gc_roots(const GcArgs& a, hipStream_t s, int num_cus);
// after launch_walk_count(a.w): the failed nodes' verdicts, then one thread per child
hipError_t launch_gc_emit(const GcArgs& a, hipStream_t s, int num_cus);
hipError_t launch_gc_status(const GcArgs& a, hipStream_t s, int num_cus);
// the level's `leaves` children once more: the distinct refs the pool lacks (a.w.nchild children)
hipError_t launch_gc_missing(const GcArgs& a, hipStream_t s, int num_cus);
hipError_t launch_gc_offsets(const GcArgs& a, hipStream_t s, int num_cus);
hipError_t launch_gc_compact(const GcArgs& a, hipStream_t s);

// bsg_engine_pool_put (bsgpu_pool.inc). d is the first-occurrence pass over the items (the run's
// records, then with refs2 its tree nodes; d.set_* the pool's index before the call, d.hdr =
// &hdr->dd). data .. arena_bytes say where an item's bytes lie, off16 and seg16 belong to the
// call, bytes .. where to the pool. launch_pool_plan writes the call's buffers and the header only;
// nnew and total16 are the header's, read back, before anything of the pool is written.
struct PoolArgs {
  DedupArgs d;
  PoolHdr* hdr;
  const uint8_t* data;       // the run's input and stream descriptors (records' bytes)
  const StreamDesc* streams;
  uint32_t nstreams;
  const ChunkRec* rec;       // [d.n1]
  const TreeNode* nodes;     // [d.n - d.n1]
  const uint8_t* arena;      // the nodes' blobs
  uint64_t arena_bytes;
  uint64_t* off16;           // [d.n + 1] exclusive prefix of the new items' lens rounded up to 16
  uint64_t* seg16;           // [nnew + 1] the same by rank: new blob k's bytes and padding
  uint8_t* bytes;            // the pool
  PoolBlob* table;
  uint64_t* index;           // [index_mask + 1] blob indices by ref
  uint64_t index_mask;
  uint64_t nblobs;           // table entries before the call
  uint64_t base;             // where the first new blob starts (a multiple of 16)
  uint64_t nnew;
  uint64_t total16;
  uint64_t* where;           // [d.n]
};
// after launch_dedup(a.d): off16, seg16 and the header's totals
hipError_t launch_pool_plan(const PoolArgs& a, hipStream_t s, int num_cus);
// the new table entries and their index slots; the new blobs' bytes and padding
hipError_t launch_pool_append(const PoolArgs& a, hipStream_t s, int num_cus);
hipError_t launch_pool_gather(const PoolArgs& a, hipStream_t s);
// where[i]: the blob that carries item i's ref, among nblobs + nnew
hipError_t launch_pool_where(const PoolArgs& a, hipStream_t s, int num_cus);

// bsg_pool_collect (bsgpu_pool.inc): src .. noff16 are a finished mark of the source pool (GcArgs),
// table .. remap belong to the destination, an empty pool whose capacity the host has held nlive
// and total to. Live blob k becomes entry rank[k] = {noff16[k], len, ref} and enters the index;
// remap[k] is that entry, or ~0 for a dead blob. The bytes are launch_gc_compact's.
struct AdoptArgs {
  const PoolBlob* src;       // [n] the source's table
  uint64_t n;
  const uint8_t* live;       // [n]
  const uint64_t* rank;      // [n + 1]
  const uint64_t* noff16;    // [n + 1]
  uint64_t nlive;            // rank[n]
  uint64_t total;            // the mark's end16
  PoolBlob* table;           // [>= nlive]
  uint64_t* index;           // [index_mask + 1] blob indices by ref, kDedupEmpty-filled
  uint64_t index_mask;
  uint64_t* remap;           // [n]
  DedupHdr* hdr;
};
hipError_t launch_pool_adopt(const AdoptArgs& a, hipStream_t s, int num_cus);

// bsg_pool_merge / bsg_pool_sync (bsgpu_pool.inc): the selected blobs of a source pool that the
// destination's index does not hold, appended behind what the destination holds. src .. index_mask
// are the two pools as they stand, isnew .. hdr belong to the call; launch_pool_probe and
// launch_pool_merge_plan write those alone and read nothing from nnew on. nnew and need_bytes are
// known after the host has read the totals back; launch_pool_merge_append runs only once it has
// held them to the destination's capacity. New blob k becomes entry dn + rank[k] =
// {base + off16[k], len, ref} and enters the index; remap[k] is the destination's entry under k's
// ref, or ~0 for an unselected blob. The bytes are launch_gc_compact's, with isnew as its live[],
// off16 as its offsets and the destination's bytes + base as its output.
struct MergeArgs {
  const PoolBlob* src;       // [n] the source's table
  uint64_t n;
  const uint8_t* sel;        // [n] a mark's live[] (null: every blob is selected)
  const PoolBlob* dtable;    // [dn] the destination's table before the call
  uint64_t dn;
  uint64_t* index;           // [index_mask + 1] the destination's blob indices by ref
  uint64_t index_mask;
  uint8_t* isnew;            // [n] selected, and the destination lacks its ref
  uint64_t* rank;            // [n + 1] exclusive prefix of isnew
  uint64_t* off16;           // [n + 1] ... of the new blobs' lens rounded up to 16
  uint64_t* part;            // [sum_parts(n)] workgroup sums of a prefix pass
  uint64_t* remap;           // [n]
  MergeHdr* hdr;
  uint64_t nnew;             // rank[n]
  uint64_t base;             // where the first new blob starts (a multiple of 16)
  uint64_t need_bytes;       // the end of the last new blob's bytes, in the destination
  uint64_t cap_blobs;        // the destination's table entries
  PoolBlob* table;           // the destination's table
};
// every selected blob probed in the destination's index: remap, isnew and the header's counts
hipError_t launch_pool_probe(const MergeArgs& a, hipStream_t s, int num_cus);
// rank and off16 over the source's blobs, then the end of the last new blob's bytes
hipError_t launch_pool_merge_plan(const MergeArgs& a, hipStream_t s, int num_cus);
// the new table entries, their index slots and their remap entries
hipError_t launch_pool_merge_append(const MergeArgs& a, hipStream_t s, int num_cus);

// bsg_engine_read (bsgpu_read.inc): byte ranges of streams out of a pool. The walk is
// bsg_engine_walk's with WalkArgs::win set (launch_walk_roots / _count / _emit), the scatter
// bsg_engine_restore's with RestoreArgs::win0 set (launch_restore_scatter); what lies between is here.
// placement, bottom-up: a leaf node's run of followed children and the records below every node
hipError_t launch_read_nrec(const WalkArgs& a, hipStream_t s, int num_cus);
// top-down: every node's first record, then the followed leaf children's records (leaf_bound:
// the level's `leaves` children, at least as many)
hipError_t launch_read_place(const WalkArgs& a, uint64_t leaf_bound, hipStream_t s, int num_cus);
// every record resolved and its blob touched; each stream's run held to cover its window
hipError_t launch_read_resolve(const RestoreArgs& a, hipStream_t s, int num_cus);
// The touched blobs (BSG_READ_VERIFY). tpre [nblobs + 1]: the exclusive prefix of touched; tlist
// [tpre[nblobs]]: their indices, ascending; each is held to the hash path's layout rules
// (RestoreHdr::invalid) and its len added to *verified.
struct TouchArgs {
  RestoreArgs r;
  uint64_t* tpre;
  uint64_t* tlist;
  uint64_t ntouched;         // tpre[nblobs], read back (the hash batches)
  uint64_t* verified;
  uint64_t* part;            // [sum_parts(nblobs)]
};
hipError_t launch_read_touched(const TouchArgs& a, hipStream_t s, int num_cus);
// touched blobs tlist[t0 .. t0 + n) as the descriptors of a hash run, and that run's records
// against their refs (RestoreHdr::bad_blob: the smallest blob index that fails)
hipError_t launch_read_descs(const TouchArgs& a, uint64_t t0, uint32_t n, StreamDesc* d,
                             hipStream_t s, int num_cus);
hipError_t launch_read_compare(const TouchArgs& a, uint64_t t0, uint32_t n, const ChunkRec* hashed,
                               const Counters* hctr, hipStream_t s, int num_cus);

// bsg_pool_put_blobs (bsgpu_blobs.inc): bsg_engine_pool_put with blobs of the caller's in the place
// of records and nodes. p is the put's block with p.d over refs (stride 32) and the spans' lens
// (stride 16); p.data .. p.arena_bytes are unused. span, src, src_bytes and refs belong to the call:
// every span lies in [0, src_bytes), held to that by the host before the upload and by every kernel
// that forms an address from one.
struct BlobPutArgs {
  PoolArgs p;
  const BlobSpan* span;      // [p.d.n]
  const uint8_t* src;
  uint64_t src_bytes;        // the end of the last blob's last byte
  uint8_t* refs;             // [p.d.n * 32] the hash runs' refs
};
// blobs [b0, b0 + n) as the descriptors of a hash run, and that run's refs into refs[]
hipError_t launch_blob_descs(const BlobPutArgs& a, uint64_t b0, uint32_t n, StreamDesc* d,
                             hipStream_t s, int num_cus);
hipError_t launch_blob_refs(const BlobPutArgs& a, uint64_t b0, uint32_t n, const ChunkRec* hashed,
                            const Counters* hctr, hipStream_t s, int num_cus);
// launch_pool_gather for the blobs: new blob k's bytes are item p.d.uniq[k]'s span of src
hipError_t launch_pool_gather_blobs(const BlobPutArgs& a, hipStream_t s);

// bsg_pool_get (bsgpu_blobs.inc): n refs probed in a pool's index, the found blobs' bytes gathered
// in request order, each rounded up to 16 with zero padding. pool .. index_mask are the pool as it
// stands and are only read; refs .. hdr belong to the call. launch_get_probe writes idx, out_off,
// touched and the header; total is out_off[n], read back and held to the output's capacity before
// launch_get_gather writes out[0 .. total).
struct GetArgs {
  const uint8_t* pool;
  uint64_t pool_bytes;
  const PoolBlob* table;
  uint64_t nblobs;
  const uint64_t* index;     // [index_mask + 1] blob indices by ref
  uint64_t index_mask;
  const uint8_t* refs;       // [n * 32]
  uint64_t n;
  uint64_t* idx;             // [n] request q's blob, or kDedupEmpty
  uint64_t* out_off;         // [n + 1] exclusive prefix of the found blobs' lens rounded up to 16
  uint64_t* part;            // [sum_parts(n)] workgroup sums of the prefix pass
  uint8_t* touched;          // [nblobs] set for every found blob (null: not wanted)
  GetHdr* hdr;
  uint64_t total;
  uint8_t* out;
};
hipError_t launch_get_probe(const GetArgs& a, hipStream_t s, int num_cus);
hipError_t launch_get_gather(const GetArgs& a, hipStream_t s);

}  // namespace bsg
