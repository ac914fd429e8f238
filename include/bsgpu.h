/*
 * bsgpu.h — C ABI of libbsgpu, the MI355X (gfx950) ingest path for BS's hashsplit chunker and
 * SHA-256 blob refs. Plain pointers and sizes only; no C++ exceptions cross this boundary.
 *
 * Reference interfaces replaced (paths relative to the bobg/bs tree):
 *   bsg_open / bsg_write / bsg_close / bsg_drain
 *       -> split.NewWriter(ctx, st, opts...)            split/split.go:44-96
 *          (*split.Writer).Write([]byte) (int, error)   split/split.go:99-101
 *          (*split.Writer).Close() error                split/split.go:104-126
 *          options Bits / MinSize / Fanout               split/split.go:137,148,161
 *       The per-byte loop they replace is hashsplit.Splitter.Write/Close (github.com/bobg/hashsplit
 *       v1.1.1, go.mod:9) with buzhash32 (github.com/chmduquesne/rollinghash v4.0.0, go.sum:61-62).
 *       The chunk records carry the ref that st.Put would compute (split/split.go:72 ->
 *       store/mem/mem.go:67 -> bs.go:24-26); the caller still calls its own Store.Put.
 *   bsg_sha256_batch
 *       -> bs.Blob.Ref() = sha256.Sum256(b)              bs.go:24-26 (many blobs at once)
 *   bsg_engine_* (device-resident batch of independent streams)
 *       -> N concurrent split.Writers, e.g. fs.Dir.AddDir's per-file writers (fs/dir.go:157-174)
 *
 * Threading: one bsg_ctx / bsg_engine per thread at a time; different contexts are
 * independent (each owns a HIP stream) and may run concurrently. Every entry point makes the
 * context's device current (hipSetDevice) so callers may migrate between OS threads.
 *
 * Errors: functions return BSG_OK (0) or a negative code; bsg_errstr() describes it.
 */
#ifndef BSGPU_H
#define BSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSG_OK 0
#define BSG_EINVAL (-22)   /* bad argument (null pointer, unaligned stream offset, ...) */
#define BSG_ENOMEM (-12)   /* host or device allocation failed */
#define BSG_EDEVICE (-5)   /* HIP runtime / kernel error */
#define BSG_ESTATE (-71)   /* Write after Close, etc. */
#define BSG_ENODEV (-19)   /* no such HIP device */
#define BSG_ENOTFOUND (-2) /* bs.ErrNotFound (store.go:63) */
#define BSG_ECORRUPT (-74) /* a fetched blob does not hash to its ref (reader verify) */
#define BSG_EIO (-1001)    /* filesystem error (store/file) */

/* split.Writer options. Zero fields take hashsplit's own defaults (SplitBits 13, MinSize 64);
 * bsg_params_default() gives split.NewWriter's defaults (16 / 1024 / fanout 8,
 * split/split.go:48,88-89). Like split.Bits / split.MinSize (split/split.go:137-152, which
 * store the value unchecked), every value is accepted: MinSize 1..63 lets the 64-byte window
 * span a boundary (allowed, only discouraged by split.go:146), and Bits > 32 never splits
 * (TrailingZeros32 is at most 32), so the whole stream is one final chunk of level 0. A cgo
 * caller maps MinSize(n <= 0) to 0 (hashsplit's default) and clamps Bits to 2^32-1. */
typedef struct bsg_params {
  uint32_t split_bits; /* Bits(n): trailing zero bits for a boundary (0 = 13) */
  uint32_t min_size;   /* MinSize(n): minimum chunk size (0 = 64) */
  uint32_t fanout;     /* Fanout(n): tree level divisor (Writer, bsg_engine_trees; 0 = 8) */
  uint32_t reserved;
} bsg_params;

/* One chunk: the bytes [offset, offset+len) of a stream, its hashsplit level (trailing zeros
 * minus split_bits, NOT yet divided by fanout; split/split.go:86 divides) and its ref. */
typedef struct bsg_chunk {
  uint64_t offset;
  uint64_t len;
  uint32_t level;
  uint32_t stream;
  uint8_t ref[32];
} bsg_chunk; /* 56 bytes */

const char* bsg_errstr(int err);
bsg_params bsg_params_default(void);
/* The buzhash32 table used when callers pass table == NULL: rollinghash's GenerateHashes(1). */
void bsg_default_table(uint32_t out[256]);
int bsg_device_count(void);
/* Optional, once per process: makes `device` current, creates its HIP context and a few HIP
 * streams (kept in the library's stream pool), initialises the copy engines, loads every kernel
 * of the split and hash paths (one tiny split and hash) and starts the host copy threads — the
 * one-time cost (~50 ms) that the first Writer of a process pays otherwise. A server calls it
 * at start-up. */
int bsg_init(int device);

/* ---- streaming split.Writer (bytes arrive from host memory) ---- */
typedef struct bsg_ctx bsg_ctx;
bsg_ctx* bsg_open(int device, const bsg_params* params, const uint32_t* table /* 256 or NULL */,
                  int* err);
/* Copies p[0..n) into pinned staging (the caller keeps ownership of p); full tiles are split
 * and hashed on the device as they fill. A stream has no length limit, as split.Writer.Write
 * (split/split.go:99-101): stream offsets are 64-bit throughout; only positions inside one
 * device tile (< 2^40 bytes of device memory) travel in 40-bit fields. */
int bsg_write(bsg_ctx* ctx, const uint8_t* p, size_t n);
/* Zero-copy Write: *p / *cap = the free rest of the current pinned staging buffer (at most
 * 64 MiB and never more than the rest of the tile; a stream's first buffer grows from 4 MiB,
 * so early windows are smaller); the caller fills up to *cap bytes there (e.g. an io.Reader
 * reads straight into it) and commits n of them. Same stream semantics as bsg_write; the
 * window is valid until the next call on ctx. */
int bsg_write_window(bsg_ctx* ctx, uint8_t** p, size_t* cap);
int bsg_write_commit(bsg_ctx* ctx, size_t n);
/* Page-locks host memory the caller owns (hipHostRegister) so that bsg_write_pinned can copy
 * from it to the device without a staging copy; bsg_host_unregister undoes it. */
int bsg_host_register(void* p, size_t n);
int bsg_host_unregister(void* p);
/* bsg_write from memory registered with bsg_host_register: the H2D reads p[0..n) directly and
 * asynchronously, so the caller keeps those bytes unchanged and registered until the chunks
 * covering them have been drained (at the latest, until bsg_close / bsg_reset returns). Same
 * stream semantics as bsg_write. */
int bsg_write_pinned(bsg_ctx* ctx, const uint8_t* p, size_t n);
/* Flushes the final chunk (hashsplit Splitter.Close). Idempotent. */
int bsg_close(bsg_ctx* ctx);
/* bsg_close in steps, so that a caller can Put the chunks of earlier tiles while the last ones
 * finish: bsg_close_begin submits the final segment without waiting (the stream is closed);
 * each bsg_close_step waits for the oldest tile still on the device and makes its chunks
 * drainable, storing the number of tiles still on the device in *left (0: as after bsg_close). */
int bsg_close_begin(bsg_ctx* ctx);
int bsg_close_step(bsg_ctx* ctx, size_t* left);
/* Number of finished chunks not yet drained, and drain up to cap of them (stream order). */
size_t bsg_pending(const bsg_ctx* ctx);
size_t bsg_drain(bsg_ctx* ctx, bsg_chunk* out, size_t cap);
/* Device tile size in bytes (default 256 MiB); call before the first write. Three tiles are
 * processed at once (BSG_STREAM_SLOTS overrides): tile i+1's split starts as soon as tile i's
 * boundaries are known, while tile i's SHA-256 is still running. Host bytes pass through a
 * ring of four pinned staging buffers of min(tile, 64 MiB), each copied to the device as soon
 * as it is full, into one of four device data slots (BSG_DATA_SLOTS). */
int bsg_set_tile(bsg_ctx* ctx, size_t tile_bytes);
/* Longest open chunk carried between tiles as bytes on the device (default 8 MiB); a longer
 * one is carried as a SHA-256 midstate, which makes the next tile wait for this tile's hashes.
 * 0 = always midstate (tests). Call before the first write. */
int bsg_set_carry_cap(bsg_ctx* ctx, size_t bytes);
/* Tests: the stream's first byte has stream offset `base` (records carry offsets from it, the
 * split is unchanged), so that offsets past 2^40 can be exercised without writing 1 TiB. Call
 * before the first write; bsg_reset goes back to 0. */
int bsg_set_stream_base(bsg_ctx* ctx, uint64_t base);
/* Start a new stream on the same context (its device and pinned buffers are kept), as a
 * pool of split.Writers would; undrained chunks of the previous stream are discarded. */
int bsg_reset(bsg_ctx* ctx);
void bsg_free(bsg_ctx* ctx);
/* Where a stream's host-to-device time went, since bsg_open / the last bsg_reset (a diagnostic:
 * an io.Copy into split.Writer is bound by the host copy, the PCIe copy or the device). Waits
 * for the context's copy stream. */
typedef struct bsg_stream_stats {
  uint64_t host_bytes;         /* bytes bsg_write copied into pinned staging */
  uint64_t host_copy_ns;       /* wall time of those copies (all copy threads together) */
  uint64_t stage_wait_ns;      /* time Writes waited for a stage's previous H2D copy */
  uint64_t h2d_bytes;          /* bytes copied host-to-device from the stages */
  uint64_t h2d_copies;         /* number of those copies */
  uint64_t h2d_busy_ns;        /* sum of their durations (HIP events on the copy stream) */
  uint64_t h2d_span_ns;        /* the first one's start to the last one's end */
  uint64_t copy_bytes_node[4]; /* host copy bytes by NUMA node of the copying thread's CPU */
  uint64_t last_tile_ns;       /* the final tile's kernels on the device (bsg_close's tail) */
  uint64_t tail_ns;            /* the last H2D copy's end to the final tile's records in host
                                * memory */
  int32_t gpu_node;            /* NUMA node of the device (sysfs; -1 unknown) */
  uint32_t stage_nodes;        /* bit mask of the NUMA nodes the pinned stages' pages are on */
  uint32_t src_nodes;          /* bit mask of the nodes of the Write sources' first pages */
  uint32_t copy_nt;            /* 1: the copies used non-temporal stores */
} bsg_stream_stats;
int bsg_stream_stats_get(bsg_ctx* ctx, bsg_stream_stats* out);

/* ---- device-resident batch of independent streams ---- */
typedef struct bsg_engine bsg_engine;
bsg_engine* bsg_engine_create(int device, const uint32_t* table /* 256 or NULL */, int* err);
void bsg_engine_destroy(bsg_engine* eng);
/* Enqueue split + hash of nstreams streams d_data[off[i] .. off[i]+len[i]) (device memory;
 * off/len are host arrays; at most 65,535 streams of < 2^40 bytes each, a device-memory bound:
 * one stream of a run lies whole in device memory).
 * Layout: d_data and every off[i] are multiples of 16 (d_data is the address the kernels load
 * from, so a base such as allocation + 4 is refused; allocation + 16 is fine). The streams may
 * lie in any order, with gaps of any size between them, and may overlap or coincide (two
 * streams on the same bytes, one a prefix or an inner part of another): each stream's records
 * depend on its own bytes alone, never on the bytes around it. A zero-length stream's off[i]
 * still counts for the allocation check below. BSG_EINVAL, before anything is enqueued, for an
 * unaligned d_data or off[i], a len[i] >= 2^40, an off[i] + len[i] that wraps, or streams that
 * leave less than BSG_READ_SLACK bytes of the allocation after them.
 * Asynchronous on the engine's stream (a run of >= 256 MiB hashes its two longest chunks on a
 * second pooled stream, which the engine's stream waits for before the run completes; see
 * BSG_KNOB_EARLY).
 * The allocation holding d_data must extend at least BSG_READ_SLACK bytes past the end of the
 * last stream (the SHA-256 loader reads whole 64-byte blocks and masks the excess). */
#define BSG_READ_SLACK 256
int bsg_engine_run(bsg_engine* eng, const uint8_t* d_data, const uint64_t* off,
                   const uint64_t* len, uint32_t nstreams, const bsg_params* params);
/* Enqueue SHA-256 of nblobs whole blobs d_data[off[i] .. off[i]+len[i]) (bs.Blob.Ref,
 * bs.go:24-26, for many blobs at once: the read-side verification of split.Reader, a store's
 * batched Puts): same constraints and the same layout freedom as bsg_engine_run (device memory,
 * d_data and every off[i] multiples of 16, any order, gaps, overlapping or coinciding blobs, at
 * most 65,535 blobs, BSG_READ_SLACK readable bytes after the last); no splitting, record i (after
 * bsg_engine_finish) carries blob i's ref, offset 0 and len[i]. Asynchronous. */
int bsg_engine_hash(bsg_engine* eng, const uint8_t* d_data, const uint64_t* off,
                    const uint64_t* len, uint32_t nblobs);
/* Wait for the run; handles candidate-buffer growth (re-runs once if needed). Returns the
 * total chunk count in *nchunks. */
int bsg_engine_finish(bsg_engine* eng, uint64_t* nchunks);
/* Device pointer to the run's chunk records (stream-major, offset order); valid until the
 * next run. */
const bsg_chunk* bsg_engine_chunks_device(const bsg_engine* eng);
/* Copy records / per-stream counts to host. */
int bsg_engine_copy_chunks(bsg_engine* eng, bsg_chunk* out, uint64_t cap);
int bsg_engine_copy_counts(bsg_engine* eng, uint64_t* counts, uint32_t nstreams);
/* The engine's HIP stream (hipStream_t), e.g. for event timing. */
void* bsg_engine_stream(bsg_engine* eng);
/* ---- split.Writer's tree and Root per stream of a run, built on the device ---- */
/* One split.Node blob of a stream's tree (split/split.proto:6-26), as PutProto would store it. */
typedef struct bsg_tree_node {
  uint64_t blob_off;   /* its serialized bytes: arena[blob_off .. blob_off + blob_len) */
  uint32_t blob_len;
  uint32_t stream;
  uint32_t height;     /* 0: a node of leaves (chunks); h: its children are nodes of height h-1 */
  uint32_t reserved;
  uint8_t ref[32];     /* SHA-256 of the blob */
} bsg_tree_node;       /* 56 bytes */
/* Builds, on the device, split.Writer's tree for every stream of the last finished
 * bsg_engine_run (fanout = that run's params.fanout, 0 = 8): TreeBuilder.Add(chunk, level/fanout)
 * per record, TreeBuilder.Root's fold of every non-empty level, the single-child prune, and
 * PutProto's ref of every node (split/split.go:51-126). Waits for completion. *nnodes /
 * *arena_bytes: totals (blobs start 16-byte aligned in the arena, the gaps are zero).
 * The node list holds exactly the blobs reachable from each stream's Root, the Root's own blob
 * included, stream-major, then height ascending, then stream offset ascending: a stream's last
 * node is its Root, and a caller that stores the nodes in list order with PutWithRef, after the
 * chunks, never stores a node before what it points to (split/split.go:71-77). When the
 * would-be root is pruned, split.Writer has also stored the single-child nodes it pruned
 * through; nothing references them and they are NOT listed.
 * BSG_EINVAL for null arguments; BSG_ESTATE unless the engine's last enqueue was a
 * bsg_engine_run that bsg_engine_finish completed successfully (not: no run, a bsg_engine_hash
 * run, an unfinished or failed run). Calling it twice on one run gives the same result. */
int bsg_engine_trees(bsg_engine* eng, uint64_t* nnodes, uint64_t* arena_bytes);
/* Root per stream (32 bytes each; all zero for an empty stream, bs.Zero) and, if node_counts is
 * not NULL, the number of nodes per stream. nstreams may be smaller than the run's: the first
 * nstreams streams are written and nothing past them; larger is BSG_EINVAL. BSG_ESTATE without
 * a tree (as the device pointers below are NULL). */
int bsg_engine_copy_roots(bsg_engine* eng, uint8_t* roots, uint64_t* node_counts, uint32_t nstreams);
/* Node records (up to cap) and the blob arena (up to arena_cap bytes) to host memory. */
int bsg_engine_copy_tree_nodes(bsg_engine* eng, bsg_tree_node* out, uint64_t cap,
                               uint8_t* arena, uint64_t arena_cap);
/* Device pointers, valid until the next run or the next bsg_engine_trees (NULL without a tree). */
const bsg_tree_node* bsg_engine_tree_nodes_device(const bsg_engine* eng);
const uint8_t* bsg_engine_tree_arena_device(const bsg_engine* eng);
const uint8_t* bsg_engine_roots_device(const bsg_engine* eng);

/* ---- which chunks of a run are new: Store.Put's `added`, decided on the device ---- */
/* A store keeps one blob per ref (store/mem/mem.go:62-77 drops a blob it has and returns
 * added = false). A bsg_refset is that knowledge kept in device memory across runs: a set of
 * 32-byte refs that only grows. A store seeds it once from ListRefs with bsg_refset_add and then
 * passes it to every bsg_engine_dedup. BSG_ENODEV (NULL) for a device that does not exist. */
typedef struct bsg_refset bsg_refset;
bsg_refset* bsg_refset_new(int device, int* err);
void bsg_refset_free(bsg_refset* s);
/* Refs in the set (0 for NULL). */
uint64_t bsg_refset_count(const bsg_refset* s);
/* Adds n refs (host memory, 32 bytes each). added (n bytes, or NULL): added[i] = 1 iff ref i was
 * not in the set and is not an earlier entry of this call. Synchronous. The set grows by
 * doubling, rehashed on the device, before an insert would pass its load limit; a failed
 * allocation returns BSG_ENOMEM and leaves the set unchanged. After a device error the set is
 * unusable: this call and every later one on it return BSG_ESTATE. BSG_EINVAL for a null set,
 * or null refs with n > 0.
 * Threading: a set carries its own mutex; engines on several threads may share one set, their
 * calls on it (this one, bsg_engine_dedup with the set) serialize. */
int bsg_refset_add(bsg_refset* s, const uint8_t* refs /* host, n x 32 */, uint64_t n,
                   uint8_t* added /* host, n bytes, or NULL */);

/* First occurrence per ref over the records r[0 .. n) of the last finished bsg_engine_run
 * (stream-major, as bsg_engine_chunks_device), on the device. Synchronous, on the engine's
 * stream. It leaves in device memory, valid until the next run or the next bsg_engine_dedup on
 * this engine:
 *   first[i]    (n entries) the smallest j with r[j].ref == r[i].ref; bit 63 is set if the ref
 *               was in `set` before this call. Record i is NEW iff first[i] == i, bit 63 clear.
 *   uniq[k]     (*nunique entries) the indices of the new records, ascending.
 *   pack_off[k] (*nunique + 1 entries) the exclusive prefix sum of the new records' len;
 *               pack_off[*nunique] == *unique_bytes.
 * The result is a function of the records and the set's contents alone, never of scheduling:
 * with set == NULL two calls give identical arrays. The records, the tree buffers and the run's
 * own state are not touched; a later bsg_engine_trees or bsg_engine_run behaves as before.
 * With a set (on the engine's device, else BSG_EINVAL): records whose ref the set holds are not
 * new, and the new records' refs have been added to the set when the call returns, so a second
 * call on the same run with the same set reports *nunique == 0 (every first[i] carries bit 63).
 * BSG_EINVAL for null eng, nunique or unique_bytes; BSG_ESTATE unless the engine's last enqueue
 * was a bsg_engine_run that bsg_engine_finish completed successfully (as bsg_engine_trees), or
 * if the set has seen a device error; BSG_ENOMEM with the set unchanged if it cannot grow. */
int bsg_engine_dedup(bsg_engine* eng, bsg_refset* set /* or NULL */, uint64_t* nunique,
                     uint64_t* unique_bytes);
/* The result to host memory: up to cap_first entries of first, up to cap_uniq of uniq and (the
 * same number + 1) of pack_off. Any of the three pointers may be NULL. BSG_ESTATE without a
 * dedup result for the current run (as the device pointers below are NULL). */
int bsg_engine_copy_dedup(bsg_engine* eng, uint64_t* first, uint64_t cap_first, uint64_t* uniq,
                          uint64_t* pack_off, uint64_t cap_uniq);
const uint64_t* bsg_engine_dedup_first_device(const bsg_engine* eng);
const uint64_t* bsg_engine_dedup_uniq_device(const bsg_engine* eng);
const uint64_t* bsg_engine_dedup_pack_off_device(const bsg_engine* eng);
/* Gathers the new records' bytes, tightly packed, into device memory:
 *   d_out[pack_off[k] .. pack_off[k + 1]) = the bytes of record uniq[k]
 *                                         = d_data[off[stream] + offset .. + len) of the run.
 * One D2H copy of unique_bytes plus uniq and pack_off then gives a store all it must Put.
 * Synchronous. The caller keeps the run's input bytes (d_data of bsg_engine_run) valid and
 * unchanged until the call returns. No byte outside [d_out, d_out + unique_bytes) is written.
 * BSG_ESTATE without a dedup result for the current run; BSG_EINVAL for a d_out that is null or
 * not a multiple of 16, for cap < unique_bytes, or when [d_out, d_out + unique_bytes) intersects
 * the run's data span (d_data up to the end of its last stream). */
int bsg_engine_pack_unique(bsg_engine* eng, uint8_t* d_out, uint64_t cap);

/* ---- streams restored on the device from a pool of blobs: split.Reader for many streams ---- */
/* The inverse of bsg_engine_dedup + bsg_engine_pack_unique (split.Reader reads a tree's chunks
 * one by one out of a store, split/split.go:169-303): every distinct blob lies once in a pool in
 * device memory, records say which blob is which part of which stream, and the streams are
 * written out in device memory.
 * Blob k is d_pool[blobs[k].off .. + blobs[k].len) and is named blobs[k].ref. If two blobs carry
 * the same ref, the one with the smaller index is used. */
typedef struct bsg_pool_blob {
  uint64_t off;
  uint64_t len;
  uint8_t ref[32];
} bsg_pool_blob; /* 48 bytes */
#define BSG_RESTORE_VERIFY 1 /* hash every pool blob on the device and hold it to its ref */
typedef struct bsg_restore_info {
  uint64_t bad_record; /* smallest failing record index, else UINT64_MAX */
  uint64_t bad_blob;   /* smallest pool blob index whose bytes do not hash to its ref, else
                        * UINT64_MAX */
  uint64_t bytes;      /* bytes written to d_out (0 on any failure) */
  uint64_t verified;   /* pool bytes hashed */
} bsg_restore_info;
/* Record i (stream, offset, len, ref; level is ignored; as bsg_engine_copy_chunks gives them)
 * says: bytes [offset, offset + len) of stream `stream` are the blob with that ref. On success
 * d_out[out_off[s] + r.offset .. + r.len) holds that blob's bytes for every record r of stream s.
 * Synchronous, on the engine's stream. The result is a function of the arguments alone, never of
 * scheduling.
 * BSG_EINVAL if a layout rule is broken: a null pointer with a non-zero count; d_out or an
 * out_off[s] not a multiple of 16; an out_off[s] + out_len[s] that wraps or exceeds out_cap; two
 * streams' output ranges that intersect, or one that intersects the pool; a blob that ends past
 * pool_bytes; a record with stream >= nstreams or len == 0; records not stream-major with
 * ascending offsets; a stream s whose records do not tile [0, out_len[s]) exactly (first offset
 * 0, no gap, no overlap, the last one's end out_len[s]; a stream of length 0 has no records).
 * With BSG_RESTORE_VERIFY only, the engine hash path's own rules (bsg_engine_hash): d_pool or a
 * blobs[k].off not a multiple of 16, a blob of 2^40 bytes or more, or less than BSG_READ_SLACK
 * readable bytes (of pool_bytes) after the last blob. Without the flag blobs may start at any
 * byte, so the tight output of bsg_engine_pack_unique is a valid pool:
 * blobs[k] = {pack_off[k], len, ref} of record uniq[k].
 * Then, in this order: BSG_ENOTFOUND if a record's ref is not in the pool (bad_record: the
 * smallest such index); BSG_ECORRUPT if a record's len is not its blob's len (bad_record) or,
 * with the flag, a blob's SHA-256 is not its ref (bad_blob; with the flag, bad_blob and verified
 * are filled in whenever the layout was valid); BSG_ESTATE if the engine has an enqueued,
 * unfinished run.
 * Every check, verification included, has finished before the first byte of d_out is written:
 * on any failure d_out is untouched. On success no byte outside the streams' output ranges is
 * written: the gaps between streams, and the bytes after a stream's end inside its last 16-byte
 * vector, stay as they were. The engine's last run stays valid: its records, dedup result and
 * tree can still be read, and a later bsg_engine_run behaves as before. */
int bsg_engine_restore(bsg_engine* eng,
                       const uint8_t* d_pool, uint64_t pool_bytes, /* device */
                       const bsg_pool_blob* blobs, uint64_t nblobs, /* host */
                       const bsg_chunk* recs, uint64_t nrecs,       /* host */
                       uint8_t* d_out, uint64_t out_cap,            /* device */
                       const uint64_t* out_off, const uint64_t* out_len,
                       uint32_t nstreams,                           /* host */
                       int flags, bsg_restore_info* info /* or NULL */);

/* ---- split trees read on the device, from Roots to records: split.NewReader for many streams ---- */
/* The inverse of bsg_engine_trees (split.NewReader reads a Root's Node and follows `nodes` down
 * to the `leaves`, split/split.go:181-303; the reachable set is split.Protect's,
 * split/split.go:306-322). The pool holds node blobs and chunk blobs side by side (nothing marks
 * which is which) and means what it means for bsg_engine_restore: blobs may start at any byte, of
 * two blobs under one ref the one with the smaller index is used, refs are trusted labels and
 * nothing is hashed here (bsg_engine_restore_walk with BSG_RESTORE_VERIFY hashes every pool blob,
 * nodes included, before a byte is written). roots[32 * s ..) is stream s's Root; 32 zero bytes
 * (bs.Zero, as bsg_engine_copy_roots gives for an empty stream) is an empty stream: size 0, no
 * node, no record, status BSG_OK. Any other Root must be in the pool.
 * A node blob is accepted only if its bytes are exactly what PutProto emits for its decoded
 * fields (`nodes` entries, then `leaves` entries, then offset if non-zero, then size if non-zero;
 * every ref 32 bytes; a Child's offset omitted when 0; minimal varints; no other field); it has
 * children of one kind only, and at least one; the first child's offset equals the node's offset
 * and the children's offsets strictly ascend; size > 0 and offset + size does not wrap; a Root's
 * offset is 0. Child i covers the bytes from its offset to the next child's offset (the last one
 * to the node's offset + size), and must meet its cover: a `nodes` child is a blob whose own
 * offset and size equal the cover, a `leaves` child a blob whose len in the blob table is the
 * cover's length (never 0). A node's `nodes` children at depth 64 (Root = 0) are refused unread,
 * which is what ends a cycle in an unverified pool. Leaf nodes need not all lie at one depth.
 * The walk visits every node whose parent passed its own checks, so what it visits is a function
 * of the arguments alone. status[s] is BSG_ENOTFOUND if stream s's Root, or a child ref of a
 * visited node that passed its checks, is not in the pool; else BSG_ECORRUPT if a visited node
 * or a child's cover breaks a rule above; else BSG_OK.
 * Returns, in this order: BSG_EINVAL, before anything is enqueued, for a null pointer with a
 * non-zero count, a blob that ends past pool_bytes, flags != 0 or nstreams > 65,535;
 * BSG_ENOTFOUND if any stream's status is that; BSG_ECORRUPT if any stream's status is that;
 * BSG_ESTATE if the engine has an enqueued, unfinished run; BSG_ENOMEM if the result cannot be
 * allocated. status and info's bad_stream, nnodes and depth are filled whenever the layout was
 * valid. Synchronous, on the engine's stream.
 * On success the engine keeps, until its next bsg_engine_walk: the records on the device
 * (stream-major, ascending offset; stream, offset, len and ref filled, level 0) and, per stream,
 * its size (the Root node's) and its record count. A walk that fails publishes nothing. The
 * engine's last run, dedup result, tree and restore buffers are not touched, and an engine needs
 * no run before it walks. */
typedef struct bsg_walk_info {
  uint64_t bad_stream; /* smallest stream index whose status is not BSG_OK, else UINT64_MAX */
  uint64_t nrecs;      /* records produced (0 on any failure) */
  uint64_t nnodes;     /* node blobs visited, over all streams (filled whenever the layout was valid) */
  uint64_t bytes;      /* sum of the streams' sizes (0 on any failure) */
  uint32_t depth;      /* deepest node visited, Root = 0 (0 if no node was visited) */
  uint32_t reserved;
} bsg_walk_info;
int bsg_engine_walk(bsg_engine* eng,
                    const uint8_t* d_pool, uint64_t pool_bytes,   /* device */
                    const bsg_pool_blob* blobs, uint64_t nblobs,  /* host */
                    const uint8_t* roots, uint32_t nstreams,      /* host, nstreams x 32 */
                    int flags,                                    /* must be 0 */
                    int32_t* status,                              /* host, nstreams, or NULL */
                    bsg_walk_info* info);                         /* or NULL */
/* The last successful walk's records (up to cap), sizes and counts (the first nstreams streams;
 * more than the walk's is BSG_EINVAL) to host memory. Any pointer may be NULL. BSG_ESTATE without
 * a successful walk (as the device pointer below is NULL). */
int bsg_engine_copy_walk(bsg_engine* eng, bsg_chunk* recs, uint64_t cap,
                         uint64_t* sizes, uint64_t* counts, uint32_t nstreams);
const bsg_chunk* bsg_engine_walk_records_device(const bsg_engine* eng);
/* bsg_engine_restore with recs = the last successful walk's records, read where they lie on the
 * device, and out_len = the walk's sizes: every rule, check, order of errors, flag and
 * bsg_restore_info field is bsg_engine_restore's. The caller reads the sizes, chooses out_off and
 * calls it; the records never cross the host link. BSG_ESTATE without a walk, BSG_EINVAL if
 * nstreams is not the walk's. */
int bsg_engine_restore_walk(bsg_engine* eng,
                            const uint8_t* d_pool, uint64_t pool_bytes,
                            const bsg_pool_blob* blobs, uint64_t nblobs,
                            uint8_t* d_out, uint64_t out_cap, const uint64_t* out_off,
                            uint32_t nstreams, int flags, bsg_restore_info* info);

/* ---- a pool garbage-collected on the device from its Roots: gc.Protect + split.Protect + gc.Run ---- */
/* The mark (gc.Protect with split.Protect, gc/gc.go:38-97 and split/split.go:306-322) finds the
 * blobs of a pool that a set of Roots reaches; the sweep (gc.Run's Deletes, as a compaction)
 * gathers them into a new pool.
 * Pool and Roots. The pool means what it means for bsg_engine_walk: blobs may start at any byte,
 * refs are trusted labels and nothing is hashed; of two blobs under one ref only the one with the
 * smaller index is ever used, the other is dead. roots is any number of refs up to 2^32 - 1 (it is
 * not bounded by 65,535). 32 zero bytes is bs.Zero and is skipped with status BSG_OK. The same
 * Root may appear many times. Any node blob may be a Root, and its offset is not held to 0
 * (gc.Protect starts anywhere).
 * What is live. A blob is live if it is the smallest-index blob of a ref that is a Root, or that an
 * expanded node names under `nodes` or `leaves`. A blob is expanded, once, if it is live through a
 * Root or a `nodes` entry; a blob named only by `leaves` entries is never read; a blob named both
 * ways is expanded.
 * Node rules. An expanded blob must meet the walk's per-node rules: exactly PutProto's bytes;
 * children of one kind, and at least one; the first child's offset equals the node's offset; child
 * offsets strictly ascend; size > 0, and offset + size does not wrap. The walk's edge rules do
 * not apply: a child is not held to its cover and a leaf's len is not compared, because
 * split.Protect follows refs and nothing else; bsg_engine_walk and bsg_engine_restore check the
 * covers when the data is read. A node that fails is not expanded further. A `nodes` entry of a
 * node at depth 64 is refused unread; a node's depth is the fewest edges from any Root, so a chain
 * of 100 nodes with a Root every 50 passes. A cycle of trusted labels ends because a blob is
 * expanded once.
 * Verdicts. status[r] speaks of Root r alone: BSG_ENOTFOUND if it is not in the pool,
 * BSG_ECORRUPT if its own blob fails the node rules, else BSG_OK. Everything below the Roots is
 * reported through bad_blob. Returns, in this order: BSG_EINVAL, before anything is enqueued, for
 * a null pointer with a non-zero count, a blob that ends past pool_bytes, or unknown flag bits;
 * BSG_ENOTFOUND if a Root, a `nodes` ref or (without BSG_GC_MISSING_LEAVES) a `leaves` ref of an
 * expanded node that passed its rules is not in the pool; BSG_ECORRUPT if an expanded node breaks
 * a rule or sits too deep; BSG_ESTATE if the engine has an enqueued, unfinished run; BSG_ENOMEM.
 * A failed mark publishes nothing and drops the previous mark's result, so a caller can never
 * sweep on a half-read tree. The set of expanded blobs, and every output, is a function of the
 * arguments alone: two calls give identical bytes. Synchronous, on the engine's stream. The
 * engine's last run, dedup result, tree, walk and restore buffers are not touched, and an engine
 * needs no run before it marks.
 * On success the engine keeps, until its next mark: live[k], one byte per pool blob, 0 or 1; and
 * the live blobs' new offsets, the exclusive prefix sum of len over the live blobs in index order,
 * once as it is and once with every term rounded up to 16 (BSG_GC_ALIGN16 in the flags of
 * bsg_engine_copy_gc and bsg_engine_gc_compact chooses). What gc.Run would Delete is
 * {blobs[k].ref : live[k] == 0}, minus the refs that a live smaller-index twin still carries. */
#define BSG_GC_MISSING_LEAVES 1  /* mark: a `leaves` ref the pool lacks is no error */
#define BSG_GC_ALIGN16        1  /* compact: every blob starts at a multiple of 16 */
typedef struct bsg_gc_info {
  uint64_t bad_root;        /* smallest root index whose status is not BSG_OK, else UINT64_MAX */
  uint64_t bad_blob;        /* smallest pool index of a visited node that fails its rules, or (if none does)
                               that names a child the pool lacks; else UINT64_MAX */
  uint64_t nlive, live_bytes;   /* 0 on any failure */
  uint64_t ndead, dead_bytes;   /* 0 on any failure */
  uint64_t nnodes;          /* distinct node blobs expanded (filled whenever the layout was valid) */
  uint64_t missing_leaves;  /* distinct `leaves` refs not in the pool (only with the flag, else 0) */
  uint32_t depth;           /* largest depth of an expanded node; a node's depth = fewest edges from any Root */
  uint32_t reserved;
} bsg_gc_info;
int bsg_engine_gc_mark(bsg_engine* eng, const uint8_t* d_pool, uint64_t pool_bytes,
                       const bsg_pool_blob* blobs, uint64_t nblobs,   /* host */
                       const uint8_t* roots, uint64_t nroots,         /* host, nroots x 32 */
                       int flags, int32_t* status /* host, nroots, or NULL */, bsg_gc_info* info);
/* The last successful mark to host memory: live, up to cap_live entries, and
 * table[j] = {new_off, len, ref} of the j-th live blob in index order, up to cap_table entries:
 * the `blobs` argument of bsg_engine_walk and bsg_engine_restore on the compacted pool. Either
 * pointer may be NULL. BSG_ESTATE without a successful mark (as the device pointer below is
 * NULL); BSG_EINVAL for unknown flag bits. */
int bsg_engine_copy_gc(bsg_engine* eng, uint8_t* live, uint64_t cap_live,
                       bsg_pool_blob* table, uint64_t cap_table, int flags);
const uint8_t*  bsg_engine_gc_live_device(const bsg_engine* eng);
/* The sweep: for every live blob, d_out[new_off[j] .. + len) = that blob's bytes, in index order.
 * With BSG_GC_ALIGN16 the padding bytes between blobs are written zero, so the output meets
 * BSG_RESTORE_VERIFY's alignment rule. *out_bytes is the end of the last live blob's bytes (0 if
 * nothing is live); no byte of d_out outside [d_out, d_out + *out_bytes) is written. Blobs of
 * len 0 occupy nothing. Before anything is enqueued: BSG_ESTATE without a mark (or with an
 * unfinished run); BSG_EINVAL if d_pool / pool_bytes are not the mark's, if d_out is null or not
 * a multiple of 16, if cap is less than the packed size, for unknown flag bits, or if the output
 * range intersects the pool: in-place compaction is out of scope. The caller keeps the pool
 * valid and unchanged from the mark until the call returns. Synchronous. */
int bsg_engine_gc_compact(bsg_engine* eng, const uint8_t* d_pool, uint64_t pool_bytes,
                          uint8_t* d_out, uint64_t cap, int flags, uint64_t* out_bytes);

/* ---- a pool that lives in device memory across runs: store/mem's Put for device-resident data ---- */
/* store/mem keeps one blob per ref and reports `added` (store/mem/mem.go:62-77). A bsg_pool is
 * that store in device memory: it owns its bytes, its blob table (bsg_pool_blob entries) and an
 * index of blob indices by ref, and bsg_engine_pool_put appends the last run's new chunks and new
 * tree nodes to it, on the device. Afterwards only a 48-byte table entry per new blob needs to
 * cross the host link, and only when the caller asks for it.
 * The pool. One allocation of cap_bytes rounded up to 16, plus BSG_READ_SLACK, zero-filled at
 * creation, and a table of cap_blobs entries. Neither ever moves, so the device pointers below
 * stay valid for the pool's life and a walk, restore or gc may hold them. The capacity is fixed and
 * the pool only ever grows (no growth past the capacity, no delete of single refs; a pool is
 * collected into another, empty pool with bsg_pool_collect, merged into one that holds something
 * with bsg_pool_merge and emptied for reuse with bsg_pool_reset, below). bsg_pool_new returns
 * NULL with BSG_ENODEV (no such device) or BSG_ENOMEM in *err.
 * Layout. Every blob starts at a multiple of 16 and the padding after it (at most 15 bytes) is
 * zero, so the pool (bsg_pool_bytes_device, with pool_bytes of bsg_pool_stat and the table of
 * bsg_pool_copy_table) is at all times a valid argument set for bsg_engine_walk,
 * bsg_engine_restore, bsg_engine_restore_walk (with and without BSG_RESTORE_VERIFY) and
 * bsg_engine_gc_mark. No two table entries carry one ref.
 * Threading: a pool carries its own mutex, held for a whole call; engines on several threads may
 * put into one pool, their calls serialize. */
typedef struct bsg_pool bsg_pool;
bsg_pool* bsg_pool_new(int device, uint64_t cap_bytes, uint64_t cap_blobs, int* err);
void bsg_pool_free(bsg_pool* p);
typedef struct bsg_pool_stats {
  uint64_t nblobs, bytes;        /* table entries; the end of the last blob's last byte */
  uint64_t cap_blobs, cap_bytes;
  uint64_t pool_bytes;           /* what to pass as pool_bytes to walk / restore / gc */
} bsg_pool_stats;
int bsg_pool_stat(const bsg_pool* p, bsg_pool_stats* out);
const uint8_t* bsg_pool_bytes_device(const bsg_pool* p); /* the d_pool argument */
const bsg_pool_blob* bsg_pool_table_device(const bsg_pool* p);
/* table[first .. first + n) to host memory, n = min(cap, nblobs - first). BSG_EINVAL for a null
 * pool, first > nblobs or a null out with cap > 0; BSG_ESTATE for a dead pool. */
int bsg_pool_copy_table(bsg_pool* p, bsg_pool_blob* out, uint64_t first, uint64_t cap);

/* Appends to the pool, in this order, the items of the last finished bsg_engine_run: with
 * BSG_POOL_CHUNKS its records, in the order of bsg_engine_chunks_device; then, with
 * BSG_POOL_NODES, its tree's nodes, in the order of bsg_engine_tree_nodes_device. Item i is
 * appended iff the pool does not hold its ref and no item j < i of this call carries it; a chunk
 * and a node with equal bytes are one blob. The k-th appended item gets table entry
 * first_blob + k = {off, len, ref} with off = align16(bytes before the call) + the sum of
 * align16(len) over the items appended before it. Chunks are therefore stored before nodes and
 * nodes in list order: a node is never in the table before what it points to
 * (split/split.go:71-77). The table, the pool's bytes and where[] are a function of the sequence
 * of puts alone, never of scheduling: two pools fed the same runs hold identical bytes.
 * All or nothing. Which items are new and how many bytes and table entries they need is decided
 * on the device and read back before anything of the pool is written. If need_bytes > cap_bytes
 * or need_blobs > cap_blobs the call returns BSG_ENOMEM with info filled, and the pool's bytes,
 * table, index, counters and where[] are unchanged (so is a put that cannot allocate its
 * workspace). A device error during the append marks the pool dead: that call returns
 * BSG_EDEVICE and every later call on the pool BSG_ESTATE, as for bsg_refset.
 * Errors, in this order: BSG_EINVAL for a null engine or pool, flags 0 or unknown bits, a pool on
 * another device than the engine, or a run whose input lies inside the pool's own allocation;
 * BSG_ESTATE unless the engine's last enqueue was a bsg_engine_run that bsg_engine_finish
 * completed (as bsg_engine_dedup), if BSG_POOL_NODES is set and no bsg_engine_trees result is
 * current for that run, or if the pool is dead; then BSG_ENOMEM or BSG_EDEVICE as above.
 * Synchronous, on the engine's stream. The caller keeps the run's input bytes valid and unchanged
 * until the call returns. The engine's run is not touched: its records, bsg_engine_dedup result,
 * tree, walk, restore and gc buffers stay as they are. info may be NULL. */
#define BSG_POOL_CHUNKS 1 /* the run's records */
#define BSG_POOL_NODES  2 /* the run's tree nodes (needs a current bsg_engine_trees result) */
typedef struct bsg_pool_put_info {
  uint64_t items;       /* records + nodes considered */
  uint64_t added;       /* blobs appended */
  uint64_t added_bytes; /* sum of their len (payload, without padding) */
  uint64_t known;       /* items whose ref the pool held before the call */
  uint64_t repeats;     /* items that repeat an earlier item of this call (such an item whose ref
                           the pool held counts under known too) */
  uint64_t first_blob;  /* nblobs before the call: the new blobs are [first_blob, first_blob + added) */
  uint64_t need_bytes, need_blobs; /* bytes / nblobs the pool would have after the call (filled
                                      on BSG_ENOMEM for want of capacity too) */
} bsg_pool_put_info;
int bsg_engine_pool_put(bsg_engine* eng, bsg_pool* pool, int flags, bsg_pool_put_info* info);
/* where[i] = the pool blob index that carries item i's ref, for the items of the last successful
 * put (up to cap of them to host memory). BSG_ESTATE before the first successful put (as the
 * device pointer below is NULL, which it also is after a put without items) or on a dead pool. */
int bsg_pool_copy_where(bsg_pool* p, uint64_t* where, uint64_t cap);
const uint64_t* bsg_pool_where_device(const bsg_pool* p);

/* ---- a pool collected into a pool: gc.Run's Delete for data that lives in device memory ---- */
/* Marks src from the Roots and appends its live blobs to dst, an empty pool; dst is then a pool
 * like any other, and a put may append to it.
 * The mark is bsg_engine_gc_mark's, rule for rule: liveness, the node rules, depth 64, the
 * verdicts, status[] and every bsg_gc_info field. It runs over src's entries as they stand when
 * the call has taken src's mutex, and reads src's table and src's own index where they lie on the
 * device: no table crosses the host link and no index is built. It becomes the engine's current
 * gc result: bsg_engine_gc_live_device and bsg_engine_copy_gc serve it (the table's entries are
 * fetched from src's device table then), and bsg_engine_gc_compact takes src's
 * bsg_pool_bytes_device / pool_bytes. That result reads src's table, so it holds only until src is
 * reset or freed.
 * The layout. Live blob k of src becomes dst's entry j = rank[k], the number of live blobs before
 * it in index order, = {noff16[k], len, ref}; the bytes are what bsg_engine_gc_compact writes with
 * BSG_GC_ALIGN16 (every blob at a multiple of 16, zero padding), and dst's `bytes` counter is the
 * end of the last live blob's bytes. remap[k] = j for a live blob and UINT64_MAX for a dead one,
 * for every k below src's nblobs at the call; dst owns remap until its next collect or reset.
 * dst's table, bytes and remap are a function of src's contents and the Roots alone.
 * All or nothing. Everything up to the readback of the totals writes the engine's gc buffers and
 * nothing of dst. If need_blobs > cap_blobs or need_bytes > cap_bytes the call returns BSG_ENOMEM
 * with info filled; after that or a failed mark dst is exactly as it was: bytes, table, index,
 * counters, remap and where[]. A device error from then on marks dst dead: that call returns
 * BSG_EDEVICE and later calls on dst BSG_ESTATE, as for a put. src is never written.
 * Errors, in this order: BSG_EINVAL for a null engine or pool, src == dst, pools or engine on
 * different devices, unknown flag bits, nroots > 2^32 - 1 or null roots with a count; BSG_ESTATE
 * if either pool is dead, dst is not empty (nblobs != 0) or the engine has an enqueued,
 * unfinished run; the mark's BSG_ENOTFOUND / BSG_ECORRUPT, with status and info->gc filled;
 * BSG_ENOMEM; BSG_EDEVICE. Synchronous, on the engine's stream. Both pools' mutexes are held for
 * the whole call and taken together, so A -> B beside B -> A on two threads cannot deadlock. */
typedef struct bsg_pool_collect_info {
  bsg_gc_info gc;                   /* exactly what bsg_engine_gc_mark fills */
  uint64_t need_bytes, need_blobs;  /* what dst would hold; also filled on BSG_ENOMEM for want of capacity */
} bsg_pool_collect_info;
int bsg_pool_collect(bsg_engine* eng, bsg_pool* src, bsg_pool* dst,
                     const uint8_t* roots, uint64_t nroots, /* host, nroots x 32 */
                     int flags,                             /* BSG_GC_MISSING_LEAVES or 0 */
                     int32_t* status /* host, nroots, or NULL */,
                     bsg_pool_collect_info* info /* or NULL */);
/* remap of the last successful collect into dst, up to cap entries to host memory. BSG_ESTATE
 * before one (as the device pointer is NULL, which it also is after a collect of an empty src) or
 * on a dead pool. */
int bsg_pool_copy_remap(bsg_pool* dst, uint64_t* remap, uint64_t cap);
const uint64_t* bsg_pool_remap_device(const bsg_pool* dst);

/* ---- a pool merged into a pool that holds something; two pools synced (store.Sync) ---- */
/* bsg_pool_merge appends to dst the selected blobs of src whose refs dst does not hold, on the
 * device: src's entries are probed in dst's index where both lie, no table crosses the host link.
 * Selection. Without BSG_MERGE_ALL the selected blobs are the live ones of bsg_pool_collect's
 * mark, rule for rule: it reads src's device table and index, fills status[] and info->gc the same
 * way, returns the same BSG_ENOTFOUND / BSG_ECORRUPT and becomes the engine's current gc result.
 * With BSG_MERGE_ALL every entry of src is selected, no mark runs, info->gc is all zero and the
 * engine's gc result is left as it was.
 * The append. Selected blob k of src is appended iff dst's index does not hold table[k].ref. Refs
 * are trusted labels: a ref that dst holds with another len counts as known and is not replaced
 * (store/mem's Put keeps the first blob, store/mem/mem.go:70-74). The appended blobs keep src's
 * index order; the j-th becomes dst's entry first_blob + j = {off, len, ref} with off =
 * align16(dst's bytes before the call) + the sum of align16(len) over the blobs appended before
 * it, the padding is zero, and dst's `bytes` is the end of the last appended blob (unchanged when
 * added == 0). dst afterwards equals, byte for byte over its allocation and entry for entry, a
 * pool into which the same blobs were put one at a time in that order; it is a function of the two
 * pools and the Roots alone, and serves puts, walk, restore, read, gc, collect and further merges
 * like any other pool. A merge into an empty dst with Roots is a bsg_pool_collect whose table
 * happens to be the same. A merge of an empty src succeeds with added == 0, and nroots == 0
 * without BSG_MERGE_ALL selects nothing and succeeds.
 * remap. dst owns a remap of src's nblobs entries at the call: remap[k] is the dst index that
 * carries blob k's ref, appended now or known before, and UINT64_MAX for an unselected blob.
 * bsg_pool_copy_remap and bsg_pool_remap_device serve it, as after a collect. dst's where[] is
 * left untouched: the indices it holds stay valid.
 * BSG_MERGE_VERIFY. After the probe and the plan, the blobs to append, and no others, are hashed
 * on the engine's hash runs and held to their refs, as BSG_READ_VERIFY does for touched blobs. A
 * mismatch returns BSG_ECORRUPT with bad_blob set, before anything of dst is written. Known and
 * unselected blobs are never hashed, so `verified` is added_bytes on success.
 * All or nothing. The mark, the probe, the plan, the verification and the readback of the totals
 * write nothing of dst. After a failed mark, a failed verification or BSG_ENOMEM (need_blobs >
 * cap_blobs, need_bytes > cap_bytes, or a workspace that cannot be allocated) dst is exactly as it
 * was: bytes, table, index, counters, remap and where[]; info is filled as far as the call came.
 * A device error after that point marks dst dead, as for a put. src is never written.
 * Errors, in this order: BSG_EINVAL for a null engine or pool, src == dst, pools or engine on
 * different devices, unknown flag bits, BSG_MERGE_ALL together with Roots or with
 * BSG_GC_MISSING_LEAVES, nroots > 2^32 - 1 or null roots with a count; BSG_ESTATE if either pool
 * is dead or the engine has an enqueued, unfinished run; the mark's codes; BSG_ECORRUPT from the
 * verification; BSG_ENOMEM; BSG_EDEVICE. Synchronous, on the engine's stream. Both pools' mutexes
 * are held for the whole call and taken together, as for bsg_pool_collect. The engine's last run,
 * its dedup, tree, walk and restore results stay valid. */
/* flags: BSG_GC_MISSING_LEAVES (1, the mark's, as for collect) */
#define BSG_MERGE_ALL    2  /* select every blob of src; no mark; roots must be NULL, nroots 0 */
#define BSG_MERGE_VERIFY 4  /* hash every blob that would be appended, and only those, first */
typedef struct bsg_pool_merge_info {
  bsg_gc_info gc;          /* what bsg_engine_gc_mark fills; all zero with BSG_MERGE_ALL */
  uint64_t selected;       /* live blobs of src (all of them with BSG_MERGE_ALL) */
  uint64_t added;          /* blobs appended to dst */
  uint64_t added_bytes;    /* sum of their len */
  uint64_t known;          /* selected blobs whose ref dst held before the call */
  uint64_t first_blob;     /* dst's nblobs before the call */
  uint64_t need_bytes, need_blobs; /* what dst would hold after; filled on capacity BSG_ENOMEM too */
  uint64_t bad_blob;       /* VERIFY: smallest src index to append whose bytes do not hash to its ref, else UINT64_MAX */
  uint64_t verified;       /* VERIFY: sum of len over the blobs hashed */
} bsg_pool_merge_info;
int bsg_pool_merge(bsg_engine* eng, bsg_pool* src, bsg_pool* dst,
                   const uint8_t* roots, uint64_t nroots, int flags,
                   int32_t* status /* host, nroots, or NULL */,
                   bsg_pool_merge_info* info /* or NULL */);
/* store.Sync (store/sync.go:14-126) for two pools: afterwards both hold the same set of refs. The
 * pools end as after bsg_pool_merge(a -> b, BSG_MERGE_ALL) followed by bsg_pool_merge(b -> a,
 * BSG_MERGE_ALL), but all or nothing across both directions: both probes, both plans, both
 * verifications (with the flag) and both capacity checks run before either pool is written, each
 * direction against the other pool as it stands at the call (what the first direction appends to
 * b, a holds already). If either direction would not fit the call returns BSG_ENOMEM with both
 * infos filled and both pools unchanged. info[0] is a -> b, info[1] b -> a, its `selected` b's
 * nblobs at the call; b's remap covers a's blobs at the call and a's remap b's. The errors are
 * merge's, with a == b in the place of src == dst and any flag but BSG_MERGE_VERIFY unknown. */
int bsg_pool_sync(bsg_engine* eng, bsg_pool* a, bsg_pool* b, int flags /* 0 or BSG_MERGE_VERIFY */,
                  bsg_pool_merge_info info[2] /* [0]: a -> b, [1]: b -> a; or NULL */);

/* ---- blobs put into a pool and got out of it by ref: bs.PutMulti / bs.GetMulti ---- */
/* bsg_pool_put_blobs is store/mem's Put (bs.PutMulti, multi.go:84-143, its batched form) for blobs
 * that are not part of a split run: fs.Dir and schema blobs, anchors, whatever a server receives.
 * Layout. Item i is d_src[off[i] .. off[i] + len[i]) under bsg_engine_hash's rules: d_src and every
 * off[i] multiples of 16, len[i] < 2^40, off[i] + len[i] without wrap, BSG_READ_SLACK readable
 * bytes after the last blob in d_src's allocation; any order, gaps, overlapping or coinciding
 * blobs and empty blobs are fine. nblobs is not capped at 65,535 (the call hashes in batches); it
 * is refused from 2^32 on.
 * Refs. Every item's SHA-256 is computed on the device, on the engine's hash runs; a ref is never
 * taken from the caller (Put computes blob.Ref()). refs_out, when given, receives them, item
 * order, also when the call ends in BSG_ENOMEM for want of capacity.
 * The append. From the refs on the call is bsg_engine_pool_put with these items in the place of
 * records and nodes: item i is appended iff the pool does not hold its ref and no item j < i
 * carries it; the k-th appended item gets entry first_blob + k at align16(bytes before the call) +
 * the sum of align16(len) over the items appended before it; padding is zero; an empty blob takes
 * an entry and no bytes. bsg_pool_put_info is filled as for a put. A pool fed a run's chunks and
 * then its nodes this way, in the order of bsg_engine_chunks_device and
 * bsg_engine_tree_nodes_device, is byte for byte and entry for entry the pool bsg_engine_pool_put
 * makes, and serves walk, restore, read, gc, collect and merge alike.
 * where[]. bsg_pool_copy_where / bsg_pool_where_device hold item i's blob index afterwards. Item
 * i's ref was added by this call iff where[i] >= first_blob (PutMulti's map[Ref]bool); the item
 * that brought the bytes is the first with that where.
 * All or nothing, as a put: BSG_ENOMEM (need_bytes > cap_bytes, need_blobs > cap_blobs, or no
 * workspace) leaves the pool and where[] untouched, with info filled in the first two cases; a
 * device error during the append marks the pool dead.
 * Errors, in this order: BSG_EINVAL for a null engine or pool, flags != 0, a null pointer with a
 * count, nblobs >= 2^32, a pool on another device, a layout rule broken, or a source that
 * intersects the pool's allocation; BSG_ESTATE for a dead pool or an engine with an enqueued,
 * unfinished run; BSG_ENOMEM; BSG_EDEVICE. nblobs == 0 succeeds and leaves where NULL.
 * Synchronous, on the engine's stream; the pool's mutex is held for the whole call. The engine's
 * last run and its dedup, tree, walk, restore and gc results stay valid. info may be NULL. */
int bsg_pool_put_blobs(bsg_engine* eng, bsg_pool* pool,
                       const uint8_t* d_src,                     /* device */
                       const uint64_t* off, const uint64_t* len, /* host, nblobs */
                       uint64_t nblobs, int flags /* 0 */,
                       uint8_t* refs_out /* host, nblobs x 32, or NULL */,
                       bsg_pool_put_info* info /* or NULL */);

/* bsg_pool_get is store/mem's Get (bs.GetMulti, multi.go:10-69, its batched form): request q, the
 * ref refs[32q .. 32q + 32), is probed in the pool's own device index; nothing of the table
 * crosses the host link.
 * Placement. idx[q] is the blob's index or UINT64_MAX. out_off[q] is the exclusive prefix sum, in
 * request order, of align16(len) for found requests and 0 for missing ones; out_off[nrefs] is the
 * total. A ref asked for twice gets two copies.
 * The result is partial, as GetMulti's: a missing ref is no error of the call, which returns
 * BSG_OK with idx[q] == UINT64_MAX and info->missing counted.
 * Output. d_out[out_off[q] .. + len) holds the blob and the padding up to the next multiple of 16
 * is written zero; no byte at or past out_off[nrefs] is written. The output is therefore itself a
 * valid source for bsg_pool_put_blobs and bsg_engine_hash (given the read slack behind it).
 * With d_out == NULL and out_cap == 0 nothing is gathered (a Has / size call); idx, out_off and
 * info are filled all the same.
 * BSG_GET_VERIFY. The distinct found blobs, and no others, are hashed on the engine's hash runs
 * and held to their refs before a byte of d_out is written, as BSG_READ_VERIFY does for touched
 * blobs. A mismatch returns BSG_ECORRUPT with bad_blob set and nothing written.
 * Errors, in this order: BSG_EINVAL for a null engine, pool or info, null refs with a count,
 * unknown flag bits, nrefs >= 2^32, d_out not a multiple of 16, d_out NULL with out_cap != 0 or
 * the reverse, a pool on another device, or an output range that intersects the pool's
 * allocation; BSG_ESTATE for a dead pool or an engine with an enqueued, unfinished run;
 * BSG_ENOMEM if need_bytes > out_cap, with info, idx and out_off filled and d_out untouched, or
 * for want of workspace; BSG_ECORRUPT; BSG_EDEVICE. The pool is never written and never marked
 * dead by a get. Synchronous, on the engine's stream; the pool's mutex is held for the whole
 * call. The engine's last run and its dedup, tree, walk, restore and gc results stay valid. */
#define BSG_GET_VERIFY 1
typedef struct bsg_pool_get_info {
  uint64_t found, missing;   /* over the request, repeats counted each time */
  uint64_t bytes;            /* sum of len over found requests */
  uint64_t need_bytes;       /* out_off[nrefs]; filled on BSG_ENOMEM too */
  uint64_t bad_blob;         /* VERIFY: smallest pool index that fails, else UINT64_MAX */
  uint64_t verified;         /* VERIFY: sum of len over the distinct blobs hashed */
} bsg_pool_get_info;
int bsg_pool_get(bsg_engine* eng, bsg_pool* pool,
                 const uint8_t* refs, uint64_t nrefs,   /* host, nrefs x 32 */
                 uint8_t* d_out, uint64_t out_cap,      /* device, or NULL with 0 */
                 int flags,
                 uint64_t* idx,      /* host, nrefs: blob index or UINT64_MAX; or NULL */
                 uint64_t* out_off,  /* host, nrefs + 1; or NULL */
                 bsg_pool_get_info* info);

/* Empties a pool for reuse, so two pools can alternate as source and destination: the counters go
 * to zero, the index, the table and the used bytes are refilled as at creation, where[] and remap
 * are dropped (their device pointers return NULL). A dead pool is usable again. Afterwards the
 * pool is indistinguishable from a new one of the same capacity: the same puts give the same
 * bytes. Synchronised before it returns. BSG_EINVAL for a null pool. */
int bsg_pool_reset(bsg_pool* p);

/* bsg_engine_walk and bsg_engine_restore_walk on a pool where it lies: the pool's device table and
 * device index in the place of the host table and the per-call index, so nothing of the pool
 * crosses the host link. Every rule, verdict, order of errors and output is theirs
 * (bsg_engine_copy_walk and bsg_engine_walk_records_device serve the result as before); two codes
 * come first: BSG_EINVAL for a null pool or one on another device than the engine, BSG_ESTATE for
 * a dead pool. The pool's mutex is held for the call. bsg_pool_restore_walk refuses an output
 * range that intersects the pool's allocation (BSG_EINVAL). */
int bsg_pool_walk(bsg_engine* eng, bsg_pool* pool, const uint8_t* roots, uint32_t nstreams,
                  int flags, int32_t* status, bsg_walk_info* info);
int bsg_pool_restore_walk(bsg_engine* eng, bsg_pool* pool, uint8_t* d_out, uint64_t out_cap,
                          const uint64_t* out_off, uint32_t nstreams, int flags,
                          bsg_restore_info* info);

/* ---- byte ranges of streams read out of a pool: split.Reader's Seek + Read for many ranges ---- */
/* split.Reader's Seek followed by Read (split/split.go:194-298) descends from the Root by the
 * children's offsets, fetches only the nodes on the way and the chunks under the requested bytes,
 * and discards the part of the first chunk before the position. bsg_engine_read does that for
 * many ranges at once: the work and the workspace grow with the bytes asked for, not with the
 * streams' sizes, and blobs far from a range need not be in the pool. The pool means what it
 * means for bsg_engine_walk: blobs may start at any byte, of two blobs under one ref the one with
 * the smaller index is used, refs are trusted labels. The same Root may appear in many ranges.
 * What a range means. Range q is bytes [offset, offset + len) of the stream under ranges[q].root,
 * offset + len saturating at 2^64 - 1. With size the Root node's size (0 for 32 zero bytes, an
 * empty stream), got[q] = min(len, size - min(offset, size)): an offset at or past the end gives
 * got[q] == 0 and status BSG_OK, the Reader's EOF with n == 0. On success
 * d_out[out_off[q] .. + got[q]) holds bytes [offset, offset + got[q]) of the stream and no other
 * byte of d_out is written: the rest of a range's len bytes, the gaps between ranges and the tail
 * of a range's last 16-byte vector stay as they were.
 * What is visited. The Root blob of every non-zero Root is visited, whatever the range, and held
 * to the walk's node rules (a Root's offset is 0). Child i of a visited node covers the bytes from
 * its offset to the next child's offset (the last one to the node's offset + size), as in the
 * walk; it is followed if and only if its cover has a byte in [offset, offset + len). A followed
 * `nodes` child is probed, read, held to its cover and validated, and a followed `leaves` child
 * probed and its table len held to its cover, exactly as in bsg_engine_walk; `nodes` children at
 * depth 64 are refused unread. A child that is not followed is neither probed nor read: the pool
 * need not hold it and its bytes are never examined, but the node that lists it must still parse
 * as a whole, and a visited node whose last child starts at or past the node's end (an empty
 * cover) is corrupt whatever the range. status[q], info and the output are therefore a function
 * of the arguments alone. status[q] is BSG_ENOTFOUND if the Root or a followed child is not in
 * the pool, else BSG_ECORRUPT if a visited node or a followed child's cover breaks a rule, else
 * BSG_OK.
 * BSG_READ_VERIFY. The structural walk runs first, on trusted labels; it is bounded and
 * range-checked whatever the bytes are. Then every distinct touched blob (the visited nodes and
 * the followed leaves) is hashed once on the engine's hash runs and held to its ref, before a
 * byte of d_out is written. Untouched blobs are not hashed, so `verified` is a fraction of the
 * pool. The hash path's layout rules (bsg_engine_hash) apply to the touched blobs only: d_pool
 * and their offsets multiples of 16, lens under 2^40, BSG_READ_SLACK readable bytes of pool_bytes
 * after each of them.
 * All or nothing. Every verdict, verification included, is in before the scatter is launched: on
 * any failure d_out is untouched and got[] is zero.
 * Returns, in this order: BSG_EINVAL, before anything is enqueued, for a null pointer with a
 * non-zero count, nranges > 65,535, unknown flag bits, d_out or an out_off[q] not a multiple of
 * 16, an out_off[q] beyond out_cap, an out_off[q] + len that exceeds out_cap when len is below
 * 2^63 (a larger len is held to the stream's size), or a blob that ends past pool_bytes;
 * BSG_EINVAL, once the sizes are back, for an out_off[q] + got[q] beyond out_cap, two ranges'
 * [out_off, out_off + got) that intersect or one that intersects the pool (got taken from the
 * Root node's size whatever the range's status); BSG_ENOTFOUND if any range's status is that;
 * BSG_ECORRUPT if any range's status is that; with the flag, BSG_EINVAL if a touched blob breaks
 * a layout rule above, then BSG_ECORRUPT if a touched blob's SHA-256 is not its ref (bad_blob);
 * BSG_ESTATE if the engine has an enqueued, unfinished run; BSG_ENOMEM; BSG_EDEVICE for a device
 * sanity word. status and info's bad_range, nnodes and depth are filled whenever both groups of
 * layout rules held, nleaves when every status is BSG_OK, bad_blob and verified when the hash
 * runs have finished. Synchronous, on the engine's stream. The read owns its workspace and publishes
 * nothing: the engine's last run, dedup result, tree, walk, restore and gc results stay valid,
 * and an engine needs no run before it reads. */
typedef struct bsg_read_range {
  uint8_t  root[32];   /* the stream's Root; 32 zero bytes: an empty stream */
  uint64_t offset;     /* Seek(offset, io.SeekStart) */
  uint64_t len;        /* len(buf) */
} bsg_read_range;      /* 48 bytes */
#define BSG_READ_VERIFY 1 /* hash every blob the read touches, and only those */
typedef struct bsg_read_info {
  uint64_t bad_range;  /* smallest range index whose status is not BSG_OK, else UINT64_MAX */
  uint64_t bad_blob;   /* with the flag: smallest touched pool blob whose bytes do not hash to its
                        * ref, else UINT64_MAX */
  uint64_t nnodes;     /* node blobs visited, over all ranges (a node shared by two ranges counts
                        * twice, as in the walk) */
  uint64_t nleaves;    /* leaf children followed, over all ranges */
  uint64_t bytes;      /* sum of got[] (0 on any failure) */
  uint64_t verified;   /* with the flag: sum of len over the distinct touched blobs */
  uint32_t depth, reserved;
} bsg_read_info;
int bsg_engine_read(bsg_engine* eng,
                    const uint8_t* d_pool, uint64_t pool_bytes,            /* device */
                    const bsg_pool_blob* blobs, uint64_t nblobs,           /* host */
                    const bsg_read_range* ranges, uint32_t nranges,        /* host */
                    uint8_t* d_out, uint64_t out_cap,                      /* device */
                    const uint64_t* out_off,                               /* host, nranges */
                    int flags,
                    int32_t* status, uint64_t* got,                        /* host, nranges, or NULL */
                    bsg_read_info* info);                                  /* or NULL */
/* bsg_engine_read on a pool where it lies, as bsg_pool_walk is bsg_engine_walk: the pool's device
 * table and device index in the place of the host table and the per-call index. Every rule,
 * verdict, order of errors and output is bsg_engine_read's; two codes come first: BSG_EINVAL for a
 * null pool or one on another device than the engine, BSG_ESTATE for a dead pool. The pool's mutex
 * is held for the call, and an output that intersects the pool's allocation is refused
 * (BSG_EINVAL). */
int bsg_pool_read(bsg_engine* eng, bsg_pool* pool, const bsg_read_range* ranges, uint32_t nranges,
                  uint8_t* d_out, uint64_t out_cap, const uint64_t* out_off, int flags,
                  int32_t* status, uint64_t* got, bsg_read_info* info);

/* Per-stage HIP event timing of later runs, and the last finished run's stage durations in
 * ms: [0] rolling scan (k_scan), [1] prefix/compact/select/chunks, [2] SHA-256 (k_sha, and the
 * early chains' tail). Timed on the engine's own stream. enable: 0 off, 1 every stage (four
 * events per run), 2 the SHA-256 stage only (two events; [0] and [1] read -1). Each event on
 * the stream costs the run time. */
int bsg_engine_profile(bsg_engine* eng, int enable);
int bsg_engine_stage_ms(const bsg_engine* eng, float out[3]);
/* Diagnostics of the last run: [0] jobs on the wave-per-chunk path, [1] its block threshold,
 * [2] longest job (blocks), [3..7] one long job's s_memtime start/end, s_memrealtime
 * start/end (100 MHz) and block count, [8..12] the same for the longest per-lane job,
 * [13] per-lane job count. */
int bsg_engine_diag(const bsg_engine* eng, uint64_t out[16]);
/* The host tail of the last finished run (BSG_KNOB_HOST_TAIL): a run of 512 MiB to
 * BSG_KNOB_LIGHT_BYTES may hash its longest chunks on up to 16 host threads while the GPU hashes
 * the rest; the data and the records stay in device memory, those chunks' bytes cross the link
 * once. [0] chunks and [1] ring bytes handed to the host (0: none, or no such run), [2] the cut
 * in SHA-256 blocks, [3] the gather kernel's time in us (HIP events), [4] the last host hash's
 * end in us after the run was enqueued, [5] the implementation (0 portable, 1 x86 SHA
 * extensions), [6] worker threads, [7] one worker's measured rate in bytes/s, [8] the run's
 * longest chunk in blocks and [9] the longest left on the GPU, [10] blocks hashed on the host,
 * [11] 1 if cpuid reports the SHA extensions. With a tail, bsg_engine_diag's longest job and
 * block total are those of the GPU's share. */
int bsg_engine_host_tail(const bsg_engine* eng, uint64_t out[12]);
/* Diagnostic timeline of the last run's k_sha, in 100 MHz s_memrealtime ticks: first wave
 * started, longest wave-mode job started / ended, last wave left per-lane mode. */
int bsg_engine_timeline(const bsg_engine* eng, uint64_t out[4]);
/* Last run's candidate count (diagnostics). */
uint64_t bsg_engine_candidates(const bsg_engine* eng);

/* Convenience: split + hash host-resident streams (copies to the device), results to host.
 * Any number of streams: they run in groups of at most 65,535 streams and ~8 GiB. Records are
 * in stream order, `stream` = the index in this call; at most cap are written, *nchunks is the
 * total. */
int bsg_split_hash_batch(int device, const uint8_t* host_data, const uint64_t* off,
                         const uint64_t* len, uint32_t nstreams, const bsg_params* params,
                         const uint32_t* table, bsg_chunk* out, uint64_t cap, uint64_t* counts,
                         uint64_t* nchunks);

/* Batched SHA-256 of n blobs base[off[i] .. off[i]+len[i]); base may be host or device memory;
 * refs receives n*32 bytes (host). base and off[i] need no alignment; the blobs may lie in any
 * order, with gaps, and may overlap or coincide. base[0 .. max(off[i]+len[i])) must be readable
 * (a small batch is copied whole, gaps included, to a private device buffer with its own read
 * slack, so nothing past the last blob is read). BSG_EINVAL if an off[i] + len[i] wraps. The
 * same holds for bsg_hasher_sum. */
int bsg_sha256_batch(int device, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                     uint32_t n, uint8_t* refs);

/* The same with persistent device buffers and a HIP stream of its own (one per thread at a
 * time), for callers that hash many small batches (tree nodes, store Puts). */
typedef struct bsg_hasher bsg_hasher;
bsg_hasher* bsg_hasher_new(int device);
int bsg_hasher_sum(bsg_hasher* h, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                   uint32_t n, uint8_t* refs);
/* The same for scattered blobs: blob i is ptrs[i][0 .. len[i]) (host memory), e.g. the chunks a
 * store holds separately. Large batches (>= 16 blobs and 4 MiB) are packed into pinned staging
 * and hashed in bsg_engine_hash mode; small ones by one blob per lane. */
int bsg_hasher_sum_ptrs(bsg_hasher* h, const uint8_t* const* ptrs, const uint64_t* len,
                        uint32_t n, uint8_t* refs);
void bsg_hasher_free(bsg_hasher* h);
/* Diagnostics: bytes of pinned host memory the hasher holds (its small-batch buffer, its
 * metadata and record buffers, its large-batch staging). A large blob hashed through the
 * small-batch path is copied from pageable memory and does not grow it. */
size_t bsg_hasher_pinned_bytes(const bsg_hasher* h);

/* Device memory helpers (so callers need no second HIP runtime): kind 0 = H2D, 1 = D2H,
 * 2 = D2D. */
void* bsg_device_malloc(int device, size_t bytes);
int bsg_device_free(int device, void* p);
int bsg_memcpy(int device, void* dst, const void* src, size_t n, int kind);
int bsg_device_synchronize(int device);

/* Utility (benchmarks/tests, not part of the reference surface): fill device memory with the
 * SplitMix64 counter stream of bs_amd/synth.py (word i = splitmix64(seed + (i+1)*0x9E37...)). */
int bsg_fill_splitmix(int device, uint8_t* d_ptr, uint64_t nbytes, uint64_t seed, void* stream);

/* ---- C++ host mirror of split.Writer / split.Reader / store/mem (bs_split.hpp), exposed for
 * C callers and tests ---- */
typedef struct bsg_store bsg_store;   /* a bs.Store; every Put's ref comes from the GPU */
bsg_store* bsg_memstore_new(int device);   /* store/mem  (store/mem/mem.go:17-124) */
/* store/file (store/file/file.go:20-154): blobs at <root>/blobs/<hex[:2]>/<hex[:4]>/<hex>. */
bsg_store* bsg_filestore_new(const char* root, int device);
void bsg_store_free(bsg_store* s);
size_t bsg_store_count(const bsg_store* s);
/* store/file writes split.Writer's chunks behind (bs::FileStore::PutBlob): at most `bytes` of
 * accepted, unwritten blobs are pending before a Put waits (default 1 GiB). BSG_EINVAL for
 * store/mem. */
int bsg_filestore_set_write_behind(bsg_store* s, uint64_t bytes);
/* Bytes of host memory a store/mem keeps alive: its own blob copies plus, once each, the Write
 * pieces its chunks alias (split.Writer hands chunks over without copying). 0 for store/file. */
size_t bsg_store_held_bytes(const bsg_store* s);
/* Get: copies min(cap, len) bytes, *n = blob length; returns BSG_ENOTFOUND if absent. */
int bsg_store_get(bsg_store* s, const uint8_t ref[32], uint8_t* out, size_t cap, size_t* n);
int bsg_store_put(bsg_store* s, const uint8_t* data, size_t n, uint8_t ref_out[32], int* added);
/* Put with a ref the caller already has (a chunk record's ref): no hash is computed, the store
 * trusts the ref (bs::RefPutter in bs_split.hpp). Needs no GPU. */
int bsg_store_put_ref(bsg_store* s, const uint8_t ref[32], const uint8_t* data, size_t n,
                      int* added);
/* ListRefs(start, f) (store.go:13-24; mem.go:39-59, file.go:83-160): refs > start in lexicographic order, up to cap of them
 * into refs (32 bytes each); returns the total count after start. */
size_t bsg_store_list_from(bsg_store* s, const uint8_t start[32], uint8_t* refs, size_t cap);
/* All refs in lexicographic order (32 bytes each, up to cap); returns the total count. */
size_t bsg_store_list(bsg_store* s, uint8_t* refs, size_t cap);
/* bs.DeleterStore.Delete (store.go:50-54) for store/mem (mem.go:79-85): absent refs are not an
 * error. BSG_EINVAL for store/file, which is not a DeleterStore in the reference. */
int bsg_store_delete(bsg_store* s, const uint8_t ref[32]);
/* split.Protect (split/split.go:306-322), gc's traversal of a split tree: the children of the
 * Node stored at ref, child nodes first (traverse[i] = 1: protect them recursively), then its
 * leaves (traverse[i] = 0). Up to cap refs (32 bytes each); *n = the number of children. */
int bsg_split_protect(bsg_store* s, const uint8_t ref[32], uint8_t* refs, uint8_t* traverse,
                      size_t cap, size_t* n);

typedef struct bsg_writer bsg_writer; /* split.NewWriter / Write / Close / Root */
bsg_writer* bsg_writer_new(int device, bsg_store* s, const bsg_params* params, size_t tile,
                           int* err);
int bsg_writer_write(bsg_writer* w, const uint8_t* p, size_t n);
int bsg_writer_close(bsg_writer* w);
/* Tests: bsg_set_stream_base for the Writer's context, before the first bsg_writer_write; the
 * Writer's tree and Root are unchanged (tree offsets start at 0, as split.Writer's). */
int bsg_writer_set_stream_base(bsg_writer* w, uint64_t base);
int bsg_writer_root(const bsg_writer* w, uint8_t out[32]);
/* Where the Writer's time went, in seconds: [0] Write copies (into its pieces and pinned
 * staging), [1] chunk records processed on its background thread (store Puts + the tree,
 * overlapping the copies), [2] Writes and Close waiting for that thread, [3] tree-node hashes
 * on the GPU, [4] Close, [5] of which waiting for the last tiles on the device, [6] tree-node
 * hash calls. */
int bsg_writer_timings(const bsg_writer* w, double out[7]);
void bsg_writer_free(bsg_writer* w);

typedef struct bsg_reader bsg_reader; /* split.NewReader / Read / Seek / Size */
bsg_reader* bsg_reader_new(bsg_store* s, const uint8_t root[32], int* err);
/* flags: BSG_READER_VERIFY = check every fetched chunk's SHA-256 against its ref: a window of
 * leaf nodes (up to 256 MiB; BSG_VERIFY_WINDOW bytes if set) per batched GPU call, the next
 * window verified in the background while this one is read; a read that needs a chunk of a
 * window that failed returns BSG_ECORRUPT. */
#define BSG_READER_VERIFY 1
bsg_reader* bsg_reader_open(bsg_store* s, const uint8_t root[32], int flags, int device,
                            int* err);
int64_t bsg_reader_read(bsg_reader* r, uint8_t* buf, size_t n); /* bytes; 0 at EOF; <0 error */
int64_t bsg_reader_seek(bsg_reader* r, int64_t off, int whence);
uint64_t bsg_reader_size(const bsg_reader* r);
/* Verify-mode diagnostics: out[0] windows verified on the reading thread, out[1] windows taken
 * from the background read-ahead, out[2] bytes verified, out[3] read-ahead windows dropped (a
 * seek made them stale). */
int bsg_reader_stats(const bsg_reader* r, uint64_t out[4]);
void bsg_reader_free(bsg_reader* r);

/* ---- test and debug knobs (process-wide; each starts from its environment variable) ---- */
#define BSG_KNOB_SEQ_WAIT 1      /* BSG_DEBUG_SEQ_WAIT: polls of a k_sha helper handshake before
                                  * it flags a device error (0: fail at once; tests) */
#define BSG_KNOB_LONG_MODE 2     /* BSG_LONG_MODE: wave-mode tiers 0 auto, 1 off, 2 all */
#define BSG_KNOB_VERIFY_WINDOW 3 /* BSG_VERIFY_WINDOW: split::Reader verify window in bytes
                                  * (0: 256 MiB), read when a Reader is opened */
#define BSG_KNOB_EARLY 4         /* BSG_EARLY: 1 (default) hashes the two longest chunks whose
                                  * ends are sure boundaries on a second stream from right after
                                  * candidate compaction (engine runs of >= 256 MiB); 0 off */
#define BSG_KNOB_POLL 5          /* BSG_POLL: 1 (default) makes bsg_engine_finish poll its stream
                                  * (with a CPU pause between queries, for at most 100 ms, then it
                                  * blocks: no interrupt wake-up latency on a step-sized run); 0
                                  * blocks in hipStreamSynchronize at once */
#define BSG_KNOB_COPY_NT 6       /* BSG_COPY_NT: 1 (default) copies Write bytes into pinned
                                  * staging (and the Writer's pieces) with non-temporal stores;
                                  * 0 uses memcpy */
#define BSG_KNOB_LIGHT_BYTES 7  /* engine runs of at most this many bytes (default 4 GiB) keep
                                  * their early chains on the engine stream and move selection
                                  * and k_sha to the second stream; larger runs the other way
                                  * (tests run one input both ways) */
#define BSG_KNOB_HOST_TAIL 8    /* BSG_HOST_TAIL: 1 (default) lets an engine run of 512 MiB to
                                  * BSG_KNOB_LIGHT_BYTES hash its longest chunks on host threads
                                  * (bsg_engine_host_tail); 0 keeps every chunk on the GPU */
#define BSG_KNOB_LAST BSG_KNOB_HOST_TAIL
int bsg_debug_set(int knob, int64_t value);
int64_t bsg_debug_get(int knob); /* -1 for an unknown knob */

#ifdef __cplusplus
}
#endif
#endif /* BSGPU_H */
