// host_blobpool.h — bsg_pool, bsg_engine_pool_put and bsg_pool_collect: a pool of blobs that lives
// in device memory across runs, the last finished run's new chunks and tree nodes appended to it,
// and a pool's live blobs collected into an empty pool (included by host_engine.h). Not
// host_pool.h (the copy threads) and not DevicePool (idle engines).
#pragma once

// The pool owns its bytes, its blob table and its index of blob indices by ref, none of which
// ever moves, and the buffers of its own passes. Every entry point takes `mu` and has
// synchronised the stream it used before it lets go, so engines on several threads may put into
// one pool.
struct bsg_pool {
  int dev = 0;
  std::mutex mu;
  DevBuf bytes, table, index;       // fixed at creation
  uint64_t cap_bytes = 0, cap_blobs = 0;
  uint64_t slots = 0;               // of index (a power of two)
  uint64_t nblobs = 0, used = 0;    // table entries; the end of the last blob's last byte
  uint64_t blob_bytes = 0;          // the blobs' lens, summed
  bool dead = false;                // a device error during an append: BSG_ESTATE from then on
  DevBuf where;                     // the last successful put's items -> blob indices
  uint64_t nwhere = 0;
  bool put_done = false;
  DevBuf remap;                     // the last collect into this pool: the source's blob indices ->
  uint64_t nremap = 0;              //   this pool's, ~0 for a dead blob
  bool collect_done = false;
  DevBuf off16, seg16, hdr;         // a put's own buffers
  PinBuf h_hdr;
  DedupWork work;
  Marks marks;                      // profile
  float ms[4] = {0, 0, 0, 0};       // profile: first occurrence + offsets, append, gather, where
  float adopt_ms = 0;               // profile: the last collect's k_pool_adopt

  static uint64_t pad16(uint64_t x) { return (x + 15) & ~15ull; }
  uint64_t pool_bytes() const { return pad16(cap_bytes) + kReadSlack; }

  int create(int device, uint64_t cbytes, uint64_t cblobs) {
    dev = device;
    cap_bytes = cbytes;
    cap_blobs = cblobs;
    slots = pow2_at_least(2 * std::max<uint64_t>(cblobs, 1));
    if (pad16(cbytes) < cbytes || cblobs > (1ull << 40)) return BSG_ENOMEM;
    MCHECK(bytes.exact(pool_bytes()));
    MCHECK(table.exact(sizeof(PoolBlob) * std::max<uint64_t>(cblobs, 1)));
    MCHECK(index.exact(8 * slots));
    MCHECK(hdr.ensure(sizeof(PoolHdr)));
    MCHECK(h_hdr.ensure(sizeof(PoolHdr)));
    HCHECK(hipMemset(bytes.p, 0, pool_bytes()));
    HCHECK(hipMemset(table.p, 0, table.cap));
    HCHECK(hipMemset(index.p, 0xFF, 8 * slots));
    // (a fill of device memory may return before it is done, and the engines' streams do not
    // wait for the null stream)
    HCHECK(hipStreamSynchronize(nullptr));
    return BSG_OK;
  }

  int readback(hipStream_t s, PoolHdr* h) {
    return read_header(h_hdr, hdr.p, s, h, [](const PoolHdr& p) { return p.dd.error; }, "pool put");
  }

  // The items of a put: the view's records (with BSG_POOL_CHUNKS), then `tree`'s nodes (null:
  // none). Which of them are new and what they need is decided on the device and read back before
  // anything of the pool is written. (The caller holds mu and has checked the states.)
  int put(const RunView& v, const TreeWork* tree, int flags, bsg_pool_put_info* info) {
    static_assert(sizeof(ChunkRec) == sizeof(TreeNode) &&
                      offsetof(ChunkRec, ref) == offsetof(TreeNode, ref) &&
                      offsetof(ChunkRec, len) == offsetof(TreeNode, blob_len),
                  "records and nodes are one kind of item");
    const hipStream_t s = v.stream;
    auto stamp = [&](size_t i) { v.profile ? marks.record(i, s) : void(); };
    const uint64_t nrec = (flags & BSG_POOL_CHUNKS) ? v.nrec : 0;
    const uint64_t nn = tree ? tree->plan.nn : 0;
    const uint64_t n = nrec + nn;
    bsg_pool_put_info out{};
    out.items = n;
    out.first_blob = out.need_blobs = nblobs;
    out.need_bytes = used;
    *info = out;
    if (!n) {
      nwhere = 0;
      put_done = true;
      return BSG_OK;
    }

    int rc;
    if ((rc = work.reserve(n))) return rc;
    MCHECK(off16.ensure(8 * (n + 1)));
    MCHECK(seg16.ensure(8 * (n + 1)));
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(v.rec);
    PoolArgs a{};
    a.d = work.args(rec + offsetof(ChunkRec, ref), sizeof(ChunkRec), rec + offsetof(ChunkRec, len),
                    sizeof(ChunkRec), n);
    a.d.n1 = nrec;
    if (nn) {
      const uint8_t* nd = tree->nodes.as<uint8_t>();
      a.d.refs2 = nd + offsetof(TreeNode, ref);
      a.d.lens2 = nd + offsetof(TreeNode, blob_len);
      a.nodes = tree->nodes.as<TreeNode>();
      a.arena = tree->arena.as<uint8_t>();
      a.arena_bytes = tree->plan.arena;
    }
    a.d.set_keys = table.as<uint8_t>() + offsetof(PoolBlob, ref);
    a.d.set_stride = sizeof(PoolBlob);
    a.d.set_tab = index.as<uint64_t>();
    a.d.set_mask = slots - 1;
    a.d.set_count = nblobs;
    a.hdr = hdr.as<PoolHdr>();
    a.d.hdr = &a.hdr->dd;
    a.data = v.d_data;
    a.streams = v.streams;
    a.nstreams = v.ns;
    a.rec = v.rec;
    a.off16 = off16.as<uint64_t>();
    a.seg16 = seg16.as<uint64_t>();
    a.bytes = bytes.as<uint8_t>();
    a.table = table.as<PoolBlob>();
    a.index = index.as<uint64_t>();
    a.index_mask = slots - 1;
    a.nblobs = nblobs;
    a.base = pad16(used);

    // first occurrence and offsets: the call's own buffers and the header, nothing of the pool
    stamp(0);
    HCHECK(hipMemsetAsync(hdr.p, 0, sizeof(PoolHdr), s));
    HCHECK(work.tab.clear(s));
    HCHECK(dbg("launch_dedup", s, launch_dedup(a.d, s, v.num_cus)));
    HCHECK(dbg("launch_pool_plan", s, launch_pool_plan(a, s, v.num_cus)));
    stamp(1);
    PoolHdr h;
    if ((rc = readback(s, &h))) return rc;
    if (h.dd.nunique > n || h.total16 % 16 || pad16(h.last_len) > h.total16 ||
        (h.dd.nunique == 0) != (h.total16 == 0) || h.dd.unique_bytes > h.total16)
      return BSG_EDEVICE;
    out.added = h.dd.nunique;
    out.added_bytes = h.dd.unique_bytes;
    out.known = h.known;
    out.repeats = h.repeats;
    out.need_blobs = nblobs + out.added;
    if (out.added) out.need_bytes = a.base + h.total16 - (pad16(h.last_len) - h.last_len);
    *info = out;
    if (out.need_bytes > cap_bytes || out.need_bytes < used || out.need_blobs > cap_blobs)
      return BSG_ENOMEM;
    DevBuf grown;  // (a failed put keeps the last one's where[])
    if (where.cap < 8 * n) MCHECK(grown.ensure(8 * n));
    a.where = grown.p ? grown.as<uint64_t>() : where.as<uint64_t>();
    a.nnew = out.added;
    a.total16 = h.total16;

    // the append: table and index, bytes, where[]
    stamp(2);
    hipError_t e = dbg("launch_pool_append", s, launch_pool_append(a, s, v.num_cus));
    stamp(3);
    if (e == hipSuccess) e = dbg("launch_pool_gather", s, launch_pool_gather(a, s));
    stamp(4);
    if (e == hipSuccess) e = dbg("launch_pool_where", s, launch_pool_where(a, s, v.num_cus));
    stamp(5);
    rc = e == hipSuccess ? readback(s, &h) : BSG_EDEVICE;
    if (rc) {  // the table, the index or the bytes may be half written
      (void)hipGetLastError();
      (void)hipStreamSynchronize(s);
      dead = true;
      return BSG_EDEVICE;
    }
    if (grown.p) where = std::move(grown);
    nwhere = n;
    put_done = true;
    nblobs = out.need_blobs;
    used = out.need_bytes;
    blob_bytes += out.added_bytes;
    for (int i = 0; i < 4; ++i) ms[i] = 0.f;
    if (v.profile) {
      ms[0] = marks.ms(0, 1);
      for (int i = 1; i < 4; ++i) ms[i] = marks.ms(i + 1, i + 2);
    }
    return BSG_OK;
  }

  // the table and the index where they lie, for a walk, a restore or a mark (the caller holds mu)
  PoolSrc source() const {
    return PoolSrc{table.as<const PoolBlob>(), index.as<uint64_t>(), slots - 1, used, blob_bytes};
  }

  // bsg_pool_collect: `src` marked from the Roots by gc (the engine's, whose current result the
  // mark becomes), then its live blobs appended to this empty pool. The mark, the offsets and the
  // readback of the totals write gc's buffers only; nothing of this pool is written before they
  // have been held to its capacity. (The caller holds both mutexes and has checked the states.)
  int collect(const RunView& v, GcWork& gc, const bsg_pool& src, const uint8_t* roots,
              uint64_t nroots, int flags, int32_t* status, bsg_pool_collect_info* info) {
    const hipStream_t s = v.stream;
    const PoolSrc ps = src.source();
    const uint64_t n = src.nblobs;
    int rc = gc.mark(v, src.bytes.as<const uint8_t>(), src.pool_bytes(), nullptr, n, roots, nroots,
                     flags, status, &info->gc, &ps);
    if (rc) return rc;
    info->need_blobs = gc.nlive;
    info->need_bytes = gc.end16;
    if (gc.nlive > cap_blobs || gc.end16 > cap_bytes) return BSG_ENOMEM;
    DevBuf map;  // (a failed collect keeps the last one's remap)
    MCHECK(map.ensure(8 * n));

    AdoptArgs a{};
    a.src = ps.table;
    a.n = n;
    a.live = gc.live.as<const uint8_t>();
    a.rank = gc.rank.as<const uint64_t>();
    a.noff16 = gc.noff16.as<const uint64_t>();
    a.nlive = gc.nlive;
    a.total = gc.end16;
    a.table = table.as<PoolBlob>();
    a.index = index.as<uint64_t>();
    a.index_mask = slots - 1;
    a.remap = map.as<uint64_t>();
    a.hdr = &hdr.as<PoolHdr>()->dd;
    if (v.profile) marks.record(6, s);
    hipError_t e = hipMemsetAsync(hdr.p, 0, sizeof(PoolHdr), s);
    if (e == hipSuccess) e = dbg("launch_pool_adopt", s, launch_pool_adopt(a, s, v.num_cus));
    if (v.profile) marks.record(7, s);
    PoolHdr h;
    rc = e == hipSuccess ? readback(s, &h) : BSG_EDEVICE;
    uint64_t wrote = 0;
    if (!rc)
      rc = gc.compact(v, src.bytes.as<const uint8_t>(), src.pool_bytes(), bytes.as<uint8_t>(),
                      cap_bytes, BSG_GC_ALIGN16, &wrote);
    if (rc || wrote != gc.end16) {  // the table, the index or the bytes may be half written
      (void)hipGetLastError();
      (void)hipStreamSynchronize(s);
      dead = true;
      return BSG_EDEVICE;
    }
    remap = std::move(map);
    nremap = n;
    collect_done = true;
    nblobs = gc.nlive;
    used = gc.end16;
    blob_bytes = info->gc.live_bytes;
    adopt_ms = v.profile ? marks.ms(6, 7) : 0.f;
    return BSG_OK;
  }

  // bsg_pool_reset: a new pool of the same capacity in the place of this one, dead or not. What a
  // put or a collect may have written is refilled: the index, the table's entries and the bytes in
  // use, or all of both after a device error. (The caller holds mu.)
  int reset() {
    const uint64_t nb = dead ? pool_bytes() : pad16(used);
    const uint64_t nt = dead ? table.cap : sizeof(PoolBlob) * nblobs;
    if (nb) HCHECK(hipMemset(bytes.p, 0, nb));
    if (nt) HCHECK(hipMemset(table.p, 0, nt));
    HCHECK(hipMemset(index.p, 0xFF, 8 * slots));
    HCHECK(hipStreamSynchronize(nullptr));  // (as create)
    where.release();
    remap.release();
    nwhere = nremap = 0;
    put_done = collect_done = false;
    nblobs = used = blob_bytes = 0;
    for (float& m : ms) m = 0.f;
    adopt_ms = 0.f;
    dead = false;
    return BSG_OK;
  }
};
