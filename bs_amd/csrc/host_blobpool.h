// host_blobpool.h — bsg_pool, bsg_engine_pool_put and bsg_pool_collect: a pool of blobs that lives
// in device memory across runs, the last finished run's new chunks and tree nodes appended to it,
// and a pool's live blobs collected into an empty pool (included by host_engine.h). The put of a
// caller's blobs (host_blobs.h) goes through the same put_items. Not host_pool.h (the copy
// threads) and not DevicePool (idle engines).
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
    const uint64_t nrec = (flags & BSG_POOL_CHUNKS) ? v.nrec : 0;
    const uint64_t nn = tree ? tree->plan.nn : 0;
    return put_items(
        v, nrec + nn, false, info,
        [&](PoolArgs& a) {
          const uint8_t* rec = reinterpret_cast<const uint8_t*>(v.rec);
          a.d.refs = rec + offsetof(ChunkRec, ref);
          a.d.lens = rec + offsetof(ChunkRec, len);
          a.d.stride = a.d.len_stride = sizeof(ChunkRec);
          a.d.n1 = nrec;
          if (nn) {
            const uint8_t* nd = tree->nodes.as<uint8_t>();
            a.d.refs2 = nd + offsetof(TreeNode, ref);
            a.d.lens2 = nd + offsetof(TreeNode, blob_len);
            a.nodes = tree->nodes.as<TreeNode>();
            a.arena = tree->arena.as<uint8_t>();
            a.arena_bytes = tree->plan.arena;
          }
          a.data = v.d_data;
          a.streams = v.streams;
          a.nstreams = v.ns;
          a.rec = v.rec;
        },
        [](const PoolArgs&) { return BSG_OK; },
        [&](const PoolArgs& a) { return dbg("launch_pool_gather", s, launch_pool_gather(a, s)); });
  }

  // A put of n items, whatever they are. items(a) names them: a.d's refs and lens, and what the
  // gather needs to find their bytes; refs(a) enqueues what makes the refs, if they do not stand
  // yet (bsg_pool_put_blobs: the hash runs; its device checks flag a.d.hdr); gather(a) launches
  // the new blobs' bytes. empty_ok: an item may have no bytes (a run's chunks and nodes all have
  // some, so new items without bytes are a fault there).
  template <class Items, class Refs, class Gather>
  int put_items(const RunView& v, uint64_t n, bool empty_ok, bsg_pool_put_info* info, Items items,
                Refs refs, Gather gather) {
    const hipStream_t s = v.stream;
    auto stamp = [&](size_t i) { v.profile ? marks.record(i, s) : void(); };
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
    PoolArgs a{};
    a.d = work.args(nullptr, 0, nullptr, 0, n);
    items(a);
    a.d.set_keys = table.as<uint8_t>() + offsetof(PoolBlob, ref);
    a.d.set_stride = sizeof(PoolBlob);
    a.d.set_tab = index.as<uint64_t>();
    a.d.set_mask = slots - 1;
    a.d.set_count = nblobs;
    a.hdr = hdr.as<PoolHdr>();
    a.d.hdr = &a.hdr->dd;
    a.off16 = off16.as<uint64_t>();
    a.seg16 = seg16.as<uint64_t>();
    a.bytes = bytes.as<uint8_t>();
    a.table = table.as<PoolBlob>();
    a.index = index.as<uint64_t>();
    a.index_mask = slots - 1;
    a.nblobs = nblobs;
    a.base = pad16(used);

    // first occurrence and offsets: the call's own buffers and the header, nothing of the pool
    HCHECK(hipMemsetAsync(hdr.p, 0, sizeof(PoolHdr), s));
    if ((rc = refs(a))) return rc;
    stamp(0);
    HCHECK(work.tab.clear(s));
    HCHECK(dbg("launch_dedup", s, launch_dedup(a.d, s, v.num_cus)));
    HCHECK(dbg("launch_pool_plan", s, launch_pool_plan(a, s, v.num_cus)));
    stamp(1);
    PoolHdr h;
    if ((rc = readback(s, &h))) return rc;
    if (h.dd.nunique > n || h.total16 % 16 || pad16(h.last_len) > h.total16 ||
        (h.dd.nunique == 0 && h.total16) || (!empty_ok && h.dd.nunique && !h.total16) ||
        h.dd.unique_bytes > h.total16)
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
    if (e == hipSuccess) e = gather(a);
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

// One direction of bsg_pool_merge / bsg_pool_sync: the selected blobs of `src` that `dst` lacks,
// appended behind what dst holds. The work owns every buffer it writes before the append, the
// remap included, so plan() and verify() write nothing of either pool and a call can run both
// directions of a sync that far before it commits either. (The caller holds both mutexes and has
// checked the states.)
struct MergeWork {
  DevBuf hdr, isnew, rank, off16, part, map, tpre, tlist, descs;
  PinBuf h_hdr;
  MergeArgs a{};
  uint64_t added_bytes = 0;
  Marks marks;                    // profile
  float ms[5] = {0, 0, 0, 0, 0};  // profile: probe, plan, verify, append, gather

  int readback(hipStream_t s, MergeHdr* h) {
    return read_header(h_hdr, hdr.p, s, h,
                       [](const MergeHdr& m) { return m.g.w.dd.error | m.r.dd.error; }, "pool merge");
  }

  // The probe and the plan. sel: a finished mark's live[] over src's blobs (null: every blob).
  // info's counts and need_* are filled; whether they fit is fits()'s to say.
  int plan(const RunView& v, const bsg_pool& src, const bsg_pool& dst, const uint8_t* sel,
           bsg_pool_merge_info* info) {
    const hipStream_t s = v.stream;
    auto stamp = [&](size_t i) { v.profile ? marks.record(i, s) : void(); };
    for (float& m : ms) m = 0.f;
    const uint64_t n = src.nblobs;
    a = MergeArgs{};
    a.n = n;
    a.dn = dst.nblobs;
    a.base = bsg_pool::pad16(dst.used);
    a.need_bytes = dst.used;
    added_bytes = 0;
    info->first_blob = info->need_blobs = dst.nblobs;
    info->need_bytes = dst.used;
    MCHECK(map.ensure(8 * n));
    if (!n) return BSG_OK;

    MCHECK(hdr.ensure(sizeof(MergeHdr)));
    MCHECK(h_hdr.ensure(sizeof(MergeHdr) + 16));
    MCHECK(isnew.ensure(n));
    MCHECK(rank.ensure(8 * (n + 1)));
    MCHECK(off16.ensure(8 * (n + 1)));
    MCHECK(part.ensure(8 * sum_parts(n)));
    a.src = src.table.as<const PoolBlob>();
    a.sel = sel;
    a.dtable = dst.table.as<const PoolBlob>();
    a.index = dst.index.as<uint64_t>();
    a.index_mask = dst.slots - 1;
    a.isnew = isnew.as<uint8_t>();
    a.rank = rank.as<uint64_t>();
    a.off16 = off16.as<uint64_t>();
    a.part = part.as<uint64_t>();
    a.remap = map.as<uint64_t>();
    a.hdr = hdr.as<MergeHdr>();
    a.cap_blobs = dst.cap_blobs;
    a.table = dst.table.as<PoolBlob>();

    stamp(0);
    HCHECK(hipMemsetAsync(hdr.p, 0, sizeof(MergeHdr), s));
    HCHECK(hipMemsetAsync(&a.hdr->r.bad_blob, 0xFF, 8, s));
    HCHECK(dbg("launch_pool_probe", s, launch_pool_probe(a, s, v.num_cus)));
    stamp(1);
    HCHECK(dbg("launch_pool_merge_plan", s, launch_pool_merge_plan(a, s, v.num_cus)));
    stamp(2);
    // the totals: the header, and the last word of each prefix
    uint64_t* tot = reinterpret_cast<uint64_t*>(h_hdr.as<uint8_t>() + sizeof(MergeHdr));
    HCHECK(hipMemcpyAsync(tot, a.rank + n, 8, hipMemcpyDeviceToHost, s));
    HCHECK(hipMemcpyAsync(tot + 1, a.off16 + n, 8, hipMemcpyDeviceToHost, s));
    MergeHdr h;
    if (int rc = readback(s, &h)) return rc;
    if (v.profile) {
      ms[0] = marks.ms(0, 1);
      ms[1] = marks.ms(1, 2);
    }
    const uint64_t nnew = tot[0], total16 = tot[1];
    if (h.selected > n || nnew + h.known != h.selected || h.end > total16 ||
        total16 - h.end > 15 || total16 % 16 || (nnew == 0 && total16) || h.added_bytes > total16)
      return BSG_EDEVICE;
    a.nnew = nnew;
    added_bytes = h.added_bytes;
    info->selected = h.selected;
    info->known = h.known;
    info->added = nnew;
    info->added_bytes = h.added_bytes;
    info->need_blobs = dst.nblobs + nnew;
    if (nnew) a.need_bytes = info->need_bytes = a.base + h.end;
    return BSG_OK;
  }

  // BSG_MERGE_VERIFY: the blobs plan() found new, and no others, hashed and held to their refs
  // (BSG_READ_VERIFY's passes, with isnew[] in the place of touched[]).
  int verify(const RunView& v, const bsg_pool& src, bsg_pool_merge_info* info) {
    const hipStream_t s = v.stream;
    info->verified = 0;
    if (!a.nnew) return BSG_OK;
    MCHECK(tpre.ensure(8 * (a.n + 1)));
    MCHECK(tlist.ensure(8 * a.nnew));
    TouchArgs t{};
    t.r.pool = src.bytes.as<const uint8_t>();
    t.r.pool_bytes = src.pool_bytes();
    t.r.blobs = a.src;
    t.r.nblobs = a.n;
    t.r.hdr = &a.hdr->r;
    t.r.touched = a.isnew;
    t.tpre = tpre.as<uint64_t>();
    t.tlist = tlist.as<uint64_t>();
    t.ntouched = a.nnew;
    t.verified = &a.hdr->verified;
    t.part = a.part;
    if (v.profile) marks.record(3, s);
    HCHECK(dbg("launch_read_touched", s, launch_read_touched(t, s, v.num_cus)));
    MergeHdr h;
    int rc;
    if ((rc = readback(s, &h))) return rc;
    // (a pool's blobs meet the hash path's layout rules by construction)
    if (h.r.invalid || h.verified != added_bytes) return BSG_EDEVICE;
    if ((rc = hash_touched(v, t, descs, src.used))) return rc;
    if (v.profile) marks.record(4, s);
    if ((rc = readback(s, &h))) return rc;
    if (v.profile) ms[2] = marks.ms(3, 4);
    info->verified = h.verified;
    info->bad_blob = h.r.bad_blob;
    return h.r.bad_blob != ~0ull ? BSG_ECORRUPT : BSG_OK;
  }

  static bool fits(const bsg_pool& dst, const bsg_pool_merge_info& info) {
    return info.need_blobs <= dst.cap_blobs && info.need_bytes <= dst.cap_bytes &&
           info.need_bytes >= dst.used;
  }

  // The append: table entries and index slots, the bytes, the counters and the remap.
  int commit(const RunView& v, const bsg_pool& src, bsg_pool& dst) {
    const hipStream_t s = v.stream;
    if (a.nnew) {
      GcArgs g{};  // the segment gather of the collect, over the new blobs
      g.w.pool = src.bytes.as<const uint8_t>();
      g.w.pool_bytes = src.pool_bytes();
      g.w.blobs = a.src;
      g.w.nblobs = a.n;
      g.g = &a.hdr->g;
      g.w.hdr = &g.g->w;
      g.live = a.isnew;
      g.coff = a.off16;
      g.total = a.need_bytes - a.base;
      g.out = dst.bytes.as<uint8_t>() + a.base;
      if (v.profile) marks.record(5, s);
      hipError_t e = dbg("launch_pool_merge_append", s, launch_pool_merge_append(a, s, v.num_cus));
      if (v.profile) marks.record(6, s);
      if (e == hipSuccess) e = dbg("launch_gc_compact", s, launch_gc_compact(g, s));
      if (v.profile) marks.record(7, s);
      MergeHdr h;
      if (e != hipSuccess || readback(s, &h)) {  // the table, the index or the bytes may be half written
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
        dst.dead = true;
        return BSG_EDEVICE;
      }
      if (v.profile) {
        ms[3] = marks.ms(5, 6);
        ms[4] = marks.ms(6, 7);
      }
    }
    dst.remap = std::move(map);
    dst.nremap = a.n;
    dst.collect_done = true;
    dst.nblobs += a.nnew;
    dst.used = a.need_bytes;
    dst.blob_bytes += added_bytes;
    return BSG_OK;
  }
};
