// host_dedup.h — bsg_engine_dedup / bsg_engine_pack_unique and bsg_refset: which records of the
// last finished split run are new, and their bytes packed. (Included by host_engine.h.)
#pragma once

namespace {

// The buffers of one first-occurrence pass (launch_dedup) over n items, and its results. An
// engine owns one for bsg_engine_dedup (run / pack), a set one for bsg_refset_add (the buffers).
struct DedupWork {
  RefTable tab;
  DevBuf first, rank, bpre, uniq, pack_off, part, hdr;
  PinBuf h_hdr;
  DedupHdr last{};
  bool valid = false;  // run() made the result from the engine's current run
  uint64_t n = 0, nunique = 0, bytes = 0;
  bool pack_funnel = false;  // measurement tooling: the aligned-load variant of k_pack
  Marks marks;               // profile: around run(), around pack()'s kernel
  float ms[2] = {0, 0};

  bool current(bool run_done) const { return valid && run_done; }  // (any enqueue clears valid)

  int reserve(uint64_t n) {
    const uint64_t n1 = n ? n : 1;
    MCHECK(tab.reserve(n1));
    MCHECK(first.ensure(8 * n1));
    MCHECK(rank.ensure(8 * (n1 + 1)));
    MCHECK(bpre.ensure(8 * (n1 + 1)));
    MCHECK(uniq.ensure(8 * n1));
    MCHECK(pack_off.ensure(8 * (n1 + 1)));
    MCHECK(part.ensure(8 * sum_parts(n1)));
    MCHECK(hdr.ensure(sizeof(DedupHdr)));
    MCHECK(h_hdr.ensure(sizeof(DedupHdr)));
    return BSG_OK;
  }

  DedupArgs args(const uint8_t* refs, uint64_t stride, const uint8_t* lens, uint64_t len_stride,
                 uint64_t n) const {
    DedupArgs a{};
    a.refs = refs;
    a.stride = stride;
    a.lens = lens;
    a.len_stride = len_stride;
    a.n = n;
    a.tab = tab.p();
    a.tab_mask = tab.mask();
    a.first = first.as<uint64_t>();
    a.rank = rank.as<uint64_t>();
    a.bpre = bpre.as<uint64_t>();
    a.uniq = uniq.as<uint64_t>();
    a.pack_off = pack_off.as<uint64_t>();
    a.part = part.as<uint64_t>();
    a.hdr = hdr.as<DedupHdr>();
    return a;
  }

  // the header to the host after everything enqueued on s; BSG_EDEVICE if a device check failed
  int readback(hipStream_t s) {
    return read_header(h_hdr, hdr.p, s, &last, [](const DedupHdr& d) { return d.error; }, "dedup");
  }

  // first occurrence per ref over the run's records (and `set`), then the new refs into the set
  int run(const RunView& v, bsg_refset* set);

  int pack(const RunView& v, uint8_t* d_out, uint64_t cap) {
    if (!current(v.run_done)) return BSG_ESTATE;
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || cap < bytes) return BSG_EINVAL;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + bytes;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(v.d_data), s1 = s0 + data_span(*v.descs);
    if (o1 < o0 || (bytes && o0 < s1 && s0 < o1)) return BSG_EINVAL;
    PackArgs a{};
    a.data = v.d_data;
    a.streams = v.streams;
    a.nstreams = v.ns;
    a.rec = v.rec;
    a.nrec = n;
    a.uniq = uniq.as<uint64_t>();
    a.pack_off = pack_off.as<uint64_t>();
    a.nunique = nunique;
    a.total = bytes;
    a.out = d_out;
    a.hdr = hdr.as<DedupHdr>();
    if (v.profile) marks.record(2, v.stream);
    HCHECK(hipMemsetAsync(hdr.p, 0, sizeof(DedupHdr), v.stream));
    HCHECK(dbg("launch_pack", v.stream, launch_pack(a, pack_funnel, v.stream)));
    if (v.profile) marks.record(3, v.stream);
    if (int rc = readback(v.stream)) return rc;
    ms[1] = v.profile ? marks.ms(2, 3) : 0.f;
    return BSG_OK;
  }
};

}  // namespace

// A set of 32-byte refs on one device: an append-only key array and an open-addressing table of
// key indices (bsgpu_dedup.inc). Every entry point takes `mu`, so engines on several threads may
// share a set; each call has synchronised the stream it used before it lets go.
struct bsg_refset {
  int dev = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;  // bsg_refset_add's own
  std::mutex mu;
  DevBuf keys, tab;
  uint64_t slots = 0;            // of tab (a power of two)
  uint64_t key_cap = 0;          // keys the key array holds
  std::atomic<uint64_t> count{0};
  bool dead = false;             // a device error: BSG_ESTATE from then on
  DevBuf staged;                 // bsg_refset_add: the caller's refs
  DedupWork work;

  // the set's part of a first-occurrence pass
  void lookup_args(DedupArgs* a) const {
    a->set_keys = keys.as<uint8_t>();
    a->set_stride = 32;
    a->set_tab = tab.as<uint64_t>();
    a->set_mask = slots - 1;
    a->set_count = count.load();
  }

  // The m new items of a finished pass `d` (its uniq[0 .. m)) become keys, on stream s: the key
  // array and the table grow first (doubling, the table rehashed on the device), and nothing of
  // the set changes unless every allocation succeeded. Synchronises s and reads the pass's
  // header (`w`) back once more for its error word.
  int add_new(const DedupArgs& d, uint64_t m, DedupWork* w, hipStream_t s) {
    if (!m) return BSG_OK;
    const uint64_t cnt = count.load(), want = cnt + m;
    uint64_t nslots = slots;
    while (want * 100 > nslots * kRefSetLoadPct) nslots <<= 1;
    uint64_t ncap = key_cap;
    while (ncap < want) ncap <<= 1;
    DevBuf ntab, nkeys;
    if (nslots != slots) MCHECK(ntab.ensure(8 * nslots));
    if (ncap != key_cap) MCHECK(nkeys.ensure(32 * ncap));
    SetArgs sa{};
    sa.keys = nkeys.p ? nkeys.as<uint8_t>() : keys.as<uint8_t>();
    sa.tab = ntab.p ? ntab.as<uint64_t>() : tab.as<uint64_t>();
    sa.mask = nslots - 1;
    sa.count = cnt;
    sa.hdr = d.hdr;
    hipError_t e = hipSuccess;
    if (nkeys.p && cnt)
      e = hipMemcpyAsync(nkeys.p, keys.p, 32 * cnt, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && ntab.p) {
      e = hipMemsetAsync(ntab.p, 0xFF, 8 * nslots, s);
      if (e == hipSuccess) e = launch_set_rehash(sa, s, num_cus);
    }
    if (e == hipSuccess) e = launch_set_add(sa, d, m, s, num_cus);
    int rc = e == hipSuccess ? w->readback(s) : BSG_EDEVICE;
    if (rc) {  // the old table may hold indices of keys that never arrived
      (void)hipGetLastError();
      (void)hipStreamSynchronize(s);
      dead = true;
      return rc;  // (the new table and keys go after the synchronisation)
    }
    if (ntab.p) {
      tab = std::move(ntab);
      slots = nslots;
    }
    if (nkeys.p) {
      keys = std::move(nkeys);
      key_cap = ncap;
    }
    count.store(want);
    return BSG_OK;
  }
};

inline int DedupWork::run(const RunView& v, bsg_refset* set) {
  if (!v.usable) return BSG_ESTATE;
  valid = false;
  std::unique_lock<std::mutex> lk;
  if (set) {
    lk = std::unique_lock<std::mutex>(set->mu);
    if (set->dead) return BSG_ESTATE;
  }
  int rc;
  const hipStream_t stream = v.stream;
  if ((rc = reserve(v.nrec))) return rc;
  if (v.profile) marks.record(0, stream);
  HCHECK(hipMemsetAsync(hdr.p, 0, sizeof(DedupHdr), stream));
  const uint8_t* rec = reinterpret_cast<const uint8_t*>(v.rec);
  DedupArgs a = args(rec + offsetof(ChunkRec, ref), sizeof(ChunkRec),
                     rec + offsetof(ChunkRec, len), sizeof(ChunkRec), v.nrec);
  if (set) set->lookup_args(&a);
  if (v.nrec) {
    HCHECK(tab.clear(stream));
    HCHECK(dbg("launch_dedup", stream, launch_dedup(a, stream, v.num_cus)));
  } else {
    HCHECK(hipMemsetAsync(pack_off.p, 0, 8, stream));
  }
  if ((rc = readback(stream))) return rc;
  const DedupHdr h = last;
  if (h.nunique > v.nrec) return BSG_EDEVICE;
  if (set && (rc = set->add_new(a, h.nunique, this, stream))) return rc;
  if (v.profile) {
    marks.record(1, stream);
    HCHECK(stream_wait(stream));
    ms[0] = marks.ms(0, 1);
  }
  n = v.nrec;
  nunique = h.nunique;
  bytes = h.unique_bytes;
  valid = true;
  return BSG_OK;
}
