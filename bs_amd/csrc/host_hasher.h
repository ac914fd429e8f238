// host_hasher.h — bsg_hasher: batched Blob.Ref() with persistent device buffers and stream (a
// Writer hashes every tree node through one, so a call costs one H2D, one launch and one D2H,
// not four allocations).
#pragma once

// Copies n blobs src[so[k] .. +sl[k]) to dst + dofs[k], on up to copy_threads() threads, each
// taking a run of whole blobs of about total / threads bytes.
static void par_gather(uint8_t* dst, const uint8_t* src, const uint64_t* so,
                       const uint8_t* const* sp, const uint64_t* sl, const uint64_t* dofs,
                       uint32_t n, uint64_t total) {
  constexpr uint64_t kPiece = 2ull << 20;  // per thread, at least
  const uint64_t nt = std::min<uint64_t>((uint64_t)copy_threads(), total / kPiece);
  auto run = [=](uint32_t a, uint32_t b) {
    for (uint32_t k = a; k < b; ++k)
      if (sl[k]) std::memcpy(dst + dofs[k], sp ? sp[k] : src + so[k], sl[k]);
  };
  if (nt <= 1) {
    run(0, n);
    return;
  }
  std::vector<std::pair<uint32_t, uint32_t>> runs;
  const uint64_t per = (total + nt - 1) / nt;
  uint32_t a = 0;
  uint64_t acc = 0;
  for (uint32_t k = 0; k < n; ++k) {
    acc += sl[k];
    if (acc >= per || k + 1 == n) {
      runs.emplace_back(a, k + 1);
      a = k + 1;
      acc = 0;
    }
  }
  parallel_for(runs.size(), [&](size_t i) { run(runs[i].first, runs[i].second); });
}

struct bsg_hasher {
  int dev = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  DevBuf data, off, len, refs;
  PinBuf h_meta;  // off[n] | len[n] staged for one H2D
  PinBuf h_small; // a small batch's host bytes, then its refs: pinned, so both copies are DMA
  // Large batches (the verifying split.Reader, bsg_sha256_batch of many blobs): the blobs are
  // packed at 16-byte offsets into pinned staging and hashed by an engine in bsg_engine_hash
  // mode, whose wave-mode chains take the longest blobs (k_sha_blobs hashes one blob per lane,
  // so a batch waits for its longest blob at per-lane speed, ~2.5x slower per block).
  static constexpr uint32_t kEngineMinBlobs = 16;
  static constexpr uint64_t kEngineMinBytes = 4ull << 20;
  static constexpr uint64_t kEngineLongBlob = 16ull << 10;  // (small batches, see sum())
  static constexpr uint64_t kEngineBatch = 256ull << 20;  // bytes per engine run (one blob may exceed)
  static constexpr uint64_t kGatherPiece = 32ull << 20;   // packed and copied to the device at once
  bsg_engine* eng = nullptr;
  PinBuf stage;
  PinBuf h_recs;  // an engine run's records, D2H
  DevBuf dstage;
  std::vector<uint64_t> aoff;

  // blob k is base + o[k], or ptrs[k] when ptrs is given (scattered blobs, e.g. a store's)
  int sum_engine(const uint8_t* base, const uint64_t* o, const uint8_t* const* ptrs,
                 const uint64_t* l, uint32_t n, uint8_t* out) {
    int err = 0;
    if (!eng && !(eng = bsg_engine_create(dev, nullptr, &err))) return err ? err : BSG_EDEVICE;
    hipStream_t es = static_cast<hipStream_t>(bsg_engine_stream(eng));
    stage.dma_only = true;  // read only by the H2D: a registered huge-page mapping pins faster
    uint64_t left = 0;      // bytes of the blobs not yet in a run
    for (uint32_t k = 0; k < n; ++k) left += l[k];
    // a small batch (see sum()) puts every blob on wave tickets: the engine's own choice keeps
    // blobs under kLongMinBlocks (64 KiB) per-lane
    eng->hash_long_mode = left < kEngineMinBytes ? 2 : -1;
    for (uint32_t i = 0; i < n;) {
      // A run is up to kEngineBatch bytes, or everything left if that is at most a quarter more:
      // every run waits for its longest blob's chain (~10 ms for a 256 MiB run), so a small
      // remainder run (a verifying Reader's window just over 256 MiB) doubled the wait.
      const uint64_t cap = left <= kEngineBatch + kEngineBatch / 4 ? UINT64_MAX : kEngineBatch;
      uint64_t bytes = 0;
      uint32_t j = i;
      aoff.clear();
      while (j < n && j - i < 65535u) {
        const uint64_t a = (bytes + 15) & ~15ull;
        if (j > i && a + l[j] > cap) break;
        aoff.push_back(a);
        bytes = a + l[j];
        left -= l[j];
        ++j;
      }
      // sized once for the largest run (a growth re-pins: ~35 ms per 256 MiB)
      const uint64_t want =
          bytes >= kEngineBatch / 2 ? std::max(bytes, kEngineBatch + kEngineBatch / 4) : bytes;
      HCHECK(stage.ensure(want + kReadSlack));
      HCHECK(dstage.ensure(want + kReadSlack));
      // gathered a piece at a time, each piece's H2D queued as soon as it is packed, so the copy
      // engine moves piece k while the host threads pack piece k+1
      for (uint32_t a = 0; a < j - i;) {
        uint32_t b = a;
        uint64_t pbytes = 0;
        while (b < j - i && (b == a || pbytes < kGatherPiece)) pbytes += l[i + b++];
        const uint64_t lo = aoff[a];
        const uint64_t hi = (b < j - i) ? aoff[b] : bytes;
        par_gather(stage.as<uint8_t>(), base, o ? o + i + a : nullptr,
                   ptrs ? ptrs + i + a : nullptr, l + i + a, aoff.data() + a, b - a, pbytes);
        if (hi > lo)
          HCHECK(hipMemcpyAsync(dstage.as<uint8_t>() + lo, stage.as<uint8_t>() + lo, hi - lo,
                                hipMemcpyHostToDevice, es));
        a = b;
      }
      int rc = bsg_engine_hash(eng, dstage.as<uint8_t>(), aoff.data(), l + i, j - i);
      uint64_t nch = 0;
      if (!rc) rc = bsg_engine_finish(eng, &nch);
      if (!rc && nch != j - i) rc = BSG_EDEVICE;
      if (rc) return rc;
      // the records through pinned memory (a D2H into a fresh pageable vector cost ~12 ms the
      // first time: the runtime pins its pages)
      HCHECK(h_recs.ensure(sizeof(bsg_chunk) * (j - i)));
      HCHECK(hipMemcpyAsync(h_recs.p, eng->out.p, sizeof(bsg_chunk) * (j - i),
                            hipMemcpyDeviceToHost, es));
      HCHECK(hipStreamSynchronize(es));
      const bsg_chunk* rec = h_recs.as<bsg_chunk>();
      for (uint32_t k = 0; k < j - i; ++k) std::memcpy(out + 32ull * (i + k), rec[k].ref, 32);
      i = j;
    }
    return BSG_OK;
  }

  int sum(const uint8_t* base, const uint64_t* o, const uint64_t* l, uint32_t n, uint8_t* out) {
    static const bool dbg_times = std::getenv("BSG_DEBUG_HASHER") != nullptr;
    const auto t_in = std::chrono::steady_clock::now();
    struct Report {  // BSG_DEBUG_HASHER: where one call's time went (stderr)
      bool on;
      std::chrono::steady_clock::time_point t0;
      uint32_t n;
      uint64_t marks[4] = {};
      ~Report() {
        if (on)
          std::fprintf(stderr, "bsgpu hasher: %u blobs, %.3f ms (ensure %.3f, copies %.3f, launch %.3f)\n",
                       n, ns_since(t0) / 1e6, marks[0] / 1e6, (marks[1] - marks[0]) / 1e6,
                       (marks[2] - marks[1]) / 1e6);
      }
    } rep{dbg_times, t_in, n};
    // a wrapped off + len would size the private copy below by a small `hi` and leave the
    // kernel a wild address: refused before anything is allocated or copied
    for (uint32_t i = 0; i < n; ++i)
      if (o[i] > UINT64_MAX - l[i]) return BSG_EINVAL;
    hipPointerAttribute_t attr;
    bool on_device = false;
    if (hipPointerGetAttributes(&attr, base) == hipSuccess)
      on_device = (attr.type == hipMemoryTypeDevice);
    else
      (void)hipGetLastError();
    uint64_t hi = 0, total = 0, longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
      hi = std::max<uint64_t>(hi, o[i] + l[i]);
      total += l[i];
      longest = std::max<uint64_t>(longest, l[i]);
    }
    if (!on_device && n >= kEngineMinBlobs && total >= kEngineMinBytes)
      return sum_engine(base, o, nullptr, l, n, out);
    // A small batch with a long blob goes to the engine too, every blob on a wave ticket: one
    // blob per lane hashes a block per ~6,000-8,000 cycles and the batch waits for its longest
    // blob, where a solo wave chain takes ~2,300 (plus ~0.1 ms of launches). A split::Writer's tree nodes are such a batch:
    // their leaf counts are geometric, so 1 GiB's 63 nodes of ~11 KB include one of ~50 KB, and
    // k_sha_blobs took 2.7-3.1 ms for them (profiles/r06_writer_trace_kernel_stats.csv). Its
    // staging stays the batch's size (< kEngineMinBytes), so a pooled hasher pins nothing big.
    if (!on_device && n >= 2 && total < kEngineMinBytes && longest >= kEngineLongBlob)
      return sum_engine(base, o, nullptr, l, n, out);
    // always hash from a private copy with kReadSlack bytes of tail padding
    HCHECK(data.ensure(hi + kReadSlack));
    HCHECK(off.ensure(8ull * n));
    HCHECK(len.ensure(8ull * n));
    HCHECK(refs.ensure(32ull * n));
    HCHECK(h_meta.ensure(16ull * n));
    std::memcpy(h_meta.p, o, 8ull * n);
    std::memcpy(h_meta.as<uint8_t>() + 8ull * n, l, 8ull * n);
    // Small host batches (tree nodes: pageable std::string) go through pinned memory, whose
    // H2D / D2H are single DMAs instead of the runtime's chunked staging of pageable memory.
    // The path is chosen by blob count, so one large blob can land here too: above
    // kEngineMinBytes its bytes are copied straight from pageable memory instead, so that a
    // pooled hasher never keeps a blob-sized pinned buffer (pinning costs ~50-65 ms per 256 MiB
    // and would stay held for the life of the process).
    const bool via_pinned = !on_device && hi <= kEngineMinBytes;
    HCHECK(h_small.ensure(std::max<uint64_t>(via_pinned ? hi : 0, 32ull * n)));
    rep.marks[0] = ns_since(t_in);
    if (hi) {
      if (on_device) {
        HCHECK(hipMemcpyAsync(data.p, base, hi, hipMemcpyDeviceToDevice, stream));
      } else if (!via_pinned) {
        HCHECK(hipMemcpyAsync(data.p, base, hi, hipMemcpyHostToDevice, stream));
      } else {
        std::memcpy(h_small.p, base, hi);
        HCHECK(hipMemcpyAsync(data.p, h_small.p, hi, hipMemcpyHostToDevice, stream));
      }
    }
    HCHECK(hipMemcpyAsync(off.p, h_meta.p, 8ull * n, hipMemcpyHostToDevice, stream));
    HCHECK(hipMemcpyAsync(len.p, h_meta.as<uint8_t>() + 8ull * n, 8ull * n,
                          hipMemcpyHostToDevice, stream));
    rep.marks[1] = ns_since(t_in);
    BlobShaArgs a{data.as<uint8_t>(), off.as<uint64_t>(), len.as<uint64_t>(), n,
                  refs.as<uint8_t>()};
    HCHECK(launch_sha_blobs(a, stream, num_cus));
    rep.marks[2] = ns_since(t_in);
    HCHECK(hipMemcpyAsync(h_small.p, refs.p, 32ull * n, hipMemcpyDeviceToHost, stream));
    HCHECK(hipStreamSynchronize(stream));
    std::memcpy(out, h_small.p, 32ull * n);
    return BSG_OK;
  }
};
