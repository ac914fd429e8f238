// bsgpu_tail.inc — the host tail's device side (see TailHdr in bsgpu_internal.h): which of a
// run's longest chunks go to the host (k_offload_hist, k_offload_cut, k_offload_take, together
// "k_offload_pick"), their bytes into the pinned ring (k_offload_gather) and the host's refs
// into their records (k_offload_fix). Included by bsgpu_kernels.hip inside namespace bsg.

// A job the host may take: a fresh final chunk (what per-lane mode starts from its LaneJob
// alone), wave-eligible, of at least `floor` blocks. *nb: its blocks.
__device__ __forceinline__ bool tail_candidate(const TailArgs& a, uint64_t j, uint32_t floor,
                                               uint32_t* nb) {
  const uint32_t info = a.jinfo[j];
  if (info == kNoJob || !(info & kJobElig)) return false;
  *nb = info & ~kJobElig;
  if (*nb < floor) return false;
  return !(a.jdesc[j].meta & kLaneJobSlow);
}

__device__ __forceinline__ uint32_t tail_floor(const TailArgs& a) {
  return a.force_cut ? a.force_cut : kTailMinBlocks;
}

// bucket of a job of nb blocks where the longest has mx: width mx / kTailBuckets + 1
__device__ __forceinline__ uint32_t tail_bucket(uint64_t mx, uint32_t nb) {
  const uint64_t b = nb / (mx / kTailBuckets + 1);
  return b < kTailBuckets ? (uint32_t)b : kTailBuckets - 1;
}

// Per bucket: the candidates, their longest, their ring bytes and blocks; aggregated in LDS, one
// global atomic per non-empty bucket and workgroup.
__global__ __launch_bounds__(256) void k_offload_hist(TailArgs a) {
  __shared__ uint32_t cnt[kTailBuckets], mxb[kTailBuckets];
  __shared__ unsigned long long rb[kTailBuckets], nbk[kTailBuckets];
  if (a.ctr->overflow || a.ctr->error) return;
  const uint64_t M = a.ctr->nchunks;
  if (M > a.chunk_cap) return;
  const uint64_t mx = a.ctr->max_nblocks;
  const uint32_t floor = tail_floor(a);
  for (uint32_t i = threadIdx.x; i < kTailBuckets; i += blockDim.x) cnt[i] = mxb[i] = 0, rb[i] = nbk[i] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    uint32_t nb;
    if (!tail_candidate(a, j, floor, &nb)) continue;
    const uint32_t b = tail_bucket(mx, nb);
    atomicAdd(&cnt[b], 1u);
    atomicMax(&mxb[b], nb);
    atomicAdd(&rb[b], (unsigned long long)tail_slot(a.jdesc[j].len));
    atomicAdd(&nbk[b], (unsigned long long)nb);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kTailBuckets; b += blockDim.x)
    if (cnt[b]) {
      atomicAdd(&a.hdr->cnt[b], cnt[b]);
      atomicMax(&a.hdr->maxb[b], mxb[b]);
      atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->rbytes[b]), rb[b]);
      atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->nblk[b]), nbk[b]);
    }
}

// The cut. Buckets are taken from the longest down; with the buckets above b taken, the GPU's
// longest chain is bucket b's longest job and the host has n chunks of B bytes:
//   gpu  = longest left x the chain's time per block
//   host = start + B / min(gather rate, all workers' rate) + the longest chunk on one worker
// (the workers hash longest first, so the last to end started at most one chunk late). The plan
// is the cut with the smallest max(gpu, host) that fits the ring and the list; no cut if none
// beats the whole chain on the GPU. force_cut (tests) takes every bucket that fits instead.
// One thread: 256 steps of a few operations.
__global__ void k_offload_cut(TailArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  TailHdr* h = a.hdr;
  const bool dead = a.ctr->overflow || a.ctr->error || a.ctr->nchunks > a.chunk_cap;
  const uint64_t mx = a.ctr->max_nblocks;
  uint64_t n = 0, B = 0, K = 0, low = kTailBuckets;  // low: the lowest bucket taken so far
  uint64_t best_cut = kTailBuckets, best_n = 0, best_B = 0, best_K = 0, best_left = mx;
  float best_cost = (float)mx * a.us_per_block;
  const uint32_t floor = tail_floor(a);
  for (int b = (int)kTailBuckets - 1; b >= -1 && !dead; --b) {
    if (b >= 0 && h->cnt[b] == 0) continue;
    // with every candidate taken, what is left is shorter than the floor
    const uint64_t left = b >= 0 ? h->maxb[b] : min((uint64_t)(floor ? floor - 1 : 0), mx);
    if (n) {
      const float gpu = (float)left * a.us_per_block;
      const float rate = fminf(a.pcie_bytes_us, a.host_bytes_us);
      const float host = 30.f + (float)B / rate + (float)(mx * 64) / a.host1_bytes_us;
      const float cost = fmaxf(gpu, host);
      if (a.force_cut || cost < best_cost) {
        best_cost = cost;
        best_cut = low, best_n = n, best_B = B, best_K = K, best_left = left;
      }
    }
    if (b < 0) break;
    if (n + h->cnt[b] > a.max_items || B + h->rbytes[b] > a.ring_bytes) break;
    n += h->cnt[b], B += h->rbytes[b], K += h->nblk[b], low = (uint64_t)b;
  }
  uint32_t at = 0;
  for (int b = (int)kTailBuckets - 1; b >= (int)best_cut; --b) {
    h->base[b] = at;
    at += h->cnt[b];
  }
  h->count = best_n;
  h->cutb = best_cut;
  h->bytes = best_B;
  h->blocks = best_K;
  h->mx_all = mx;
  h->mx_left = best_left;
  if (best_n) {  // k_sha's tiers are those of what stays
    a.ctr->max_nblocks = best_left;
    a.ctr->total_blocks -= best_K;
  }
}

// The planned chunks out of k_sha's queues and into the list, longest bucket first.
__global__ __launch_bounds__(256) void k_offload_take(TailArgs a) {
  TailHdr* h = a.hdr;
  if (h->count == 0) return;
  const uint64_t M = a.ctr->nchunks;
  const uint64_t mx = h->mx_all;
  const uint32_t floor = tail_floor(a), cutb = (uint32_t)h->cutb;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    uint32_t nb;
    if (!tail_candidate(a, j, floor, &nb)) continue;
    const uint32_t b = tail_bucket(mx, nb);
    if (b < cutb) continue;
    const LaneJob d = a.jdesc[j];
    const uint64_t slot = tail_slot(d.len);
    const uint32_t i = h->base[b] + atomicAdd(&h->fill[b], 1u);
    const uint64_t off = atomicAdd(reinterpret_cast<unsigned long long*>(&h->ring_head),
                                   (unsigned long long)slot);
    if (i >= h->count || i >= a.max_items || off + slot > a.ring_bytes) {  // the plan counted it
      atomicOr(reinterpret_cast<unsigned long long*>(&a.ctr->error), 32ull);
      continue;
    }
    TailItem it;
    it.job = j;
    it.start = d.start;
    it.len = d.len;
    it.off = off + (d.dptr & 15u);
    it.stream = d.stream;
    it.level = d.meta & ~kLaneJobSlow;
    a.dlist[i] = it;
    a.dsrc[i] = d.dptr;
    a.jinfo[j] = kNoJob;
    atomicAdd(reinterpret_cast<unsigned long long*>(&h->taken), 1ull);
  }
}

__device__ __forceinline__ void store_release_system(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The chunks' bytes into the pinned ring, one workgroup per chunk at a time, longest first. Source
// and destination agree modulo 16, so all but the chunk's first and last few bytes move as
// 16-byte vectors. Every thread orders its stores before the system (the host), the workgroup
// meets, and one thread hands the host the item and raises its flag.
constexpr uint32_t kGatherThreads = 1024;
constexpr uint32_t kGatherWGs = 64;
__global__ __launch_bounds__(kGatherThreads) void k_offload_gather(TailArgs a) {
  const TailHdr* h = a.hdr;
  // a plan k_offload_take could not fill is flagged (error 32); the host is told of no chunks
  const bool ok = !a.ctr->overflow && !a.ctr->error && h->taken == h->count;
  const uint64_t n = ok ? min(h->count, (uint64_t)a.max_items) : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the cut in blocks: the lowest taken bucket's lower edge, and never under the floor
    a.hmeta[1] = max(h->cutb * (h->mx_all / kTailBuckets + 1), (uint64_t)tail_floor(a));
    a.hmeta[2] = h->bytes;
    a.hmeta[3] = h->mx_all;
    a.hmeta[4] = h->mx_left;
    a.hmeta[5] = h->blocks;
    __hip_atomic_store(&a.hmeta[0], n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const TailItem it = a.dlist[i];
    if (it.off <= a.ring_bytes && it.len <= a.ring_bytes - it.off) {
      const uint8_t* src = reinterpret_cast<const uint8_t*>(a.dsrc[i]);
      uint8_t* dst = a.ring + it.off;
      const uint64_t head = min(it.len, (uint64_t)((16u - (uint32_t)(a.dsrc[i] & 15u)) & 15u));
      const uint64_t nvec = (it.len - head) / 16;
      const uint64_t tail0 = head + 16 * nvec;
      if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
      if (tail0 + threadIdx.x < it.len) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
      const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
      uint4* d4 = reinterpret_cast<uint4*>(dst + head);
      uint64_t v = threadIdx.x;
      for (; v + 3 * kGatherThreads < nvec; v += 4 * kGatherThreads) {
        const uint4 x0 = s4[v], x1 = s4[v + kGatherThreads], x2 = s4[v + 2 * kGatherThreads],
                    x3 = s4[v + 3 * kGatherThreads];
        d4[v] = x0;
        d4[v + kGatherThreads] = x1;
        d4[v + 2 * kGatherThreads] = x2;
        d4[v + 3 * kGatherThreads] = x3;
      }
      for (; v < nvec; v += kGatherThreads) d4[v] = s4[v];
    }
    if (threadIdx.x == 0) a.hlist[i] = it;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) store_release_system(a.hready + i, 1u);
  }
}

// The host's refs into the chunks' records (the twin of k_early_fix).
__global__ __launch_bounds__(256) void k_offload_fix(TailArgs a) {
  if (a.ctr->overflow || a.ctr->error) return;
  const uint64_t n = min(a.hdr->count, (uint64_t)a.max_items);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const TailItem it = a.dlist[i];
    if (it.job >= a.chunk_cap) continue;
    ChunkRec r;
    r.offset = it.start;
    r.len = it.len;
    r.level = it.level;
    r.stream = it.stream;
    for (int k = 0; k < 32; ++k) r.ref[k] = a.d_refs[32 * i + k];
    a.out[it.job] = r;
  }
}

hipError_t launch_tail_pick(const TailArgs& a, uint64_t job_bound, hipStream_t s, int num_cus) {
  const uint32_t grid = grid_for(job_bound, 256, 4u * (uint32_t)num_cus);
  hipLaunchKernelGGL(k_offload_hist, dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_offload_cut, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_offload_take, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tail_gather(const TailArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_offload_gather, dim3(kGatherWGs), dim3(kGatherThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tail_fix(const TailArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_offload_fix, dim3(16), dim3(256), 0, s, a);
  return hipGetLastError();
}
