"""Job censuses on the count edges of k_sha's tier split (k_lens, k_thresh, k_order, k_bucket_scan
and the ticket arithmetic of sha_wave_job), and a model of the split. Shared by
test_tier_cases_cpu.py, which holds every case to the counts it claims, and
test_gpu_tier_counts.py, which runs the cases on the device. No test in here.

sha_edges.py pins the SHA-256 lengths on every path with one census (16 helped solo chains, 21
group jobs, 41 pair jobs, 15 lane jobs). Here the lengths are plain and the census moves: fewer
than kSolo wave jobs, exactly kSolo, full and ragged last tickets, pair tickets with no group
ticket before them, no solo or group ticket at all, an empty per-lane queue, the thresholds to
the block and to the bucket, the ticket budget of half the waves, a loaded launch, and more job
slots than one grid pass of k_lens / k_order.

The model (model()) restates what k_thresh and k_bucket_scan compute, from DESIGN §4.4 and the
kernels' comments, over a plain list of block counts:

    w      = (mx + kLptBuckets) // kLptBuckets          bucket width; job of n blocks: bucket
                                                        (mx - n) // w, bucket b's top mx - b * w
    light  = total * 10 < mx * 64 * waves
    tlen   = max(mx * (light ? 48 : 55) // 100, total * 9 // (10 * 64 * waves), kLongMinBlocks)
    cap    = kSolo + kGroup * (waves / 2 - kSolo)       jobs that half the waves' tickets hold
    group  : the longest buckets b with top(b) >= tlen and (jobs in buckets 0..b) <= cap
    t8     = n8 if n8 <= kSolo else kSolo + ceil((n8 - kSolo) / kGroup)
    tlen2  = max(mx * (light ? 30 : 34) // 100, kLongMinBlocks)
    cap2   = (waves / 2 - t8) * kPairGroup
    pair   : the next buckets with top(b) >= tlen2 and (jobs in them so far) <= cap2
    helped = min(n8, kSolo, waves / 2) on a light launch, else 0
    wave_tickets = t8 + ceil(pair jobs / kPairGroup)

A bucket qualifies by its top length, so with w > 1 a job up to w - 1 blocks under a threshold
still takes the longer path (case F-w3). KNOB_LONG_MODE 1 sends every job to a lane, 2 every
job to a solo or group ticket. The percentages and counts are read from the sources
(constants()), so a retune moves the model; the cases' literals are derived by hand for 256 CUs
(waves = 1024) and the present constants, and test_tier_cases_cpu.py fails where a retune moves
one: re-derive it then.

Layout. Every case but I and J is one bsg_engine_hash call whose blobs are aliased over one
random buffer of 1 MiB (buffer()): blob i is buffer[off[i] : off[i] + len[i]] with off a multiple
of 16, every (off, len) pair distinct, so every expected ref differs and a dropped or
mis-sliced job shows. The expected refs are hashlib's, cached per (off, len): the host hashes
each distinct pair once for all cases, and the device buffer stays small while total_blocks is
large (case G hashes 0.9 GB of aliased bytes). The GPU test first runs the same layout over the
complemented buffer on the same engine, so every stale ref would be wrong.
"""
import hashlib
import os
import re

import numpy as np

import sha_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bs_amd", "csrc")
READ_SLACK = 256                  # BSG_READ_SLACK
BUF_BYTES = 1 << 20               # the aliased buffer: longer than the longest blob (10,000 blocks)


# ---------------------------------------------------------------------------------------------
# Constants, from the sources
# ---------------------------------------------------------------------------------------------
_CONSTANTS = {}


def constants() -> dict:
    """kSolo, kGroup, kPairGroup, kLongMinBlocks, kLptBuckets, the four tier percentages, the
    waves per CU and the CU count an engine assumes before it asks the device (read once)."""
    if _CONSTANTS:
        return dict(_CONSTANTS)
    out = {}

    def one(text, pattern, name):
        m = re.findall(pattern, text, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])

    with open(os.path.join(CSRC, "bsgpu_internal.h")) as f:
        text = f.read()
    one(text, r"^#define\s+BSG_SOLO\s+(\d+)\b", "kSolo")
    assert len(re.findall(r"^constexpr\s+uint32_t\s+kSolo\s*=\s*BSG_SOLO\s*;", text, re.M)) == 1
    for name in ("kGroup", "kPairGroup", "kLongMinBlocks", "kLptBuckets"):
        one(text, r"^constexpr\s+(?:uint32_t|int)\s+%s\s*=\s*(\d+)\s*;" % name, name)
    with open(os.path.join(CSRC, "bsgpu_kernels.hip")) as f:
        text = f.read()
    for name in ("BSG_TLEN_PCT", "BSG_TLEN_PCT_LIGHT", "BSG_PAIR_PCT", "BSG_PAIR_PCT_LIGHT"):
        one(text, r"^#define\s+%s\s+(\d+)\s*$" % name, name)
    with open(os.path.join(CSRC, "host_engine.h")) as f:
        text = f.read()
    one(text, r"^\s*a\.waves\s*=\s*(\d+)u\s*\*\s*\(uint32_t\)num_cus\s*;", "waves_per_cu")
    one(text, r"^\s*int\s+num_cus\s*=\s*(\d+)\s*;", "num_cus")
    _CONSTANTS.update(out)
    return out


def waves(cus: int | None = None) -> int:
    c = constants()
    return c["waves_per_cu"] * (c["num_cus"] if cus is None else cus)


def grid_slots(cus: int | None = None) -> int:
    """Job slots of one grid pass of k_lens / k_order: 4 * CUs workgroups of 256 threads."""
    return waves(cus) * 256


# ---------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------
def model(nblocks_list, waves, long_mode=0) -> dict:
    """What Engine.diag() and Engine.tiers() report for a launch whose jobs have these block
    counts (all of them fresh chunks or whole blobs), plus `light`, `tlen`, `tlen2`, `cap`,
    `bucket_width` and `tier`: 'group' | 'pair' | 'lane' per job, in the order given."""
    c = constants()
    solo, grp, pgrp, floor = c["kSolo"], c["kGroup"], c["kPairGroup"], c["kLongMinBlocks"]
    nb = [int(n) for n in nblocks_list]
    mx, total = max(nb, default=0), sum(nb)
    w = (mx + c["kLptBuckets"]) // c["kLptBuckets"]
    light = total * 10 < mx * 64 * waves
    tlen = max(mx * (c["BSG_TLEN_PCT_LIGHT"] if light else c["BSG_TLEN_PCT"]) // 100,
               total * 9 // (10 * 64 * waves), floor)
    half = waves // 2
    cap = solo + grp * (half - solo if half > solo else 0)
    if long_mode == 2:
        tlen, cap = 0, float("inf")
    # buckets, longest first; a bucket's jobs and its top length
    bucket = [min((mx - n) // w, c["kLptBuckets"] - 1) for n in nb]
    count = {}
    for b in bucket:
        count[b] = count.get(b, 0) + 1
    used = sorted(count)

    def top(b):
        return max(mx - b * w, 0)

    nlb8, n8, seen = 0, 0, 0             # nlb8: the first bucket that is not a group bucket
    for b in used:
        seen += count[b]
        if long_mode == 1 or top(b) < tlen or seen > cap:
            break
        nlb8, n8 = b + 1, seen
    else:
        nlb8 = c["kLptBuckets"]
    # (an empty bucket between two used ones qualifies or not with the next used one below it,
    # which holds no job of it: only the used buckets matter for the counts)
    t8 = n8 if n8 <= solo else solo + -(-(n8 - solo) // grp)
    pct2 = c["BSG_PAIR_PCT_LIGHT"] if light else c["BSG_PAIR_PCT"]
    tlen2, nlb, nlong = None, nlb8, n8
    if pct2 > 0 and long_mode == 0:
        tlen2 = max(mx * pct2 // 100, floor)
        cap2 = (half - t8 if half > t8 else 0) * pgrp
        seen = 0
        for b in used:
            if b < nlb8:
                continue
            seen += count[b]
            if top(b) < tlen2 or seen > cap2:
                break
            nlb, nlong = b + 1, n8 + seen
    helped = min(n8, solo, half) if light and long_mode == 0 else 0
    tier = ["group" if b < nlb8 else "pair" if b < nlb else "lane" for b in bucket]
    assert tier.count("group") == n8 and tier.count("pair") == nlong - n8
    return {"max_nblocks": mx, "total_blocks": total, "bucket_width": w, "light": light,
            "tlen": tlen, "tlen2": tlen2, "cap": cap, "nlong_grp": n8, "tickets_grp": t8,
            "nlong": nlong, "nshort": len(nb) - nlong, "helped": helped,
            "wave_tickets": t8 + -(-(nlong - n8) // pgrp), "tier": tier}


COUNTS = ("nlong_grp", "tickets_grp", "helped", "nlong", "nshort", "wave_tickets")


def reported(diag, tiers) -> dict:
    """The model's keys out of Engine.diag() and Engine.tiers()."""
    return {"max_nblocks": diag["max_nblocks"], "total_blocks": diag["total_blocks"],
            "nlong": diag["nlong"], "nshort": diag["nshort"],
            "wave_tickets": tiers["wave_tickets"], "nlong_grp": tiers["nlong_grp"],
            "tickets_grp": tiers["tickets_grp"], "helped": tiers["helped"]}


def expected_report(m) -> dict:
    return {k: m[k] for k in ("max_nblocks", "total_blocks") + COUNTS}


# ---------------------------------------------------------------------------------------------
# Layout: blobs aliased over one buffer
# ---------------------------------------------------------------------------------------------
_BUF = []


def buffer() -> np.ndarray:
    """BUF_BYTES random bytes and READ_SLACK more behind them (read-only, shared by all cases)."""
    if not _BUF:
        b = np.random.default_rng(0x71E5).integers(0, 256, BUF_BYTES + READ_SLACK, dtype=np.uint8)
        b.setflags(write=False)
        _BUF.append(b)
    return _BUF[0]


def layout(nblocks_list):
    """(off, lens) for blobs of the given block counts over buffer(): the c-th blob of a block
    count n (in the order given) takes the length of n blocks with L % 64 = (56 + c) % 64 (the
    length word in a block of its own first, then the exact multiple, ...) and an offset that
    steps by 16 every 64 blobs, by 293 * 16 with c % 7 and by 2051 * 16 with n % 4, so no two
    blobs share (off, len) and the set of pairs depends only on how many blobs each block count
    has."""
    nth, off, lens = {}, [], []
    for n in nblocks_list:
        n = int(n)
        c = nth.get(n, 0)
        lo = max(64 * (n - 1) - 8, 1)           # the shortest length of n blocks (no empty blob:
        per = 64 * (n - 1) + 56 - lo            # two would share a ref); 64 lengths, 55 for n = 1
        assert n >= 1 and c // per < 293, (n, c)
        lens.append(lo + c % per)
        off.append(16 * (c // per + 293 * (c % 7) + 2051 * (n % 4)))
        nth[n] = c + 1
        assert E.nblocks(lens[-1]) == n and off[-1] + lens[-1] <= BUF_BYTES
    return off, lens


_REFS = {}


def refs(off, lens):
    """hashlib's SHA-256 of every blob, cached per (off, len)."""
    buf, out = buffer(), []
    for o, n in zip(off, lens):
        r = _REFS.get((o, n))
        if r is None:
            r = _REFS[(o, n)] = hashlib.sha256(buf[o:o + n]).digest()
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------------
# The case table (bsg_engine_hash). Literals: for waves = 1024, derived by hand below.
# ---------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, blocks, want, light=True, seed=None, why=""):
        self.name, self.want, self.light, self.why = name, dict(want), light, why
        blocks = [int(n) for n in blocks]
        if seed is not None:                    # long jobs scattered over the job indices
            np.random.default_rng(seed).shuffle(blocks)
        self.blocks = blocks
        self.off, self.lens = layout(blocks)

    def refs(self):
        return refs(self.off, self.lens)


def _short(k, seed):
    """k jobs of 1 to 900 blocks: under the 64 KiB floor (kLongMinBlocks), so never on a wave."""
    return [int(n) for n in np.random.default_rng([seed, 900]).integers(1, 901, k)]


def _want(n8, t8, helped, nlong, nshort, tickets):
    return dict(zip(COUNTS, (n8, t8, helped, nlong, nshort, tickets)))


def _ceil(a, b):
    return -(-a // b)


A_COUNTS = (1, 2, 15, 16, 17, 23, 24, 25)
B_COUNTS = (1, 31, 32, 33, 64)
E_COUNTS = (16, 17, 3984, 3985)

# A: the longest job has at most 2,100 blocks, so tlen = max(2100 * 48 // 100 = 1008, 1024) = 1024
# = tlen2: every job of 2,000 blocks or more is a group job, none a pair job.
#        n: (helped, tickets_grp)
A_WANT = {1: (1, 1), 2: (2, 2), 15: (15, 15), 16: (16, 16),
          17: (16, 17),      # one group ticket with seven empty slots
          23: (16, 17), 24: (16, 17),   # ... with one empty slot, and full
          25: (16, 18)}
# B: the longest job has 3,400 blocks: tlen = 3400 * 48 // 100 = 1632, tlen2 = max(1020, 1024).
# The 16 jobs of 3,355 to 3,400 blocks are solo jobs, the p of 1,100 to 1,600 blocks pair jobs.
#        p: wave_tickets
B_WANT = {1: 17, 31: 17, 32: 17,     # 32: a full pair ticket
          33: 18, 64: 18}            # 64: two full ones


def _pair_band(p):
    return [1100 + (500 * i) // max(p - 1, 1) for i in range(p)]   # 1,100 .. 1,600, distinct


def _build():
    cases = []

    def add(*a, **k):
        cases.append(Case(*a, **k))

    for n in A_COUNTS:
        helped, t8 = A_WANT[n]
        add(f"A-n{n}", [2100 - 3 * i for i in range(n)] + _short(200, n),
            _want(n, t8, helped, n, 200, t8), seed=100 + n,
            why="n wave jobs, all at or above tlen: solo tickets up to kSolo, then group tickets")
    for p in B_COUNTS:
        add(f"B-p{p}", [3400 - 3 * i for i in range(16)] + _pair_band(p) + _short(200, 50 + p),
            _want(16, 16, 16, 16 + p, 200, B_WANT[p]), seed=200 + p,
            why="exactly kSolo solo jobs, no group ticket, p pair jobs")
    # C: as B with 3 solo jobs: j0 of the pair ticket is n8 = 3, t8 = 3 < kSolo
    add("C-pairs-after-3", [3400, 3397, 3394] + _pair_band(5) + _short(200, 60),
        _want(3, 3, 3, 8, 200, 4), seed=300,
        why="a pair ticket that starts at job 3, after fewer than kSolo solo tickets")
    # D: as B with 8 group jobs (1,700 .. 1,770 >= 1,632) and 32 pair jobs, nothing else:
    # 16 + 1 tickets, then one full pair ticket; the per-lane queue is empty
    add("D-no-lane-job", [3400 - 3 * i for i in range(16)] + [1700 + 10 * i for i in range(8)]
        + _pair_band(32), _want(24, 17, 16, 56, 0, 18), seed=400,
        why="nshort = 0: every job on a wave ticket, full last group and pair tickets")
    # E: N jobs of exactly kLongMinBlocks = 1,024 blocks share bucket 0, whose top is 1,024 =
    # tlen = tlen2. cap = 16 + 8 * (512 - 16) = 3,984: N = 3,984 fills it (16 + 3,968 / 8 = 512
    # tickets = waves / 2); N = 3,985 exceeds it, so no bucket is a group bucket and all jobs
    # go to ceil(3985 / 32) = 125 pair tickets (cap2 = 512 * 32). Light: N * 10,240 < 2^26.
    e_want = {16: _want(16, 16, 16, 16, 0, 16), 17: _want(17, 17, 16, 17, 0, 17),
              3984: _want(3984, 512, 16, 3984, 0, 512), 3985: _want(0, 0, 0, 3985, 0, 125)}
    for n in E_COUNTS:
        add(f"E-equal{n}", [1024] * n, e_want[n],
            why="equal lengths at the floor: one bucket against cap")
    add("E-floor", [1023] * 100, _want(0, 0, 0, 0, 100, 0),
        why="one block under kLongMinBlocks: no wave job")
    # F-w1: the longest 4,000 blocks (width 1): tlen = 1,920, tlen2 = 1,200 to the block
    add("F-w1", [4000, 1920, 1919, 1200, 1199] + _short(50, 70), _want(2, 2, 2, 4, 51, 3),
        seed=500, why="1920 group, 1919 and 1200 pair, 1199 lane")
    # F-w3: the longest 10,000 blocks: width (10000 + 4096) // 4096 = 3, tlen = 4,800, tlen2 =
    # 3,000. Bucket 1,733 holds 4,801 .. 4,799 (top 4,801 >= tlen): group, 4,799 included;
    # bucket 1,734 (4,798 .. 4,796) pair. Bucket 2,333 holds 3,001 .. 2,999 (top 3,001 >= tlen2):
    # pair, 2,999 included; bucket 2,334 (2,998 .. 2,996) lane.
    add("F-w3", [10000, 4801, 4800, 4799, 4798, 4797, 3001, 3000, 2999, 2998, 2997]
        + _short(50, 71), _want(4, 4, 4, 9, 52, 5), seed=501,
        why="the bucket, not the job, decides: 4799 group, 4798 pair, 2999 pair, 2998 lane")
    # G: 20 jobs of 2,081 .. 2,100 blocks (41,810 blocks) and k jobs of 1,000 blocks. Light iff
    # total * 10 < 2100 * 65,536 = 137,625,600. k = 14,000: 140,418,100, loaded: tlen = max(2100 *
    # 55 // 100 = 1155, 14,041,810 * 9 // 655,360 = 192, 1024), helped = 0, the solo tickets run
    # unhelped; tlen2 = max(714, 1024), so the 1,000-block jobs stay per lane. k = 13,000:
    # 130,418,100, light: helped = 16.
    longs = [2100 - i for i in range(20)]
    add("G-loaded", longs + [1000] * 14000, _want(20, 17, 0, 20, 14000, 17), light=False,
        seed=600, why="a loaded launch in auto mode: unhelped solo tickets")
    add("G-light", longs + [1000] * 13000, _want(20, 17, 16, 20, 13000, 17), seed=600,
        why="the same just under the load threshold")
    # H: every block count 1 .. 2,500 once (width 1, every bucket another rank): tlen = 1,200,
    # tlen2 = 1,024: 1,301 group jobs on 16 + ceil(1285 / 8) = 177 tickets, 176 pair jobs on 6.
    add("H-sort", list(range(1, 2501)), _want(1301, 177, 16, 1477, 1023, 183), seed=700,
        why="the counting sort: 2,500 buckets of one job each")
    return cases


# H under KNOB_LONG_MODE 1 (every job per lane) and 2 (every job on a solo or group ticket:
# 16 + ceil(2484 / 8) = 327 tickets)
H_MODE_WANT = {1: _want(0, 0, 0, 0, 2500, 0), 2: _want(2500, 327, 0, 2500, 0, 327)}

_CASES = []


def cases():
    if not _CASES:
        _CASES.extend(_build())
    return _CASES


NAMES = ([f"A-n{n}" for n in A_COUNTS] + [f"B-p{p}" for p in B_COUNTS]
         + ["C-pairs-after-3", "D-no-lane-job"] + [f"E-equal{n}" for n in E_COUNTS]
         + ["E-floor", "F-w1", "F-w3", "G-loaded", "G-light", "H-sort"])


def get(name) -> Case:
    return next(c for c in cases() if c.name == name)


# ---------------------------------------------------------------------------------------------
# Split runs: I (more job slots than one grid pass) and J (one planted run)
# ---------------------------------------------------------------------------------------------
I_BITS, I_MIN = 2, 1              # a chunk every few bytes
I_PASSES = (1, 2)                 # chunks + streams = passes * grid_slots + 1


def slots_stream(oracle, table, passes, cus=None, seed=0x51075):
    """(stream, its records by the oracle): SplitMix bytes at Bits 2 / MinSize 1, cut at the end
    of chunk number passes * grid_slots(cus), so that the run's job slots (one per record and one
    per stream) are one more than `passes` grid passes of k_lens / k_order hold. A prefix that
    ends at a chunk end splits into the same chunks, without a tail."""
    from bs_amd.synth import splitmix_array
    want = passes * grid_slots(cus)
    data = splitmix_array(seed, 6 * want)
    recs = oracle.split(table, data, bits=I_BITS, min_size=I_MIN)
    assert len(recs) > want, (len(recs), want)
    end = int(recs["offset"][want - 1] + recs["len"][want - 1])
    data = np.ascontiguousarray(data[:end])
    return data, oracle.split(table, data, bits=I_BITS, min_size=I_MIN)


J_BITS, J_MIN = 28, 1024
J_LONG = (2100, 2050, 2000)       # blocks; everything else under the floor
J_WANT = _want(3, 3, 3, 3, 40, 3)


def planted_run():
    """(streams, planned lengths per stream): a stream that splits into 3 chunks of 2,000 to 2,100
    blocks among 37 of 17 to 900 blocks (sha_edges.planted_stream, Bits 28), a second of two
    short chunks and a third that is one forced chunk: 43 records, then three stream slots that
    hold no job. tlen = tlen2 = 1,024 as in case A."""
    rng = np.random.default_rng(0x7A)
    short = [int(n) for n in rng.integers(17, 901, 39)]
    first = short[:37] + list(J_LONG)
    rng.shuffle(first)
    lens = [[E.length(b, E.TAILS[i % 5]) for i, b in enumerate(first)],
            [E.length(b, E.TAILS[i % 5]) for i, b in enumerate(short[37:])]]
    streams = [E.planted_stream(v, 0x7A + s) for s, v in enumerate(lens)]
    streams.append(rng.integers(0, 256, 5000, dtype=np.uint8))
    return streams, lens + [[5000]]
