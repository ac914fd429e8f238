"""Small planted runs for the host tail (k_offload_hist, k_offload_cut, k_offload_take,
k_offload_gather, the hash workers, k_offload_fix), and a model of the forced cut.
Shared by test_tail_cases_cpu.py, which holds every builder and the model to their claims against
the oracle, and by test_gpu_host_tail.py and test_gpu_host_tail_edges.py, which run the cases on the
device with Engine.set_host_tail(0, force_cut=..., ring_bytes=...). No test in here.

The cases are built like the early chains' (early_cases.Case, make(), L, _c): every chunk ends in
a planted window, so its length, and with the stream's 16-byte aligned offset its start address
modulo 16, is chosen. A case's note says how it is run: force_cut, ring_bytes, and what the case
is about.

The model (model()) restates the forced path of bsgpu_tail.inc. In a one-shot engine run every
record is a fresh final chunk, so a record is a candidate once it has `force_cut` blocks:

    blocks(len)   (len + 8) // 64 + 1; mx is the run's longest
    bucket        min(blocks // (mx // 256 + 1), 255)
    slot(len)     (len + 16 + 255) & ~255, the chunk's place in the ring
    the cut       whole non-empty buckets from the top, while the list (count <= max_items) and
                  the ring (slot bytes <= ring_bytes) hold the bucket as well
    longest left  the longest candidate of the first bucket left; min(force_cut - 1, mx) when
                  every candidate is taken; mx when none is
    cut_blocks    the lowest taken bucket's lower edge, at least force_cut; 0 when none is taken
"""
import contextlib

import numpy as np

import early_cases as C
import sha_edges as E

L, _c = C.L, C._c
BUCKETS, MAX_ITEMS, SLOT = 256, 4096, 256     # kTailBuckets, kTailMaxItems, kTailSlotAlign
MIN_BLOCKS = 256                              # kTailMinBlocks: the cost model's floor
GATHER_WGS, GATHER_THREADS = 64, 1024         # k_offload_gather's grid
RING = 4 << 20                                # a ring that holds every case but the list limits
SHORT = [1100, 1300, 1197, 1250, 1111, 1400]  # 18 to 22 blocks


# ---------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------
def blocks(n):
    return (int(n) + 8) // 64 + 1


def slot(n):
    return (int(n) + 16 + SLOT - 1) & ~(SLOT - 1)


def width(mx):
    return mx // BUCKETS + 1


def bucket(mx, nb):
    return min(nb // width(mx), BUCKETS - 1)


def model(lens, force_cut, ring_bytes, max_items=MAX_ITEMS):
    """The forced cut over a run's record lengths (all streams together): {"taken": the set of
    record indices, "chunks", "bytes", "host_blocks", "longest_blocks", "longest_left_blocks",
    "cut_blocks"}."""
    assert force_cut >= 1 and len(lens)
    nb = [blocks(n) for n in lens]
    mx = max(nb)
    per = {}
    for i, b in enumerate(nb):
        if b >= force_cut:
            per.setdefault(bucket(mx, b), []).append(i)
    taken, nbytes, left, lowest = [], 0, None, None
    for b in sorted(per, reverse=True):
        add = sum(slot(lens[i]) for i in per[b])
        if len(taken) + len(per[b]) > max_items or nbytes + add > ring_bytes:
            left = max(nb[i] for i in per[b])
            break
        taken += per[b]
        nbytes += add
        lowest = b
    if not taken:
        left = mx
    elif left is None:
        left = min(force_cut - 1, mx)
    return {"taken": set(taken), "chunks": len(taken), "bytes": nbytes,
            "host_blocks": sum(nb[i] for i in taken), "longest_blocks": mx,
            "longest_left_blocks": left,
            "cut_blocks": max(lowest * width(mx), force_cut) if taken else 0}


PLAN_FIELDS = ("chunks", "bytes", "host_blocks", "longest_blocks", "longest_left_blocks",
               "cut_blocks")


# ---------------------------------------------------------------------------------------------
# The gather's split of a chunk at a device address
# ---------------------------------------------------------------------------------------------
def gather_split(addr, n):
    """(head, nvec, tail) bytes/vectors of k_offload_gather's copy of n bytes from `addr`."""
    head = min(n, (16 - addr) & 15)
    nvec = (n - head) // 16
    return head, nvec, n - head - 16 * nvec


def starts(case, records):
    """The records' start addresses relative to the run's (16-byte aligned) buffer."""
    return [case.off[r[4]] + r[0] for r in records]


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
def plan(longs, tail=("r", 700)):
    """Two short chunks, then every chunk of `longs` followed by a short one, then the tail."""
    out = _c(SHORT[0], SHORT[1])
    for i, n in enumerate(longs):
        out += _c(n, SHORT[(i + 2) % len(SHORT)])
    return out + [tail]


def three():
    """Three chunks far longer than the rest (test_gpu_host_tail.py's main case)."""
    return C.Case("tail-three", [plan([L(2050, 55), L(1705, 56), L(1333, 1)])], 101)


def gather_ends():
    """Streams of one planted chunk of 1100 + r bytes and a forced final chunk of t bytes. The
    first chunk starts on the 16-byte grid (the stream's offset), the final one at every residue
    a = (1100 + r) % 16; with head = (16 - a) & 15 its length is below head, head, between head
    and head + 16, head + 16, and head + 32 + k for a k that takes every value modulo 16."""
    plans, meta = [], []
    for a in range(16):
        r = (a - 1100) % 16
        head = (16 - a) & 15
        ts = [head + 1 + a % 15, head + 16, head + 32 + (7 * a + 3) % 16]
        if head >= 1:
            ts.append(head)
        if head >= 2:
            ts += [head - 1, 1]
        for t in ts:
            plans.append([("c", 1100 + r + 16 * (len(plans) % 3)), ("r", t)])
            meta.append((a, head, t))
    c = C.Case("tail-gather-ends", plans, 201)
    c.note.update(force_cut=1, ring_bytes=RING, finals=meta)
    return c


LOOP_NVEC = (1023, 1024, 1025, 3071, 3072, 3073, 4095, 4096, 4097, 7169)
_LOOP_RESIDUE = (0, 5, 11, 0, 1, 15, 8, 3, 0, 13)
_LOOP_TAIL = (0, 1, 15, 7, 0, 9, 3, 0, 12, 5)


def gather_loop():
    """One stream: for every nvec of LOOP_NVEC a short chunk as long as puts the next chunk's
    start at a chosen residue, then a chunk of head + 16 nvec + tail bytes. The 4x-unrolled loop
    (v + 3 x 1024 < nvec) is not entered at 3072 and entered by thread 0 alone at 3073; at 1024
    no thread has a second vector, at 1025 thread 0 has."""
    pl, o, longs = [], 0, []
    for nvec, a, tb in zip(LOOP_NVEC, _LOOP_RESIDUE, _LOOP_TAIL):
        s = 1100 + (a - (o + 1100)) % 16
        n = ((16 - a) & 15) + 16 * nvec + tb
        pl += _c(s, n)
        longs.append((o + s, n, nvec))
        o += s + n
    c = C.Case("tail-gather-loop", [pl + [("r", 700)]], 202)
    c.note.update(force_cut=1, ring_bytes=RING, longs=longs)
    return c


def many_chunks():
    """One stream of 230 planted chunks of 1100 to 3000 bytes drawn from 100 lengths: with
    force_cut = 1 each of the gather's 64 workgroups copies three or four chunks."""
    rng = np.random.default_rng(203)
    pool = rng.integers(1100, 3001, 100)
    lens = [int(pool[k]) for k in rng.integers(0, len(pool), 230)]
    c = C.Case("tail-many-chunks", [_c(*lens) + [("r", 700)]], 203)
    c.note.update(force_cut=1, ring_bytes=RING, lens=lens)
    return c


LIST_BLOCKS = range(3, 39)        # list-limit (a): 36 block counts, one bucket each
LIST_PER = 115
LIST_RING = 16 << 20


def list_limit_a():
    """4,140 chunks of 3 to 38 blocks, 115 of each, in a shuffled order, and a final chunk of 20
    blocks: 4,141 candidates in 36 buckets one block wide. The 35 buckets from the top hold
    4,026, the last one 115 more: it is left whole. At MinSize 128, so that the run stays under
    6 MB (at MinSize 1024 the chunks would begin at 17 blocks, 10 MB)."""
    rng = np.random.default_rng(204)
    nb = rng.permutation(np.repeat(np.array(LIST_BLOCKS), LIST_PER))
    lens = [64 * (int(b) - 1) + (13 * i) % 56 for i, b in enumerate(nb)]
    c = C.Case("tail-list-a", [_c(*lens) + [("r", L(20, 5))]], 204)
    c.min_size = 128
    c.note.update(force_cut=1, ring_bytes=LIST_RING)
    return c


def _one_bucket(name, count, seed):
    lens = [1080 + (29 * i) % 64 for i in range(count - 1)]     # 18 blocks each
    c = C.Case(name, [_c(*lens) + [("r", 1100)]], seed)
    c.note.update(force_cut=1, ring_bytes=LIST_RING)
    return c


def list_limit_b():
    """4,096 chunks of 18 blocks, the forced final one among them: the list at equality."""
    return _one_bucket("tail-list-b", MAX_ITEMS, 205)


def list_limit_c():
    """4,097 chunks of 18 blocks: one bucket that does not fit; nothing is taken."""
    return _one_bucket("tail-list-c", MAX_ITEMS + 1, 206)


RING_BUCKETS = ((519, 520, 520), (510, 511, 512, 512), (495, 496, 497, 495, 497), (480, 481, 482))


def ring_limit():
    """mx = 520 blocks, buckets 3 blocks wide; 3, 4, 5 and 3 chunks in buckets 173, 170, 165 and
    160, in a mixed order, short chunks between them. ring_values() gives the three rings."""
    order = [(k, i) for k, g in enumerate(RING_BUCKETS) for i in range(len(g))]
    order = [order[k] for k in np.random.default_rng(207).permutation(len(order))]
    longs = [L(RING_BUCKETS[k][i], E.TAILS[(k + i) % 5]) for k, i in order]
    c = C.Case("tail-ring", [plan(longs)], 207)
    c.note.update(force_cut=MIN_BLOCKS)
    return c


def ring_values(lens):
    """{name: (ring_bytes, buckets taken)} from the slot sums of the top four buckets of a
    ring_limit run with the record lengths `lens`."""
    mx = max(blocks(n) for n in lens)
    per = {}
    for n in lens:
        if blocks(n) >= MIN_BLOCKS:
            per.setdefault(bucket(mx, blocks(n)), []).append(slot(n))
    top = [per[b] for b in sorted(per, reverse=True)]
    two = sum(top[0]) + sum(top[1])
    return {"equal": (two, 2), "one-less": (two - 1, 1),
            "three-and-a-slot": (two + sum(top[2]) + min(top[3]), 3)}


FLOOR_BLOCKS = range(999, 1009)
FLOOR_CUTS = (1004, 1007, 1008)


def floor_in_bucket():
    """mx = 2050 blocks, buckets 9 blocks wide: one chunk each of 999 to 1007 blocks (bucket 111)
    and of 1008 (bucket 112). The forced floors lie inside bucket 111, at its last block count
    and at bucket 112's first."""
    longs = [L(2050, 55)] + [L(b, E.TAILS[b % 5]) for b in FLOOR_BLOCKS]
    c = C.Case("tail-floor", [plan(longs)], 208)
    c.note.update(ring_bytes=RING)
    return c


def overflow_rerun():
    """70,000 zero bytes give a candidate at every position, past the first estimate of 65,536:
    the first run overflows with its tail stood down, and finish() runs it again."""
    pl = _c(1100, 1100) + [("r", 100), ("z", 70000)] + \
        _c(1500, L(2050, 55), 1300, L(1705, 56), 1200, L(1333, 1)) + [("r", 700)]
    c = C.Case("tail-overflow", [pl], 209)
    c.note.update(force_cut=1000, ring_bytes=RING)
    return c


CASES = {"tail-three": three, "tail-gather-ends": gather_ends, "tail-gather-loop": gather_loop,
         "tail-many-chunks": many_chunks, "tail-list-a": list_limit_a, "tail-list-b": list_limit_b,
         "tail-list-c": list_limit_c, "tail-ring": ring_limit, "tail-floor": floor_in_bucket,
         "tail-overflow": overflow_rerun}
_BUILT = {}


def get(table, name):
    """The built case `name` (built once per session)."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]().build(table)
    return _BUILT[name]


def expect(case, oracle, table):
    """early_cases.expect: the oracle's records, counts per stream and candidates."""
    return C.expect(case, oracle, table)


def rec_lens(want):
    return [r[1] for r in want["records"]]


# ---------------------------------------------------------------------------------------------
# Running a case on the device (the GPU tests' shared helpers)
# ---------------------------------------------------------------------------------------------
def tuples(ch):
    return [(int(c["offset"]), int(c["len"]), int(c["level"]), bytes(c["ref"]).hex(),
             int(c["stream"])) for c in ch]


@contextlib.contextmanager
def device(gpu, case):
    host = case.buffer()
    buf = gpu.DeviceBuffer(host.size)
    try:
        buf.from_host(host)
        yield buf
    finally:
        buf.free()


def run(eng, buf, case):
    eng.run(buf.ptr, case.off, case.lens, bits=case.bits, min_size=case.min_size)


def result(eng):
    return {"records": tuples(eng.chunks()), "counts": [int(x) for x in eng.counts()],
            "tail": eng.diag()["host_tail"], "early": eng.tiers()["early"]}


def split(gpu, case, early=False, **tail):
    with device(gpu, case) as buf:
        eng = gpu.Engine()
        try:
            eng.set_host_tail(0, **tail)
            if early:
                eng.set_early_min(0)
            run(eng, buf, case)
            eng.finish()
            return result(eng)
        finally:
            eng.close()


def check(got, want, what):
    bad = next((i for i, (g, w) in enumerate(zip(got["records"], want["records"])) if g != w),
               min(len(got["records"]), len(want["records"])))
    assert got["records"] == want["records"], (what, "first difference at record", bad,
                                               want["records"][bad:bad + 1],
                                               got["records"][bad:bad + 1])
    assert got["counts"] == want["counts"], what
