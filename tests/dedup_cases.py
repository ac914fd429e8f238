"""Inputs and the model for bsg_engine_dedup / bsg_refset / bsg_engine_pack_unique.

The model is a dict from ref bytes to first index over the ORACLE's records of the same bytes;
expected first / uniq / pack_off and the packed bytes follow from it. Every builder returns host
streams (uint8 arrays) and the split parameters; tests/test_dedup_cpu.py holds each builder to
the properties it claims, tests/test_gpu_dedup.py and tests/test_gpu_dedup_wide.py run them on
the device."""
from __future__ import annotations

import os
import re

import numpy as np

from bs_amd.synth import edit_stream, splitmix_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bs_amd", "csrc")
IN_SET = 1 << 63


def constants() -> dict:
    """The set's starting size and load limit and the pack tile, read from the source."""
    out = {}
    with open(os.path.join(CSRC, "bsgpu_internal.h")) as f:
        text = f.read()
    for name in ("kRefSetSlots0", "kRefSetLoadPct", "kPackTile"):
        m = re.findall(r"^constexpr\s+uint(?:32|64)_t\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


def doubling_points(k: int = 2) -> list[int]:
    """The key counts at which a set's table is full to its load limit: one more key doubles it."""
    c = constants()
    return [(c["kRefSetSlots0"] << j) * c["kRefSetLoadPct"] // 100 for j in range(k)]


# ---- layout and the oracle's records ----------------------------------------------------------
def place(streams):
    """Streams packed at 16-byte offsets: (host buffer, off, lens)."""
    off, o = [], 0
    for d in streams:
        off.append(o)
        o += (len(d) + 15) & ~15
    host = np.zeros(max(o, 16), dtype=np.uint8)
    for d, p in zip(streams, off):
        host[p:p + len(d)] = d
    return host, off, [len(d) for d in streams]


def oracle_records(O, table, streams, bits, min_size):
    """The oracle's records of every stream, stream-major, `stream` filled in."""
    parts = []
    for s, d in enumerate(streams):
        r = O.split(table, np.ascontiguousarray(d), bits=bits, min_size=min_size).copy()
        r["stream"] = s
        parts.append(r)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=O.CHUNK_DTYPE)


# ---- the model -----------------------------------------------------------------------------
def first_index(refs, seen=frozenset()):
    """refs: a list of bytes. Returns (first, new): first[i] = the smallest j with refs[j] ==
    refs[i], | IN_SET if refs[i] is in `seen`; new = the indices i with first[i] == i."""
    where, first, new = {}, [], []
    for i, r in enumerate(refs):
        j = where.setdefault(r, i)
        if r in seen:
            first.append(j | IN_SET)
        else:
            first.append(j)
            if j == i:
                new.append(i)
    return first, new


def brute_first(refs, seen=frozenset()):
    """first_index by comparing every pair."""
    first, new = [], []
    for i, r in enumerate(refs):
        j = min(k for k in range(i + 1) if refs[k] == r)
        inset = any(r == q for q in seen)
        first.append(j | (IN_SET if inset else 0))
        if j == i and not inset:
            new.append(i)
    return first, new


def ref_list(recs):
    return [r.tobytes() for r in recs["ref"]]


def expected(recs, seen=frozenset()):
    """(first, uniq, pack_off) as uint64 arrays for records `recs` and the set `seen`."""
    first, new = first_index(ref_list(recs), seen)
    lens = [int(recs["len"][i]) for i in new]
    pack_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) if new \
        else np.zeros(1, np.uint64)
    return (np.array(first, dtype=np.uint64), np.array(new, dtype=np.uint64), pack_off)


def packed(streams, recs, uniq) -> bytes:
    """The host copies of the new chunks, concatenated."""
    out = []
    for i in uniq:
        r = recs[int(i)]
        d = streams[int(r["stream"])]
        out.append(bytes(d[int(r["offset"]):int(r["offset"]) + int(r["len"])]))
    return b"".join(out)


# ---- builders: (streams, bits, min_size) ------------------------------------------------------
MIB = 1 << 20


def edited_copies():
    """BASELINE configs[4] scaled to 2 x 1 MiB: stream B = stream A with 16 seeded edits
    (overwrite / insert / delete) of 256 bytes. More than half of B's chunks are A's."""
    a = splitmix_array(0xB5B52026, MIB)
    b = edit_stream(a, 5, sites=16, span=256)
    return [a, b], 8, 64


def residues():
    """512 KiB of SplitMix at Bits 5 / MinSize 64 (about 5,000 chunks of every length residue),
    listed after 80 excerpts of 2,000 bytes of itself: each excerpt's chunks are duplicates when
    the long stream reaches them, which shifts the packed offset against the source offset by
    another amount, so every pair (source address mod 16, packed offset mod 16) occurs."""
    d = splitmix_array(77, 512 << 10)
    cuts = [d[3000 + 6400 * j:5000 + 6400 * j] for j in range(80)]
    return cuts + [d], 5, 64


def tiny_chunks():
    """4 KiB at Bits 1 / MinSize 1: chunks of 1 to a few bytes; the 1-byte ones have only 256
    values, so at least a third of the chunks repeat an earlier one and the new ones lie between
    them (packing skips segments, and many segments share one 16-byte vector)."""
    return [splitmix_array(31, 4 << 10)], 1, 1


def zeros():
    """An all-zero stream at MinSize 64: every chunk but possibly the last is identical."""
    return [np.zeros(10_000, dtype=np.uint8)], 6, 64


def one_chunk_streams(n: int = 3000):
    """n one-chunk streams (Bits 33 never splits) of 64 bytes; every third repeats the stream two
    before it."""
    out = []
    for s in range(n):
        seed = s - 2 if s % 3 == 2 else s
        out.append(splitmix_array(9000 + seed, 64))
    return out, 33, 64


def long_segment():
    """One 3 MiB stream at Bits 33: a single chunk longer than the pack tile, at an odd length."""
    return [splitmix_array(41, 3 * MIB + 5)], 33, 64


def long_among_short(n: int = 2000):
    """That chunk with n one-chunk streams of 64-200 bytes before it and n after it."""
    rng = np.random.default_rng(12)
    lens = rng.integers(64, 201, 2 * n)
    short = [splitmix_array(50_000 + s, int(m)) for s, m in enumerate(lens)]
    return short[:n] + long_segment()[0] + short[n:], 33, 64


def shared_halves():
    """Two groups of 8 streams of 24 KiB: the first 4 streams of each group are the same bytes,
    the other 4 differ (two engines, one set)."""
    common = [splitmix_array(600 + s, 24 << 10) for s in range(4)]
    own = [[splitmix_array(700 + 10 * g + s, 24 << 10) for s in range(4)] for g in range(2)]
    return [common + own[0], common + own[1]], 7, 64


def planted_refs() -> np.ndarray:
    """Host refs for bsg_refset_add, (n, 32) uint8, in this order:
    64 that share their first 8 bytes and differ only in byte 31; 64 equal except in byte 8;
    4,096 random ones that all share their low 16 bits (bytes 0 and 1); an all-zero and an
    all-0xFF ref; then exact repeats of 200 earlier entries."""
    rng = np.random.default_rng(4)
    a = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (64, 1))
    a[:, 31] = np.arange(64)
    b = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (64, 1))
    b[:, 8] = np.arange(64) + 100
    c = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    c[:, 0], c[:, 1] = 0x34, 0x12
    d = np.stack([np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)])
    base = np.concatenate([a, b, c, d])
    again = base[rng.integers(0, len(base), 200)]
    return np.concatenate([base, again])


def random_refs(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


# ---- more than one grid pass, and the table's end (tests/test_gpu_dedup_wide.py) --------------
def wide_counts(cus: int):
    """(T, N0). T: the threads of one pass of an engine_grid launch on `cus` CUs, so item T is a
    thread's second trip; N0 = max(T, 256 x kSumTile): from N0 items on k_sum_mid also sums two
    parts per thread. Both from the source (walk_cases.grid_caps)."""
    import walk_cases as W
    t = W.grid_threads(cus)
    return t, max(t, 256 * W.grid_caps()["kSumTile"])


def packed_gather(streams, recs, uniq) -> bytes:
    """packed() as one numpy gather, for runs of several hundred thousand records."""
    host, off, _ = place(streams)
    u = np.asarray(uniq, dtype=np.int64)
    lens = recs["len"][u].astype(np.int64)
    src = np.asarray(off, dtype=np.int64)[recs["stream"][u]] + recs["offset"][u].astype(np.int64)
    dst = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return host[np.repeat(src - dst[:-1], lens) + np.arange(dst[-1])].tobytes()


def wide_facts(recs, first, uniq, t: int, main: int) -> dict:
    """What wide_run claims, counted from the records and the model's result: the records, the new
    ones, those whose first occurrence lies more than t records back, the duplicates inside
    stream `main` and the distinct record lengths."""
    f = np.asarray(first, dtype=np.int64)
    i = np.arange(len(f))
    return {"nrec": len(recs), "nunique": len(uniq), "far": int((f < i - t).sum()),
            "dups_in_main": int(((f < i) & (recs["stream"] == main)).sum()),
            "nlens": len(np.unique(recs["len"]))}


def wide_ok(facts: dict, t: int, n0: int) -> bool:
    return (facts["nrec"] > n0 + 100 and facts["nunique"] > t + 100 and facts["far"] >= 1000
            and facts["dups_in_main"] >= 1000 and facts["nlens"] >= 16)


WIDE_EXCERPTS = 80


def wide_run(O, table, cus: int):
    """A run of more than N0 new records: ((streams, bits, min_size), the oracle's records).
    Streams: 80 excerpts of 2,000 bytes spread over the main stream (their chunks are duplicates
    where the main stream reaches them, so rank[i] departs from i early); the main stream,
    SplitMix at Bits 1 / MinSize 8 (records of 8 to some 25 bytes), 10.5 bytes per record of N0
    and a quarter more until wide_ok holds; and a copy of at least 64 KiB from byte 4,096 of the
    main stream, whose chunks repeat records more than T back."""
    t, n0 = wide_counts(cus)
    size = int(10.5 * n0)
    while True:
        main = splitmix_array(0x51DE, size)
        step = size // WIDE_EXCERPTS
        cuts = [main[3000 + step * j:5000 + step * j] for j in range(WIDE_EXCERPTS)]
        streams = cuts + [main, main[4096:4096 + max(64 << 10, size // 64)].copy()]
        recs = oracle_records(O, table, streams, 1, 8)
        first, uniq, _ = expected(recs)
        if wide_ok(wide_facts(recs, first, uniq, t, WIDE_EXCERPTS), t, n0):
            return (streams, 1, 8), recs
        size += size // 4


def wide_small(main):
    """A small run at wide_run's parameters that shares content with it: a slice of the main
    stream between two streams of its own."""
    return [splitmix_array(0x51DF, 30_000), main[100_000:160_000].copy(),
            splitmix_array(0x51E0, 20_001)], 1, 8


def past_grid_refs(cus: int, repeats: int = 4096):
    """Host refs for three bsg_refset_add calls on one set: (a, b, c, P).
    a: n1 = T + 101 distinct random refs. b: the P - n1 fresh refs that bring the count to P, the
    first doubling point >= n1, the first `repeats` of them leading; among the rest, at random
    places, repeats of refs of a, and from entry T + repeats on a repeat of each leading ref (more
    than T entries after its first occurrence). b is longer than T + 2 x repeats. c: one fresh
    ref, the one that doubles a table of P keys."""
    t, _ = wide_counts(cus)
    n1 = t + 101
    p = next(x for x in doubling_points(50) if x >= n1)
    refs = random_refs(33, p + 1)
    a, fresh, c = refs[:n1], refs[n1:p], refs[p:]
    rng = np.random.default_rng(34)
    f = len(fresh)
    assert f >= repeats
    nold = max(f // 4, t + 3 * repeats - f)
    total = f + nold + repeats
    b = np.zeros((total, 32), dtype=np.uint8)
    b[:repeats] = fresh[:repeats]
    rep_at = t + repeats + rng.choice(total - t - repeats, repeats, replace=False)
    b[rep_at] = fresh[:repeats]
    rest = np.setdiff1d(np.arange(repeats, total), rep_at)
    old_at = rng.choice(rest, nold, replace=False)
    b[old_at] = a[rng.integers(0, n1, nold)]
    b[np.setdiff1d(rest, old_at)] = fresh[repeats:]
    return a, b, c, p


def same_ref(n: int) -> np.ndarray:
    """n copies of one ref."""
    return np.tile(random_refs(35, 1), (n, 1))


def two_ref_stream(table, n: int):
    """planting.level_stream's run of n level-0 chunks of 64 bytes at Bits 8 / MinSize 64: two
    distinct windows in turn, so two distinct refs."""
    import planting
    return [planting.level_stream(table, 8, np.zeros(n, dtype=np.int64))], 8, 64


WRAP_HEAD = 48   # refs whose first 8 bytes are 0xFF: their home is the last slot of any table
WRAP_LOW = 48    # refs whose first 8 bytes are the integers 0 .. 47: their homes are slots 0 .. 47


def wrap_base() -> np.ndarray:
    """The 96 distinct refs of wrap_refs: 48 with an all-0xFF head (the first 16 differ only in
    byte 31, the others anywhere in bytes 8 .. 31), then 48 with heads 0 .. 47, little-endian."""
    rng = np.random.default_rng(58)
    ff = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (WRAP_HEAD, 1))
    ff[:16, 31] = np.arange(16) + 7
    ff[16:, 8:] = rng.integers(0, 256, (WRAP_HEAD - 16, 24), dtype=np.uint8)
    ff[:, :8] = 0xFF
    lo = rng.integers(0, 256, (WRAP_LOW, 32), dtype=np.uint8)
    lo[:, :8] = np.arange(WRAP_LOW, dtype="<u8").view(np.uint8).reshape(WRAP_LOW, 8)
    return np.concatenate([ff, lo])


def wrap_refs() -> np.ndarray:
    """wrap_base with exact repeats of 15 refs of either kind, shuffled: the probe sequence of the
    0xFF heads steps off the table's last slot and goes on from slot 0 through the homes of the
    others, whatever the table's size."""
    rng = np.random.default_rng(59)
    base = wrap_base()
    again = np.concatenate([base[rng.choice(WRAP_HEAD, 15, replace=False)],
                            base[WRAP_HEAD + rng.choice(WRAP_LOW, 15, replace=False)]])
    both = np.concatenate([base, again])
    return both[rng.permutation(len(both))]


def wrap_absent() -> np.ndarray:
    """A ref with an all-0xFF head that wrap_base does not hold."""
    r = wrap_base()[20].copy()
    r[9] ^= 0x5A
    return r


WRAP_FILL = 8


def end_fillers() -> np.ndarray:
    """8 refs with the heads 2^64 - 2 .. 2^64 - 9: their homes are the 8 slots before the last
    one of any table. With wrap_base in the table too, its last 9 slots are taken."""
    r = random_refs(63, WRAP_FILL)
    r[:, :8] = (~np.arange(1, WRAP_FILL + 1, dtype="<u8")).view(np.uint8).reshape(WRAP_FILL, 8)
    return r


def wrap_run():
    """400 KB at Bits 6 / MinSize 64, about 3,000 records: SHA-256 refs cannot be planted, but of
    so many some twenty have their home in the last 9 slots of a new set's table (near_end)."""
    return [splitmix_array(71, 300_000), splitmix_array(72, 100_001)], 6, 64


def near_end(recs, slots: int, k: int = WRAP_FILL + 1) -> np.ndarray:
    """The indices of the records whose ref's home is one of the last k slots of `slots`."""
    heads = np.ascontiguousarray(recs["ref"][:, :8]).view("<u8").ravel()
    return np.flatnonzero((heads & np.uint64(slots - 1)) >= np.uint64(slots - k))


def home(ref, slots: int) -> int:
    """The slot a probe for `ref` starts at: its first 8 bytes, little-endian, modulo the size."""
    return int.from_bytes(bytes(ref[:8]), "little") & (slots - 1)


def probe_slots(refs, slots: int) -> dict:
    """Plain linear probing of the distinct refs in list order into a table of `slots`:
    {ref bytes: slot}."""
    tab, where = [None] * slots, {}
    for r in refs:
        k = bytes(r)
        if k in where:
            continue
        s = home(r, slots)
        while tab[s] is not None:
            s = (s + 1) % slots
        tab[s] = k
        where[k] = s
    return where
