"""Where the bytes lie: pure-numpy builders of stream layouts for the engine and the hashers.

include/bsgpu.h lets a caller hand bsg_engine_run / bsg_engine_hash / bsg_split_hash_batch /
bsg_sha256_batch / bsg_hasher_sum a base plus arbitrary off[i], len[i]: any order, gaps,
overlapping and coinciding streams. Every builder here returns

    (buffer_size, [(off, len, seed)], description)

Stream i is buffer[off : off + len] and holds splitmix_array(seed, len); buffer_size covers every
stream plus READ_SLACK bytes. Streams that overlap carry seeds that agree on the shared bytes
(sub_seed), so one buffer satisfies all of them. tests/test_layouts_cpu.py holds the builders to
their claims; tests/test_gpu_layouts.py runs them on the device.
"""
from __future__ import annotations

import numpy as np

from bs_amd.synth import GAMMA, splitmix_array

READ_SLACK = 256  # BSG_READ_SLACK
LENS = [0, 1, 63, 64, 65, 2047, 2048, 2049, 4097, 70_001]
GAPS = [16, 48, 256, 4096]
SMALL = ("gaps", "descending", "shuffled", "aliased", "empties")
POISONS = (0x00, 0xFF, "random")
_MASK = (1 << 64) - 1


def align16(x: int) -> int:
    return (x + 15) & ~15


def sub_seed(seed: int, byte_off: int) -> int:
    """The seed of the stream that starts byte_off (a multiple of 8) bytes into the stream of
    `seed`: word i of seed S is splitmix64(S + (i + 1) * GAMMA), so skipping w words is
    S + w * GAMMA."""
    assert byte_off % 8 == 0
    return (seed + (byte_off // 8) * int(GAMMA)) & _MASK


def _ascending(seed0: int = 100):
    """LENS in ascending address order, GAPS (cycled) between one stream's end, rounded up to
    16, and the next stream's start."""
    streams, o = [], 0
    for i, n in enumerate(LENS):
        streams.append((o, n, seed0 + i))
        o = align16(o + n) + GAPS[i % len(GAPS)]
    return streams


def _size(streams) -> int:
    return max([o + n for o, n, _ in streams] + [0]) + READ_SLACK


def gaps():
    s = _ascending()
    return _size(s), s, "ascending, gaps of 16, 48, 256 and 4096 bytes"


def descending():
    s = _ascending()[::-1]
    return _size(s), s, "the streams of `gaps` listed in descending address order"


def shuffled():
    s = _ascending()
    order = np.random.default_rng(5).permutation(len(s))
    assert list(order) != sorted(order) and list(order) != sorted(order, reverse=True)
    s = [s[i] for i in order]
    return _size(s), s, "the streams of `gaps`, shuffled"


# aliased: index of each declared relation's streams in the list (tests check them)
ALIAS_SAME = (9, 10)        # the same (off, len) twice
ALIAS_PREFIX = (9, 11)      # [1] is a proper prefix of [0]
ALIAS_INTERIOR = (9, 12)    # [1] starts at a 16-aligned interior offset of [0], and ends inside
ALIAS_TAIL = (9, 13)        # [1] starts inside [0] and runs past its end: they share [0]'s tail


def aliased():
    s = _ascending()
    o, n, seed = s[9]
    assert n == 70_001
    s.append((o, n, seed))                                      # 10: the same bytes again
    s.append((o, 4097, seed))                                   # 11: a prefix
    s.append((o + 2048, 2049, sub_seed(seed, 2048)))            # 12: inside, 16-aligned start
    s.append((o + 65_536, 8192, sub_seed(seed, 65_536)))        # 13: shares only the tail
    # every length of LENS on aliased bytes too: prefixes of the long stream, listed before it
    pre = [(o, m, seed) for m in LENS[:-1]]
    s = s + pre
    return _size(s), s, ("`gaps` plus the long stream again, a prefix of it, a stream inside it, "
                         "one sharing only its tail, and prefixes of every length")


# empties: indices of the zero-length streams
EMPTY_AT = (0, 1, 4, 12, 13)


def empties():
    a = _ascending()
    last_o, last_n, _ = a[-1]
    s = [(0, 0, 1), (a[1][0], 0, 2)]            # at the start; sharing off with a non-empty one
    s += a[1:3]
    s.append((a[3][0] - 16, 0, 3))              # between others (in a gap)
    s += a[3:]
    s.append((align16(last_o + last_n), 0, 4))  # at the end of the last stream
    s.append((a[0][0], 0, 5))                   # LENS' own empty stream, listed last
    assert [i for i, (_, n, _) in enumerate(s) if n == 0] == list(EMPTY_AT)
    return _size(s), s, ("zero-length streams at the start, on a non-empty stream's off, in a "
                         "gap, at the end of the last stream, and last in the list")


def build(name: str):
    return {"gaps": gaps, "descending": descending, "shuffled": shuffled, "aliased": aliased,
            "empties": empties}[name]()


def stream_bytes(seed: int, n: int) -> np.ndarray:
    return splitmix_array(seed, n)


def _poison(poison, n: int, at: int = 0) -> np.ndarray:
    """n poison bytes for buffer offsets [at, at + n): a byte value, or "random"."""
    if isinstance(poison, str):
        assert poison == "random"
        lo = at // 8 * 8
        return splitmix_array(sub_seed(0xBAD5EED, lo), at - lo + n)[at - lo:]
    return np.full(n, poison, dtype=np.uint8)


def fill(layout, poison) -> np.ndarray:
    """The whole buffer: every stream's bytes, `poison` on every byte outside all streams."""
    size, streams, _ = layout
    buf = _poison(poison, size)
    for o, n, seed in streams:
        buf[o:o + n] = stream_bytes(seed, n)
    return buf


def pieces(layout, poison, slack: int = READ_SLACK):
    """fill() for a buffer too large to build: [(off, bytes)] over the union of every stream's
    [off, off + len + slack), streams written, `poison` on the rest of each piece. Nothing else
    of the buffer is touched."""
    size, streams, _ = layout
    iv = sorted((o, o + n + slack) for o, n, _ in streams)
    merged = []
    for lo, hi in iv:
        if merged and lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    out = []
    for lo, hi in merged:
        assert hi <= size
        b = _poison(poison, hi - lo, lo)
        for o, n, seed in streams:
            if lo <= o and o + n <= hi:
                b[o - lo:o - lo + n] = stream_bytes(seed, n)
        out.append((lo, b))
    return out


def covered(layout) -> np.ndarray:
    """bool per buffer byte: inside at least one stream."""
    size, streams, _ = layout
    m = np.zeros(size, dtype=bool)
    for o, n, _ in streams:
        m[o:o + n] = True
    return m


# ---- k_sha's address regions (job_region, bsgpu_kernels.hip) -------------------------------
REGION_BYTES = 1 << 30      # kRegionBytes: regions are on only for a span above it
MIN_REGION_JOBS = 4096      # kMinRegionJobs


def expected_region(off_of_first_byte: int, R: int, span: int) -> int:
    """Region 0 .. R-1 of a per-lane job whose first data byte is d_data[off_of_first_byte]."""
    o = off_of_first_byte
    if o <= 0 or R <= 1:
        return 0
    return min(o * R // max(span, 1), R - 1)


def expected_nregions(span: int, jobs: int, waves: int = 1024) -> int:
    """k_bucket_scan's R: one region per GiB of span, at least MIN_REGION_JOBS jobs each, at
    most waves / 16 (4 waves per CU: 64 on 256 CUs) and 256."""
    rmax = min(256, max(waves // 16, 1))
    return min(rmax, -(-span // REGION_BYTES), max(jobs // MIN_REGION_JOBS, 1))


def span_of(streams) -> int:
    """RunPlan::data_span: bytes from d_data to the end of the last stream (at least 1)."""
    return max([o + n for o, n, _ in streams] + [1])


GIB = 1 << 30
SPARSE_SIZE = 4 * GIB + (8 << 20) + READ_SLACK
_G1, _G2 = 1288490192, 2576980384  # about 1.2 and 2.4 GiB, multiples of 16


def group(at: int, seed0: int, nbytes: int = 4 << 20, nstreams: int = 4):
    """nstreams streams of odd lengths, about nbytes together, from `at` on with GAPS between."""
    per = nbytes // nstreams
    s, o = [], at
    for i in range(nstreams):
        n = per - 1 - 37 * i
        s.append((o, n, seed0 + i))
        o = align16(o + n) + GAPS[i % len(GAPS)]
    return s


def sparse(case: str):
    """The sparse layouts of one SPARSE_SIZE buffer (test_gpu_layouts part d)."""
    assert _G1 % 16 == 0 and _G2 % 16 == 0
    if case == "three_groups":
        s = group(0, 1000) + group(_G1, 2000) + group(_G2, 3000)
        d = "groups at 0, 1.2 and 2.4 GiB: R = 3, the first stream at d_data itself"
    elif case == "empty_region":
        s = group(0, 1000) + group(_G2, 3000)
        d = "groups at 0 and 2.4 GiB: R = 3 with region 1 empty"
    elif case == "last_region":
        s = [(0, 16, 4000)] + group(_G2, 3000) + group(_G2 + (5 << 20), 3100)
        d = "every stream in the last region but one 16-byte stream at offset 0"
    elif case == "border_inside":
        # span 1.5 GiB, R = 2: the border o * 2 // span == 1 lies at span / 2
        span = 3 * GIB // 2
        s = [(span // 2 - (2 << 20), 4 << 20, 5000), (span - 4096, 4096, 5001)]
        d = "a 4 MiB stream across the border of two regions"
    elif case == "past_4gib":
        s = group(0, 1000) + group((1 << 32) + 16, 6000)
        d = "a group at off >= 2^32 + 16: R = 5, data_off past 32 bits"
    elif case == "few_jobs":
        s = [(0, (512 << 10) - 1, 7000), (_G1, (512 << 10) + 1, 7001)]
        d = "span above 1 GiB with under 8,192 jobs: R = 1"
    else:
        raise KeyError(case)
    assert max(o + n for o, n, _ in s) + READ_SLACK <= SPARSE_SIZE
    return SPARSE_SIZE, s, d


SPARSE = ("three_groups", "empty_region", "last_region", "border_inside", "past_4gib",
          "few_jobs")
