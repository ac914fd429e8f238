"""Chunk lengths on k_sha's SHA-256 edges, one list per path, and streams that split into exactly
those chunks (shared by test_gpu_sha_tiers.py and test_gpu_blob_hash.py; no test in here).

A message of L bytes takes nblocks = (L + 8) // 64 + 1 blocks. L % 64 decides the last blocks:
up to 55 the padding and the length word fit behind the data; from 56 the length word spills into
a block of its own (56, 63); 0 and 1 are the exact block multiples. nblocks relative to a path's
ring fill (64 blocks for a helped solo chain, two halves that alternate; 8 for a group ticket; 2
for a pair ticket) decides how many blocks the last fill holds and which half it lands in.

Which path a job takes depends on its length relative to the longest of the run (k_bucket_scan).
The lists below are laid out for a lightly loaded run whose longest job has 3,457 blocks: the 16
longest (HELPED) run as helped solo chains, GROUP on group tickets, PAIR on pair tickets, LANE one
per lane. The tests assert those counts through Engine.tiers(); when the thresholds are retuned
and a count moves, re-choose the block counts here."""
import numpy as np

TAILS = (56, 0, 55, 1, 63)  # L % 64, cycled through every list

# fills of 64: nblocks = 63, 0, 1 (mod 64), at an even number of fills (3456 = 54 x 64,
# 3328 = 52, 1792 = 28) and an odd one (3392 = 53, 1856 = 29, 1728 = 27)
HELPED = [3457, 3456, 3455, 3329, 3328, 3327, 1857, 1856, 1855, 1793, 1792, 1791, 1729, 1728,
          1727, 3392]
# fills of 8: nblocks = 0, 1, 7 (mod 8); 21 jobs = two full tickets whose chains end on
# different fills, and a last ticket with three empty slots
GROUP = [n + d for n in range(1720, 1671, -8) for d in (0, 1, -1)]
# fills of 2: even and odd nblocks, from 1,650 down to 1,050 in one ticket's 32 jobs, and nine
# in a last ticket with 23 empty slots
PAIR = [1650 - 15 * i for i in range(41)]
# one per lane: from a chunk of exactly MinSize (1024 bytes: 17 blocks, tail 0) up to just
# under the wave paths
LANE = [18, 17, 19, 63, 64, 65, 127, 128, 129, 500, 777, 1000, 1023, 1024, 1030]


def length(nblocks: int, tail: int) -> int:
    """The L with (L + 8) // 64 + 1 == nblocks and L % 64 == tail."""
    n = 64 * (nblocks - (1 if tail <= 55 else 2)) + tail
    assert (n + 8) // 64 + 1 == nblocks and n % 64 == tail
    return n


def nblocks(n: int) -> int:
    return (int(n) + 8) // 64 + 1


def tier_lengths() -> dict:
    """{'helped' | 'group' | 'pair' | 'lane': [L, ...]}: every block count above with a tail from
    TAILS, so that each class (nblocks mod 64 in HELPED, mod 8 in GROUP, parity in PAIR) meets
    every tail."""
    out = {}
    for name, blocks in (("helped", HELPED), ("group", GROUP), ("pair", PAIR), ("lane", LANE)):
        out[name] = [length(b, TAILS[i % 5]) for i, b in enumerate(blocks)]
    return out


def boundary_patch(seed: int) -> np.ndarray:
    """65 bytes that end a chunk wherever they end: a 64-byte window of period 32, whose rolling
    hash is 0 (test_oracle.py::test_period32_windows_hash_to_zero), so a boundary at any Bits, of
    level 32 - Bits; the byte before it breaks the period, so the window one byte earlier is
    not such a window too."""
    unit = np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)
    return np.concatenate([[unit[31] ^ 0xFF], unit, unit]).astype(np.uint8)


def plant(data: np.ndarray, lens, seed: int):
    """Writes boundary_patch(seed) into data to end at every cumulative sum of lens (each at
    least 65); yields (offset, patch) for a caller that mirrors the writes elsewhere. The caller
    checks with the oracle that no natural candidate splits a chunk."""
    patch = boundary_patch(seed)
    end = 0
    for n in lens:
        end += int(n)
        data[end - 65:end] = patch
        yield end - 65, patch


def early_lengths(long_pair, seed: int, total: int = (256 << 20) + 4096) -> list:
    """Chunk lengths of a stream of at least `total` bytes (an engine run takes early chains from
    256 MiB): chunks of 200,000 to 400,000 bytes, and the two of long_pair (longer than those)
    a third and two thirds of the way in, each after a chunk of at least MinSize."""
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < total:
        lens.append(int(rng.integers(200_000, 400_000)))
    k = len(lens)
    lens[k // 3], lens[2 * k // 3] = long_pair
    while sum(lens) < total:
        lens.append(int(rng.integers(200_000, 400_000)))
    assert min(long_pair) > 400_000
    return lens


def planted_stream(lens, seed: int) -> np.ndarray:
    """Random bytes that split into exactly lens (see plant)."""
    data = np.random.default_rng(seed).integers(0, 256, int(sum(lens)), dtype=np.uint8)
    for _ in plant(data, lens, seed):
        pass
    return data


def check_tiers(diag, tiers, planned, njobs):
    """The counters of a run whose jobs are tier_lengths(): every list on its path.
    The counts are those of the lists, and the tickets follow k_bucket_scan's formula: the 16
    longest jobs solo, eight to a group ticket, 32 to a pair ticket."""
    print("sha tiers:", tiers, {k: diag[k] for k in ("nlong", "nshort", "max_nblocks")})
    n8, nlong = tiers["nlong_grp"], diag["nlong"]
    assert tiers["helped"] == 16 == len(planned["helped"])
    assert n8 > 16 and n8 == 16 + len(planned["group"])
    assert nlong > n8 and nlong - n8 == len(planned["pair"])
    assert diag["nshort"] > 0 and diag["nshort"] == njobs - nlong
    assert tiers["tickets_grp"] == 16 + -(-(n8 - 16) // 8)
    assert tiers["wave_tickets"] == tiers["tickets_grp"] + -(-(nlong - n8) // 32)
    assert diag["wave_tickets"] == tiers["wave_tickets"]
    # more than one group and one pair ticket, the last of each with empty slots
    assert n8 - 16 > 8 and (n8 - 16) % 8 != 0
    assert nlong - n8 > 32 and (nlong - n8) % 32 != 0
    assert tiers["early"] == (False, False)
    assert diag["max_nblocks"] == max(map(nblocks, planned["helped"]))
