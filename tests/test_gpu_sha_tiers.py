"""k_sha's five SHA-256 paths at chosen chunk lengths, in split runs. The streams are built so
that the chunker cuts them into exactly the planned lengths (sha_edges.py), unaligned chunk
starts included; the engine's own path choice (no knob) then puts those lengths on helped solo
chains, group tickets, pair tickets and single lanes at once, or the two longest on the early
chains, which Engine.tiers() shows. Every record is compared with the CPU oracle's."""
import numpy as np
import pytest

import sha_edges as E

pytestmark = pytest.mark.gpu

BITS, MIN_SIZE = 28, 1024  # about one natural candidate per 256 MiB; a planted one has level 4


def as_tuples(ch):
    return [(int(c["offset"]), int(c["len"]), int(c["level"]), bytes(c["ref"]).hex()) for c in ch]


@pytest.fixture(scope="module")
def tier_stream(oracle, table):
    """One stream of 93 chunks, 8.7 MB: sha_edges.tier_lengths() in a shuffled order. The
    oracle must cut it into exactly those lengths: a natural candidate that split a planted
    chunk would move it to another path unnoticed."""
    tiers = E.tier_lengths()
    lens = [n for v in tiers.values() for n in v]
    np.random.default_rng(1).shuffle(lens)
    data = E.planted_stream(lens, 1)
    want = oracle.split(table, data, bits=BITS, min_size=MIN_SIZE)
    assert want["len"].tolist() == lens
    assert set(want["level"].tolist()) == {32 - BITS}
    # wave-path chunks start at every residue mod 16 (bsg_engine_hash only takes aligned blobs)
    wave = set(tiers["helped"] + tiers["group"] + tiers["pair"])
    assert {int(c["offset"]) % 16 for c in want if int(c["len"]) in wave} == set(range(16))
    return data, want, tiers


def test_planted_tiers_device_run(gpu, tier_stream):
    """A device-resident Engine.run of the planted stream: all four k_sha paths in one launch
    (the counters say so), every record the oracle's."""
    data, want, planned = tier_stream
    buf = gpu.DeviceBuffer(data.size)
    eng = gpu.Engine()
    try:
        buf.from_host(data)
        eng.run(buf.ptr, [0], [data.size], bits=BITS, min_size=MIN_SIZE)
        assert eng.finish() == len(want)
        got = eng.chunks()
        bad = [(int(w["len"]), E.nblocks(w["len"])) for g, w in zip(got, want)
               if bytes(g["ref"]) != bytes(w["ref"])]
        assert not bad, bad
        assert as_tuples(got) == as_tuples(want)
        # the jobs: one per chunk (the stream ends at a boundary, so it leaves no tail job)
        E.check_tiers(eng.diag(), eng.tiers(), planned, len(want))
    finally:
        eng.close()
        buf.free()


def test_planted_tiers_host_batch(gpu, tier_stream):
    """The same stream from host memory through bsg_split_hash_batch, beside a short second
    stream (so the planted one does not start the packed buffer's only stream)."""
    data, want, _ = tier_stream
    rng = np.random.default_rng(2)
    short = rng.integers(0, 256, 5000, dtype=np.uint8)
    ch, counts = gpu.split_hash_batch([short, data], bits=BITS, min_size=MIN_SIZE)
    assert counts.tolist() == [1, len(want)]
    assert int(ch[0]["len"]) == 5000
    assert as_tuples(ch[1:]) == as_tuples(want)


@pytest.mark.parametrize("carry_cap", [0, 1 << 20], ids=["midstate", "bytes"])
def test_planted_tiers_streaming(gpu, tier_stream, carry_cap):
    """The stream through the streaming splitter in tiles of 1 MiB + 3: eight tile ends cut
    through chunks, wave-path lengths among them, so those chunks are continued in the next
    tile (from a SHA-256 midstate, or from carried bytes) and k_lens keeps them on single lanes,
    while the chunks inside a tile still go to the wave paths that tile's lengths give."""
    data, want, planned = tier_stream
    tile = (1 << 20) + 3
    wave = set(planned["helped"] + planned["group"] + planned["pair"])
    cut = [int(c["len"]) for c in want for k in range(tile, data.size, tile)
           if int(c["offset"]) < k < int(c["offset"] + c["len"])]
    assert len(cut) == data.size // tile and wave.intersection(cut), cut
    w = gpu.StreamingSplitter(bits=BITS, min_size=MIN_SIZE, tile=tile, carry_cap=carry_cap)
    try:
        got = []
        for i in range(0, data.size, 3 << 20):
            w.write(data[i:i + (3 << 20)])
            got.append(w.drain())
        w.close()
        got.append(w.drain())
    finally:
        w.free()
    assert as_tuples(np.concatenate(got)) == as_tuples(want)


# --------------------------------------------------------------------------------------------
# Early chains (k_early) at chosen lengths
# --------------------------------------------------------------------------------------------
EARLY_SEED = 7


@pytest.fixture(scope="module")
def early_base():
    from bs_amd.synth import splitmix_array
    return splitmix_array(0xEA51, 258 << 20)


@pytest.mark.parametrize("pair", [((8192, 0), (8193, 56)), ((8256, 55), (8257, 63)),
                                  ((8191, 56), (8255, 0))],
                         ids=lambda p: "-".join(f"{b}b{t}" for b, t in p))
def test_early_chains_at_fill_edges(gpu, oracle, table, early_base, pair):
    """A split run of 256.4 MiB whose two longest chunks, about 0.5 MiB each, the early chains
    take: (blocks, L % 64) on and next to a multiple of the chain's 64-block fill, at an even
    number of fills (8192 = 128 x 64) and an odd one (8256 = 129 x 64), the length word in the
    last data block or in a block of its own. Device bytes: fill_splitmix plus the planted
    boundaries, every 200,000 to 400,000 bytes; the host mirror is the same for the oracle,
    which must cut it into exactly the planned lengths. With the early chains on, both slots
    hash a chunk and the longest chain's stamps are the early chain's (it starts before k_sha);
    with them off k_sha hashes the two as helped solo chains; the records are the oracle's both
    ways."""
    longs = [E.length(b, t) for b, t in pair]
    lens = E.early_lengths(longs, EARLY_SEED)
    n = sum(lens)
    assert n >= 256 << 20  # engine runs below that take no early chains
    host = early_base[:n].copy()
    buf = gpu.DeviceBuffer(n)
    try:
        gpu.fill_splitmix(buf.ptr, n, 0xEA51)
        gpu.synchronize()
        for off, patch in E.plant(host, lens, EARLY_SEED):
            buf.from_host(patch, off)
        want = oracle.split(table, host, bits=BITS, min_size=MIN_SIZE)
        assert want["len"].tolist() == lens
        assert sorted(want["len"].tolist())[-2:] == sorted(longs)
        got = {}
        for on in (1, 0):
            with gpu.debug_knob(gpu.KNOB_EARLY, on):
                eng = gpu.Engine()
                try:
                    eng.run(buf.ptr, [0], [n], bits=BITS, min_size=MIN_SIZE)
                    assert eng.finish() == len(want)
                    got[on] = (eng.chunks(), eng.diag(), eng.tiers())
                finally:
                    eng.close()
    finally:
        buf.free()
    for on in (1, 0):
        ch, diag, tiers = got[on]
        print("early", on, tiers, diag.get("timeline_us"), diag.get("long"))
        bad = [(int(w["len"]), E.nblocks(w["len"])) for g, w in zip(ch, want)
               if bytes(g["ref"]) != bytes(w["ref"])]
        assert not bad, (on, bad)
        assert as_tuples(ch) == as_tuples(want), on
    # the stamped chain: early slot 0 holds the longest chunk; k_sha's ticket 0 is the head of
    # the longest-first order, which sorts by buckets of a few blocks, so either of two chunks
    # one block apart
    assert got[1][1]["long"]["blocks"] == max(b for b, _ in pair), got[1][1]
    assert got[0][1]["long"]["blocks"] in [b for b, _ in pair], got[0][1]
    assert got[1][2]["early"] == (True, True) and got[0][2]["early"] == (False, False)
    assert got[1][1]["timeline_us"]["long_start"] < 0, got[1][1]
    assert got[0][1]["timeline_us"]["long_start"] >= 0, got[0][1]
