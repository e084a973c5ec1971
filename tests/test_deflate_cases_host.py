"""The catalogue of tests/deflate_cases.py held against zlib, without a GPU: every accepted member is a valid DEFLATE stream that
zlib inflates to the case's payload, every refused one is refused by zlib (or by its trailer), and each case reaches the path of
csrc/vlr_inflate.hip it is named for — shown from the encoder's books, not from its name.  tests/test_gpu_inflate_streams.py gives
the same members to the kernel and expects zlib's bytes: this file is the proof that its inputs are valid and that zlib speaks."""
import zlib

import pytest

import deflate_cases as dc


@pytest.fixture(scope="module")
def cat():
    return dc.catalogue()


def _group(cat, g):
    cs = cat.group(g)
    assert cs, g
    return cs


def test_the_catalogue_has_what_the_kernel_is_to_be_held_against(cat):
    assert cat.groups == ["long codes", "overlap grid", "ring edge and far matches", "dynamic-header forms", "block structure"]
    names = [(c.group, c.name) for c in cat.accepted + cat.refused]
    assert len(set(names)) == len(names)
    assert len(cat.accepted) >= 100 and len(cat.refused) >= 25
    for c in cat.refused:
        reasons = c.reason if isinstance(c.reason, frozenset) else {c.reason}
        assert reasons and reasons <= set(range(1, 10)), c     # a reason of the inflate kernel (CRC mismatches are the CRC kernel's)


def test_every_member_is_within_the_bgzf_limits(cat):
    for c in cat.accepted + cat.refused:
        members = dc.split_members(c.data)
        assert len(members) == c.n_members, c
        for stream, crc, isize in members:
            assert 18 + len(stream) + 8 <= dc.BGZF_MAX and isize <= dc.BGZF_MAX, c


def test_zlib_inflates_every_accepted_member_to_the_payload(cat):
    for c in cat.accepted:
        got = b""
        for stream, crc, isize in dc.split_members(c.data):
            d = zlib.decompressobj(-15)
            out = d.decompress(stream)
            assert d.eof and d.unused_data == b"", c
            assert len(out) == isize and zlib.crc32(out) == crc, c
            got += out
        assert c.payload is not None and got == c.payload, c
        assert c.payload == c.model, c            # (the encoder's model agrees; nothing is expected from it)


def test_zlib_refuses_every_refused_member(cat):
    for c in cat.refused:
        (stream, crc, isize), = dc.split_members(c.data)
        try:
            d = zlib.decompressobj(-15)
            out = d.decompress(stream)
        except zlib.error:
            continue
        assert not d.eof or len(out) != isize, c   # the stream does not end, or ends with another size than the trailer's


def test_long_code_cases_use_15_bit_codes_in_each_class_and_a_48_bit_token(cat):
    cs = _group(cat, "long codes")
    for cls in ("literal", "length5", "eob", "dist13"):
        hits = [c for c in cs if c.stats.used.get(cls) == 15]
        assert hits, cls
        for c in hits:     # used often, in many blocks: the long codes start at many bit offsets
            assert c.stats.n_symbols >= 400 and c.stats.blocks >= 20, c
    assert max(c.stats.max_token_bits for c in cs) == 48 == 15 + 5 + 15 + 13
    # longest code exactly at and one above the single-lookup tables (kLitBits = 10, kDistBits = 9)
    longest = {(max(c.stats.used[k] for k in ("literal", "length", "eob")), c.stats.used["dist"]) for c in cs}
    assert {(10, 9), (11, 10), (15, 15)} <= longest
    # far matches behind long codes: the bit-serial walk of the batch loop feeds the far copy too
    assert any(d + l > dc.RING for c in cs for d, l in c.stats.pairs)


def test_the_grid_holds_every_distance_and_length_listed(cat):
    cs = _group(cat, "overlap grid")
    pairs = set().union(*(c.stats.pairs for c in cs))
    want = dc.grid_pairs()
    assert len(want) > 4000 and {d for d, _ in want} == set(range(1, 259))
    for dist in (1, 2, 100, 258):
        ls = dc.grid_lengths(dist)
        assert {3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 257, 258} <= set(ls)
        assert {min(258, max(3, x)) for x in (dist - 1, dist, dist + 1, 2 * dist - 1, 2 * dist, 2 * dist + 1)} <= set(ls)
    assert set(want) <= pairs
    assert set(dc.ring_size_pairs()) <= pairs
    assert {(dc.RING - l, l) for l in (3, 64, 65, 258)} <= pairs and {(l, l) for l in (3, 64, 65, 258)} <= pairs
    assert all(d + l <= dc.RING for d, l in pairs)               # the grid is the near path's
    # every match of the grid copies fresh random bytes: `dist` literals stand right in front of it
    for c in cs[:-1]:
        end = 300
        for pos, dist, length in c.stats.matches:
            assert pos - end == dist, (c, pos, dist)
            end = pos + length


def test_the_far_cases_reach_the_ring_edge_and_the_largest_distance(cat):
    cs = _group(cat, "ring edge and far matches")
    assert len(cs) == 16 and [c.n_members for c in cs] == [1] + [2] * 15
    for k, c in enumerate(cs):                                   # output shift k: k plain bytes in front of the member
        assert dc.split_members(c.data)[0][2] == (k if k else len(c.payload))
    st = cs[0].stats
    assert len(st.out) > dc.SEED_FAR >= 33000 and [t for t, _ in st.headers[:2]] == [0, 0]
    sums = {d + l for d, l in st.pairs}
    for length in (3, 64, 65, 258):
        for s in (4095, 4096, 4097, 4098):
            assert (s - length, length) in st.pairs
    assert {dc.RING, dc.FAR} <= sums
    for dist in (8192, 16384, 32767, 32768):
        assert {(dist, 3), (dist, 258)} <= st.pairs
    m = st.matches
    ph = m[st.marks["phases"]:st.marks["phases"] + 4]
    assert [(pos - dist) % 4 for pos, dist, _ in ph] == [0, 1, 2, 3] and all(dist + l > dc.RING for _, dist, l in ph)
    assert all(ph[i + 1][0] == ph[i][0] + ph[i][2] for i in range(3))          # consecutive
    a, b = m[st.marks["chain"]], m[st.marks["chain_end"]]
    assert a[1] + a[2] > dc.RING and b[1] + b[2] > dc.RING
    assert b[0] - b[1] == a[0] and b[2] == a[2]                                # B's source is A's output
    assert all(d + l <= dc.RING for _, d, l in m[st.marks["chain"] + 1:st.marks["chain_end"]])   # near matches between them
    tail = m[st.marks["chain_end"] + 1:]
    kinds = [d + l > dc.RING for _, d, l in tail]
    assert kinds.count(True) >= 20 and kinds.count(False) >= 20 and any(x != y for x, y in zip(kinds, kinds[1:]))


def test_the_header_forms_are_the_ones_named(cat):
    cs = {c.name: c for c in _group(cat, "dynamic-header forms")}

    def header(c):
        """HLIT, HDIST, HCLEN of the first dynamic block, read back from the stream."""
        stream = dc.split_members(c.data)[0][0]
        at = next(p for t, p in c.stats.headers if t == 2)
        v = int.from_bytes(stream, "little") >> (at + 3)
        return (v & 31) + 257, ((v >> 5) & 31) + 1, ((v >> 10) & 15) + 4

    assert header(cs["HDIST = 1 with length 0"])[1] == 1 and not cs["HDIST = 1 with length 0"].stats.pairs
    assert header(cs["a single 1-bit distance code, symbol 0"])[1] == 1 and cs["a single 1-bit distance code, symbol 0"].stats.used["dist"] == 1
    assert cs["a single 1-bit distance code, symbol 6"].stats.used["dist"] == 1
    assert header(cs["HLIT = 257"])[0] == 257
    assert header(cs["HLIT = 286, HDIST = 30"])[:2] == (286, 30)
    assert {(24577, 258), (24999, 257)} <= cs["HLIT = 286, HDIST = 30"].stats.pairs
    assert header(cs["HCLEN = 19"])[2] == 19 and 15 in cs["HCLEN = 19"].stats.cl_symbols
    assert header(cs["HCLEN = 5"])[2] == 5
    assert 16 in cs["repeat 16 across the literal/distance boundary"].stats.cl_symbols
    assert 18 in cs["repeat 18 across the literal/distance boundary"].stats.cl_symbols
    assert {16, 17, 18} <= cs["16 directly after 17 and 18"].stats.cl_symbols
    assert header(cs["distance codes declared and not used"])[1] == 30 and not cs["distance codes declared and not used"].stats.pairs
    assert cs["end-of-block code of length 1"].stats.used["eob"] == 1
    assert len(cs) == 12


def test_the_block_structure_cases_are_the_ones_named(cat):
    cs = {c.name: c for c in _group(cat, "block structure")}
    c = cs["300 dynamic blocks of two to five symbols"]
    assert c.stats.blocks == 300 and {t for t, _ in c.stats.headers} == {2} and 600 <= c.stats.n_symbols <= 1500
    assert [t for t, _ in cs["fixed, dynamic and stored alternating"].stats.headers] == [1, 2, 0] * 30
    for phase in range(8):                                       # every stored-phase case really enters at its phase
        h = cs["stored block entered at bit phase %d" % phase].stats.headers
        assert [t for t, _ in h] == [1, 0, 1] and h[1][1] % 8 == phase
    h = cs["zero-length stored blocks first, in the middle and last"].stats.headers
    assert [t for t, _ in h] == [0, 1, 0, 2, 0]
    assert cs["an empty fixed block as the only block"].payload == b"" and cs["an empty fixed block as the only block"].stats.blocks == 1
    assert len(cs["the largest stored block a member holds"].data) == dc.BGZF_MAX
    want = set(dc.header_positions())
    assert len(want) == 54
    for off in (256, 512, 768):
        for delta in range(-4, 5):
            assert 8 * off + delta in want and 8 * (off - 18) + delta in want
    got = {c.stats.headers[1][1] for n, c in cs.items() if n.startswith("block header at stream bit")}
    assert got == want
    assert cs["400 members of one byte"].n_members == 400 and len(cs["400 members of one byte"].payload) == 400
