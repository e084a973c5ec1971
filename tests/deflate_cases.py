"""A DEFLATE (RFC 1951) *encoder* for tests, and the catalogue of BGZF members built with it.

zlib's compressor emits what its match finder and its Huffman builder choose.  The format allows much more, and other writers
(libdeflate, htslib at other levels, third parties) use it: codes of up to 15 bits, matches at every distance up to 32 768 and every
overlap, dynamic headers in forms zlib never writes, any sequence of blocks.  The encoder here writes exactly the symbols, the code
lengths and the code-length-code sequence its caller names, and keeps the books on what it wrote (`Deflate.used`, `.pairs`,
`.matches`, `.max_token_bits`, `.headers`), so that tests/test_deflate_cases_host.py can show that a case reaches the path it is
named for.  tests/test_gpu_inflate_streams.py gives the members to csrc/vlr_inflate.hip.

Two lists: `catalogue().accepted` (zlib inflates each to `payload`, which is zlib's output, never the encoder's model) and
`catalogue().refused` (zlib raises, stops before the end, or the trailer disagrees; `reason` is the INFL_* code of
csrc/vlr_gpuio.h the kernel has to give, or a set of them where the bytes that follow the member decide).

Left out of both lists on purpose: sets of code lengths that zlib refuses as *incomplete* (fewer codes than the lengths allow,
other than a single distance code).  The kernel decodes them; see DESIGN.md 3e.

No dependency beyond zlib, struct and numpy; nothing here needs a GPU."""
import struct
import zlib

import numpy as np

# the reasons of csrc/vlr_gpuio.h
(INFL_OK, INFL_BAD_BLOCK_TYPE, INFL_BAD_STORED, INFL_BAD_CODE_LENGTHS, INFL_OVERSUBSCRIBED, INFL_BAD_SYMBOL, INFL_BAD_DISTANCE,
 INFL_OUTPUT_OVERRUN, INFL_INPUT_OVERRUN, INFL_SIZE_MISMATCH, INFL_CRC_MISMATCH) = range(11)

BGZF_MAX = 65536                      # BSIZE and ISIZE of a member (SAM spec 4.1)
RING, FAR = 4096, 4097                # csrc/vlr_inflate.hip: a match with dist + len > RING reads the flushed output

# ---- RFC 1951 3.2.5: length and distance symbols
LEN_BASE, LEN_EXTRA = [], []
for _k in range(28):
    _xb = 0 if _k < 8 else (_k >> 2) - 1
    LEN_BASE.append(3 + _k if _k < 8 else 3 + ((4 + (_k & 3)) << _xb))
    LEN_EXTRA.append(_xb)
LEN_BASE.append(258); LEN_EXTRA.append(0)
DIST_BASE, DIST_EXTRA = [], []
for _s in range(30):
    _xb = 0 if _s < 4 else (_s >> 1) - 1
    DIST_BASE.append(1 + _s if _s < 4 else 1 + ((2 + (_s & 1)) << _xb))
    DIST_EXTRA.append(_xb)
assert LEN_BASE[:9] == [3, 4, 5, 6, 7, 8, 9, 10, 11] and LEN_BASE[24:] == [131, 163, 195, 227, 258] and LEN_EXTRA[24:28] == [5] * 4
assert DIST_BASE[:6] == [1, 2, 3, 4, 5, 7] and DIST_BASE[28:] == [16385, 24577] and DIST_EXTRA[29] == 13

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]   # RFC 1951 3.2.7
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                            # RFC 1951 3.2.6
FIXED_DIST = [5] * 32
DEFAULT_CL = [4] * 13 + [5] * 6      # a complete code-length code with every symbol in it (13/16 + 6/32 = 1): HCLEN = 19


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258."""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


_LEN_SYM = [None] * 3 + [length_symbol(n) for n in range(3, 259)]
_DIST_SYM = {}


def _dist_sym(d):
    r = _DIST_SYM.get(d)
    if r is None:
        r = _DIST_SYM[d] = distance_symbol(d)
    return r


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """Canonical Huffman codes (RFC 1951 3.2.2) of a list of code lengths, already bit-reversed for the LSB-first writer.
    An over-subscribed set still gets codes (masked to their length): the refused cases need its header, not its symbols."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(0)
        else:
            out.append(_rev(nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
    return out


def kraft(lens):
    """Sum of 2^-l in units of 2^-15: 32768 = complete, more = over-subscribed."""
    return sum(1 << (15 - l) for l in lens if l)


def flat_lengths(k):
    """Code lengths of a complete code of k >= 2 symbols, as even as possible."""
    assert k >= 2
    m = k.bit_length() - 1
    short = (2 << m) - k
    return [m] * short + [m + 1] * (k - short) if short < k else [m] * k


def ladder(n):
    """1, 2, ..., n-1, n, n: a complete set whose longest code has n bits."""
    return list(range(1, n)) + [n, n]


def rle(lens):
    """A code-length-code sequence for `lens`: (symbol,) for a plain length, (16 | 17 | 18, count) for a repeat."""
    seq, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                c = min(run, 138); seq.append((18, c)); run -= c
            if run >= 3:
                seq.append((17, run)); run = 0
            seq += [(0,)] * run
        else:
            seq.append((v,)); run -= 1
            while run >= 3:
                c = min(run, 6); seq.append((16, c)); run -= c
            seq += [(v,)] * run
        i = j
    return seq


def expand(seq):
    """What a code-length-code sequence says (16 after 17/18 repeats zero, like zlib and the kernel)."""
    out = []
    for s in seq:
        if s[0] < 16:
            out.append(s[0])
        elif s[0] == 16:
            out += [out[-1]] * s[1]
        else:
            out += [0] * s[1]
    return out


class BitWriter:
    """LSB-first bit string (RFC 1951 3.1.1)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 32:
            self.buf += (self.acc & 0xffffffff).to_bytes(4, "little")
            self.acc >>= 32
            self.n -= 32

    def pos(self):
        return len(self.buf) * 8 + self.n

    def align(self):
        if self.n & 7:
            self.bits(0, 8 - (self.n & 7))

    def raw(self, data):
        assert self.n & 7 == 0
        while self.n:
            self.buf.append(self.acc & 255); self.acc >>= 8; self.n -= 8
        self.buf += data

    def getvalue(self):
        nb = (self.n + 7) >> 3
        return bytes(self.buf) + (self.acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")


class Deflate:
    """One raw DEFLATE stream under construction.  Symbols of a Huffman block are given as
         int 0..255            a literal
         (length, distance)    a match
         ("L", symbol)         a bare literal/length symbol, nothing behind it (286, 287 of the fixed code)
         ("M", length symbol, extra value, distance symbol, extra value)   a match by its raw symbols (distance symbols 30, 31)
    `out` is the encoder's model of the inflated bytes (raw symbols are not modelled); the tests expect zlib's bytes, and the
    host test holds the model against them."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.used = {}            # class of symbol -> longest code it was written with: literal, length, length5, eob, dist, dist13
        self.pairs = set()        # (distance, length)
        self.matches = []         # (output offset, distance, length)
        self.max_token_bits = 0
        self.headers = []         # (block type, bit position of the header in the stream)
        self.n_symbols = 0

    @property
    def blocks(self):
        return len(self.headers)

    def _use(self, cls, n):
        if self.used.get(cls, 0) < n:
            self.used[cls] = n

    def _header(self, final, btype):
        self.headers.append((btype, self.w.pos()))
        self.w.bits(int(bool(final)) | (btype << 1), 3)

    def stored(self, data, final=False, length=None, nlen=None):
        """A stored block; `length` and `nlen` override the LEN and NLEN fields (refused cases)."""
        self._header(final, 0)
        self.w.align()
        ln = len(data) if length is None else length
        self.w.bits(ln, 16)
        self.w.bits((ln ^ 0xffff) if nlen is None else nlen, 16)
        self.w.raw(data)
        self.out += data
        return self

    def bad_type(self, final=True):
        self._header(final, 3)
        return self

    def _symbols(self, symbols, lcode, llen, dcode, dlen, eob):
        w, out = self.w, self.out
        bits = w.bits
        for s in symbols:
            if type(s) is int:
                n = llen[s]
                assert n, "literal %d has no code" % s
                bits(lcode[s], n)
                out.append(s)
                if n > self.used.get("literal", 0):
                    self.used["literal"] = n
                tok = n
            elif type(s[0]) is int:
                length, dist = s
                ls, lxb, lxv = _LEN_SYM[length]
                ds, dxb, dxv = _dist_sym(dist)
                ln, dn = llen[ls], dlen[ds]
                assert ln and dn, "match (%d, %d) has no code" % (length, dist)
                bits(lcode[ls], ln); bits(lxv, lxb); bits(dcode[ds], dn); bits(dxv, dxb)
                assert dist <= len(out), "distance %d at offset %d" % (dist, len(out))
                self.matches.append((len(out), dist, length))
                self.pairs.add((dist, length))
                start = len(out) - dist
                if dist >= length:
                    out += out[start:start + length]
                else:
                    out += (bytes(out[start:]) * (length // dist + 1))[:length]
                self._use("length", ln); self._use("dist", dn)
                if lxb == 5:
                    self._use("length5", ln)
                if dxb == 13:
                    self._use("dist13", dn)
                tok = ln + lxb + dn + dxb
            elif s[0] == "L":
                bits(lcode[s[1]], llen[s[1]])
                tok = llen[s[1]]
            else:
                _, ls, lxv, ds, dxv = s
                bits(lcode[ls], llen[ls]); bits(lxv, LEN_EXTRA[ls - 257]); bits(dcode[ds], dlen[ds]); bits(dxv, DIST_EXTRA[ds] if ds < 30 else 0)
                tok = 0
            if tok > self.max_token_bits:
                self.max_token_bits = tok
        self.n_symbols += len(symbols)
        if eob:
            bits(lcode[256], llen[256])
            self._use("eob", llen[256])

    def fixed(self, symbols=(), final=False, eob=True):
        self._header(final, 1)
        self._symbols(symbols, _FIXED_LCODE, FIXED_LIT, _FIXED_DCODE, FIXED_DIST, eob)
        return self

    def dynamic(self, symbols, lit_lens, dist_lens, final=False, cl_seq=None, cl_lens=None, hclen=None, eob=True):
        """A dynamic block with HLIT = len(lit_lens), HDIST = len(dist_lens), the code-length code `cl_lens` (by symbol, first `hclen`
        of CL_ORDER written) and the code-length-code sequence `cl_seq` (default: rle of the lengths), all written as given."""
        assert 257 <= len(lit_lens) <= 288 and 1 <= len(dist_lens) <= 32
        self._header(final, 2)
        w = self.w
        cl_lens = list(DEFAULT_CL if cl_lens is None else cl_lens)
        if hclen is None:
            hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
        assert all(cl_lens[CL_ORDER[i]] == 0 for i in range(hclen, 19))
        cl_seq = rle(list(lit_lens) + list(dist_lens)) if cl_seq is None else cl_seq
        w.bits(len(lit_lens) - 257, 5); w.bits(len(dist_lens) - 1, 5); w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cc = canonical(cl_lens)
        for s in cl_seq:
            assert cl_lens[s[0]], "code-length symbol %d has no code" % s[0]
            w.bits(cc[s[0]], cl_lens[s[0]])
            if s[0] == 16:
                assert 3 <= s[1] <= 6; w.bits(s[1] - 3, 2)
            elif s[0] == 17:
                assert 3 <= s[1] <= 10; w.bits(s[1] - 3, 3)
            elif s[0] == 18:
                assert 11 <= s[1] <= 138; w.bits(s[1] - 11, 7)
        self.cl_symbols = getattr(self, "cl_symbols", set()) | {s[0] for s in cl_seq}
        self._symbols(symbols, canonical(lit_lens), lit_lens, canonical(dist_lens), dist_lens, eob)
        return self

    def getvalue(self):
        return self.w.getvalue()


_FIXED_LCODE, _FIXED_DCODE = canonical(FIXED_LIT), canonical(FIXED_DIST)


def member(deflate_bytes, payload, isize=None, crc=None):
    """One BGZF member (SAM spec 4.1) around a raw DEFLATE stream, with the CRC32 and ISIZE of `payload` (or the ones given)."""
    isize = len(payload) if isize is None else isize
    crc = zlib.crc32(payload) if crc is None else crc
    bsize = 18 + len(deflate_bytes) + 8
    assert bsize <= BGZF_MAX, bsize
    assert isize <= BGZF_MAX, isize
    head = b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + deflate_bytes + struct.pack("<II", crc, isize)


def split_members(data):
    """(deflate bytes, crc, isize) of every BGZF member of a byte string."""
    out, off = [], 0
    while off < len(data):
        assert data[off:off + 4] == b"\x1f\x8b\x08\x04" and data[off + 12:off + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", data, off + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", data, off + bsize - 8)
        out.append((data[off + 18:off + bsize - 8], crc, isize))
        off += bsize
    assert off == len(data)
    return out


def zlib_inflate(deflate_bytes):
    """(bytes, reached the end of the stream, unused input) from zlib's raw inflate; raises zlib.error."""
    d = zlib.decompressobj(-15)
    out = d.decompress(deflate_bytes)
    return out, d.eof, d.unused_data


class Case:
    """`data`: one BGZF member (`n_members` of them for the stream cases).  Accepted: `payload` is what zlib inflates the members to
    (None: zlib refused — the host test says so), `model` the encoder's own idea of it.  Refused: `reason`, an INFL_* code or a
    frozenset of them."""

    def __init__(self, group, name, data, stats=None, payload=None, model=None, reason=None, n_members=1):
        self.group, self.name, self.data, self.stats = group, name, data, stats
        self.payload, self.model, self.reason, self.n_members = payload, model, reason, n_members

    def __repr__(self):
        return "%s / %s" % (self.group, self.name)


def _zlib_payload(deflate_bytes):
    try:
        out, eof, rest = zlib_inflate(deflate_bytes)
    except zlib.error:
        return None
    return out if eof and not rest else None


def _accepted(group, name, d):
    """A finished Deflate as a case: the member carries the CRC and ISIZE of what zlib makes of the stream."""
    stream = d.getvalue()
    pl = _zlib_payload(stream)
    return Case(group, name, member(stream, pl if pl is not None else bytes(d.out)), stats=d, payload=pl, model=bytes(d.out))


def _plain_member(payload):
    """`payload` in one final stored block."""
    return member(Deflate().stored(payload, final=True).getvalue(), payload)


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ======================================================================================================= accepted: long codes
_LIT_POOL = [257, 0x41, 281, 0x7a, 258, 0x00, 284, 0xff, 285, 0x9c, 265, 0x20, 273, 0x0a, 270, 0x80, 262, 0x33, 282, 0x55]
_DIST_POOL = [0, 16, 23, 4, 28, 10, 22, 29, 24, 1, 26, 8, 20, 2, 25, 12, 27, 14, 18, 6]
SEED_FAR = 33001   # bytes of stored blocks in front of the members whose matches reach back up to 32 768


def _ladder_alphabet(n, long_syms, pool, last):
    """n + 1 symbols with the lengths 1 .. n-1, n, n: `long_syms` get the two longest codes, `last` (if not among them) the
    length n - 1."""
    short = [s for s in pool if s not in long_syms and s != last][:n - 1 - (0 if last in long_syms or last is None else 1)]
    if last is not None and last not in long_syms:
        short.append(last)
    assert len(short) == n - 1 and len(long_syms) == 2
    return dict(list(zip(short, range(1, n))) + [(long_syms[0], n), (long_syms[1], n)])


def long_code_case(name, seed, lit_n, dist_n, lit_long, dist_long):
    """Stored random bytes, then dynamic blocks over a literal/length ladder of longest code `lit_n` and a distance ladder of
    longest code `dist_n`, every symbol of both drawn equally often, so that the long ones start at every bit offset."""
    rng = np.random.default_rng(seed)
    la = _ladder_alphabet(lit_n, lit_long, _LIT_POOL, 256)
    da = _ladder_alphabet(dist_n, dist_long, _DIST_POOL, None)
    lit_lens = [0] * (max(la) + 1)
    for s, l in la.items():
        lit_lens[s] = l
    lit_lens += [0] * (257 - len(lit_lens))
    dist_lens = [0] * (max(da) + 1)
    for s, l in da.items():
        dist_lens[s] = l
    assert kraft(lit_lens) == 32768 and kraft(dist_lens) == 32768
    d = Deflate()
    d.stored(_rand(rng, 20001)).stored(_rand(rng, SEED_FAR - 20001))
    lsyms, dsyms = sorted(la), sorted(da)
    size, blocks, cur = SEED_FAR, [], []
    while size < 64800 and sum(map(len, blocks)) + len(cur) < 2600:
        s = lsyms[int(rng.integers(len(lsyms)))]
        if s == 256:
            blocks.append(cur); cur = []
        elif s < 256:
            cur.append(s); size += 1
        else:
            k = s - 257
            length = LEN_BASE[k] + int(rng.integers(1 << LEN_EXTRA[k]))
            if k == 27:
                length = min(length, 257)   # (258 has its own symbol)
            ds = dsyms[int(rng.integers(len(dsyms)))]
            dist = DIST_BASE[ds] + int(rng.integers(1 << DIST_EXTRA[ds]))
            cur.append((length, min(dist, size))); size += length
    blocks.append(cur)
    for i, b in enumerate(blocks):
        d.dynamic(b, lit_lens, dist_lens, final=i == len(blocks) - 1)
    return _accepted("long codes", name, d)


def _long_cases():
    return [
        long_code_case("15-bit literals, distance ladder to 15", 101, 15, 15, (0x7a, 0xff), (4, 10)),
        long_code_case("15-bit length symbols with 5 extra bits, 15-bit distance symbols with 13: 48-bit tokens", 102, 15, 15, (281, 284), (28, 29)),
        long_code_case("15-bit end of block", 103, 15, 15, (256, 0x20), (29, 1)),
        long_code_case("longest literal/length code 10 (the table index), distance 9", 104, 10, 9, (0x41, 281), (28, 0)),
        long_code_case("longest literal/length code 11, distance 10", 105, 11, 10, (284, 0x00), (29, 16)),
    ]


# ======================================================================================================= accepted: overlap grid
def grid_lengths(dist):
    want = {3, 4, 5, 63, 64, 65, 66, 127, 128, 129, dist - 1, dist, dist + 1, 2 * dist - 1, 2 * dist, 2 * dist + 1, 257, 258}
    return sorted({min(258, max(3, x)) for x in want})


def grid_pairs():
    return [(dist, length) for dist in range(1, 259) for length in grid_lengths(dist)]


def ring_size_pairs():
    return [(dist, length) for length in (3, 64, 65, 258) for dist in (length, length + 1, RING - 1 - length, RING - length)]


def _grid_cases():
    """Every (distance, length) of the grid behind `distance` fresh random literals: the bytes a match copies are never periodic."""
    rng = np.random.default_rng(201)
    cases, d, size, block = [], None, 0, []

    def close():
        nonlocal d, block
        if d is not None:
            d.fixed(block, final=True)
            cases.append(_accepted("overlap grid", "member %d" % (len(cases) + 1), d))
        d, block = None, []

    for dist, length in grid_pairs():
        if d is not None and size + dist + length > 65000:
            close()
        if d is None:
            d = Deflate().stored(_rand(rng, 300)); size = 300
        block += list(_rand(rng, dist)); block.append((length, dist)); size += dist + length
        if len(block) > 4000:
            d.fixed(block); block = []
    close()
    d = Deflate().stored(_rand(rng, 4400))
    block = []
    for dist, length in ring_size_pairs():
        block += list(_rand(rng, 7)); block.append((length, dist))
    d.fixed(block, final=True)
    cases.append(_accepted("overlap grid", "distances at the match length and at the ring size", d))
    return cases


# ======================================================================================================= accepted: ring edge, far matches
def far_member():
    """33 001 stored random bytes, then Huffman-coded matches around dist + len = 4096 | 4097, at the largest distances, at the
    four byte phases of the far copy's word load, a far match that reads what the far match before it wrote, and far matches
    between literals and near matches."""
    rng = np.random.default_rng(301)
    d = Deflate()
    d.stored(_rand(rng, 20001)).stored(_rand(rng, SEED_FAR - 20001))
    marks = {}
    b = []
    for length in (3, 64, 65, 258):
        for s in (RING - 1, RING, RING + 1, RING + 2):
            b += list(_rand(rng, 3)); b.append((length, s - length))
    d.fixed(b)
    b = []
    for dist in (8192, 16384, 32767, 32768):
        for length in (3, 258):
            b += list(_rand(rng, 2)); b.append((length, dist))
    d.fixed(b)
    # four far matches in a row whose sources start at byte offsets 0, 1, 2, 3 mod 4 of the member
    pos, b = len(d.out), []
    marks["phases"] = len(d.matches)
    for i in range(4):
        dist = 6000 + ((pos - i - 6000) % 4)
        assert (pos - dist) % 4 == i
        b.append((5, dist)); pos += 5
    d.fixed(b)
    # far match A; 4 080 bytes of literals and near matches (four flushes); far match B whose source is exactly A's output
    marks["chain"] = len(d.matches)
    b, pos_a = [(258, 9000)], len(d.out)
    pos = pos_a + 258
    for j in range(17):
        b += list(_rand(rng, 40)); b.append((200, 300 + 17 * j)); pos += 240
    b.append((258, pos - pos_a))
    marks["chain_end"] = marks["chain"] + 18
    d.fixed(b)
    # far matches between literals and near matches, in a dynamic block (flat code over what it uses)
    b = []
    for j in range(12):
        b += list(_rand(rng, 100)); b.append((50, 77)); b.append((37, 5000 + 311 * j)); b.append((258, RING - 258)); b.append((11, 20000 + j))
    ll = [0] * 286
    used = sorted({s for s in b if type(s) is int} | {256} | {_LEN_SYM[s[0]][0] for s in b if type(s) is not int})
    for s, l in zip(used, flat_lengths(len(used))):
        ll[s] = l
    du = sorted({_dist_sym(s[1])[0] for s in b if type(s) is not int})
    dl = [0] * 30
    for s, l in zip(du, flat_lengths(len(du))):
        dl[s] = l
    d.dynamic(b, ll, dl, final=True)
    d.marks = marks
    return d


def _far_cases():
    d = far_member()
    first = _accepted("ring edge and far matches", "output shift 0", d)
    cases = [first]
    rng = np.random.default_rng(302)
    for k in range(1, 16):
        lead = _rand(rng, k)
        pl = None if first.payload is None else lead + first.payload
        cases.append(Case("ring edge and far matches", "output shift %d" % k, _plain_member(lead) + first.data, stats=d, payload=pl, model=lead + first.model, n_members=2))
    return cases


# ======================================================================================================= accepted: dynamic-header forms
def _lens_for(symbols, lengths, size):
    out = [0] * size
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


def _header_cases():
    rng = np.random.default_rng(401)
    G, cases = "dynamic-header forms", []

    def add(name, d):
        cases.append(_accepted(G, name, d))

    abcd = [0x61, 0x62, 0x63, 0x64]
    text = [abcd[i] for i in rng.integers(0, 4, 500)]
    # HDIST = 1 with length 0: no distance code at all
    add("HDIST = 1 with length 0", Deflate().dynamic(text, _lens_for(abcd + [256], [2, 2, 2, 3, 3], 257), [0], final=True))
    # a single distance code of one bit (zlib accepts this one incomplete set)
    ll = _lens_for(abcd + [256, 257, 258, 259, 260], flat_lengths(9), 261)
    sy = text[:40] + [(3 + i % 4, 1) for i in range(60)] + text[40:90] + [(6, 1)] * 5
    add("a single 1-bit distance code, symbol 0", Deflate().dynamic(sy, ll, [1], final=True))
    sy = text[:40] + [(3 + i % 4, 9 + i % 4) for i in range(60)]
    add("a single 1-bit distance code, symbol 6", Deflate().dynamic(sy, ll, [0] * 6 + [1], final=True))
    # HLIT = 257: literals and end of block, no length symbol
    add("HLIT = 257", Deflate().dynamic(list(_rand(rng, 700)), [8] * 255 + [9, 9], [0], final=True))
    # HLIT = 286 and HDIST = 30, symbols 285 and 29 used
    d = Deflate().stored(_rand(rng, 25000))
    sy = []
    for k in range(29):
        ds = (7 * k + 3) % 30
        sy += list(_rand(rng, 5)); sy.append((LEN_BASE[k] + (1 << LEN_EXTRA[k]) // 2 if k < 28 else 258, min(25000, DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) // 3)))
    sy += [(258, 24577), (257, 24999), (3, 1), (258, 1)]
    add("HLIT = 286, HDIST = 30", d.dynamic(sy, flat_lengths(286), flat_lengths(30), final=True))
    # HCLEN = 19: the code-length code has a code for 15, the last of its order; nothing repeated
    la = _ladder_alphabet(15, (0x7a, 258), _LIT_POOL, 256)
    ll = _lens_for(list(la), list(la.values()), 286)
    dl = ladder(15) + [0] * 14
    sy = [s for s in la if s < 256] * 20 + [(4, 3), (3, 100)] * 10
    add("HCLEN = 19", Deflate().dynamic(sy, ll, dl, cl_seq=[(l,) for l in ll + dl], final=True))
    # HCLEN = 5, the least a valid block can have: 16, 17, 18 without a code, then 0 and 8.  (HCLEN = 4 can only say "all lengths
    # zero": there is no code for 256 then; it is among the refused cases.)
    ll = [8] * 255 + [0, 8]
    cl = [0] * 19
    cl[0] = cl[8] = 1
    add("HCLEN = 5", Deflate().dynamic(list(_rand(rng, 300).replace(b"\xff", b"\x00")), ll, [0], cl_lens=cl, cl_seq=[(l,) for l in ll + [0]], hclen=5, final=True))
    # repeat code 16 from the literal/length lengths into the distance lengths
    ll = _lens_for(abcd + [256, 258, 259], [4, 4, 4, 4, 2, 2, 2], 260)
    dl = [2, 2, 2, 2]
    seq = rle(ll[:259]) + [(16, 5)]
    assert expand(seq) == ll + dl and seq[-2] == (2,)
    sy = text[:50] + [(4, 1), (5, 2), (4, 3), (5, 4)] * 6
    add("repeat 16 across the literal/distance boundary", Deflate().dynamic(sy, ll, dl, cl_seq=seq, final=True))
    # repeat code 18 from the literal/length lengths into the distance lengths
    ll = _lens_for(abcd + [256, 257, 258, 259, 260, 261], flat_lengths(10), 286)
    dl = [0] * 5 + [1, 1]
    seq = rle(ll[:262]) + [(18, 29), (1,), (1,)]
    assert expand(seq) == ll + dl
    sy = text[:50] + [(3 + i % 5, 7 + i % 6) for i in range(40)]
    add("repeat 18 across the literal/distance boundary", Deflate().dynamic(sy, ll, dl, cl_seq=seq, final=True))
    # 16 directly after 17 and after 18: repeats the zero
    ll = [0] * 286
    for s, l in zip([0x61, 0x70, 0x90, 256, 257], [2, 2, 2, 3, 3]):
        ll[s] = l
    seq = [(18, 97), (2,), (17, 3), (16, 6), (16, 5), (2,), (18, 20), (16, 6), (16, 5), (2,), (18, 100), (16, 6), (16, 5), (3,), (3,), (18, 28)] + [(2,), (2,), (2,), (2,)]
    dl = [2, 2, 2, 2]
    assert expand(seq) == ll + dl, [i for i, (a, b_) in enumerate(zip(expand(seq), ll + dl)) if a != b_][:4]
    sy = [[0x61, 0x70, 0x90][i] for i in rng.integers(0, 3, 200)] + [(3, 1), (3, 4)] * 5
    add("16 directly after 17 and 18", Deflate().dynamic(sy, ll, dl, cl_seq=seq, final=True))
    # distance codes declared, none used
    add("distance codes declared and not used", Deflate().dynamic(text, _lens_for(abcd + [256], [2, 2, 2, 3, 3], 257), flat_lengths(30), final=True))
    # end of block with a code of one bit
    two = [[0x78, 0x79][i] for i in rng.integers(0, 2, 300)]
    d = Deflate()
    for i in range(5):
        d.dynamic(two[60 * i:60 * i + 60], _lens_for([0x78, 0x79, 256], [2, 2, 1], 257), [0], final=i == 4)
    add("end-of-block code of length 1", d)
    return cases


# ======================================================================================================= accepted: block structure
def _small_dynamic(d, rng, i, final=False):
    """A dynamic block of two to five symbols over an alphabet of its own."""
    a, b_ = int(rng.integers(0, 256)), int(rng.integers(0, 255))
    b_ += b_ >= a
    ll = _lens_for([a, b_, 256, 257, 260], [2, 2, 2, 3, 3], 261)
    sy = [a, b_] + [(3, 1), (6, 2), a][:i % 4]
    return d.dynamic(sy, ll, [1, 1], final=final)


def header_positions():
    """Bit positions a block header is put at: within +-4 bits of the compressed-byte offsets 256, 512, 768, counted from the start
    of the DEFLATE stream and from the start of the member (18 bytes of header in front of it)."""
    return [8 * (off - lead) + delta for off in (256, 512, 768) for lead in (0, 18) for delta in range(-4, 5)]


def _block_cases():
    rng = np.random.default_rng(501)
    G, cases = "block structure", []

    def add(name, d):
        cases.append(_accepted(G, name, d))

    d = Deflate()
    for i in range(300):
        _small_dynamic(d, rng, i, final=i == 299)
    add("300 dynamic blocks of two to five symbols", d)
    d = Deflate()
    for i in range(30):
        d.fixed(list(_rand(rng, 3 + i)) + [(3 + i, 1 + i)])
        _small_dynamic(d, rng, i)
        d.stored(_rand(rng, 1 + 7 * i), final=i == 29)
    add("fixed, dynamic and stored alternating", d)
    # a stored block entered at each bit phase: the fixed block in front of it takes 3 + 8 a + 9 b + 7 bits
    for phase in range(8):
        b9 = (phase - 2) % 8
        d = Deflate().fixed([int(x) % 144 for x in _rand(rng, 5)] + [144 + int(x) % 112 for x in _rand(rng, b9)])
        d.stored(_rand(rng, 100)).fixed([1, 2, 3], final=True)
        add("stored block entered at bit phase %d" % phase, d)
    d = Deflate().stored(b"").fixed(list(_rand(rng, 20))).stored(b"")
    _small_dynamic(d, rng, 3).stored(b"", final=True)
    add("zero-length stored blocks first, in the middle and last", d)
    add("an empty fixed block as the only block", Deflate().fixed(final=True))
    add("an empty fixed block as the last block", Deflate().fixed(list(_rand(rng, 30))).fixed(final=True))
    d = Deflate().stored(_rand(rng, 10)).fixed().fixed(list(_rand(rng, 10))).fixed()
    add("empty fixed blocks between others", _small_dynamic(d, rng, 2, final=True))
    add("the largest stored block a member holds", Deflate().stored(_rand(rng, BGZF_MAX - 18 - 8 - 5), final=True))
    for T in header_positions():
        b9 = next(b for b in range(8) if (T - 10 - 9 * b) % 8 == 0)
        a8 = (T - 10 - 9 * b9) // 8
        sy = [int(x) % 144 for x in _rand(rng, a8)]
        for j in range(b9):
            sy.insert(int(rng.integers(len(sy))), 144 + int(rng.integers(112)))
        d = Deflate().fixed(sy)
        assert d.w.pos() == T
        _small_dynamic(d, rng, 3)
        d.stored(_rand(rng, 9))
        _small_dynamic(d, rng, 1, final=True)
        add("block header at stream bit %d" % T, d)
    data, pl = [], []
    for i in range(400):
        x = _rand(rng, 1)
        dd = Deflate().stored(x, final=True) if i % 2 else Deflate().fixed([x[0]], final=True)
        data.append(member(dd.getvalue(), x)); pl.append(x)
    zl = [_zlib_payload(s) for m in data for s, _, _ in split_members(m)]
    cases.append(Case(G, "400 members of one byte", b"".join(data), payload=None if None in zl else b"".join(zl), model=b"".join(pl), n_members=400))
    return cases


# ======================================================================================================= refused
def _refused_cases():
    rng = np.random.default_rng(601)
    cases = []

    def add(group, name, d, reason, isize, payload=None, tail=8, crc=None):
        """`tail` zero bytes behind the last written bit stay inside the member, so that a decoder which reads a few bits past
        the error still reads this member's bytes.  ISIZE leaves room: a refusal is for the named reason, not for the size."""
        stream = d.getvalue() + bytes(tail)
        cases.append(Case(group, name, member(stream, payload if payload is not None else bytes(isize), isize=isize, crc=crc), stats=d, reason=reason))

    abcd = [0x61, 0x62, 0x63, 0x64]
    ok_lit = _lens_for(abcd + [256, 257], [2, 2, 2, 3, 4, 4], 258)
    G = "code lengths"
    add(G, "over-subscribed literal/length set", Deflate().dynamic([], _lens_for(abcd + [256, 257], [2, 2, 2, 2, 3, 3], 258), [1, 1], final=True, eob=False), INFL_OVERSUBSCRIBED, 64)
    add(G, "over-subscribed distance set", Deflate().dynamic([], ok_lit, [1, 1, 1], final=True, eob=False), INFL_OVERSUBSCRIBED, 64)
    cl = [0] * 19
    cl[0], cl[2], cl[3], cl[4] = 1, 2, 2, 2
    add(G, "over-subscribed code-length set", Deflate().dynamic([], ok_lit, [1, 1], cl_lens=cl, cl_seq=[], final=True, eob=False), INFL_OVERSUBSCRIBED, 64)
    add(G, "repeat 16 as the first length", Deflate().dynamic([], ok_lit, [1, 1], cl_seq=[(16, 3)] + rle(ok_lit[3:] + [1, 1]), final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    add(G, "repeat 18 past HLIT + HDIST", Deflate().dynamic([], ok_lit + [0] * 12, [1, 1], cl_seq=rle(ok_lit) + [(18, 15)], final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    add(G, "repeat 16 past HLIT + HDIST", Deflate().dynamic([], ok_lit, [1, 1], cl_seq=rle(ok_lit + [1]) + [(16, 3)], final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    add(G, "no code for 256", Deflate().dynamic([], _lens_for(abcd + [257, 258], [2, 2, 2, 3, 4, 4], 259), [1, 1], final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    cl = [0] * 19
    cl[0] = cl[18] = 1
    add(G, "HCLEN = 4: every length zero, no code for 256", Deflate().dynamic([], [0] * 257, [0], cl_lens=cl, hclen=4, final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    add(G, "HLIT field 30 (287 codes)", Deflate().dynamic([], flat_lengths(287), [1, 1], final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    add(G, "HLIT field 31 (288 codes)", Deflate().dynamic([], flat_lengths(288), [1, 1], final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    add(G, "HDIST field 30 (31 codes)", Deflate().dynamic([], ok_lit, flat_lengths(31), final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    add(G, "HDIST field 31 (32 codes)", Deflate().dynamic([], ok_lit, flat_lengths(32), final=True, eob=False), INFL_BAD_CODE_LENGTHS, 64)
    G = "symbols and blocks"
    add(G, "block type 3", Deflate().fixed(abcd).bad_type(), INFL_BAD_BLOCK_TYPE, 64)
    for s in (286, 287):
        add(G, "symbol %d in a fixed block" % s, Deflate().fixed(abcd * 5 + [("L", s)], final=True), INFL_BAD_SYMBOL, 64)
    for s in (30, 31):
        add(G, "distance symbol %d in a fixed block" % s, Deflate().fixed(abcd * 5 + [("M", 257, 0, s, 0)], final=True), INFL_BAD_DISTANCE, 64)
    ll = _lens_for(abcd + [256, 257, 258, 259, 260], flat_lengths(9), 261)
    d = Deflate().dynamic(abcd * 5 + [(3, 1)], ll, [1], eob=False, final=True)
    d.w.bits(canonical(ll)[257], ll[257]); d.w.bits(1, 1)         # length 3, then the distance code '1' that no symbol has
    d.w.bits(canonical(ll)[256], ll[256])
    add(G, "the unused code of a single-code distance set", d, INFL_BAD_DISTANCE, 64)
    G = "distances and output"
    add(G, "distance 1 at position 0", Deflate().fixed([("M", 257, 0, 0, 0)] + abcd, final=True), INFL_BAD_DISTANCE, 64)
    d = Deflate().fixed(list(_rand(rng, 100)), eob=False, final=True)
    ds, dxb, dxv = distance_symbol(101)
    d.w.bits(_FIXED_LCODE[260], 7); d.w.bits(_FIXED_DCODE[ds], 5); d.w.bits(dxv, dxb); d.w.bits(0, 7)
    add(G, "distance 101 at position 100", d, INFL_BAD_DISTANCE, 200)
    d = Deflate().stored(_rand(rng, 5000))
    d._header(True, 1)
    ds, dxb, dxv = distance_symbol(32768)
    d.w.bits(_FIXED_LCODE[285], 8); d.w.bits(_FIXED_DCODE[ds], 5); d.w.bits(dxv, dxb); d.w.bits(0, 7)
    add(G, "distance 32 768 at position 5000 (a far match)", d, INFL_BAD_DISTANCE, 5000 + 258)
    d = Deflate().stored(_rand(rng, 2000)).fixed(list(_rand(rng, 50)) + [(20, 1000)], final=True)
    add(G, "a match that runs past ISIZE by one byte", d, INFL_OUTPUT_OVERRUN, len(d.out) - 1, payload=bytes(d.out[:-1]), tail=0)
    G = "sizes"
    d = Deflate().stored(_rand(rng, 2000)).fixed(list(_rand(rng, 50)) + [(20, 1000)], final=True)
    add(G, "output one byte short of ISIZE", d, INFL_SIZE_MISMATCH, len(d.out) + 1, payload=bytes(d.out) + b"\0", tail=0)
    # no final block: what the decoder meets behind the last block is the member's trailer.  The last literal is chosen so
    # that the CRC32's low three bits read as "not final, block type 3" there — one reason, whatever follows the member.
    # (3 + 14 x 8 + 6 x 9 + 7 bits: the block ends on a byte boundary, no padding bit is read as a header)
    for x in range(144, 256):
        d = Deflate().fixed(list(b"no final block") + [200, 201, 202, 203, 204, x])
        if zlib.crc32(bytes(d.out)) & 7 == 6:
            break
    assert d.w.pos() % 8 == 0 and zlib.crc32(bytes(d.out)) & 7 == 6
    add(G, "no final block: the input ends, the trailer reads as block type 3", d, INFL_BAD_BLOCK_TYPE, len(d.out), payload=bytes(d.out), tail=0)
    # cut in the middle of a block: the decoder goes on through the trailer and what follows the member, as fixed-code symbols
    d = Deflate().fixed([int(x) % 144 for x in _rand(rng, 6000)], final=True)
    stream = d.getvalue()[:3000]
    cases.append(Case(G, "a block cut in the middle: the input ends", member(stream, bytes(d.out)), stats=d,
                      reason=frozenset([INFL_BAD_SYMBOL, INFL_BAD_DISTANCE, INFL_OUTPUT_OVERRUN, INFL_INPUT_OVERRUN])))
    x = _rand(rng, 100)
    add(G, "stored block with a wrong NLEN", Deflate().stored(x, final=True, nlen=(100 ^ 0xffff) ^ 0x0100), INFL_BAD_STORED, 100, payload=x, tail=0)
    add(G, "stored block longer than the remaining input", Deflate().stored(x, final=True, length=120), INFL_INPUT_OVERRUN, 120, tail=0)
    return cases


class Catalogue:
    def __init__(self):
        self.accepted = _long_cases() + _grid_cases() + _far_cases() + _header_cases() + _block_cases()
        self.refused = _refused_cases()
        self.groups = []
        for c in self.accepted:
            if c.group not in self.groups:
                self.groups.append(c.group)

    def group(self, g):
        return [c for c in self.accepted if c.group == g]


_CATALOGUE = None


def catalogue():
    """Built once per process (a second or two of Python)."""
    global _CATALOGUE
    if _CATALOGUE is None:
        _CATALOGUE = Catalogue()
    return _CATALOGUE
