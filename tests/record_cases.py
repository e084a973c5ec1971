"""Hand-built observation records (format v15 in BCF2) and BAM records for the device reader's scan, decode and split kernels
(csrc/vlr_decode.hip): the forms the project's own writer and the reference's files never hold.

Every case carries its file bytes, a group, a name and — for an accepted case — the table the readers must deliver, STATED from the
numbers the builder encoded (u32 bit patterns of the nine float columns, the flags word, third-allele evidence, the offsets, the
site strings, the priors): nothing here is read back from a decoder.  tests/test_record_cases_host.py proves the inputs and the
expectations without a GPU (obsfmt / bcfio and the host reader), tests/test_gpu_record_cases.py gives the same bytes to the kernels.

Wire format (preprocessing/mod.rs:818-1038, utils/mod.rs:449-474 of the reference; BCF2.2 §6.3): a per-observation vector is
bincode(Vec<T>) — u64 count, then per element [u8 Option tag] [u32 MiniLogProb tag + f16 | f32] or [u8] or [u32] — cut into
little-endian u16 words (an odd byte count is padded with one zero byte), each word one integer of an INFO vector.  A reader keeps the
low 16 bits of every integer, so a vector may be typed int8 (words 0..127 and 0xff88..0xffff, sign-extended), int16 (all words but
0x8000..0x8007, the reserved MISSING / END_OF_VECTOR range) or int32.

What the int8 width cannot hold (shown here once, relied on by the grid's list of unreachable cells):
  * a byte at an odd stream position is the HIGH byte of a word and must be 0x00 (low byte <= 0x7f) or 0xff (low byte >= 0x88);
  * so the canonical Option tag 1 cannot stand at an odd position: a Some at odd parity needs the NON-CANONICAL tag 0xff behind a byte
    >= 0x88.  bincode proper refuses such a tag; obsfmt, the host reader and the device reader all take any non-zero tag as Some, and
    the odd-parity int8 arm of rec_decode_kernel (the sign extension of its fifth word) can be reached in no other way.  The cells
    that need it are marked `nc` in the books;
  * Option<MiniLogProb> Some(F32) at EVEN parity puts the MiniLogProb tag's low byte (1) at an odd position: unreachable;
  * Option<u8> Some at ODD parity: the byte in front is always a None tag (0), the tag would have to be 0: unreachable.
"""
import math
import struct

import numpy as np

from varlociraptor_amd import abi, alignprops, bcfio

NAN_BITS = 0x7FC00000
SEG = 65536                       # kSeg of vlr_decode.hip: one anchor per 64 KiB of the inflated records

MINI = ["PROB_MAPPING", "PROB_ALT", "PROB_REF", "PROB_MISSED_ALLELE", "PROB_SAMPLE_ALT", "PROB_DOUBLE_OVERLAP", "PROB_HIT_BASE"]
MINI_COL = ["prob_mapping", "prob_alt", "prob_ref", "prob_missed_allele", "prob_sample_alt", "prob_double_overlap", "prob_hit_base"]
ENUMS = ["STRAND", "READ_ORIENTATION", "READ_POSITION", "ALT_LOCUS"]
BITS = ["SOFTCLIPPED", "PAIRED", "IS_MAX_MAPQ"]
HP_ART, HP_VAR, HP_LEN, THIRD = "PROB_HOMOPOLYMER_ARTIFACT_OBSERVABLE", "PROB_HOMOPOLYMER_VARIANT_OBSERVABLE", "HOMOPOLYMER_INDEL_LEN", "THIRD_ALLELE_EVIDENCE"
CHAIN_KIND = dict([(f, "M") for f in MINI] + [(HP_ART, "OM"), (HP_VAR, "OM"), (HP_LEN, "O8"), (THIRD, "O32")])

# dictionary indices of the header: keys of 5.., 300.. and 40 000.. are typed int8, int16 and int32 by every writer
KEYS = {"LowQual": 2,
        "PROB_MAPPING": 5, "PROB_REF": 300, "PROB_ALT": 40000, "PROB_MISSED_ALLELE": 6, "PROB_SAMPLE_ALT": 301, "PROB_DOUBLE_OVERLAP": 40001,
        "PROB_HIT_BASE": 7, "STRAND": 8, "READ_ORIENTATION": 302, "READ_POSITION": 40002, "ALT_LOCUS": 9, "SOFTCLIPPED": 10, "PAIRED": 303,
        "IS_MAX_MAPQ": 40003, HP_ART: 11, HP_VAR: 304, HP_LEN: 40004, THIRD: 12, "IMPRECISE": 13, "EVENT": 305, "MATEID": 40005,
        "HETEROZYGOSITY": 14, "SOMATIC_EFFECTIVE_MUTATION_RATE": 306,
        "XI": 15, "XF": 16, "XS": 17, "XFLAG": 18, "DECOY": 19, "XM": 307}
_TYPES = {"IMPRECISE": ("0", "Flag"), "EVENT": ("1", "String"), "MATEID": ("1", "String"), "HETEROZYGOSITY": ("A", "Float"),
          "SOMATIC_EFFECTIVE_MUTATION_RATE": ("A", "Float"), "XF": (".", "Float"), "XS": ("1", "String"), "XFLAG": ("0", "Flag")}
CONTIGS = ["chrA", "chrB"]
DEFAULT_ORDER = MINI[:1] + ["PROB_REF", "PROB_ALT"] + MINI[3:6] + ["STRAND", "READ_ORIENTATION", "SOFTCLIPPED", "PAIRED", "READ_POSITION", "PROB_HIT_BASE",
                                                                    "IS_MAX_MAPQ", "ALT_LOCUS", THIRD, HP_ART, HP_VAR, HP_LEN]


def header_text():
    lines = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed">', '##FILTER=<ID=LowQual,Description="low quality",IDX=2>']
    lines += ["##contig=<ID=%s,length=100000000>" % c for c in CONTIGS]
    lines.append("##varlociraptor_observation_format_version=15")
    for name, idx in KEYS.items():
        if name == "LowQual":
            continue
        number, ty = _TYPES.get(name, (".", "Integer"))
        lines.append('##INFO=<ID=%s,Number=%s,Type=%s,Description="hand-built",IDX=%d>' % (name, number, ty, idx))
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    return "\n".join(lines) + "\n"


def file_head():
    text = header_text().encode() + b"\x00"
    return b"BCF\x02\x02" + struct.pack("<I", len(text)) + text


HEADER_BYTES = len(file_head())


def bgzf(payload, member=0xFF00):
    out = bytearray()
    for o in range(0, len(payload), member):
        out += bcfio._bgzf_block(payload[o:o + member])
    return bytes(out) + bcfio._BGZF_EOF


def bcf_file(records, member=0xFF00):
    return bgzf(file_head() + b"".join(records), member)


# ---------------------------------------------------------------------------------------------------------------- numbers
def half_bits(h):
    """f16 bit pattern -> f32 bit pattern, in integers: sign | exponent | mantissa << 13, subnormals normalised, NaN payloads kept."""
    s, e, m = (h >> 15) << 31, (h >> 10) & 0x1F, h & 0x3FF
    if e == 0:
        if m == 0:
            return s
        k = 11 - m.bit_length()               # shifts until bit 10 is set
        return s | ((113 - k) << 23) | (((m << k) & 0x3FF) << 13)
    if e == 31:
        return s | 0x7F800000 | (m << 13)
    return s | ((e + 112) << 23) | (m << 13)


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def fnv1a_key(s):
    """group_key of a haplotype identifier (64-bit FNV-1a, lowest bit set; 0 = ungrouped)."""
    if s is None:
        return 0
    h = 0xCBF29CE484222325
    for c in s.encode():
        h = ((h ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h | 1


# ---------------------------------------------------------------------------------------------------------------- typed values
_DT = {1: "<i1", 2: "<i2", 3: "<i4"}


def enc_desc(n, t, len_t=0):
    if n < 15:
        return bytes([(n << 4) | t])
    lt = len_t or (1 if n <= 127 else 2 if n <= 32767 else 3)
    assert n <= (127, 32767, 2 ** 31 - 1)[lt - 1]
    return bytes([0xF0 | t, 0x10 | lt]) + np.array([n], _DT[lt]).tobytes()


def enc_ints(vals, t, len_t=0):
    return enc_desc(len(vals), t, len_t) + np.asarray(vals, np.int64).astype(_DT[t]).tobytes()


def enc_key(name, t=0):
    k = KEYS[name]
    return enc_ints([k], t or (1 if k <= 127 else 2 if k <= 32767 else 3))


def stream_words(stream):
    b = bytes(stream) + (b"\x00" if len(stream) & 1 else b"")
    return np.frombuffer(b, "<u2").astype(np.int64)


def natural_width(words):
    """The width the writers choose (they store the words as non-negative integers)."""
    m = int(words.max()) if len(words) else 0
    return 1 if m <= 127 else 2 if m <= 32767 else 3


def words_as(words, t):
    """The integers of width t whose low 16 bits are the words; ValueError where the width cannot hold them (or only as a reserved value)."""
    if t == 3:
        return words
    v = np.where(words >= 0x8000, words - 65536, words)
    lo, hi = ((-120, 127), (-32760, 32767))[t - 1]
    if len(v) and (v.min() < lo or v.max() > hi):
        raise ValueError("words do not fit width %d" % t)
    return v


# ---------------------------------------------------------------------------------------------------------------- bincode streams
def _u64(v):
    return struct.pack("<Q", v)


def _mini_bytes(k, v):
    return struct.pack("<IH", 0, v) if k == "h" else struct.pack("<II", 1, v)


def _mini_bits(k, v):
    return half_bits(v) if k == "h" else v


def mini_stream(elems):
    ks = set(k for k, _ in elems)
    if len(elems) > 64 and len(ks) == 1:    # (large vectors of one variant: the same bytes, built by numpy)
        k = ks.pop()
        a = np.zeros(len(elems), np.dtype([("tag", "<u4"), ("v", "<u2" if k == "h" else "<u4")]))
        a["tag"] = 0 if k == "h" else 1
        a["v"] = [v for _, v in elems]
        return _u64(len(elems)) + a.tobytes()
    return _u64(len(elems)) + b"".join(_mini_bytes(k, v) for k, v in elems)


def opt_mini_stream(elems):
    out = [_u64(len(elems))]
    for e in elems:
        out.append(b"\x00" if e is None else bytes([e[2] if len(e) > 2 else 1]) + _mini_bytes(e[0], e[1]))
    return b"".join(out)


def _val_tag(e):
    return e if isinstance(e, tuple) else (e, 1)


def opt_u8_stream(elems):
    return _u64(len(elems)) + b"".join(b"\x00" if e is None else bytes([_val_tag(e)[1], _val_tag(e)[0]]) for e in elems)


def opt_u32_stream(elems):
    return _u64(len(elems)) + b"".join(b"\x00" if e is None else bytes([_val_tag(e)[1]]) + struct.pack("<I", _val_tag(e)[0]) for e in elems)


def enum_stream(vals):
    return _u64(len(vals)) + np.asarray(vals, np.int64).astype("<u4").tobytes()


def bitvec_stream(form, bits, n_blocks=None, n_bits=None):
    """bv::BitVec<u8>: ("some": tag 1, u64 blocks, the bytes, u64 bits) or ("none": tag 0, u64 bits)."""
    n = len(bits)
    if form == "none":
        return b"\x00" + _u64(n if n_bits is None else n_bits)
    blocks = np.packbits(np.asarray(bits, bool), bitorder="little").tobytes()
    if n_blocks is not None:
        blocks = (blocks + bytes(n_blocks))[:n_blocks]
    return b"\x01" + _u64(len(blocks)) + blocks + _u64(n if n_bits is None else n_bits)


def walk_chain(kind, stream):
    """The elements of a chain vector's stream as (start parity, form, non-canonical tag); raises if the stream does not end with its
    last element (a zero padding byte is taken off by the caller).  Forms: f16 f32 | none some16 some32 | none some."""
    n, = struct.unpack_from("<Q", stream, 0)
    j, out = 8, []
    for _ in range(n):
        par = j & 1
        if kind == "M":
            tag, = struct.unpack_from("<I", stream, j)
            assert tag in (0, 1)
            out.append((par, "f16" if tag == 0 else "f32", False))
            j += 6 if tag == 0 else 8
            continue
        t = stream[j]
        if t == 0:
            out.append((par, "none", False))
            j += 1
        elif kind == "OM":
            tag, = struct.unpack_from("<I", stream, j + 1)
            assert tag in (0, 1)
            out.append((par, "some16" if tag == 0 else "some32", t != 1))
            j += 7 if tag == 0 else 9
        else:
            out.append((par, "some", t != 1))
            j += 2 if kind == "O8" else 5
    assert j == len(stream), (kind, j, len(stream))
    return out


GRID_WIDTHS = (1, 2, 3)
GRID = frozenset([("M", w, 0, f) for w in GRID_WIDTHS for f in ("f16", "f32")] +
                 [("OM", w, p, f) for w in GRID_WIDTHS for p in (0, 1) for f in ("none", "some16", "some32")] +
                 [(k, w, p, f) for k in ("O8", "O32") for w in GRID_WIDTHS for p in (0, 1) for f in ("none", "some")])
UNREACHABLE = frozenset([("OM", 1, 0, "some32"), ("O8", 1, 1, "some")])            # (the module's docstring says why)
NEEDS_NONCANONICAL_TAG = frozenset([("OM", 1, 1, "some16"), ("OM", 1, 1, "some32"), ("O32", 1, 1, "some")])


# ---------------------------------------------------------------------------------------------------------------- one record
def default_mini(c, n, big=False):
    if big:                                   # positive halves: every word below 0x8000, the natural width is int16
        return [("h", 0x4900 + ((7 * i + c) & 0xFF)) for i in range(n)]
    return [("f", f32_bits(-(0.25 + 0.5 * i + c))) if (i + c) % 3 == 0 else ("h", 0xC900 + ((7 * i + 13 * c) & 0xFF)) for i in range(n)]


ORIENT_VALUES = [0, 1, 2, 3, 4, 5, 6, 7, 8]


class Rec:
    """One record: what is encoded AND what the readers must deliver for it."""

    def __init__(self, n, big=False):
        self.n = n
        self.mini = {f: default_mini(c, n, big) for c, f in enumerate(MINI)}
        i = np.arange(n)
        self.enums = {"STRAND": (i % 4).tolist(), "READ_ORIENTATION": [ORIENT_VALUES[k % 9] for k in range(n)], "READ_POSITION": (i % 2).tolist(),
                      "ALT_LOCUS": (i % 3).tolist()}
        self.bits = {"SOFTCLIPPED": ("some", (i % 5 == 1)), "PAIRED": ("some", (i % 2 == 0)), "IS_MAX_MAPQ": ("some", (i % 7 != 3))}
        self.hp_art = self.hp_var = self.hp_len = self.third = None
        self.width, self.len_width, self.key_width = {}, {}, {}
        self.order, self.extras, self.drop, self.raw_stream, self.raw_words = None, [], set(), {}, {}
        self.chrom, self.pos, self.id, self.ref, self.alts, self.filter = 0, 100, "", "A", ["C"], []
        self.imprecise = self.event = self.mateid = self.het = self.som = None
        self.l_shared_add = 0
        self.string_key = None

    # ---- what is encoded
    def streams(self):
        s = {f: mini_stream(self.mini[f]) for f in MINI}
        s.update({f: enum_stream(self.enums[f]) for f in ENUMS})
        s.update({f: bitvec_stream(*self.bits[f]) for f in BITS})
        if self.hp_art is not None:
            s[HP_ART], s[HP_VAR], s[HP_LEN] = opt_mini_stream(self.hp_art), opt_mini_stream(self.hp_var), opt_u8_stream(self.hp_len)
        if self.third is not None:
            s[THIRD] = opt_u32_stream(self.third)
        s.update(self.raw_stream)
        return s

    def encode(self):
        """(record bytes, books): books lists every vector as (field, width, stream)."""
        entries, books = {}, []
        for f, st in self.streams().items():
            if f in self.drop:
                continue
            words = self.raw_words[f] if f in self.raw_words else stream_words(st)
            t = self.width.get(f) or natural_width(words)
            books.append((f, t, st))
            entries[f] = enc_key(f, self.key_width.get(f, 0)) + enc_ints(words_as(words, t), t, self.len_width.get(f, 0))
        if self.imprecise is not None:
            entries["IMPRECISE"] = enc_key("IMPRECISE", self.key_width.get("IMPRECISE", 0)) + self.imprecise       # b"\x11\x01" or b"\x00"
        for name, v in (("EVENT", self.event), ("MATEID", self.mateid)):
            if v is not None:
                entries[name] = enc_key(name) + bcfio._enc_str(v)
        for name, v in (("HETEROZYGOSITY", self.het), ("SOMATIC_EFFECTIVE_MUTATION_RATE", self.som)):
            if v is not None:
                entries[name] = enc_key(name) + bcfio._enc_floats([v])
        order = list(self.order or DEFAULT_ORDER) + ["IMPRECISE", "EVENT", "MATEID", "HETEROZYGOSITY", "SOMATIC_EFFECTIVE_MUTATION_RATE"]
        assert set(entries) <= set(order)
        info = [entries[f] for f in order if f in entries]
        for at, raw in sorted(self.extras, key=lambda x: -x[0]):
            info.insert(min(at, len(info)), raw)
        if self.string_key is not None:
            info[self.string_key[0]] = bcfio._enc_str(self.string_key[1]) + info[self.string_key[0]][2:]
        shared = bcfio._enc_str(self.id) + b"".join(bcfio._enc_str(a) for a in [self.ref] + self.alts)
        shared += bcfio._enc_ints(self.filter) if self.filter else b"\x00"
        shared += b"".join(info)
        fixed = struct.pack("<iiiIII", self.chrom, self.pos - 1, len(self.ref), bcfio.FLOAT_MISSING, ((1 + len(self.alts)) << 16) | len(info), 0)
        return struct.pack("<II", 24 + len(shared) + self.l_shared_add, 0) + fixed + shared, books

    # ---- what must come out
    def expect(self):
        n = self.n
        cols = {}
        for f, name in zip(MINI, MINI_COL):
            cols[name] = np.array([_mini_bits(k, v) for k, v in self.mini[f]], np.uint32)
        for name, elems in (("prob_hp_artifact", self.hp_art), ("prob_hp_variant", self.hp_var)):
            cols[name] = np.array([NAN_BITS if (elems is None or e is None) else _mini_bits(e[0], e[1]) for e in (elems or [None] * n)], np.uint32)
        fl = np.zeros(n, np.int64)
        st, orient, rp, al = (np.asarray(self.enums[f], np.int64) for f in ENUMS)
        fl |= (st & 3) << abi.F_STRAND_SHIFT
        oc = np.full(n, abi.ORIENT_OTHER, np.int64)
        oc[orient == 0], oc[orient == 1], oc[orient == 8] = abi.ORIENT_F1R2, abi.ORIENT_F2R1, abi.ORIENT_NONE
        fl |= oc << abi.F_ORIENT_SHIFT
        fl |= np.where(rp == 0, abi.F_READPOS_MAJOR, 0)
        fl |= (al & 3) << abi.F_ALTLOCUS_SHIFT
        for f, bit in zip(BITS, (abi.F_SOFTCLIPPED, abi.F_PAIRED, abi.F_MAX_MAPQ)):
            if self.bits[f][0] == "some":
                fl |= np.where(np.asarray(self.bits[f][1], bool), bit, 0)
        if self.hp_len is not None:
            for i, e in enumerate(self.hp_len):
                if e is not None:
                    fl[i] |= abi.F_HP_LEN_VALID | (_val_tag(e)[0] << abi.F_HP_LEN_SHIFT)
        cols["flags"] = fl.astype(np.uint32)
        third = np.array([-1 if (self.third is None or e is None) else _val_tag(e)[0] for e in (self.third or [None] * n)], np.int64)
        hap = self.event if self.event else ("-".join(sorted([self.id, self.mateid])) if self.mateid else None)
        prior = lambda x: float("nan") if x is None else -float(np.float32(x)) * math.log(10.0) / 10.0
        return dict(n=n, cols=cols, third=third, site=(CONTIGS[self.chrom], self.pos, self.ref, ",".join(self.alts) if self.alts else "."),
                    id=self.id or ".", imprecise=self.imprecise is not None, hap=hap, het_ln=prior(self.het), som_ln=prior(self.som),
                    is_hp=self.hp_art is not None and n > 0)


class Case:
    def __init__(self, group, name, recs=(), refused=False, raw_records=None, chunk=None, meta=None):
        self.group, self.name, self.refused = group, name, refused
        self.recs = list(recs)
        enc = [r.encode() for r in self.recs]
        self.records = list(raw_records) if raw_records is not None else [e[0] for e in enc]
        self.books = [b for e in enc for b in e[1]]
        self.expect = None if refused else [r.expect() for r in self.recs]
        self.data = bcf_file(self.records)
        self.chunk = chunk                      # chunk_records the case is (also) read with
        self.meta = meta or {}

    def __repr__(self):
        return "<%s: %s>" % (self.group, self.name)


def file_of(cases):
    """One file of the records of several accepted cases, and its stated table."""
    return bcf_file([r for c in cases for r in c.records]), [e for c in cases for e in c.expect]


def table_of(expects):
    """The stated table of a file: the expectations of its records, concatenated."""
    cat = lambda f, dt: np.concatenate([f(e) for e in expects]).astype(dt) if expects else np.zeros(0, dt)
    t = dict(n_loci=len(expects), obs_offset=np.concatenate([[0], np.cumsum([e["n"] for e in expects])]).astype(np.uint32),
             third=cat(lambda e: e["third"], np.int64), sites=[e["site"] for e in expects], ids=[e["id"] for e in expects],
             imprecise=np.array([e["imprecise"] for e in expects], np.uint8), het_ln=np.array([e["het_ln"] for e in expects], np.float64),
             som_ln=np.array([e["som_ln"] for e in expects], np.float64), group_key=np.array([fnv1a_key(e["hap"]) for e in expects], np.uint64),
             haps=[e["hap"] for e in expects])
    t["cols"] = {k: cat(lambda e, k=k: e["cols"][k], np.uint32) for k, _ in abi.OBS_COLUMNS}
    first, rep = {}, []
    for l, h in enumerate(t["haps"]):
        rep.append(first.setdefault(h, l) if h is not None else l)
    t["group_representative"] = np.array(rep, np.int64)
    return t


def _same_floats(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def check_native(chunks, want, what=""):
    """The tables a native reader delivered ((PileupBatch, Sites) per chunk, in order) against the stated table: == on bit patterns."""
    L = sum(b.n_loci for b, _ in chunks)
    assert L == want["n_loci"], "%s: %d records, %d stated" % (what, L, want["n_loci"])
    l0 = 0
    for b, sites in chunks:
        assert b.n_samples == 1
        l1 = l0 + b.n_loci
        o0, o1 = int(want["obs_offset"][l0]), int(want["obs_offset"][l1])
        assert np.array_equal(b.obs_offset, want["obs_offset"][l0:l1 + 1] - want["obs_offset"][l0]), "%s: offsets of records %d.." % (what, l0)
        for k, dt in abi.OBS_COLUMNS:
            got = b.columns[k]
            assert got.dtype == dt
            got = got.view(np.uint32)
            exp = want["cols"][k][o0:o1]
            if not np.array_equal(got, exp):
                i = int(np.nonzero(got != exp)[0][0])
                raise AssertionError("%s: column %s, observation %d (of the file: %d): %#010x, stated %#010x" % (what, k, i, o0 + i, int(got[i]), int(exp[i])))
        assert np.array_equal(np.asarray(b.extra["third_allele_evidence"], np.int32), want["third"][o0:o1].astype(np.int32)), "%s: third-allele evidence" % what
        for l in range(b.n_loci):
            assert sites[l] == want["sites"][l0 + l], "%s: site of record %d: %r, stated %r" % (what, l0 + l, sites[l], want["sites"][l0 + l])
            assert sites.record_id(l) == want["ids"][l0 + l], "%s: ID of record %d" % (what, l0 + l)
        assert np.array_equal(np.asarray(sites.imprecise), want["imprecise"][l0:l1]), "%s: IMPRECISE" % what
        assert _same_floats(b.extra["prior_het_ln"], want["het_ln"][l0:l1]), "%s: HETEROZYGOSITY" % what
        assert _same_floats(b.extra["prior_som_ln"], want["som_ln"][l0:l1]), "%s: SOMATIC_EFFECTIVE_MUTATION_RATE" % what
        assert np.array_equal(np.asarray(b.extra["group_key"]), want["group_key"][l0:l1]), "%s: group keys" % what
        if len(chunks) == 1:
            assert np.array_equal(np.asarray(b.extra["group_representative"]), want["group_representative"]), "%s: group representatives" % what
        l0 = l1


# ---------------------------------------------------------------------------------------------------------------- group: chain grid
_NC = 0xFF                                    # the non-canonical Some tag (module docstring)


def _grid_int8():
    """int8 width: every sequence below was laid out byte by byte so that each word is 0..127 or 0xff88..0xffff."""
    m = [("h", 0x0000), ("f", 0x007F0012), ("h", 0x007F), ("h", 0xFF88), ("f", 0xFF90FF88), ("h", 0x0001), ("h", 0x0040), ("f", 0x00010000)]
    # Option<MiniLogProb>, start byte in comments
    a8 = [("h", 0x7C00),                      # 8   even some16: +inf; its high byte 0x7c pairs with the None tag behind
          None,                               # 15  odd  none
          ("h", 0x9000),                      # 16  even some16; high byte 0x90 pairs with the tag 0xff behind
          ("h", 0x0001, _NC),                 # 23  odd  some16 (nc): the smallest subnormal
          ("h", 0xFC00),                      # 30  even some16: -inf
          ("f", 0xFF900012, _NC),             # 37  odd  some32 (nc): the payload's top byte is the SIGN EXTENSION of the step's fifth word
          None, None]                         # 46 even none, 47 odd none -> 48: ends with the vector's last word
    b8 = [None, None,                         # 8, 9
          ("h", 0x7E00),                      # 10  even some16: NaN
          None,                               # 17
          ("h", 0x8800),                      # 18  even some16
          ("f", 0x007F0001, _NC),             # 25  odd  some32 (nc)
          ("h", 0x0400),                      # 34  even some16: the smallest normal
          None]                               # 41  -> 42
    l8 = [0, None, None, 0, 0, None, None, 0]                                          # 8 10 11 12 14 16 17 18 -> 20
    l7 = [0, 0, None, None, 0, 0, None]                                                # -> 19: one padding byte
    t8 = [0x90FF9900, (0x00070005, _NC), None, None, 0x22001100, None, None, None]     # 8 13 18 19 20 25 26 27 -> 28
    return m, (a8, b8, l8, t8), (a8[:7], b8[:7], l7, t8[:7])


def _grid_wide(w):
    """int16 / int32: canonical tags, every form at both parities (every Option<MiniLogProb> and Option<u32> element has an odd size:
    the parity alternates; an Option<u8> None flips it)."""
    m = [("h", 0xC900), ("f", 0xBF000000), ("h", 0x8008), ("h", 0x7C00), ("f", 0x3F800000), ("h", 0xFC00), ("h", 0x7E01), ("h", 0x03FF)]
    if w == 3:
        m[2], m[6] = ("h", 0x8000), ("f", 0x80008001)        # -0.0; words of the reserved int16 range
    a8 = [("h", 0x0001), ("h", 0xFBFF), ("f", 0xC1200000), ("f", 0x7F800000), None, None, ("h", 0x83FF), None]
    b8 = [None, ("f", 0xFF800000), ("h", 0x7C01), None, ("f", 0x00000001), ("h", 0x0400), None, ("h", 0xC900)]
    l8 = [5, None, 0xFB, None, 0x7F, None, 0x81, None]        # (0x80 = -128 is obsfmt's own None marker: not used)
    t8 = [0xFFFFFFFE, 70000, None, None, 1, None, 0x12348009, None]
    if w == 3:
        t8[6] = 0x80008001
    l7 = l8[:7]
    return m, (a8, b8, l8, t8), (a8[:7], b8[:7], l7, t8[:7])


def _grid_cases():
    out = []
    for w in GRID_WIDTHS:
        m, full, cut = _grid_int8() if w == 1 else _grid_wide(w)
        wname = "int%d" % (8, 16, 32)[w - 1]
        r = Rec(len(m))
        for c, f in enumerate(MINI):
            r.mini[f] = m[c:] + m[:c]
            r.width[f] = w
        out.append(Case("chain grid", "MiniLogProb in %s" % wname, [r]))
        for tag, (a, b, l, t) in (("ends with the last word", full), ("ends one padding byte before the last word", cut)):
            r = Rec(len(a))
            r.hp_art, r.hp_var, r.hp_len, r.third = a, b, l, t
            for f in (HP_ART, HP_VAR, HP_LEN, THIRD):
                r.width[f] = w
            out.append(Case("chain grid", "Option vectors in %s, last element %s" % (wname, tag), [r]))
        # the last vector of the last record of the file: a chain vector of this width is the record's last INFO entry
        for f, n in ((HP_VAR, len(cut[1])), (THIRD, len(full[3])), (MINI[6], len(m))):
            r = Rec(n)
            if f != MINI[6]:
                r.hp_art, r.hp_var, r.hp_len, r.third = (full if n == len(full[0]) else cut)
                for g in (HP_ART, HP_VAR, HP_LEN, THIRD):
                    r.width[g] = w
            else:
                r.mini[f] = m
            r.width[f] = w
            r.order = [x for x in DEFAULT_ORDER if x != f] + [f]
            out.append(Case("chain grid", "%s in %s is the last vector of the file" % (f, wname), [r]))
    return out


# ---------------------------------------------------------------------------------------------------------------- group: all halves
def _halves_cases():
    """All 65 536 f16 patterns under tag 0 in EVERY PROB_* vector: 64 records of 1 024 observations, column c shifted by c * 9 362."""
    recs = []
    for r_ in range(64):
        r = Rec(1024, big=True)
        base = np.arange(r_ * 1024, (r_ + 1) * 1024)
        for c, f in enumerate(MINI):
            r.mini[f] = [("h", int(h)) for h in (base + c * 9362) & 0xFFFF]
        r.pos = 1000 + r_
        recs.append(r)
    return [Case("all halves", "every f16 pattern in every PROB vector", recs)]


# ---------------------------------------------------------------------------------------------------------------- group: flags and bit vectors
def _flag_cases():
    out = []
    rng = np.random.default_rng(20)
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 130):
        i = np.arange(n)
        # (a) Some-form bit vectors in their natural widths; SOFTCLIPPED all clear: int8 up to n = 8
        r = Rec(n)
        r.enums["READ_ORIENTATION"] = [(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 300, 70000)[k % 12] for k in range(n)]
        r.bits = {"SOFTCLIPPED": ("some", np.zeros(n, bool)), "PAIRED": ("some", rng.random(n) < 0.5), "IS_MAX_MAPQ": ("some", rng.random(n) < 0.9)}
        out.append(Case("flags and bit vectors", "n = %d, Some-form bit vectors" % n, [r]))
        # (b) None-with-count forms, homopolymer fields with mixed None, third-allele evidence up to 2^32 - 2
        r = Rec(n)
        r.bits = {"SOFTCLIPPED": ("none", np.zeros(n, bool)), "PAIRED": ("some", i % 3 == 0), "IS_MAX_MAPQ": ("none", np.zeros(n, bool))}
        r.hp_art = [None if k % 3 == 0 else ("h", 0xC000 + k) if k % 3 == 1 else ("f", f32_bits(-0.125 * k)) for k in range(n)]
        r.hp_var = [("h", 0xD000 + k) if k % 4 == 0 else None for k in range(n)]
        r.hp_len = [None if k % 2 else (k * 37 + 1) & 0x7F for k in range(n)]
        r.third = [None if k % 3 == 1 else (0xFFFFFFFE, 0, 1, 0x7FFFFFFF, 0x80000000)[k % 5] for k in range(n)]
        r.enums["STRAND"] = [3 - (k % 4) for k in range(n)]
        out.append(Case("flags and bit vectors", "n = %d, None-form bit vectors, homopolymer fields, third-allele evidence" % n, [r]))
    # enum vectors in all three widths, the bit vectors forced wider than needed (int8 holds a bit vector only at n = 0: the low byte of
    # the block count stands at an odd position)
    for w in GRID_WIDTHS:
        r = Rec(8)
        r.bits = {"SOFTCLIPPED": ("some", np.zeros(8, bool)), "PAIRED": ("none", np.zeros(8, bool)), "IS_MAX_MAPQ": ("some", np.array([1, 0, 1, 1, 0, 0, 1, 0], bool))}
        for f in ENUMS + (BITS if w > 1 else []):
            r.width[f] = w
        out.append(Case("flags and bit vectors", "enum vectors (and bit vectors) forced to int%d" % (8, 16, 32)[w - 1], [r]))
    r = Rec(130)
    r.bits = {f: ("some", rng.random(130) < 0.5) for f in BITS}          # dense: words above 32 767, int32
    out.append(Case("flags and bit vectors", "n = 130, dense bit vectors", [r]))
    r = Rec(9)
    r.bits["PAIRED"] = ("some", np.ones(9, bool), 4)                      # more blocks than the bits need
    out.append(Case("flags and bit vectors", "n = 9, four blocks for nine bits", [r]))
    return out


# ---------------------------------------------------------------------------------------------------------------- group: scan
def _unknown_entries():
    return [enc_key("XI") + enc_ints([1, -2, 3], 1), enc_key("XI") + enc_ints([300, -300] * 10, 2, 3), enc_key("XI") + enc_ints([70000, -70000, -2147483648, -2147483647], 3),
            enc_key("XF") + bcfio._enc_floats([0.5, None, 2.0]), enc_key("XS") + bcfio._enc_str("between the fields, longer than fifteen bytes"),
            enc_key("XFLAG") + b"\x11\x01", enc_key("XFLAG") + b"\x00", enc_key("XM") + b"\x00", enc_key("XI", 3) + enc_ints([-128, -127], 1)]


def _scan_cases():
    out = []
    r = Rec(5)
    r.hp_art, r.hp_var, r.hp_len, r.third = [None, ("h", 0xC900), None, ("f", 0xC1200000), None], [None] * 5, [1, None, 2, None, 3], [None, 7, None, 8, None]
    r.order = DEFAULT_ORDER[::-1]
    out.append(Case("scan", "INFO entries in reverse order", [r]))
    r = Rec(5)
    r.order = DEFAULT_ORDER[5:] + DEFAULT_ORDER[:5]
    r.key_width = {"PROB_MAPPING": 2, "PROB_MISSED_ALLELE": 3, "PROB_REF": 3, "STRAND": 2, "SOFTCLIPPED": 3, "IMPRECISE": 2}
    r.imprecise = b"\x11\x01"
    out.append(Case("scan", "keys typed wider than needed", [r]))
    r = Rec(5)
    r.len_width = {"PROB_MAPPING": 2, "PROB_REF": 3, "PROB_ALT": 3, "STRAND": 2, "READ_POSITION": 3, "SOFTCLIPPED": 2, "PAIRED": 3}
    out.append(Case("scan", "overflow lengths forced wider", [r]))
    r = Rec(40)
    r.third = [k if k % 2 else None for k in range(40)]
    out.append(Case("scan", "overflow lengths in int8 and int16", [r]))
    r = Rec(11000, big=True)
    out.append(Case("scan", "vectors of more than 32 767 words", [r]))
    r = Rec(6)
    r.hp_art, r.hp_var, r.hp_len, r.third = [("h", 0xC900)] * 6, [None] * 6, [4] * 6, [9] * 6
    r.extras = [(k * 2, e) for k, e in enumerate(_unknown_entries())]
    out.append(Case("scan", "unknown keys of every type between the fields", [r]))
    # the cold fields
    for name, kw in (("ID empty, SNV", dict()),
                     ("ID long", dict(id="rs1234567890-a-rather-long-identifier;second")),
                     ("symbolic allele, IMPRECISE as a typed 1", dict(ref="N", alts=["<DEL>"], imprecise=b"\x11\x01", id="sv1")),
                     ("multi-base alleles, IMPRECISE as a MISSING value", dict(ref="ACGTACGTACGTACGTACGT", alts=["A", "ACGTAC"], imprecise=b"\x00")),
                     ("no ALT allele", dict(alts=[])),
                     ("FILTER", dict(filter=[KEYS["LowQual"]], chrom=1, pos=99999999)),
                     ("EVENT", dict(event="ev7", ref="G", alts=["G[chrB:5000["], id="bnd_a")),
                     ("EVENT again", dict(event="ev7", ref="T", alts=["]chrA:100]T"], id="bnd_b", chrom=1, pos=5000)),
                     ("MATEID", dict(mateid="bnd_z", ref="G", alts=["G[chrB:7000["], id="bnd_y")),
                     ("MATEID of the mate", dict(mateid="bnd_y", ref="C", alts=["]chrA:100]C"], id="bnd_z", chrom=1)),
                     ("prior overrides", dict(het=30.0, som=12.5)),
                     ("one prior override, EVENT and MATEID", dict(som=60.25, event="ev9", mateid="m", id="x"))):
        r = Rec(3)
        for k, v in kw.items():
            setattr(r, k, v)
        out.append(Case("scan", "cold fields: " + name, [r]))
    return out


# ---------------------------------------------------------------------------------------------------------------- group: refused
def _refused_cases():
    """One case per reason.  Each was read along its path through rec_scan_kernel and rec_decode_kernel: d_typed keeps every vector
    inside the record's shared block; the chain step stops a lane whose next element would end behind the vector (its later reads
    are at the vector's first bytes); the flags pass runs only when every length check passed; a count above 2^28 or above what
    PROB_MAPPING can hold ends the scan before the table is sized."""
    out = []

    def add(name, r):
        out.append(Case("refused", name, [r], refused=True))
    r = Rec(4); r.mini["PROB_REF"] = [("h", 0xC900), ("f", 0xBF000000), ("h", 0xC901), ("h", 0xC902)]
    s = bytearray(mini_stream(r.mini["PROB_REF"])); s[14:18] = struct.pack("<I", 2)          # the tag of the second element
    r.raw_stream["PROB_REF"] = bytes(s)
    add("a MiniLogProb tag of 2", r)
    r = Rec(4); r.raw_stream["PROB_ALT"] = mini_stream(default_mini(1, 5))
    add("PROB_ALT counts five, the record four", r)
    r = Rec(4); r.raw_stream["STRAND"] = enum_stream([0, 1, 2])
    add("STRAND counts three, the record four", r)
    r = Rec(4); r.mini["PROB_HIT_BASE"] = [("h", 0xC900)] * 3 + [("f", 0xBF000000)]
    r.raw_words["PROB_HIT_BASE"] = stream_words(mini_stream(r.mini["PROB_HIT_BASE"]))[:-1]
    add("PROB_HIT_BASE ends inside its last element", r)
    r = Rec(4); r.hp_art, r.hp_var, r.hp_len, r.third = [None] * 4, [None] * 4, [1, None, 2, None], None
    r.raw_words[HP_LEN] = stream_words(opt_u8_stream(r.hp_len))[:-1]
    add("HOMOPOLYMER_INDEL_LEN ends inside its last element", r)
    r = Rec(4); r.raw_words["READ_POSITION"] = stream_words(enum_stream(r.enums["READ_POSITION"]))[:-1]
    add("READ_POSITION too short", r)
    r = Rec(9); r.bits["PAIRED"] = ("some", np.ones(9, bool), None, 8)
    add("PAIRED with nbits 8 for nine observations", r)
    r = Rec(9); r.bits["SOFTCLIPPED"] = ("none", np.zeros(9, bool), None, 10)
    add("SOFTCLIPPED None with a count of ten for nine observations", r)
    r = Rec(9); r.bits["IS_MAX_MAPQ"] = ("some", np.ones(9, bool), 1)
    add("IS_MAX_MAPQ with one block for nine bits", r)
    r = Rec(9); s = bitvec_stream("some", np.ones(9, bool)); r.raw_stream["PAIRED"] = s[:1] + _u64(200) + s[9:]
    add("PAIRED with more blocks than the vector holds", r)
    r = Rec(4); r.drop.add("ALT_LOCUS")
    add("ALT_LOCUS missing", r)
    r = Rec(4); r.drop.add("PROB_MAPPING")
    add("PROB_MAPPING missing", r)
    r = Rec(4); r.string_key = (3, "A")
    add("a string-typed key", r)
    r = Rec(4); r.l_shared_add = 1000
    add("l_shared beyond the record", r)
    r = Rec(4); s = mini_stream(r.mini["PROB_MAPPING"]); r.raw_stream["PROB_MAPPING"] = _u64((1 << 28) + 1) + s[8:]
    add("a count above 2^28", r)
    r = Rec(4); s = mini_stream(r.mini["PROB_MAPPING"]); r.raw_stream["PROB_MAPPING"] = _u64(1 << 20) + s[8:]
    add("a count the PROB_MAPPING vector cannot hold", r)
    return out


# ---------------------------------------------------------------------------------------------------------------- group: split decoys, BCF
FILL = 0xEE                                   # a filler byte: l_shared = 0xeeeeeeee is implausible at every offset inside it


def header_plausible(buf, o, avail, n_contigs=len(CONTIGS), n_hdr_samples=0):
    """Plain transcription of header_plausible(..., with_id = true) of vlr_decode.hip."""
    if o + 33 > avail:
        return False
    ls, li, chrom, pos = struct.unpack_from("<IIii", buf, o)
    if ls < 26 or ls >= (1 << 24) or li >= (1 << 28):
        return False
    if chrom < 0 or (n_contigs > 0 and chrom >= n_contigs) or pos < -1:
        return False
    nai, nfs = struct.unpack_from("<II", buf, o + 24)
    if (nai >> 16) < 1 or (nfs & 0xFFFFFF) != n_hdr_samples:
        return False
    return (buf[o + 32] & 15) == 7


def anchor_of(buf, seg, avail=None):
    """rec_anchor_kernel: the first offset at or behind seg * SEG that is plausible and whose successor, if buffered, is too (None: none)."""
    avail = len(buf) if avail is None else avail
    o = seg * SEG
    while o + 33 <= avail:
        if header_plausible(buf, o, avail):
            ls, li = struct.unpack_from("<II", buf, o)
            nxt = o + 8 + ls + li
            if nxt + 33 > avail or header_plausible(buf, nxt, avail):
                return o
        o += 1
    return None


def fake_head(l_shared=26, chrom=1, pos0=999):
    """33 bytes that satisfy header_plausible with an ID descriptor, and one filler byte: the next head may follow at + 8 + 26."""
    return struct.pack("<IIiiiIII", l_shared, 0, chrom, pos0, 1, bcfio.FLOAT_MISSING, 2 << 16, 0) + b"\x07" + bytes([FILL])


def _decoy_payload(pre, heads, total):
    body = bytes([FILL]) * pre + heads
    assert len(body) <= total and total % 4 == 0
    return body + bytes([FILL]) * (total - len(body))


def _carrier(k, payload):
    """A small record whose FIRST INFO entry is the int32 vector DECOY with `payload` as its bytes; returns (record, offset of the payload)."""
    r = Rec(3)
    r.pos = 500 + k
    r.id = "d%d" % k
    entry = enc_key("DECOY") + bytes([0xF3, 0x13]) + struct.pack("<i", len(payload) // 4) + payload
    r.extras = [(0, entry)]
    raw, _ = r.encode()
    at = raw.index(entry) + len(entry) - len(payload)
    return r, raw, at


def _decoy_file(n_records, fill_len, decoys):
    """Records that each carry `fill_len` filler bytes; decoys: (offset RELATIVE TO THE FIRST RECORD, head bytes), ascending — the record
    that reaches an offset gets a payload that puts the heads exactly there.  Returns (recs, raws, starts)."""
    recs, raws, starts, at = [], [], [], 0
    todo = list(decoys)
    for k in range(n_records):
        r, raw, p0 = _carrier(k, _decoy_payload(0, b"", fill_len))
        if todo and todo[0][0] < at + len(raw):
            b, heads = todo.pop(0)
            pre = b - (at + p0)
            assert pre >= 0, "the offset falls in front of the payload: choose another filler length"
            r, raw, p0 = _carrier(k, _decoy_payload(pre, heads, max(fill_len, (pre + len(heads) + 64 + 3) // 4 * 4)))
            assert raw[b - at:b - at + len(heads)] == heads
        recs.append(r); raws.append(raw); starts.append(at)
        at += len(raw)
    assert not todo
    starts.append(at)
    return recs, raws, starts


def _decoy_cases():
    two = fake_head() + fake_head()
    lone = fake_head(l_shared=(1 << 24) - 1)           # its successor lies behind every file of this catalogue: the arm without a successor test
    out = []

    def add(name, n_records, fill_len, decoys, chunk=None, control=False):
        recs, raws, starts = _decoy_file(n_records, fill_len, decoys)
        at = [b for b, _ in decoys]
        if control:
            for b in at:                           # one byte: the ID descriptor of the first fake head is no string any more
                k = max(i for i in range(n_records) if starts[i] <= b)
                raw = bytearray(raws[k]); assert raw[b - starts[k] + 32] == 0x07; raw[b - starts[k] + 32] = 0x00
                raws[k] = bytes(raw)
        out.append(Case("split decoys, BCF", name, recs, raw_records=raws, chunk=chunk, meta=dict(decoys=at, starts=starts, control=control)))
    add("(a) one decoy in the record that straddles the first boundary", 24, 4096, [(SEG, two)])
    add("(b) control: the same file, the decoy's ID descriptor changed", 24, 4096, [(SEG, two)], control=True)
    add("(c) a decoy whose successor lies behind the buffered bytes", 24, 4096, [(SEG, lone)])
    # (d) records of about 12 KiB, read seven at a time: the first request's boundary is 65 536 behind the first record, the second
    # request's 65 536 behind the eighth record
    _, _, st = _decoy_file(24, 12288, [(SEG, two)])
    add("(d) decoys in two segments, read seven records at a time", 24, 12288, [(SEG, two), (st[7] + SEG, two)], chunk=7)
    out[-1].meta["origins"] = [0, st[7]]      # the read positions the two boundaries are counted from
    # (e) a record of more than four segments: the decoy at the second boundary inside it (the anchors of segments 1 and 2 both find it)
    recs, raws, starts = [], [], []
    at = 0
    for k in range(12):
        if k == 3:
            r, raw, p0 = _carrier(k, _decoy_payload(0, b"", 4096))
            pre = 2 * SEG - (at + p0)
            r, raw, p0 = _carrier(k, _decoy_payload(pre, two, (pre + 2 * SEG + 30000) // 4 * 4))
        else:
            r, raw, p0 = _carrier(k, _decoy_payload(0, b"", 4096))
        recs.append(r); raws.append(raw); starts.append(at); at += len(raw)
    starts.append(at)
    out.append(Case("split decoys, BCF", "(e) a record of more than four segments, the decoy in a middle one", recs, raw_records=raws,
                    meta=dict(decoys=[2 * SEG], starts=starts, control=False)))
    return out


# ---------------------------------------------------------------------------------------------------------------- group: split decoys, BAM
BAM_CONTIGS = [("b1", 40000), ("b2", 5000)]


def bam_reference():
    rng = np.random.default_rng(77)
    return {name: rng.choice(np.frombuffer(b"ACGT", np.uint8), size=ln).tobytes() for name, ln in BAM_CONTIGS}


def bam_head_plausible(buf, o, avail, n_refs=len(BAM_CONTIGS)):
    """Plain transcription of bam_head_plausible of vlr_decode.hip."""
    if o + 36 > avail:
        return False
    bs, tid, pos, l_rn, _mapq, bin_, n_cig, _flag, l_seq, mtid, mpos = struct.unpack_from("<IiiBBHHHiii", buf, o)
    if bs < 32 or bs >= (1 << 28):
        return False
    if tid < -1 or tid >= n_refs or mtid < -1 or mtid >= n_refs or pos < -1 or mpos < -1:
        return False
    if l_rn < 1 or l_seq < 0:
        return False
    if 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return False
    if o + 36 + l_rn <= avail and buf[o + 36 + l_rn - 1] != 0:
        return False
    return bin_ in (4681 + (pos >> 14), 585 + (pos >> 17), 73 + (pos >> 20), 9 + (pos >> 23), 1 + (pos >> 26), 0)


def bam_anchor_of(buf, seg, avail=None):
    avail = len(buf) if avail is None else avail
    o = seg * SEG
    while o + 36 <= avail:
        if bam_head_plausible(buf, o, avail):
            nxt = o + 4 + struct.unpack_from("<I", buf, o)[0]
            if nxt + 36 > avail or bam_head_plausible(buf, nxt, avail):
                return o
        o += 1
    return None


def fake_bam_head():
    """40 bytes: block_size 36, a fixed head that fits it, the read name "" (its NUL), three filler bytes: the next head follows at + 40."""
    return struct.pack("<IiiBBHHHiiii", 36, 0, 100, 1, 0, 4681, 0, 0, 0, -1, -1, 0) + b"\x00" + bytes([FILL]) * 3


class BamCase:
    def __init__(self, name, records, meta):
        self.group, self.name, self.records, self.meta = "split decoys, BAM", name, records, meta
        self.contigs = BAM_CONTIGS
        self.data = alignprops.bgzf_compress(alignprops.encode_bam(BAM_CONTIGS, records))

    def __repr__(self):
        return "<%s: %s>" % (self.group, self.name)


def plain_bam_records(n, seed=5, aux_for=None):
    ref = bam_reference()["b1"].decode()
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        pos = int(rng.integers(0, 39000))
        ln = int(rng.integers(30, 120))
        cig = [("M", ln)] if k % 4 else [("M", ln // 2), ("D", 2), ("M", ln - ln // 2)]
        rlen = sum(l for _, l in cig if _ != "D")
        seq = ref[pos:pos + ln // 2] + ref[pos + ln // 2 + 2:pos + 2 + ln] if len(cig) == 3 else ref[pos:pos + ln]
        assert len(seq) == rlen
        flag = (0x1 | 0x40) if k % 3 else 0
        aux = aux_for(k) if aux_for else b""
        out.append(alignprops.encode_record(0, pos, int(rng.integers(1, 61)), flag, cig, seq, 0 if flag else -1, pos + 150 if flag else -1,
                                            300 + k % 50 if flag else 0, aux, name="r%d" % k))
    return out


def _bam_decoy_cases():
    out = []
    for control in (False, True):
        heads = fake_bam_head() + fake_bam_head()
        if control:
            heads = heads[:36] + b"x" + heads[37:]          # the read name of the first fake head no longer ends in NUL
        recs, at, done = [], 0, None
        for k, raw in enumerate(plain_bam_records(900, seed=6)):
            if done is None and at + len(raw) + 400 > SEG:
                # this record takes a B:C array that reaches the boundary: the fake heads start exactly there
                p0 = len(raw) + 8                            # tag, 'B', subtype, count
                pre = SEG - (at + p0)
                assert pre >= 0
                arr = list(bytes([FILL]) * pre + heads + bytes([FILL]) * 64)
                aux = alignprops.aux_field("XD", "B", ("C", arr))
                body = raw[4:] + aux
                raw = struct.pack("<I", len(body)) + body
                assert raw[SEG - at:SEG - at + len(heads)] == heads
                done = SEG
            recs.append(raw)
            at += len(raw)
        starts = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).tolist()
        out.append(BamCase("(b) control: the fake head's read name has no NUL" if control else "(a) one decoy in a B:C array across the first boundary",
                           recs, dict(decoys=[done], starts=starts, control=control)))
    return out


# ---------------------------------------------------------------------------------------------------------------- the catalogue
class Catalogue:
    def __init__(self):
        self.accepted = _grid_cases() + _halves_cases() + _flag_cases() + _scan_cases()
        self.refused = _refused_cases()
        self.decoys = _decoy_cases()
        self.bam = _bam_decoy_cases()
        self.groups = ["chain grid", "all halves", "flags and bit vectors", "scan"]

    def group(self, g):
        return [c for c in self.accepted + self.refused + self.decoys + self.bam if c.group == g]


_CAT = []


def catalogue():
    if not _CAT:
        _CAT.append(Catalogue())
    return _CAT[0]
