"""The catalogue of tests/record_cases.py held against the Python restatement (obsfmt / bcfio, alignprops) and the host reader
(csrc/vlr_ingest.cpp), without a GPU: every accepted record decodes to the table the builder STATED, every refused one is refused by
both, every cell of the chain grid is reached (shown by walking the encoded streams, not by a case's name), every decoy is where
the split kernels will look first and passes a plain transcription of their plausibility test, every control fails it.
tests/test_gpu_record_cases.py gives the same bytes to the kernels: this file is the proof that its inputs and expectations hold."""
import os
import struct

import numpy as np
import pytest

import record_cases as rc
from varlociraptor_amd import abi, alignprops, engine, ingest, obsfmt


@pytest.fixture(scope="module")
def cat():
    return rc.catalogue()


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as fh:
        fh.write(data)
    return p


def _host(path, chunk=1 << 20):
    rd = ingest.ObsReader([path], chunk_records=chunk, device=None)
    out = list(rd)
    rd.close()
    return out


def test_names_are_unique_and_the_groups_are_there(cat):
    every = cat.accepted + cat.refused + cat.decoys + cat.bam
    names = [(c.group, c.name) for c in every]
    assert len(set(names)) == len(names)
    assert [g for g in cat.groups if not cat.group(g)] == []
    assert len(cat.refused) >= 10 and len(cat.decoys) == 5 and len(cat.bam) == 2
    assert all(not c.refused and c.expect for c in cat.accepted) and all(c.refused and c.expect is None for c in cat.refused)


def test_every_cell_of_the_chain_grid_is_reached(cat):
    """Walks the bincode stream of every chain vector of the group (the builder's books hold field, width and stream)."""
    reached, nc = set(), set()
    last_word, one_pad, last_of_file = set(), set(), set()
    for c in cat.group("chain grid"):
        for f, w, stream in c.books:
            if f not in rc.CHAIN_KIND:
                continue
            kind = rc.CHAIN_KIND[f]
            for par, form, noncanonical in rc.walk_chain(kind, stream):
                reached.add((kind, w, par, form))
                if noncanonical:
                    nc.add((kind, w, par, form))
            if kind != "M":
                (one_pad if len(stream) & 1 else last_word).add((kind, w))
        # the record's last INFO entry, the last bytes of the file's records: which vector, in which width
        order = c.recs[-1].order or rc.DEFAULT_ORDER
        f, w, stream = [bk for bk in c.books if bk[0] == [x for x in order if x in {k[0] for k in c.books}][-1]][-1]
        if f in rc.CHAIN_KIND and c.records[-1].endswith(rc.words_as(rc.stream_words(stream), w).astype(rc._DT[w]).tobytes()):
            last_of_file.add((rc.CHAIN_KIND[f], w))
    assert len(rc.GRID) == 48
    assert rc.GRID - reached == rc.UNREACHABLE, sorted(rc.GRID - reached)
    assert reached <= rc.GRID
    assert nc == rc.NEEDS_NONCANONICAL_TAG            # a non-canonical Option tag stands only where the canonical one cannot
    for w in rc.GRID_WIDTHS:
        for kind in ("OM", "O8", "O32"):
            assert (kind, w) in last_word and (kind, w) in one_pad, (kind, w)
        assert {("M", w), ("OM", w), ("O32", w)} <= last_of_file, (w, last_of_file)


def test_the_unreachable_cells_are_unreachable():
    """The two cells no int8 vector can hold, whatever the Option tag and the payload.  Some(F32) at even parity: the word of the
    Option tag and the MiniLogProb tag's low byte is 0x01??.  Option<u8> Some at odd parity: an element starts at an odd byte only
    behind a None that started at an even one (a Some is two bytes long), so its tag shares a word with that None's 0: 0x??00."""
    for tag in range(1, 256):
        with pytest.raises(ValueError):
            rc.words_as(rc.stream_words(rc.opt_mini_stream([("f", 0, tag)])), 1)
        with pytest.raises(ValueError):
            rc.words_as(rc.stream_words(rc.opt_u8_stream([None, (0, tag)])), 1)
    assert [p_ for p_, _, _ in rc.walk_chain("O8", rc.opt_u8_stream([5, 6, 7]))] == [0, 0, 0]
    assert [p_ for p_, _, _ in rc.walk_chain("O8", rc.opt_u8_stream([None, 6, None, 7]))] == [0, 1, 1, 0]


def test_the_half_formula_is_numpys_conversion():
    h = np.arange(65536, dtype=np.uint16)
    want = h.view(np.float16).astype(np.float32).view(np.uint32)
    got = np.array([rc.half_bits(int(x)) for x in h], np.uint32)
    nan = np.isnan(h.view(np.float16))
    assert nan.sum() == 2046
    assert np.array_equal(got[~nan], want[~nan])
    # NaN: sign, all-ones exponent and the payload kept in the top mantissa bits
    assert np.array_equal(got[nan], ((h[nan].astype(np.uint32) >> 15) << 31) | 0x7F800000 | ((h[nan].astype(np.uint32) & 0x3FF) << 13))


def test_all_halves_holds_every_pattern_in_every_column(cat):
    c, = cat.group("all halves")
    for f in rc.MINI:
        seen = np.zeros(65536, bool)
        for g, w, stream in c.books:
            if g == f:
                assert w in (2, 3)                     # (the writers' width: int16 where a record's patterns are all below 0x8000)
                a = np.frombuffer(stream, np.dtype([("tag", "<u4"), ("v", "<u2")]), offset=8)
                assert not a["tag"].any()
                seen[a["v"]] = True
        assert seen.all(), f


def test_flags_group_reaches_what_it_is_named_for(cat):
    cs = cat.group("flags and bit vectors")
    assert {r.n for c in cs for r in c.recs} >= {0, 1, 7, 8, 9, 63, 64, 65, 130}
    forms = set()
    for c in cs:
        for f, w, stream in c.books:
            if f in rc.BITS:
                forms.add(("some" if stream[0] else "none", w))
    assert forms == {(a, w) for a in ("some", "none") for w in (1, 2, 3)}, forms
    for f, values in (("STRAND", {0, 1, 2, 3}), ("READ_ORIENTATION", {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 300, 70000}), ("READ_POSITION", {0, 1}), ("ALT_LOCUS", {0, 1, 2})):
        assert {v for c in cs for r in c.recs for v in r.enums[f]} >= values, f
    assert {w for c in cs for f, w, _ in c.books if f in rc.ENUMS} == {1, 2, 3}
    assert any(r.hp_art is None for c in cs for r in c.recs) and any(r.hp_art and None in r.hp_art and any(r.hp_art) for c in cs for r in c.recs)
    assert any(r.third is None for c in cs for r in c.recs) and any(r.third and 0xFFFFFFFE in r.third for c in cs for r in c.recs)


def test_scan_group_reaches_what_it_is_named_for(cat):
    cs = cat.group("scan")
    raw = b"".join(r for c in cs for r in c.records)
    for width, marker in ((1, b"\x11"), (2, b"\x12"), (3, b"\x13")):
        for lt in (1, 2, 3):                           # overflow lengths: descriptor 0xF?, then the length typed int8 / int16 / int32
            assert bytes([0xF0 | width, 0x10 | lt]) in raw or (width, lt) in ((1, 3), (1, 2)), (width, lt)
    keyw = {(f, w) for c in cs for r in c.recs for f, w in r.key_width.items()}
    assert {w for _, w in keyw} == {2, 3}
    assert any(c.recs[0].order == rc.DEFAULT_ORDER[::-1] for c in cs)
    assert any(len(rc.stream_words(s)) > 32767 for c in cs for _, _, s in c.books)
    assert any(len(r.extras) >= 9 for c in cs for r in c.recs)


def _check_obsfmt(path, want, what):
    batch, sites = obsfmt.read_observation_vcf([path])
    assert batch.n_loci == want["n_loci"], what
    assert np.array_equal(batch.obs_offset, want["obs_offset"]), what
    for k, _ in abi.OBS_COLUMNS:
        got = batch.columns[k]
        if k == "flags":
            assert np.array_equal(got, want["cols"][k]), (what, k)
            continue
        exp = want["cols"][k]
        nan = np.isnan(exp.view(np.float32))
        # (obsfmt goes through Python floats: a NaN's payload is not kept there; NaN-ness is compared, bits elsewhere)
        assert np.array_equal(np.isnan(got), nan), (what, k)
        assert np.array_equal(got.view(np.uint32)[~nan], exp[~nan]), (what, k)
    assert np.array_equal(np.asarray(batch.extra["third_allele_evidence"], np.int64), want["third"]), what
    assert [tuple(s) for s in sites] == want["sites"], what
    assert batch.extra["haplotype"] == want["haps"], what
    for l, (het, som) in enumerate(batch.extra["prior_overrides"]):
        for got, exp in ((het, want["het_ln"][l]), (som, want["som_ln"][l])):
            assert (got is None and np.isnan(exp)) or got == exp, (what, l)


@pytest.mark.parametrize("group", ["chain grid", "all halves", "flags and bit vectors", "scan", "split decoys, BCF"])
def test_accepted_cases_decode_to_the_stated_table(cat, tmp_path, group):
    cs = [c for c in cat.group(group) if not c.refused]
    assert cs
    for i, c in enumerate(cs):
        p = _write(tmp_path, "c%d.bcf" % i, c.data)
        want = rc.table_of(c.expect)
        _check_obsfmt(p, want, repr(c))
        rc.check_native(_host(p), want, repr(c))
        if c.chunk:
            rc.check_native(_host(p, c.chunk), want, repr(c))
    if not group.startswith("split"):
        data, expects = rc.file_of(cs)
        p = _write(tmp_path, "group.bcf", data)
        want = rc.table_of(expects)
        rc.check_native(_host(p), want, group)
        rc.check_native(_host(p, 1), want, group)


def _refuses(read, path, errors):
    try:
        read(path)
    except errors:
        return True
    return False


def test_refused_cases_are_refused_by_both_readers(cat, tmp_path):
    ok = cat.group("scan")[0]
    accepted = []
    for i, c in enumerate(cat.refused):
        p = _write(tmp_path, "r%d.bcf" % i, c.data)
        q = _write(tmp_path, "m%d.bcf" % i, rc.bcf_file(ok.records + c.records + ok.records))   # between two accepted records
        for path in (p, q):
            if not _refuses(_host, path, engine.EngineError):
                accepted.append(("host reader", c.name, path == q))
            if not _refuses(lambda x: obsfmt.read_observation_vcf([x]), path, Exception):
                accepted.append(("obsfmt", c.name, path == q))
    assert accepted == []


def test_bcf_decoys_are_where_the_anchor_kernel_looks_first(cat):
    for c in cat.decoys:
        buf = b"".join(c.records)
        starts = c.meta["starts"]
        assert starts[-1] == len(buf)
        for origin, d in zip(c.meta.get("origins", [0] * len(c.meta["decoys"])), c.meta["decoys"]):
            assert origin in starts
            view = buf[origin:]
            seg, rem = divmod(d - origin, rc.SEG)
            assert rem == 0 and seg >= 1                          # at the boundary itself
            nxt = min(s for s in starts if s >= d)
            assert d not in starts and nxt > d                    # before the next true start, and no true start itself
            # the whole file buffered, and only as much as a first request is sure to hold (131 072 bytes and the members that reach them)
            for avail in (len(view), min(len(view), (2 * rc.SEG // 0xFF00 + 1) * 0xFF00 - rc.HEADER_BYTES % 0xFF00)):
                got = rc.anchor_of(view, seg, avail)
                if c.meta["control"]:
                    assert not rc.header_plausible(view, d - origin, avail), c
                    assert got == nxt - origin, (c, got)
                else:
                    assert rc.header_plausible(view, d - origin, avail), c
                    assert got == d - origin, (c, got)
        if "(c)" in c.name:                                       # the arm without a successor test
            d = c.meta["decoys"][0]
            assert d + 8 + struct.unpack_from("<I", buf, d)[0] + 33 > len(buf)
        if "(e)" in c.name:
            k = max(i for i, s in enumerate(starts) if s <= c.meta["decoys"][0])
            assert starts[k + 1] - starts[k] > 4 * rc.SEG and rc.anchor_of(buf, 1) == c.meta["decoys"][0]
    a, b = cat.decoys[0], cat.decoys[1]
    assert len(a.data) and sum(x != y for x, y in zip(b"".join(a.records), b"".join(b.records))) == 1


def _bam_files(tmp_path, c, name):
    fasta = str(tmp_path / "ref.fa")
    if not os.path.exists(fasta):
        alignprops.write_fasta(fasta, rc.bam_reference())
    return fasta, _write(tmp_path, name, c.data)


def test_bam_decoys_and_the_restatements_counts(cat, tmp_path):
    counts = []
    for i, c in enumerate(cat.bam):
        buf = b"".join(c.records)
        d, = c.meta["decoys"]
        starts = c.meta["starts"]
        assert d == rc.SEG and d not in starts
        nxt = min(s for s in starts if s >= d)
        got = rc.bam_anchor_of(buf, 1)
        if c.meta["control"]:
            assert not rc.bam_head_plausible(buf, d, len(buf)) and got == nxt
        else:
            assert rc.bam_head_plausible(buf, d, len(buf)) and got == d
        fasta, bam = _bam_files(tmp_path, c, "b%d.bam" % i)
        n = alignprops.count_bams(fasta, [bam], 10 ** 9)
        assert n.n_taken + n.n_skipped == len(c.records) and n.n_taken > 800
        counts.append(n)
    # the decoy is aux data: both files count alike
    assert np.array_equal(counts[0].transitions, counts[1].transitions) and counts[0].hops == counts[1].hops
    assert counts[0].insert_sizes == counts[1].insert_sizes
