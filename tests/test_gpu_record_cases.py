"""rec_scan_kernel, rec_decode_kernel and the record split (rec_anchor_kernel / bam_anchor_kernel, the verified walk and its serial
fallback; csrc/vlr_decode.hip) on the hand-built records of tests/record_cases.py: every cell of the chain grid (element kind x
integer width x start parity x form), all 65 536 f16 patterns, pileups around the 64-observation step of the flags pass with bit
vectors in both forms and three widths, INFO entries permuted, keys and overflow lengths in every width, unknown keys of every
type, records that must be refused — each for its own reason — and payload bytes that look like a record head exactly where the
anchor kernels look first.

The expected tables are the ones the builder STATED from the numbers it encoded (tests/test_record_cases_host.py shows, without a
GPU, that obsfmt and the host reader decode every accepted case to them, refuse every refused one, and that every decoy passes a
transcription of the plausibility test); they are compared with == on bit patterns.

Reads behind a vector.  The chain step of rec_decode_kernel loads 20 bytes from an element's address and masks what lies behind the
stream.  The address is at most the vector's end: a lane whose next element would end behind the vector stops (`j + size > nbytes`)
and reads at the vector's first bytes from then on; d_typed keeps every vector inside the record's shared block, the walk keeps the
record inside the inflated bytes; and vlr_dev_file_feed_pieces never inflates into a buffer with fewer than 64 bytes behind the new
end (`wr + inflated_bytes + 64 > cap` compacts into an allocation of `live + inflated + 64` bytes and a quarter more).  So the
last element of the last vector of the last record of a file reads at most 20 of those 64 bytes.  An absent optional vector reads
the record's first 20 bytes (a record is at least 32 long).  Every refused case was read along its path before it was put into
the catalogue (record_cases._refused_cases says what bounds its reads); none is there to make the device fault."""
import os

import numpy as np
import pytest

import record_cases as rc
from varlociraptor_amd import alignprops, engine, ingest, synth

pytestmark = pytest.mark.gpu

WHOLE = 1 << 20


@pytest.fixture(scope="module")
def cat():
    return rc.catalogue()


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as fh:
        fh.write(data)
    return p


def _dev(path, chunk=WHOLE, host_columns=True):
    rd = ingest.ObsReader([path] if isinstance(path, str) else path, chunk_records=chunk, device=0, host_columns=host_columns)
    out = []
    try:
        for b, sites in rd:
            if not host_columns:
                b.extra["native_table"].fetch_columns()
            out.append((b, sites))
    finally:
        rd.close()
    return out


@pytest.mark.parametrize("group", ["chain grid", "all halves", "flags and bit vectors", "scan"])
def test_accepted_cases_give_the_stated_table(cat, tmp_path, group):
    cs = cat.group(group)
    assert cs
    for i, c in enumerate(cs):                       # each case alone: a failure names it
        p = _write(tmp_path, "c%d.bcf" % i, c.data)
        rc.check_native(_dev(p), rc.table_of(c.expect), repr(c))
    data, expects = rc.file_of(cs)                   # the group as one file: other record offsets, many records per launch
    p = _write(tmp_path, "group.bcf", data)
    want = rc.table_of(expects)
    rc.check_native(_dev(p, WHOLE), want, group + ", whole")
    rc.check_native(_dev(p, 1), want, group + ", one record per request")
    rc.check_native(_dev(p, WHOLE, host_columns=False), want, group + ", columns fetched from the device")


def test_refused_cases_are_refused(cat, tmp_path):
    ok = cat.group("scan")[0]
    want_ok = rc.table_of(ok.expect + ok.expect)
    p = _write(tmp_path, "ok.bcf", rc.bcf_file(ok.records + ok.records))
    rc.check_native(_dev(p), want_ok, "two accepted records")
    for i, c in enumerate(cat.refused):
        p = _write(tmp_path, "r%d.bcf" % i, c.data)
        with pytest.raises(engine.EngineError):
            tables = _dev(p)
            raise AssertionError("%r was read: %d table(s)" % (c, len(tables)))
        # between two accepted records the read fails as well
        q = _write(tmp_path, "m%d.bcf" % i, rc.bcf_file(ok.records + c.records + ok.records))
        with pytest.raises(engine.EngineError):
            tables = _dev(q)
            raise AssertionError("%r between two accepted records was read: %d table(s)" % (c, len(tables)))


def test_bcf_decoys_take_the_serial_walk_and_the_control_does_not(cat, tmp_path):
    for i, c in enumerate(cat.decoys):
        p = _write(tmp_path, "d%d.bcf" % i, c.data)
        ingest.device_timings(reset=True)
        got = _dev(p, c.chunk or WHOLE)
        walks = ingest.device_timings(reset=True)["serial_walks"]
        print("%r: serial_walks %d, %d request(s)" % (c, walks, len(got)))
        rc.check_native(got, rc.table_of(c.expect), repr(c))
        if c.meta["control"]:
            assert walks == 0, c
        else:
            assert walks >= 1, c


def _same_counts(dev, cpu):
    assert np.array_equal(dev.transitions, cpu.transitions)
    assert dev.hops == cpu.hops and dev.insert_sizes == cpu.insert_sizes
    for k in ("max_del", "max_ins", "frac_max_softclip", "max_read_len", "max_mapq", "n_taken", "n_skipped", "n_not_usable", "n_softclips",
              "n_not_paired", "n_not_first", "n_mate_unmapped", "n_tid_mismatch"):
        assert getattr(dev, k) == getattr(cpu, k), k


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ref") / "ref.fa")
    alignprops.write_fasta(p, rc.bam_reference())
    return p


def test_bam_decoy_takes_the_serial_walk_and_the_control_does_not(cat, tmp_path, fasta):
    for i, c in enumerate(cat.bam):
        bam = _write(tmp_path, "b%d.bam" % i, c.data)
        cpu = alignprops.count_bams(fasta, [bam], 10 ** 9)
        dev = alignprops.count_bams_device(fasta, [bam], 10 ** 9, 0)
        print("%r: serial walks %d" % (c, dev.seconds[9]))
        _same_counts(dev, cpu)
        if c.meta["control"]:
            assert dev.seconds[9] == 0, c
        else:
            assert dev.seconds[9] >= 1, c
        for w in (40000, 1 << 17):                   # forced small windows: other boundaries, the same counts
            _same_counts(alignprops.count_bams_device(fasta, [bam], 10 ** 9, 0, window_bytes=w), cpu)


def _inflated_bytes(path):
    import gzip
    with gzip.open(path, "rb") as fh:
        return len(fh.read())


def _bcf_record_bytes(path):
    import gzip
    import struct
    with gzip.open(path, "rb") as fh:
        d = fh.read()
    return len(d) - 9 - struct.unpack_from("<I", d, 5)[0]


def test_ordinary_files_take_the_parallel_split(tmp_path, golden_dir, fasta):
    """If the plausibility test became too strict, every split would fall back to one lane walking the whole chunk and every other
    test would stay green: conforming files must end with the counter at 0."""
    b = synth.generate(synth.config3(), 2500, seed=31)
    paths = []
    for s in range(b.n_samples):
        p = str(tmp_path / ("s%d.bcf" % s))
        ingest.write_observations(p, b, s)
        paths.append(p)
    assert _inflated_bytes(paths[0]) > 100 * rc.SEG
    for chunk in (WHOLE, 333):
        ingest.device_timings(reset=True)
        n = sum(bt.n_loci for bt, _ in _dev(paths, chunk))
        t = ingest.device_timings(reset=True)
        assert n == 2500 and t["serial_walks"] == 0, (chunk, t["serial_walks"])
    normal = os.path.join(golden_dir, "flamegraph_profiling", "normal.bcf")
    if _bcf_record_bytes(normal) > rc.SEG:             # (its records span more than one segment)
        ingest.device_timings(reset=True)
        assert sum(bt.n_loci for bt, _ in _dev(normal)) > 0
        assert ingest.device_timings(reset=True)["serial_walks"] == 0
    bam = str(tmp_path / "plain.bam")
    alignprops.write_bam(bam, rc.BAM_CONTIGS, rc.plain_bam_records(4000, seed=9))
    assert _inflated_bytes(bam) > 4 * rc.SEG
    dev = alignprops.count_bams_device(fasta, [bam], 10 ** 9, 0)
    _same_counts(dev, alignprops.count_bams(fasta, [bam], 10 ** 9))
    assert dev.seconds[9] == 0
