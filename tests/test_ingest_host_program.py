"""The parsers of the front door under the sanitizers (no GPU): csrc/vlr_ingest_host.cpp links the host units vlr_bgzf.cpp, vlr_ingest.cpp
and vlr_callsfile.cpp — BGZF members, the BCF2 container, bincode vectors, VCF text — into a stand-alone program built with
-fsanitize=address,undefined (nothing is preloaded into any process).  It runs over the fixtures, where its digest of the observation
table must be the one computed here from ingest.read_observations, and over damaged copies of them, where every input must end in a
digest or in the library's error text: never in a sanitizer report, a device entry point or a signal."""
import glob
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import host_program
from varlociraptor_amd import abi, ingest

OBS = ["normal.bcf", "normal.vcf"]
# the per-byte pass, which reads its input thousands of times, runs on the header and the leading records up to this many inflated
# bytes, two records at the least (fdr/ev_2.bcf inflates to 6.7 MB): a record is parsed on its own, and what damage to the first one
# does to the framing shows at the record right behind it and at the end of the file.  Truncations and the zeroed block take the whole file.
DAMAGE_BYTES = 16 << 10


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_ingest_host", extra_sources=("vlr_bgzf.cpp", "vlr_ingest.cpp", "vlr_callsfile.cpp"),
                              libs=("-lz", "-ldl", "-lpthread"))


def calls_files(golden_dir):
    return [os.path.join(golden_dir, "flamegraph_profiling", "calls.bcf")] + sorted(glob.glob(os.path.join(golden_dir, "fdr", "*.bcf")))


def run(program, mode, *args):
    """[(input name, exit code of the input, its output lines)] of one run; fails on anything but a clean end of the process"""
    r = subprocess.run([program, mode] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    out = []
    for line in r.stdout.split("\n"):
        if line.startswith("@"):
            out.append([line[1:], None, []])
        elif line.startswith("="):
            out[-1][1] = int(line[1:])
        elif line:
            out[-1][2].append(line)
    last = out[-1][0] if out else "(none)"
    assert r.returncode in (0, 2) and not r.stderr, "exit %d at input %s of %s\n%s" % (r.returncode, last, args, r.stderr[-3000:])
    assert all(code in (0, 2) for _, code, _ in out), out[-1]
    assert r.returncode == max([code for _, code, _ in out] + [0])
    return out


def check_outcome(mode, name, code, lines):
    """exit 0 with a digest (whose passes agree), or exit 2 with the library's error text"""
    if code == 2:
        assert re.match(r"error -?\d+: \S", lines[-1]), (name, lines)
        return
    if mode == "obs":
        assert [l.split()[0] for l in lines] == ["whole", "stream1", "stream7"], (name, lines)
        assert len({l.split(" ", 1)[1] for l in lines}) == 1, (name, lines)
    else:
        assert [l.split()[0] for l in lines] == ["plain", "ann_af"], (name, lines)
        assert lines[1].startswith("ann_af " + lines[0].split(" ", 1)[1] + " n_ann="), (name, lines)


def table_digest(path):
    """the program's digest of the table of one observation file, from ingest.read_observations (vlr_ingest_host.cpp says what it covers)"""
    batch, sites = ingest.read_observations([path], threads=2)
    arrays = [np.diff(batch.obs_offset.astype(np.int64)).astype(np.uint32)]
    arrays += [batch.columns[name] for name, _ in abi.OBS_COLUMNS]   # the nine columns, then flags
    arrays += [batch.extra["third_allele_evidence"]]
    arrays += [batch.locus[name] for name, _ in abi.LOCUS_COLUMNS]
    arrays += [sites.pos, sites.heterozygosity_ln, sites.somatic_effective_mutation_rate_ln, sites.imprecise, sites.group_key]
    crcs = [zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]
    text = b"".join(s.encode() + b"\0" for l in range(len(sites)) for s in (sites.chrom(l), sites.record_id(l), sites[l][2], sites[l][3]))
    crcs.append(zlib.crc32(text))
    assert len(crcs) == 22
    return "n_loci=%d n_obs=%d checksum=%08x" % (batch.n_loci, batch.n_obs, zlib.crc32(struct.pack("<22I", *crcs)))


@pytest.mark.parametrize("name", OBS)
def test_observation_digest_equals_the_library_s(program, golden_dir, name):
    """vlr_obs_read and the streaming reader at 1 and 7 records per call, compiled for the sanitizers, give the table libvlr.so gives"""
    path = os.path.join(golden_dir, "flamegraph_profiling", name)
    (_, code, lines), = run(program, "obs", path)
    assert code == 0, lines
    want = table_digest(path)
    assert lines == ["%s %s" % (p, want) for p in ("whole", "stream1", "stream7")]


def test_calls_files_are_read_the_same_with_and_without_ann_af(program, golden_dir):
    """open_calls + read_call_records, variant_types and tags_prob_sum over every record of every calls fixture"""
    files = calls_files(golden_dir)
    out = run(program, "calls", *files)
    assert [n for n, _, _ in out] == files
    for name, code, lines in out:
        assert code == 0, (name, lines)
        check_outcome("calls", name, code, lines)
        n = int(re.search(r"n_records=(\d+)", lines[0]).group(1))
        assert n > 0 and "n_variants=%d n_sums=%d " % (n, n) in lines[0], (name, lines)   # single-ALT records, every one typed
    # the AF values are read when asked for: one per record and sample in the fixture of the end-to-end run
    assert out[0][2][1].endswith(" n_ann=0 n_af=11")


def inflated(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def damage_base(raw):
    """the header and the leading records of an inflated file; (bytes, [start, end) of the first record)"""
    if raw[:5] != b"BCF\2\2":
        k = next(m.start() + 1 for m in re.finditer(b"\n", raw) if raw[m.start() + 1:m.start() + 2] not in (b"#", b""))
        e = raw.index(b"\n", k) + 1
        return raw[:raw.index(b"\n", e) + 1], (k, e)   # (text: the header lines and two records)
    p = first = 9 + struct.unpack("<I", raw[5:9])[0]
    ends = []
    while p + 8 <= len(raw) and (len(ends) < 2 or p <= DAMAGE_BYTES):
        ls, li = struct.unpack("<II", raw[p:p + 8])
        p += 8 + ls + li
        ends.append(p)
    keep = max([e for e in ends if e <= DAMAGE_BYTES] + ends[:2])
    return raw[:keep], (first, ends[0])


def truncations(n):
    return sorted(set(list(range(64)) + [n // 2, n - 37]))


@pytest.mark.parametrize("mode,rel", [("obs", "flamegraph_profiling/" + n) for n in OBS] +
                         [("calls", "flamegraph_profiling/calls.bcf")] + [("calls", "fdr/" + n) for n in
                                                                         ("ev_2.bcf", "ev_4.bcf", "local1.bcf", "local2.bcf", "local2_smart.bcf", "local3.bcf")])
def test_damaged_inputs_end_in_a_digest_or_an_error_text(program, golden_dir, tmp_path, mode, rel):
    """Truncation at each of the first 64 bytes, at the middle and 37 bytes before the end — of the inflated bytes written as an
    uncompressed file, and of the BGZF file itself —, 64 zeroed bytes at one third, and over the first record each byte in turn set
    to 0xff: exit 0 with a digest or exit 2 with the library's error text, whatever the damage."""
    path = os.path.join(golden_dir, rel)
    whole = inflated(path)
    prefix, (r0, r1) = damage_base(whole)
    files = []

    def case(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        files.append(p)

    for k in truncations(len(whole)):
        case("cut%d" % k, whole[:k])
    third = len(whole) // 3
    case("zero", whole[:third] + bytes(64) + whole[third + 64:])
    blob = open(path, "rb").read()
    if blob[:2] == b"\x1f\x8b":
        for k in truncations(len(blob)):
            case("bgzf_cut%d" % k, blob[:k])
    out = run(program, mode, *files)
    assert [n for n, _, _ in out] == [str(f) for f in files]
    for name, code, lines in out:
        check_outcome(mode, name, code, lines)
    # a file that ends inside its magic, its header or a record is refused (the uncompressed copy cut at a record boundary is a file)
    refused = {os.path.basename(n) for n, code, _ in out if code == 2}
    assert {"cut%d" % k for k in range(1, 64)} | {"cut%d" % (len(whole) // 2), "cut%d" % (len(whole) - 37)} <= refused
    case("first_record", prefix)
    out = run(program, mode, files[-1], "ff", r0, r1)
    assert [n for n, _, _ in out] == [str(o) for o in range(r0, r1)]
    for name, code, lines in out:
        check_outcome(mode, name, code, lines)
    assert any(code == 2 for _, code, _ in out) and (mode == "calls" or any(code == 0 for _, code, _ in out))


def test_header_line_cut_in_front_of_its_body_is_no_dictionary_entry(program, tmp_path):
    """Found by the truncations of normal.vcf: a ##FILTER / ##INFO / ##FORMAT / ##contig line without its '<' made parse_header take a
    substring at npos, and the exception left the library through its C ABI.  Such a line is skipped now."""
    files = []
    for i, line in enumerate(("##INFO", "##INFO=", "##FILTER=ID=x", "##FORMAT=", "##contig=", "##contig=ID=1")):
        files.append(tmp_path / ("h%d.vcf" % i))
        files[-1].write_text("##fileformat=VCFv4.2\n" + line)
    for name, code, lines in run(program, "obs", *files):
        assert code == 2 and "invalid observation format" in lines[-1], (name, lines)
    ok = tmp_path / "ok.vcf"
    ok.write_text("##fileformat=VCFv4.2\n##varlociraptor_observation_format_version=15\n##INFO=\n##contig=\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    (_, code, lines), = run(program, "obs", ok)
    assert code == 0 and lines[0].startswith("whole n_loci=0 n_obs=0 "), lines
