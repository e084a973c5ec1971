"""Copies the DATA of single-sample SNV / MNV reference testcases into tests/golden/bam/<name>/ — the BAM, ref.fa and scenario.yaml
verbatim, variant.tsv = CHROM/POS/ID/REF/ALT of the first record of candidates.vcf — after running each one on the CPU:
restatement (varlociraptor_amd/basecalls.py) -> pileup -> oracle, against the `expected:` block of its testcase.yaml.  A case whose call
meets the block is copied; every case gets an entry in tests/golden/bam/BASECALLS.md with its expectation, the call obtained and,
where it misses, the likely reason.  Run where the reference's testcases are (the fixtures travel, the reference does not):

    python tools/make_basecall_fixtures.py <testcases directory> test_giab_03 test_giab_07 ...
"""
import glob
import os
import re
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DST = os.path.join(ROOT, "tests", "golden", "bam")


def expected_block(path):
    """the expressions of `expected: allelefreqs / posteriors` of a testcase.yaml"""
    freqs, posts, mode = [], [], None
    inside = False
    for line in open(path):
        if line.startswith("expected:"):
            inside = True
            continue
        if inside:
            if line.strip() and not line.startswith(" "):
                break
            s = line.strip()
            if s.startswith("allelefreqs"):
                mode = freqs
            elif s.startswith("posteriors"):
                mode = posts
            elif s.startswith("- ") and mode is not None:
                mode.append(s[2:].strip())
    return freqs, posts


def holds(freqs, posts, vaf, phred):
    ok = True
    for e in freqs:
        m = re.match(r"^\S+\s*(==|!=|<=|>=|<|>)\s*([0-9.eE+-]+)$", e)
        ok &= bool(eval("%r %s %s" % (vaf, m.group(1), m.group(2))))
    for e in posts:
        ok &= bool(eval(e, {"__builtins__": {}}, dict(phred)))
    return ok


def call_case(src, name):
    import bam_pairs as bp
    from oracle import oracle
    from varlociraptor_amd import basecalls, cli
    d = os.path.join(src, name)
    bam, = glob.glob(os.path.join(d, "*.bam"))
    rec = [l for l in open(os.path.join(d, "candidates.vcf")) if not l.startswith("#")][0].rstrip("\n").split("\t")[:5]
    cand = [(rec[0], int(rec[1]) - 1, rec[3].encode(), rec[4].encode())]
    sup = basecalls.allele_supports(bam, os.path.join(d, "ref.fa"), cand, device="cpu")
    batch = basecalls.pileup(sup, cand)
    sc = cli.scenario_from_yaml(os.path.join(d, "scenario.yaml"), contig=rec[0])
    res = oracle.call(sc, batch)
    return bam, rec, len(sup[0]), float(res.map_vaf[0, 0]), bp.phred_by_event(sc, res.ln_posterior[0])


def main():
    src, names = sys.argv[1], sys.argv[2:]
    from oracle import oracle
    oracle.build()
    lines = ["# SNV / MNV testcases scored from their BAM (tools/make_basecall_fixtures.py)", "",
             "Restatement -> `basecalls.pileup` -> oracle on the CPU, one observation per fragment, no artifact hypotheses, no `max_depth`, every",
             "read scored from its alignment (`realign_indel_reads=False`).  `kept`: the call meets the testcase's own `expected:` block and the",
             "data is held here; tests/basecall_cases.py restates the block as a predicate.", "",
             "| testcase | variant | fragments | expected | MAP VAF obtained | kept |", "|---|---|---|---|---|---|"]
    for name in names:
        freqs, posts = expected_block(os.path.join(src, name, "testcase.yaml"))
        bam, rec, n, vaf, phred = call_case(src, name)
        ok = holds(freqs, posts, vaf, phred)
        what = "; ".join(freqs + posts)
        shown = {k: round(v, 4) for k, v in phred.items() if any(k in p for p in posts)}
        note = "yes" if ok else "no — likely: reads with indel operations are realigned by the reference (`realign_indel_reads`), no artifact hypotheses, no `max_depth`"
        lines.append("| %s | %s:%s %s>%s | %d | `%s` | %.4g %s | %s |" % (name, rec[0], rec[1], rec[3], rec[4], n, what, vaf, shown if shown else "", note))
        print(name, rec, "fragments", n, "vaf", vaf, shown, "OK" if ok else "MISS")
        if not ok:
            continue
        d = os.path.join(DST, name)
        os.makedirs(d, exist_ok=True)
        for f in (bam, os.path.join(src, name, "ref.fa"), os.path.join(src, name, "scenario.yaml")):
            shutil.copyfile(f, os.path.join(d, os.path.basename(f)))
        with open(os.path.join(d, "variant.tsv"), "w") as out:
            out.write("#CHROM\tPOS\tID\tREF\tALT\n" + "\t".join(rec) + "\n")
    with open(os.path.join(DST, "BASECALLS.md"), "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
