"""Copies the DATA that tests/fragment_cases.py needs of single-sample SNV / MNV reference testcases into tests/golden/bam/<name>/ and
runs each one on the CPU: restatement (varlociraptor_amd/fragments.py) -> `fragments.pileup` -> oracle, against the `expected:` block of
its testcase.yaml.  For every case it writes `properties.json` (the `properties:` string of the sample in testcase.yaml, verbatim), and
— only where the directory does not hold them yet, files that are there stay untouched — the BAM, ref.fa, scenario.yaml and variant.tsv
(CHROM/POS/ID/REF/ALT of the first record of candidates.vcf).  Every case gets a row in tests/golden/bam/FRAGMENTS.md with its
expectation, the observations formed, the MAP VAF obtained and, where it misses, the likely reason; a case that misses is never
adjusted for.  Run where the reference's testcases are (the fixtures travel, the reference does not):

    python tools/make_fragment_fixtures.py <testcases directory> test_giab_07 test_giab_30 ...
"""
import glob
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DST = os.path.join(ROOT, "tests", "golden", "bam")


def properties_string(path):
    """the `properties:` value of the (single) sample of a testcase.yaml"""
    import yaml
    y = yaml.safe_load(open(path))
    sample, = y["samples"].values()
    return sample["properties"]


def call_case(d, omit_mapq_adjustment=False):
    """(candidate record, observations, MAP VAF, PHRED by event) of the case held in directory d (with properties.json)"""
    import bam_pairs as bp
    from oracle import oracle
    from varlociraptor_amd import cli, fragments
    bam, = glob.glob(os.path.join(d, "*.bam"))
    rec = open(os.path.join(d, "variant.tsv")).read().split("\n")[1].split("\t")
    cand = [(rec[0], int(rec[1]) - 1, rec[3].encode(), rec[4].encode())]
    props = json.load(open(os.path.join(d, "properties.json")))
    tabs = fragments.observations(bam, os.path.join(d, "ref.fa"), cand, props, device="cpu", omit_mapq_adjustment=omit_mapq_adjustment)
    batch, _ = fragments.pileup(tabs, cand)
    sc = cli.scenario_from_yaml(os.path.join(d, "scenario.yaml"), contig=rec[0])
    res = oracle.call(sc, batch)
    return rec, len(tabs[0]), float(res.map_vaf[0, 0]), bp.phred_by_event(sc, res.ln_posterior[0])


def main():
    from make_basecall_fixtures import expected_block, holds
    src, names = sys.argv[1], sys.argv[2:]
    from oracle import oracle
    oracle.build()
    lines = ["# SNV / MNV testcases as fragments from their BAM (tools/make_fragment_fixtures.py)", "",
             "Restatement (`fragments.observations`, device=\"cpu\") -> `fragments.pileup` -> oracle on the CPU: one observation per fragment from all",
             "valid records in the window, fragment features and artifact hypotheses on, the MAPQ adjustment on, no `max_depth`, every read scored",
             "from its alignment (no realignment of indel-bearing reads).  `met`: the call meets the testcase's own `expected:` block;",
             "tests/fragment_cases.py restates the block as a predicate.  The last column is the MAP VAF with `--omit-mapq-adjustment`.", "",
             "| testcase | variant | observations | expected | MAP VAF obtained | met | without the adjustment |", "|---|---|---|---|---|---|---|"]
    for name in names:
        s = os.path.join(src, name)
        d = os.path.join(DST, name)
        os.makedirs(d, exist_ok=True)
        bam, = glob.glob(os.path.join(s, "*.bam"))
        rec = [l for l in open(os.path.join(s, "candidates.vcf")) if not l.startswith("#")][0].rstrip("\n").split("\t")[:5]
        for f in (bam, os.path.join(s, "ref.fa"), os.path.join(s, "scenario.yaml")):
            if not os.path.exists(os.path.join(d, os.path.basename(f))):
                shutil.copyfile(f, os.path.join(d, os.path.basename(f)))
        if not os.path.exists(os.path.join(d, "variant.tsv")):
            with open(os.path.join(d, "variant.tsv"), "w") as out:
                out.write("#CHROM\tPOS\tID\tREF\tALT\n" + "\t".join(rec) + "\n")
        with open(os.path.join(d, "properties.json"), "w") as out:
            out.write(properties_string(os.path.join(s, "testcase.yaml")) + "\n")
        freqs, posts = expected_block(os.path.join(s, "testcase.yaml"))
        rec, n, vaf, phred = call_case(d)
        _, _, vaf_omit, phred_omit = call_case(d, omit_mapq_adjustment=True)
        ok = holds(freqs, posts, vaf, phred)
        shown = {k: round(v, 4) for k, v in phred.items() if any(k in p for p in posts)}
        note = "yes" if ok else ("no — likely: " + ("the MAPQ adjustment (met without it)" if holds(freqs, posts, vaf_omit, phred_omit) else
                                                    "reads with indel operations are realigned by the reference, no `max_depth`"))
        lines.append("| %s | %s:%s %s>%s | %d | `%s` | %.4g %s | %s | %.4g |" % (name, rec[0], rec[1], rec[3], rec[4], n, "; ".join(freqs + posts), vaf, shown if shown else "",
                                                                               note, vaf_omit))
        print(name, rec, "observations", n, "vaf", vaf, shown, "OK" if ok else "MISS", "omit:", vaf_omit)
    with open(os.path.join(DST, "FRAGMENTS.md"), "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
