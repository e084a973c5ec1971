"""Adds to a testcase already held under tests/golden/bam/<name>/ (tools/make_fragment_fixtures.py put it there with the FIRST record of
its candidates.vcf) ALL candidate alleles of its multi-allelic site as `alt_variants.tsv` (CHROM/POS/ID/REF/ALT per ALT allele, in file
order: data of the reference's testcase, nothing else), runs the site on the CPU — restatement with realignment of indel-bearing reads
(varlociraptor_amd/fragments.py) -> `fragments.pileup` -> oracle — without and with `alt_variants`, against the `expected:` block of
the testcase, and writes tests/golden/bam/ALTVARIANTS.md.  A case that misses is never adjusted for.  Run where the reference's
testcases are (the fixtures travel, the reference does not):

    python tools/make_altvariant_fixtures.py <testcases directory> test_giab_30
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DST = os.path.join(ROOT, "tests", "golden", "bam")

NOT_ADDED = [
    "| test_giab_25 | 1:1291 | two insertions (`AG`, `AGAG`) into an `AG` repeat | `NA12878 < 1.0` | not added: the block is met by almost any call, and the site is a "
    "repeat where the reference's `homopolymer_indel_len` and the read-inferred third allele (both not mirrored) take part |",
    "| test_giab_34 | 2:1123 | five deletions of 2 .. 13 `T` from a homopolymer of 26 | none (a crash test: \"previously led to a crash caused by likelihoods becoming all "
    "zero\") | not added: no block to meet, and a homopolymer site as above |",
]


def candidates_of(d):
    """[(contig, 0-based position, REF, ALT)] of <d>/alt_variants.tsv, in file order"""
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(d, "alt_variants.tsv")) if l.strip() and not l.startswith("#")]
    return [(r[0], int(r[1]) - 1, r[3].encode(), r[4].encode()) for r in rows]


def call_site(d, alt_variants, device="cpu", fasta=None):
    """per candidate allele of the site held in d: (observations, observations that support the allele, MAP VAF, PHRED by event);
    `fasta`: an indexed copy of the held ref.fa, which a device needs"""
    import bam_pairs as bp
    from oracle import oracle
    from varlociraptor_amd import cli, fragments
    bam, = glob.glob(os.path.join(d, "*.bam"))
    cand = candidates_of(d)
    pj = json.load(open(os.path.join(d, "properties.json")))
    spec = fragments.RealignSpec(64, "exact", *fragments.gap_hop_of(pj))
    tabs = fragments.observations(bam, fasta or os.path.join(d, "ref.fa"), cand, pj, device=device, realign=spec, alt_variants=alt_variants)
    batch, _ = fragments.pileup(tabs, cand)
    sc = cli.scenario_from_yaml(os.path.join(d, "scenario.yaml"), contig=cand[0][0])
    res = oracle.call(sc, batch)
    return [(len(t), int((t.prob_alt > t.prob_ref).sum()), float(res.map_vaf[k, 0]), bp.phred_by_event(sc, res.ln_posterior[k])) for k, t in enumerate(tabs)]


def main():
    from make_basecall_fixtures import expected_block, holds
    src, names = sys.argv[1], sys.argv[2:]
    from oracle import oracle
    oracle.build()
    lines = ["# Multi-allelic sites among the reference testcases (tools/make_altvariant_fixtures.py)", "",
             "Looked for: two or more candidate alleles at one `(CHROM, POS)` (one record with several ALTs, or adjacent records) in the `candidates.vcf` of every",
             "testcase of the reference (150 files).  Three have one: `test_giab_30`, `test_giab_25`, `test_giab_34`.  None of the fixtures held here had a second allele",
             "before; `alt_variants.tsv` of a case below holds all alleles of its site, `variant.tsv` keeps the first one for the tests that always read it.", "",
             "Restatement (`fragments.observations`, device=\"cpu\", realignment of indel-bearing reads, pair HMM mode `exact`, window 64) -> `fragments.pileup` -> oracle,",
             "all alleles of the site in one call, without and with `alt_variants`.  Per allele: observations, how many of them support the allele, MAP VAF.  `met`: every",
             "allele's call meets the testcase's `expected:` block.  Nothing is tuned.", "",
             "| testcase | site | alleles | expected | without `alt_variants` | with `alt_variants` | met |", "|---|---|---|---|---|---|---|"]
    for name in names:
        s, d = os.path.join(src, name), os.path.join(DST, name)
        recs = [l.rstrip("\n").split("\t")[:5] for l in open(os.path.join(s, "candidates.vcf")) if not l.startswith("#") and l.strip()]
        with open(os.path.join(d, "alt_variants.tsv"), "w") as out:
            out.write("#CHROM\tPOS\tID\tREF\tALT\n")
            for r in recs:
                for a in r[4].split(","):
                    out.write("\t".join(r[:4] + [a]) + "\n")
        freqs, posts = expected_block(os.path.join(s, "testcase.yaml"))
        cells, ok = [], True
        for flag in (False, True):
            got = call_site(d, flag)
            ok = ok and all(holds(freqs, posts, vaf, ph) for _, _, vaf, ph in got)
            cells.append("; ".join("%d, %d, %.4g" % g[:3] for g in got))
            print(name, "alt_variants" if flag else "alone", got)
        cand = candidates_of(d)
        lines.append("| %s | %s:%d | %s | `%s` | %s | %s | %s |" % (name, cand[0][0], cand[0][1] + 1, ", ".join("%s>%s" % (c[2].decode(), c[3].decode()) for c in cand),
                                                                "; ".join(freqs + posts), cells[0], cells[1], "yes" if ok else "no"))
    lines += NOT_ADDED
    lines += ["", "With `alt_variants` an MNV that has other alleles at its position realigns every enclosing read (mnv.rs:83), not only the reads with an I / D operation:",
              "that, and the reads that carry one of the other alleles, is where the two columns differ."]
    with open(os.path.join(DST, "ALTVARIANTS.md"), "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
