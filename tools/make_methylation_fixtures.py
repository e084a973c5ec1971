"""Copies the DATA of the reference's methylation testcases into tests/golden/bam/<name>/ — the BAM, ref.fa, scenario.yaml,
properties.json (the `properties:` string of the sample, verbatim), variant.tsv (CHROM / POS / ID / REF / ALT of the first record of
candidates.vcf), recorded.json (the recorded observation columns of that record, decoded by obsfmt.decode_record_info: what the
reference wrote when the testcase was made) and case.json (the read type of the testcase's options and its `expected:` lines); files
that are there stay untouched — and runs each case, and the cases that are already there, on the CPU: restatement
(`methylation.tables`, device="cpu") -> `fragments.pileup` -> oracle.  tests/golden/bam/METHYLATION.md gets, per case, the observation
count against the recorded one, the largest deviation of the f32-coded prob_ref / prob_alt values from the recordings (sorted
multisets after the writer's MiniLogProb coding; the f16-coded ones must be equal), and whether the call meets `expected:`; a case that
misses is never adjusted for.  Run where the reference's testcases are (the fixtures travel, the reference does not):

    python tools/make_methylation_fixtures.py <testcases directory> test_prinz_call_meth_1 test_prinz_call_meth_2 test_prinz_af_scan test_mapq_meth test_prinz_pacbio_zero
"""
import glob
import json
import os
import re
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DST = os.path.join(ROOT, "tests", "golden", "bam")
CASES = ("test_prinz_call_meth_1", "test_prinz_call_meth_2", "test_prinz_af_scan", "test_mapq_meth", "test_prinz_pacbio_zero")


def copy_case(s, d):
    import yaml
    from make_basecall_fixtures import expected_block
    from varlociraptor_amd import obsfmt
    y = yaml.safe_load(open(os.path.join(s, "testcase.yaml")))
    os.makedirs(d, exist_ok=True)
    (sample, v), = y["samples"].items()
    for f in ("ref.fa", "scenario.yaml", v["path"]):
        if not os.path.exists(os.path.join(d, os.path.basename(f))):
            shutil.copyfile(os.path.join(s, f), os.path.join(d, os.path.basename(f)))
    if not os.path.exists(os.path.join(d, "properties.json")):
        with open(os.path.join(d, "properties.json"), "w") as out:
            out.write(v["properties"] + "\n")
    line = [l for l in open(os.path.join(s, "candidates.vcf")) if not l.startswith("#")][0].rstrip("\n").split("\t")
    if not os.path.exists(os.path.join(d, "variant.tsv")):
        with open(os.path.join(d, "variant.tsv"), "w") as out:
            out.write("#CHROM\tPOS\tID\tREF\tALT\n" + "\t".join(line[:5]) + "\n")
    if not os.path.exists(os.path.join(d, "recorded.json")):
        info = dict(kv.split("=", 1) if "=" in kv else (kv, "") for kv in line[7].split(";"))
        cols = obsfmt.decode_record_info(info)
        rec = {k: [None if x != x else (float(x) if abs(float(x)) != float("inf") else ("-inf" if x < 0 else "inf")) for x in cols[k].astype(float)]
               for k in ("prob_mapping", "prob_ref", "prob_alt", "prob_missed_allele", "prob_sample_alt", "prob_double_overlap", "prob_hit_base")}
        rec["flags"] = [int(x) for x in cols["flags"]]
        with open(os.path.join(d, "recorded.json"), "w") as out:
            json.dump(rec, out)
            out.write("\n")
    if not os.path.exists(os.path.join(d, "case.json")):
        freqs, posts = expected_block(os.path.join(s, "testcase.yaml"))
        readtype = re.search(r'"methylation_readtype":"([A-Za-z]+)"', v["options"]).group(1).lower()
        with open(os.path.join(d, "case.json"), "w") as out:
            json.dump({"mode": "generic", "sample": sample, "methylation_readtype": readtype, "expected": {"allelefreqs": freqs, "posteriors": posts}}, out)
            out.write("\n")


def load_case(name):
    """(directory, BAM, properties, candidate record, case settings, recorded columns) of a held case"""
    d = os.path.join(DST, name)
    bam, = glob.glob(os.path.join(d, "*.bam"))
    rec = open(os.path.join(d, "variant.tsv")).read().split("\n")[1].split("\t")
    recorded = json.load(open(os.path.join(d, "recorded.json")))
    for k in recorded:
        if k != "flags":
            recorded[k] = [float(x) if x is not None else float("nan") for x in recorded[k]]
    return d, bam, json.load(open(os.path.join(d, "properties.json"))), rec, json.load(open(os.path.join(d, "case.json"))), recorded


def case_tables(name, device="cpu", accept_any_flag=False):
    """(candidate, processed pileup) of a held case"""
    from varlociraptor_amd import alignprops, methylation
    d, bam, pj, rec, case, _ = load_case(name)
    names = [c for c, _ in alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)[0]]
    cand = [(rec[0], int(rec[1]) - 1, rec[3].encode(), rec[4].encode())]
    tab, = methylation.tables(bam, [methylation.MethLocus(names.index(rec[0]), int(rec[1]) - 1)], pj, case["methylation_readtype"], device, accept_any_flag=accept_any_flag)
    return cand, tab


def deviation(tab, recorded):
    """(f16-coded values all equal?, largest absolute deviation of the f32-coded ones, the column it stands in) of prob_ref / prob_alt
    against the recordings, as sorted multisets after the writer's MiniLogProb coding; None when the counts differ"""
    import numpy as np
    from varlociraptor_amd.synth import minilogprob_round
    if len(tab) != len(recorded["prob_ref"]):
        return None
    mine = sorted(zip(minilogprob_round(tab.prob_ref).astype(float), minilogprob_round(tab.prob_alt).astype(float)))
    theirs = sorted(zip(recorded["prob_ref"], recorded["prob_alt"]))
    f16_equal, worst, where = True, 0.0, ""
    for (mr, ma), (tr, ta) in zip(mine, theirs):
        for col, m, t in (("prob_ref", mr, tr), ("prob_alt", ma, ta)):
            if m == t:
                continue
            if float(np.float16(t)) == t and t < -10.0:      # an f16-coded recording
                f16_equal = False
            d = abs(m - t) if np.isfinite(m) and np.isfinite(t) else float("inf")
            if d > worst:
                worst, where = float(d), col
    return f16_equal, worst, where


def call(name, cand, tab):
    """(MAP VAFs, PHRED by event, met?) of the case's call through the oracle"""
    from make_indel_fragment_fixtures import met, phreds, scenario_of, vafs_of
    from oracle import oracle
    from varlociraptor_amd import fragments
    d, _, _, rec, case, _ = load_case(name)
    sc, omit = scenario_of(d, name, rec[0], [rec[0]])
    res = oracle.call(sc, fragments.pileup([tab], cand, omit)[0])
    vafs = vafs_of(sc, [(case["sample"],)], res)
    ph = phreds(sc, res.ln_posterior[0])
    return vafs, ph, met(case["expected"]["allelefreqs"], case["expected"]["posteriors"], vafs, ph)


def main():
    from oracle import oracle
    oracle.build()
    src, names = sys.argv[1], (sys.argv[2:] or list(CASES))
    lines = ["# Methylation testcases from their BAM (tools/make_methylation_fixtures.py)", "",
             "Restatement (`methylation.tables`, device=\"cpu\") -> `fragments.pileup` -> oracle on the CPU, with the read type of the testcase's",
             "options.  *observations*: ours / the recorded ones of candidates.vcf (`recorded.json`).  *deviation*: prob_ref / prob_alt against the",
             "recordings as sorted multisets after the writer's MiniLogProb coding — are the f16-coded values equal, and the largest absolute",
             "difference of the f32-coded ones.  The annotated case's recordings predate the flag rule `read_invalid`: its row compares",
             "with `accept_any_flag=True`, and states the count under the rule as the source has it.  `met`: the call (rule as the source",
             "has it) meets the testcase's own `expected:` block.  Nothing is tuned.", "",
             "Each case directory holds the BAM, `ref.fa` and `scenario.yaml` verbatim, `properties.json` = the `properties:` string of the sample,",
             "`variant.tsv`, `recorded.json` = the observation columns that the testcase's `candidates.vcf` holds for the candidate, decoded, and",
             "`case.json` = the read type of the testcase's options and its `expected:` lines.  Used by `tests/test_methylation_host.py` and",
             "`tests/test_gpu_methylation.py`.", "",
             "| testcase | candidate | read type | observations | f16-coded equal | largest f32 deviation | expected | MAP VAF | met |", "|---|---|---|---|---|---|---|---|---|"]
    worst_all = 0.0
    for name in names:
        copy_case(os.path.join(src, name), os.path.join(DST, name))
        _, _, _, rec, case, recorded = load_case(name)
        annotated = case["methylation_readtype"] == "annotated"
        cand, tab = case_tables(name)
        cmp_tab = case_tables(name, accept_any_flag=True)[1] if annotated else tab
        dev = deviation(cmp_tab, recorded)
        vafs, ph, ok = call(name, cand, tab)
        n_text = "%d / %d" % (len(cmp_tab), len(recorded["prob_ref"])) + (" (%d with `read_invalid`)" % len(tab) if annotated else "")
        exp = "; ".join(case["expected"]["allelefreqs"] + case["expected"]["posteriors"])
        if dev is None:
            lines.append("| %s | %s:%s | %s | %s | counts differ | | `%s` | %.4g | %s |" % (name, rec[0], rec[1], case["methylation_readtype"], n_text, exp, list(vafs.values())[0], "yes" if ok else "no"))
        else:
            worst_all = max(worst_all, dev[1])
            lines.append("| %s | %s:%s | %s | %s | %s | %.3g%s | `%s` | %.4g | %s |" % (name, rec[0], rec[1], case["methylation_readtype"], n_text, "yes" if dev[0] else "NO", dev[1],
                                                                                  " (%s)" % dev[2] if dev[2] else "", exp, list(vafs.values())[0], "yes" if ok else "no"))
        print(lines[-1])
    lines += ["", "Largest f32 deviation over the cases: %.3g; tests/test_methylation_host.py allows twice that." % worst_all,
              "", "MAX_F32_DEVIATION = %r" % float(worst_all)]
    with open(os.path.join(DST, "METHYLATION.md"), "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
