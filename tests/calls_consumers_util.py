"""Shared by the tests of `filter-calls posterior-odds` and `estimate mutational-burden`: the golden calls files with the events
they are filtered for, and the run-time edit that makes chosen records of the mutational-burden fixture coding."""
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TMB_VCF = os.path.join(GOLDEN, "mutational_burden", "annotated.vcf")
TMB_EVENTS = ["SOMATIC_TUMOR_LOW", "SOMATIC_TUMOR_MEDIUM", "SOMATIC_TUMOR_HIGH"]

# (file, events): every one of these headers passes the PHRED check
ODDS_CASES = [
    (os.path.join(GOLDEN, "flamegraph_profiling", "calls.bcf"), ["PRESENT"]),
    (os.path.join(GOLDEN, "fdr", "ev_2.bcf"), ["SOMATIC"]),
    (os.path.join(GOLDEN, "fdr", "ev_4.bcf"), ["SOMATIC_TUMOR"]),
    (os.path.join(GOLDEN, "fdr", "local1.bcf"), ["SOMATIC"]),
    (os.path.join(GOLDEN, "fdr", "local2.bcf"), ["SOMATIC"]),
    (os.path.join(GOLDEN, "fdr", "local2_smart.bcf"), ["SOMATIC"]),
    (os.path.join(GOLDEN, "fdr", "local3.bcf"), ["GERMLINE", "SOMATIC_TUMOR_LOW"]),
    # other events on the small files, so that they keep some records and drop others
    (os.path.join(GOLDEN, "flamegraph_profiling", "calls.bcf"), ["ABSENT"]),
    (os.path.join(GOLDEN, "fdr", "ev_4.bcf"), ["ABSENT"]),
    (os.path.join(GOLDEN, "fdr", "ev_4.bcf"), ["GERMLINE_HET", "GERMLINE_HOM"]),
    (os.path.join(GOLDEN, "fdr", "ev_2.bcf"), ["GERMLINE", "ABSENT"]),
]
ODDS_IDS = [os.path.basename(p) + ":" + "+".join(e) for p, e in ODDS_CASES]

CODING = (0, 2, 3, 5, 8, 13, 18, 19, 21, 30, 38)  # records made coding (fields 7 and 13 of the first ANN entry)
BIOTYPE_ONLY = (1, 20)                             # field 7 alone: field 13 stays empty, so still not coding


def edited_tmb_vcf(path, coding=CODING, biotype_only=BIOTYPE_ONLY, tumor_af=None):
    """Writes a copy of the fixture in which the first ANN entry of the chosen records is coding.  In the fixture field 13 (the
    protein position) is empty in every ANN entry, so setting field 7 to protein_coding alone does not pass is_valid_variant:
    the records of `coding` get both fields, those of `biotype_only` field 7 only.  tumor_af: {record index: AF text} to replace
    the tumor sample's AF (the fixture's are mostly 0)."""
    out, k = [], 0
    for line in open(TMB_VCF):
        if line.startswith("#"):
            out.append(line)
            continue
        f = line.rstrip("\n").split("\t")
        if k in coding or k in biotype_only:
            info = f[7].split(";")
            for i, kv in enumerate(info):
                if kv.startswith("ANN="):
                    entries = kv[4:].split(",")
                    fields = entries[0].split("|")
                    fields[7] = "protein_coding"
                    if k in coding:
                        fields[13] = "12/345"
                    entries[0] = "|".join(fields)
                    info[i] = "ANN=" + ",".join(entries)
            f[7] = ";".join(info)
        if tumor_af and k in tumor_af:
            keys = f[8].split(":")
            vals = f[10].split(":")
            vals[keys.index("AF")] = tumor_af[k]
            f[10] = ":".join(vals)
        out.append("\t".join(f) + "\n")
        k += 1
    with open(path, "w") as fh:
        fh.writelines(out)
    return k


TUMOR_AF = {0: "0.25", 2: "0.5", 3: "1", 5: "0.10101010101010101", 8: "0.3", 13: "0.75", 18: "0.2", 19: "0.05", 21: "0.9", 30: "0.15", 38: "0.6"}
