"""Copies the DATA of reference testcases (one sample, or several: each sample with its own BAM and properties) with a plain deletion / insertion candidate into tests/golden/bam/<name>/ (the
BAM, ref.fa, scenario.yaml, variant.tsv = CHROM/POS/ID/REF/ALT of the first record of candidates.vcf, properties.json = the
`properties:` string of the sample, verbatim; files that are there stay untouched) and runs each one, and the cases that are already
there, on the CPU: restatement (`fragments.observations`, device="cpu", indel_candidates) -> `fragments.pileup` -> oracle, per
fragment (validity rule, mate merge, insert-size support, prob_sample_alt), and — from the same realigned members — per read (one
observation per overlapping member that carries a strand, prob_sample_alt = ln 1, no artifact hypotheses: what `bam_pairs.
single_end_pileup` forms), against the `expected:` block of the testcase.yaml.  Every case gets a row in tests/golden/bam/INDELS.md; a
case that misses is never adjusted for.  Run where the reference's testcases are (the fixtures travel, the reference does not):

    python tools/make_indel_fragment_fixtures.py <testcases directory> test59 test_giab_08 issue_154 test_false_negative_indel_call test_giab_06 test_giab_12
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


def samples_of(d):
    """[(sample name or None, BAM, properties)] of the case held in directory d: one sample with properties.json, or one per
    properties.<sample>.json with <sample>.bam"""
    if os.path.exists(os.path.join(d, "properties.json")):
        bam, = glob.glob(os.path.join(d, "*.bam"))
        return [(None, bam, json.load(open(os.path.join(d, "properties.json"))))]
    out = []
    for p in sorted(glob.glob(os.path.join(d, "properties.*.json"))):
        sample = os.path.basename(p)[len("properties."):-len(".json")]
        out.append((sample, os.path.join(d, sample + ".bam"), json.load(open(p))))
    return out


def scenario_of(d, name, contig, names):
    """(scenario, omit_bias_mask) of the case: its scenario.yaml, or the embedded tumor-normal scenario with the purity and the omitted
    biases that case.json took from the testcase.yaml"""
    from varlociraptor_amd import abi, cli
    from varlociraptor_amd.scenario import tumor_normal
    for p in (os.path.join(d, "scenario.yaml"), os.path.join(ROOT, "tests", "golden", "testcases", name, "scenario.yaml")):
        if os.path.exists(p):
            return cli.scenario_from_yaml(p, **({"contig": contig} if contig in names else {})), 0
    case = json.load(open(os.path.join(d, "case.json")))
    bits = {"strand": abi.BIAS_STRAND, "read_orientation": abi.BIAS_ORIENTATION, "read_position": abi.BIAS_POSITION, "softclip": abi.BIAS_SOFTCLIP,
            "homopolymer": abi.BIAS_HOMOPOLYMER, "alt_locus": abi.BIAS_ALTLOCUS}
    mask = 0
    for k in case.get("omit", []):
        mask |= bits[k]
    return tumor_normal(float(case["purity"])), mask


def candidate_of(d):
    rec = open(os.path.join(d, "variant.tsv")).read().split("\n")[1].split("\t")
    return rec, [(rec[0], int(rec[1]) - 1, rec[3].encode(), rec[4].encode())]


def spec_of(pj):
    from varlociraptor_amd import fragments
    return fragments.RealignSpec(64, "exact", *fragments.gap_hop_of(pj))


def join_samples(batches):
    """the batch of one locus with the samples' pileups one behind the other (obs_offset index = locus * n_samples + sample)"""
    import numpy as np
    from varlociraptor_amd import abi
    from varlociraptor_amd.batch import PileupBatch
    if len(batches) == 1:
        return batches[0]
    off = np.concatenate(([0], np.cumsum([b.n_obs for b in batches]))).astype(np.uint32)
    cols = {k: np.concatenate([b.columns[k] for b in batches]) for k, _ in abi.OBS_COLUMNS}
    return PileupBatch(len(batches), off, cols, {k: batches[0].locus[k] for k, _ in abi.LOCUS_COLUMNS})


def sample_order(sc, samples):
    """the samples in the scenario's order"""
    if len(samples) == 1:
        return samples
    by = {s[0]: s for s in samples}
    return [by[k] for k in sc.samples]


def phreds(sc, row):
    """{"PROB_<EVENT>": PHRED} of a posterior row: column 0 = absent, then the scenario's events, the last one = artifact (include/vlr.h)"""
    import math
    import bam_pairs as bp
    ph = bp.phred_by_event(sc, row)
    tiny = lambda v: -10.0 * float(v) / math.log(10.0)
    ph["PROB_ABSENT"] = tiny(row[0])
    if len(row) > 1 + len(sc.event_names):
        ph["PROB_ARTIFACT"] = tiny(row[1 + len(sc.event_names)])
    return ph


def vafs_of(sc, samples, res):
    return {(s[0] if s[0] is not None else "sample"): float(res.map_vaf[0, k]) for k, s in enumerate(samples)}


def vaf_text(vafs):
    """the MAP VAFs as INDELS.md writes them"""
    return "%.4g" % list(vafs.values())[0] if len(vafs) == 1 else ",".join("%s=%.4g" % (k, v) for k, v in sorted(vafs.items()))


def met(freqs, posts, vafs, phred):
    """does the call meet the `expected:` block?  allelefreqs name the sample (a single-sample case: whatever name stands there)"""
    class Names(dict):
        def __missing__(self, k):
            if len(vafs) == 1:
                return list(vafs.values())[0]
            raise KeyError(k)
    ok = True
    for e in freqs:
        ok &= bool(eval(e.replace("&&", " and ").replace("||", " or "), {"__builtins__": {}}, Names(vafs)))
    for e in posts:
        ok &= bool(eval(e.replace("&&", " and ").replace("||", " or "), {"__builtins__": {}}, dict(phred, inf=float("inf"))))
    return ok


def fragment_tables(d, sample, device="cpu", fasta=None):
    """the processed pileup of the case's candidate in one sample (name, BAM, properties), per fragment"""
    from varlociraptor_amd import fragments
    _, cand = candidate_of(d)
    return fragments.observations(sample[1], fasta or os.path.join(d, "ref.fa"), cand, sample[2], device=device, indel_candidates=spec_of(sample[2]))


def call_case(name, device="cpu", fasta=None):
    """(candidate record, {"fragment" | "read": (observations, {sample: MAP VAF}, PHRED by event)}) of the case held in
    tests/golden/bam/<name>; every sample is preprocessed on its own with its own properties.  `device`: where the per-fragment
    tables are formed (the per-read column is always the restatement); `fasta`: a copy of the case's ref.fa with its index, which the
    kernels read through (the fixtures hold the reference without one)"""
    import numpy as np
    import bam_pairs as bp
    from oracle import oracle
    from varlociraptor_amd import alignprops, fragments, readwindows as rw, realign
    d = os.path.join(DST, name)
    rec, cand = candidate_of(d)
    samples = samples_of(d)
    names = [c for c, _ in alignprops.bam_header(alignprops.inflate_bgzf(samples[0][1]), samples[0][1])[0]]
    sc, omit = scenario_of(d, name, rec[0], names)
    samples = sample_order(sc, samples)
    out = {}
    tabs = [fragment_tables(d, s, device, fasta) for s in samples]
    batch = join_samples([fragments.pileup(t, cand, omit)[0] for t in tabs])
    res = oracle.call(sc, batch)
    out["fragment"] = (sum(len(t[0]) for t in tabs), vafs_of(sc, samples, res), phreds(sc, res.ln_posterior[0]))
    # per read: the same realigned members, each overlapping one on its own
    seqs = rw.read_fasta(os.path.join(d, "ref.fa"))
    site = fragments.indel_site(seqs[rec[0]], names.index(rec[0]), cand[0][1], cand[0][2], cand[0][3], 64, name)
    loc = site.locus
    batches, n = [], 0
    for _, bam, pj in samples:
        recs = rw.read_bam(bam)[1]
        rs = fragments.restate_indel(recs, [site], fragments.props_of(pj), False, spec_of(pj), {site.ref_id: seqs[rec[0]].upper()})
        keep = [e for e in rs.evidences if not e.ev.status and rw.overlaps(recs[e.ev.record], site.start, site.end)]
        sup = [realign.normalize_support(e.ln_ref, e.ln_alt) for e in keep]
        pile = bp.IndelCase(loc.kind, loc.start, loc.end, loc.len_diff, loc.alt_allele, [(recs[e.ev.record], None, None, None) for e in keep])
        batches.append(bp.single_end_pileup(pile, np.array([a for _, a in sup]), np.array([r for r, _ in sup])))
        n += len(keep)
    res = oracle.call(sc, join_samples(batches))
    out["read"] = (n, vafs_of(sc, samples, res), phreds(sc, res.ln_posterior[0]))
    return rec, out


def copy_case(s, d, name):
    """the data of testcase directory s into fixture directory d; files that are there stay untouched"""
    import yaml
    y = yaml.safe_load(open(os.path.join(s, "testcase.yaml")))
    os.makedirs(d, exist_ok=True)
    have_scenario = any(os.path.exists(p) for p in (os.path.join(d, "scenario.yaml"), os.path.join(ROOT, "tests", "golden", "testcases", name, "scenario.yaml")))
    files = [os.path.join(s, "ref.fa")] + ([os.path.join(s, "scenario.yaml")] if not have_scenario else [])
    single = len(y["samples"]) == 1
    for sample, v in y["samples"].items():
        if single:
            if not glob.glob(os.path.join(d, "*.bam")):
                files.append(os.path.join(s, v["path"]))
            pp = os.path.join(d, "properties.json")
        else:
            if not os.path.exists(os.path.join(d, sample + ".bam")):
                shutil.copyfile(os.path.join(s, v["path"]), os.path.join(d, sample + ".bam"))
            pp = os.path.join(d, "properties.%s.json" % sample)
        if not os.path.exists(pp):
            with open(pp, "w") as out:
                out.write(v["properties"] + "\n")
    for f in files:
        if os.path.exists(f) and not os.path.exists(os.path.join(d, os.path.basename(f))):
            shutil.copyfile(f, os.path.join(d, os.path.basename(f)))
    if y.get("mode") == "TumorNormal" and not os.path.exists(os.path.join(d, "case.json")):   # settings of the testcase.yaml, as data
        omit = [k[len("omit_"):-len("_bias")] for k in y if k.startswith("omit_") and k.endswith("_bias") and y[k]]
        with open(os.path.join(d, "case.json"), "w") as out:
            json.dump({"mode": "tumor-normal", "purity": y["purity"], "omit": omit}, out)
            out.write("\n")
    if not os.path.exists(os.path.join(d, "variant.tsv")):
        rec = [l for l in open(os.path.join(s, "candidates.vcf")) if not l.startswith("#")][0].rstrip("\n").split("\t")[:5]
        with open(os.path.join(d, "variant.tsv"), "w") as out:
            out.write("#CHROM\tPOS\tID\tREF\tALT\n" + "\t".join(rec) + "\n")


def main():
    from make_basecall_fixtures import expected_block
    from varlociraptor_amd import fragments
    src, names = sys.argv[1], sys.argv[2:]
    from oracle import oracle
    oracle.build()
    lines = ["# Deletion / insertion testcases as fragments from their BAM (tools/make_indel_fragment_fixtures.py)", "",
             "Restatement (`fragments.observations`, device=\"cpu\", `indel_candidates`) -> `fragments.pileup` -> oracle on the CPU, pair HMM mode",
             "`exact`, window 64, gap / homopolymer parameters of the sample's properties; every sample of a case is preprocessed on its own with",
             "its own properties and the samples are called together with the testcase's scenario.  *per fragment*: one observation per fragment",
             "with the validity rule, the mate merge, the insert-size support of a deletion and `prob_sample_alt`.  *per read*: one observation per",
             "overlapping realigned record that carries a strand, `prob_sample_alt` = ln 1, no artifact hypotheses.  `met`: the call meets the",
             "testcase's own `expected:` block (an empty block is met by any call).  Observations are summed over the samples.  Nothing is tuned.", "",
             "| testcase | candidate | expected | per read: observations, MAP VAF, met | per fragment: observations, MAP VAF, met |", "|---|---|---|---|---|"]
    for name in names:
        s, d = os.path.join(src, name), os.path.join(DST, name)
        copy_case(s, d, name)
        rec, _ = candidate_of(d)
        freqs, posts = expected_block(os.path.join(s, "testcase.yaml"))
        head = "| %s | %s:%s %s>%s | `%s` |" % (name, rec[0], rec[1], rec[3], rec[4], "; ".join(freqs + posts))
        try:
            rec, got = call_case(name)
        except (fragments.FragPileupError, fragments.PreprocessError) as e:   # what the path refuses is a row too
            lines.append("%s refused | refused: %s |" % (head, str(e).replace("|", "/")))
            print(name, "refused:", e)
            continue
        cells = []
        for how in ("read", "fragment"):
            n, vafs, phred = got[how]
            ok = met(freqs, posts, vafs, phred)
            shown = {k: round(v, 4) for k, v in phred.items() if any(k in p for p in posts)}
            cells.append("%d, %s %s, %s" % (n, vaf_text(vafs), shown if shown else "", "yes" if ok else "no"))
            print(name, how, n, vafs, shown, "OK" if ok else "MISS")
        lines.append("%s %s | %s |" % (head, cells[0], cells[1]))
    with open(os.path.join(DST, "INDELS.md"), "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
