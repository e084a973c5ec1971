"""`python -m varlociraptor_amd call variants generic --scenario S.yaml --obs name=path.vcf ... [> calls.vcf]`
(also `filter-calls control-fdr`, `filter-calls posterior-odds` (odds.py), `estimate contamination` (contamination.py),
`estimate mutational-burden` (burden.py) and `preprocess variants` for SNV / MNV candidates (fragments.py))

Mirror of the reference's `call variants` surface (src/cli.rs:684-735) for text observation VCFs (format v15):
`generic` with a scenario YAML (grammar/mod.rs:129-144) and `tumor-normal --tumor --normal --purity`
(src/cli.rs:1151-1172).  Model evaluation runs on the GPU engine; there is no CPU path.
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict

from . import abi
# the driver lives in calldriver.py; what callers and tests reach through this module:
from .calldriver import (MODEL_MODE_MASK, CallChunk, CallProcessor, CandidateFilter, ContaminationCandidateFilter,  # noqa: F401
                         call_variants, model_modes)
from .scenario import Contamination, Inheritance, Sample, Scenario, Species, tumor_normal


def _contig_value(defn, contig: str, what: str):
    """PloidyDefinition / UniverseDefinition (grammar/mod.rs:280-312, 503-523): a plain value or a contig map with `all`."""
    if isinstance(defn, dict):
        if contig in defn:
            return defn[contig]
        if "all" in defn:
            return defn["all"]
        raise ValueError("%s for contig %r not found and no 'all' entry" % (what, contig))  # Ploidy/UniverseContigNotFound
    return defn


def _num(v):
    """YAML 1.1 (PyYAML) reads `1e-3` as a string, serde_yaml (the reference) as a float: accept both."""
    return None if v is None else float(v)


def scenario_from_yaml(path: str, contig: str = "all") -> Scenario:
    """Scenario as `Caller::configure_model` sees it on `contig` (calling.rs:632-718): contig maps of universes and
    ploidies and sex-specific species ploidies (grammar/mod.rs:314-345) are resolved here."""
    import yaml
    with open(path) as fh:
        y = yaml.safe_load(fh)
    species = None
    sp = y.get("species") or None
    if sp:
        vf = sp.get("variant-fractions", {}) or {}
        species = Species(heterozygosity=_num(sp.get("heterozygosity")), germline_mutation_rate=_num(sp.get("germline-mutation-rate")),
                          somatic_effective_mutation_rate=_num(sp.get("somatic-effective-mutation-rate")), ploidy=None,
                          fraction_indel=vf.get("indel", 0.0125), fraction_mnv=vf.get("mnv", 0.001), fraction_sv=vf.get("sv", 0.01))
    samples: Dict[str, Sample] = {}
    for name, sd in y["samples"].items():
        sd = sd or {}
        cont = sd.get("contamination")
        inh = sd.get("inheritance")
        inheritance = None
        if inh:
            if "mendelian" in inh:
                inheritance = Inheritance(abi.INHERIT_MENDELIAN, tuple(inh["mendelian"]["from"]))
            elif "clonal" in inh:
                inheritance = Inheritance(abi.INHERIT_CLONAL, (inh["clonal"]["from"],), bool(inh["clonal"]["somatic"]))
            elif "subclonal" in inh:
                inheritance = Inheritance(abi.INHERIT_SUBCLONAL, (inh["subclonal"]["from"],))
        universe = sd.get("universe")
        if universe is not None:
            universe = _contig_value(universe, contig, "universe")
        # Sample::contig_ploidy (grammar/mod.rs:581-593): the sample's own definition wins over the species'
        ploidy = sd.get("ploidy")
        if ploidy is not None:
            ploidy = int(_contig_value(ploidy, contig, "ploidy"))
        elif sp and sp.get("ploidy") is not None:
            pd = sp["ploidy"]
            if isinstance(pd, dict) and set(pd) <= {"male", "female"}:  # SexPloidyDefinition::Specific
                sex = sd.get("sex")
                if sex is None:
                    raise ValueError("sex specific ploidy definition found but no sex specified in sample %r" % name)
                if sex not in pd:
                    raise ValueError("ploidy definition for %s not found" % sex)
                pd = pd[sex]
            ploidy = int(_contig_value(pd, contig, "ploidy"))
        samples[name] = Sample(
            resolution=float(sd.get("resolution", 0.01)), universe=universe,
            contamination=Contamination(cont["by"], float(cont["fraction"])) if cont else None, ploidy=ploidy,
            somatic_effective_mutation_rate=_num(sd.get("somatic-effective-mutation-rate")),
            germline_mutation_rate=_num(sd.get("germline-mutation-rate")), inheritance=inheritance)
    sc = Scenario(samples, dict(y["events"]), species=species, expressions=dict(y.get("expressions") or {}))
    sc.validate()  # Scenario::vaftrees -> validate (grammar/mod.rs:206-279): OverlappingEvents
    return sc


def _write_kept(kept, reader, output, n_total):
    """The kept records of a filter-calls command: as BCF with the input's header, or a CHROM/POS/ID/REF/ALT table on stdout."""
    if output:
        from .bcfio import BcfWriter
        with BcfWriter(output, reader.header_text) as w:
            for rec in kept:
                w.write_raw(rec["raw"])
    else:
        print("#CHROM\tPOS\tID\tREF\tALT")
        for rec in kept:
            print("\t".join(str(rec[k]) for k in ("chrom", "pos", "id", "ref", "alt")))
    print(f"{len(kept)} of {n_total} records kept", file=sys.stderr)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="varlociraptor_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    call = sub.add_parser("call").add_subparsers(dest="what", required=True)
    variants = call.add_parser("variants")
    for flag, bit in (("--omit-strand-bias", abi.BIAS_STRAND), ("--omit-read-orientation-bias", abi.BIAS_ORIENTATION),
                      ("--omit-read-position-bias", abi.BIAS_POSITION), ("--omit-softclip-bias", abi.BIAS_SOFTCLIP),
                      ("--omit-homopolymer-artifact-detection", abi.BIAS_HOMOPOLYMER), ("--omit-alt-locus-bias", abi.BIAS_ALTLOCUS)):
        variants.add_argument(flag, action="store_const", const=bit, default=0)
    variants.add_argument("--full-prior", action="store_true")
    variants.add_argument("--device", type=int, default=0)
    variants.add_argument("--output", help="calls file (.bcf = BCF2, anything else text VCF; default stdout)")
    mode = variants.add_subparsers(dest="mode", required=True)
    g = mode.add_parser("generic")
    g.add_argument("--scenario", required=True)
    g.add_argument("--obs", nargs="+", required=True, metavar="NAME=PATH")
    t = mode.add_parser("tumor-normal")
    t.add_argument("--tumor", required=True)
    t.add_argument("--normal", required=True)
    t.add_argument("--purity", type=float, required=True)
    fc = sub.add_parser("filter-calls").add_subparsers(dest="what", required=True)
    cf = fc.add_parser("control-fdr")  # cli.rs FilterMethod::ControlFDR
    cf.add_argument("calls")
    cf.add_argument("--events", nargs="+", required=True)
    cf.add_argument("--fdr", type=float, required=True)
    cf.add_argument("--mode", choices=["local-smart", "local-strict", "global-smart", "global-strict"], default="local-smart")
    cf.add_argument("--smart-retain-artifacts", action="store_true")
    cf.add_argument("--var", choices=["SNV", "MNV", "INS", "DEL", "BND", "INV", "DUP", "REP"])
    cf.add_argument("--minlen", type=int)
    cf.add_argument("--maxlen", type=int)
    cf.add_argument("--device", default="cpu")
    cf.add_argument("--output", "-o", help="BCF file for the kept records (default: a CHROM/POS/ID/REF/ALT table on stdout)")
    po = fc.add_parser("posterior-odds", help="keep the alleles whose odds against the given events stay below --odds (cli.rs:812-824)")
    po.add_argument("calls")
    po.add_argument("--events", nargs="+", required=True)
    po.add_argument("--odds", choices=["none", "barely", "positive", "strong", "very-strong"], required=True, help="Kass-Raftery evidence at which an allele is removed")
    po.add_argument("--device", default="0", help="HIP device index, or 'cpu' for the Python restatement")
    po.add_argument("--output", "-o", help="BCF file for the kept records (default: a CHROM/POS/ID/REF/ALT table on stdout)")
    est = sub.add_parser("estimate").add_subparsers(dest="what", required=True)
    emb = est.add_parser("mutational-burden", help="expected coding variants per megabase by minimum VAF from annotated calls (cli.rs:493-530)")
    emb.add_argument("calls")
    emb.add_argument("--events", nargs="+", required=True)
    emb.add_argument("--sample", nargs="+", required=True, dest="samples")
    emb.add_argument("--coding-genome-size", type=float, default=3e7)
    emb.add_argument("--mode", choices=["hist", "curve", "multibar", "table"], required=True)
    emb.add_argument("--vaf-cutoff", type=float, default=0.2, help="minimum VAF of the multibar mode")
    emb.add_argument("--device", default="0", help="HIP device index, or 'cpu' for the Python restatement")
    emb.add_argument("--output", "-o", help="output file (default stdout)")
    ea = est.add_parser("alignment-properties", help="estimate insert size, CIGAR maxima, gap / homopolymer parameters and the wildtype "
                        "homopolymer error model of a sample (cli.rs:423-448)")
    ea.add_argument("reference", help="FASTA file of the reference genome (indexed with samtools faidx)")
    ea.add_argument("--bams", nargs="+", required=True, help="BAM files of one sample (or of samples prepared the same way)")
    ea.add_argument("--num-records", type=int, help="number of records to sample (default: from the BAM indices, which are then required)")
    ea.add_argument("--device", default="0", help="HIP device index, or 'cpu' for the pure-Python restatement")
    ec = est.add_parser("contamination", help="estimate the contamination of a sample by a contaminant (cli.rs:460-497)")
    ec.add_argument("--sample", required=True, help="observations of the presumably contaminated sample")
    ec.add_argument("--contaminant", required=True, help="observations of the presumably contaminating sample")
    ec.add_argument("--prior-estimate", type=float, help="prior estimate of the contamination (1 - purity); needs --prior-considered-cells")
    ec.add_argument("--prior-considered-cells", type=int, help="number of cells the prior estimate was made from")
    ec.add_argument("--output", help="posterior table (TSV; default stdout)")
    ec.add_argument("--output-plot", help="vega-lite plot of the prior and posterior densities of purity (JSON)")
    ec.add_argument("--output-max-vaf-variants", help="chrom,pos of the observations at the maximum MAP VAF (CSV)")
    ec.add_argument("--device", type=int, default=0)
    pre = sub.add_parser("preprocess").add_subparsers(dest="what", required=True)
    pv = pre.add_parser("variants", help="observations of SNV / MNV candidates from a BAM file, one per fragment (cli.rs:241-390)")
    pv.add_argument("reference", help="FASTA file of the reference genome")
    pv.add_argument("--candidates", required=True, help="candidate variants (VCF or BCF)")
    pv.add_argument("--bam", required=True)
    pv.add_argument("--alignment-properties", help="JSON of `estimate alignment-properties` (default: estimated from --bam on the device)")
    pv.add_argument("--atomic-candidate-variants", action="store_true", help="required: SNV / MNV candidates are scored from the read's alignment unless a flag below realigns")
    pv.add_argument("--omit-mapq-adjustment", action="store_true")
    pv.add_argument("--max-depth", type=int, default=200, help="loci above it are counted in a warning and processed whole")
    pv.add_argument("--score-indel-reads-from-alignment", action="store_true",
                    help="score a read with an insertion or deletion as it is aligned (the reference realigns it; without this flag or "
                    "--realign-indel-reads such a read is an error)")
    pv.add_argument("--realign-indel-reads", action="store_true",
                    help="realign a read with an insertion or deletion against the ref and the alt allele, as the reference does by default")
    pv.add_argument("--indel-candidates", action="store_true",
                    help="build deletion and insertion candidates too, one observation per fragment with the insert-size support of a deletion "
                    "(without it such a candidate is an error)")
    pv.add_argument("--methylation-read-type", choices=["converted", "annotated"],
                    help="build methylation candidates (ALT <METH>) too: 'converted' for bisulfite / EM-seq reads, 'annotated' for reads with "
                    "MM / ML tags (cli.rs:367-371; without it such a candidate is an error)")
    pv.add_argument("--alt-variants", action="store_true",
                    help="score a realigned read against the other ALT alleles at the candidate's (CHROM, POS) too, as the reference does: a read "
                    "that carries another allele of a multi-allelic site then counts against the candidate (without it every candidate is "
                    "scored as if it were alone at its position)")
    pv.add_argument("--indel-window", type=int, default=64, help="bases of a read realigned on either side of the candidate (at most 64, cli.rs:877)")
    pv.add_argument("--pairhmm-mode", choices=["exact", "fast", "homopolymer"], default="exact")
    pv.add_argument("--device", default="0", help="HIP device index, or 'cpu' for the Python restatement")
    pv.add_argument("--output", required=True, help="observation BCF")
    a = ap.parse_args(argv)
    import os
    if a.cmd == "preprocess":
        from . import fragments
        if a.realign_indel_reads and a.score_indel_reads_from_alignment:
            ap.error("--realign-indel-reads and --score-indel-reads-from-alignment exclude each other")
        if not 1 <= a.indel_window <= fragments.MAX_INDEL_WINDOW:
            ap.error("--indel-window must be 1 .. %d" % fragments.MAX_INDEL_WINDOW)
        try:
            n = fragments.preprocess_variants(a.reference, a.candidates, a.bam, a.output, a.alignment_properties, "cpu" if a.device == "cpu" else int(a.device),
                                              a.atomic_candidate_variants, a.omit_mapq_adjustment, a.max_depth, a.score_indel_reads_from_alignment,
                                              warn=lambda m: print(f"[WARN] {m}", file=sys.stderr),
                                              realign=fragments.RealignSpec(a.indel_window, a.pairhmm_mode) if a.realign_indel_reads else None,
                                              indel_candidates=fragments.RealignSpec(a.indel_window, a.pairhmm_mode) if a.indel_candidates else None,
                                              methylation_readtype=a.methylation_read_type, alt_variants=a.alt_variants)
        except (fragments.PreprocessError, fragments.FragPileupError, fragments.InvalidReadOrientationInfo, fragments.EngineError) as e:
            print(f"error: {e}", file=sys.stderr)
            sys.exit(1)
        print(f"{n} records written", file=sys.stderr)
        return
    if a.cmd == "call" and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        # one process per GPU (torchrun): `nccl` is RCCL on ROCm; VLR_DIST_BACKEND=gloo for hosts with fewer GPUs than ranks
        import torch
        import torch.distributed as tdist
        backend = os.environ.get("VLR_DIST_BACKEND", "nccl")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        a.device = local % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(a.device)
        tdist.init_process_group(backend, **({"device_id": torch.device("cuda", a.device)} if backend == "nccl" else {}))
    if a.cmd == "estimate" and a.what == "alignment-properties":
        from . import alignprops
        if a.num_records is not None and a.num_records < 0:
            ap.error("--num-records must not be negative")
        rc = alignprops.run_cli(a.reference, a.bams, a.num_records, "cpu" if a.device == "cpu" else int(a.device))
        if rc:
            sys.exit(rc)
        return
    if a.cmd == "estimate" and a.what == "mutational-burden":
        from . import burden
        out = open(a.output, "w") if a.output else None
        try:
            burden.estimate(a.calls, a.events, a.samples, a.coding_genome_size, a.mode, cutoff=a.vaf_cutoff, device=a.device, out=out)
        finally:
            if out:
                out.close()
        return
    if a.cmd == "estimate":
        # cli.rs:1292-1298: both prior options or neither, and at least one cell
        if (a.prior_estimate is None) != (a.prior_considered_cells is None) or (a.prior_considered_cells is not None and a.prior_considered_cells <= 0):
            ap.error("invalid prior contamination estimate: give --prior-estimate together with --prior-considered-cells > 0")
        from . import contamination
        prior = (a.prior_estimate, a.prior_considered_cells) if a.prior_estimate is not None else None
        contamination.estimate_contamination(a.sample, a.contaminant, output=a.output, output_plot=a.output_plot,
                                             output_max_vaf_variants=a.output_max_vaf_variants, prior_estimate=prior, device=a.device)
        return
    if a.cmd == "filter-calls" and a.what == "posterior-odds":
        from . import odds
        from .bcfio import BcfReader
        min_level = odds.LEVELS.index(a.odds)
        if a.output and a.device != "cpu" and os.environ.get("VLR_INGEST", "native") != "python":
            # the whole command in the engine (vlr_calls_filter_odds): BCF in, kept records out, decisions on the device
            kept_n, total_n = odds.filter_calls_native(a.calls, a.output, a.events, min_level, device=odds._device_index(a.device))
            print(f"{kept_n} of {total_n} records kept", file=sys.stderr)
            return
        r = BcfReader(a.calls)
        recs = list(r)
        kept = odds.filter_by_odds(recs, r.header_lines, a.events, min_level, device=a.device)
        _write_kept(kept, r, a.output, len(recs))
        return
    if a.cmd == "filter-calls":
        from . import fdr
        vartype = None
        if a.var:
            rng = (a.minlen or 0, a.maxlen if a.maxlen is not None else 1 << 62) if (a.minlen is not None or a.maxlen is not None) else None
            vartype = (a.var, rng)
        if a.output and str(a.device).startswith("cuda") and os.environ.get("VLR_INGEST", "native") != "python":
            # the whole command in the engine (vlr_calls_filter_fdr): BCF in, kept records out, threshold search on the device
            dev = int(str(a.device).split(":")[1]) if ":" in str(a.device) else 0
            kept_n, total_n = fdr.filter_calls_native(a.calls, a.output, a.events, a.fdr, vartype=vartype, local=a.mode.startswith("local"),
                                                      smart=a.mode.endswith("smart"), smart_retain_artifacts=a.smart_retain_artifacts, device=dev)
            print(f"{kept_n} of {total_n} records kept", file=sys.stderr)
            return
        from .bcfio import BcfReader
        r = BcfReader(a.calls)
        recs = list(r)
        tags = [l.split("ID=")[1].split(",")[0] for l in r.header_lines if l.startswith("##INFO") and "ID=PROB_" in l]
        kept = fdr.control_fdr(recs, a.events, a.fdr, vartype=vartype, local=a.mode.startswith("local"), smart=a.mode.endswith("smart"),
                               smart_retain_artifacts=a.smart_retain_artifacts, header_tags=tags, device=a.device)
        # utils::filter_calls (filtration/fdr.rs:58-62, utils/mod.rs:288-374): the kept records go out as BCF with the input's
        # header.  Records pass through in their original encoding (calls written by `call variants` carry one ALT per record,
        # so there are no ALT alleles to trim; a multi-ALT record is kept whole when any of its alleles is kept).
        _write_kept(kept, r, a.output, len(recs))
        return
    omit = (a.omit_strand_bias | a.omit_read_orientation_bias | a.omit_read_position_bias | a.omit_softclip_bias |
            a.omit_homopolymer_artifact_detection | a.omit_alt_locus_bias)
    if a.mode == "generic":
        full_prior = a.full_prior

        def sc(contig, _path=a.scenario):
            r = scenario_from_yaml(_path, contig)
            r.full_prior = full_prior
            return r
        obs = dict(kv.split("=", 1) for kv in a.obs)
    else:
        sc = tumor_normal(a.purity)
        obs = {"tumor": a.tumor, "normal": a.normal}
    if not callable(sc):
        sc.full_prior = a.full_prior
    call_variants(sc, obs, omit_mask=omit, device=a.device, output=a.output)


if __name__ == "__main__":
    main()
