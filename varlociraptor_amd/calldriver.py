"""The driver behind `call variants` (calling.rs:296-741 of the reference): `call_variants` reads observation files a chunk at a
time, evaluates every chunk on the GPU engine and hands the calls to the native calls writer or to a CallProcessor.

The parts, in the order a run meets them: `Switches` (the environment, read once per call), `ModelCache` (one scenario per contig and
model mode), `PlanCache` (one engine plan per scenario signature), `Evaluator` (the results of one chunk), `Pipeline` (reader
thread, evaluation loop, writer thread), the endings `finish_sharded` / `finish_single`, and `call_python`, the Python restatement
of the same path.  cli.py re-exports what callers use.
"""
from __future__ import annotations

import copy
import json
import os
import queue
import sys
import tempfile
import threading
import time
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from . import abi, callsfmt, dist as vdist, engine, ingest as vingest, obsfmt
from .batch import CallResults
from .scenario import Scenario

# model_mode of the reference (calling.rs:413-418): (check_read_orientation_bias, check_read_position_bias, check_softclip_bias,
# check_homopolymer_artifact_detection).  check_strand_bias and the alt-locus check are NOT part of it: a precise indel and an
# imprecise SV of one contig share a model, its `last_rid` and therefore the variant-specific prior of the contig's first record.
MODEL_MODE_MASK = abi.BIAS_ORIENTATION | abi.BIAS_POSITION | abi.BIAS_SOFTCLIP | abi.BIAS_HOMOPOLYMER

FIELDS = ("ln_posterior", "ln_marginal", "map_vaf", "map_bias", "best_event", "status", "afd_count", "afd_vaf", "afd_lnprob")


def model_modes(locus_flags):
    return (np.asarray(locus_flags) & MODEL_MODE_MASK).astype(int)


def _scenario_signature(sc: Scenario):
    return tuple((n, s.universe, s.ploidy) for n, s in sc.samples.items()) + (sc.variant_heterozygosity_ln, sc.variant_somatic_effective_mutation_rate_ln)


def _contig_mode(key, contig_names):
    """(contig name, model mode) of a record key `contig index * 256 + mode`"""
    return contig_names[int(key) // 256] if contig_names else "all", int(key) % 256


class CallChunk:
    """What a CallProcessor sees of one chunk of records, in input order: the pileups (`batch`), the site columns (`sites`:
    contig, pos, ref / alt through sites.ref(l) ...), the results (`results`: ln_posterior[l][k] for out_names[k], map_vaf,
    map_bias, status, AFD lists) and `loci`, the indices of these records within the chunk the reader delivered."""

    def __init__(self, batch, sites, results, out_names, sample_names, loci, offset=0):
        self.batch, self.sites, self.results, self.out_names, self.sample_names, self.loci = batch, sites, results, out_names, sample_names, loci
        self.offset = offset   # records of the file(s) delivered before this chunk: offset + loci = record numbers


class CallProcessor:
    """Plug point of the driver, calling.rs:964-975 (`CallProcessor{setup, process_call, finalize}`): what is done with the calls.
    The default (processor=None) is the reference's CallWriter (calling.rs:977-1006): the calls file.  `estimate contamination`
    (estimation/contamination.rs:371-399) plugs a collector in here.  process_calls is the batched form of process_call: one
    invocation per chunk of the streaming reader, records in input order."""

    def setup(self, out_names, sample_names):
        return None

    def process_calls(self, chunk: "CallChunk"):
        raise NotImplementedError

    def finalize(self):
        return None


class CandidateFilter:
    """calling.rs:1008-1020 (`CandidateFilter::filter(work_item, sample_names) -> bool`), vectorised over a chunk: returns a boolean
    array, True = the record is processed (evaluated and handed to the processor), False = skipped as in calling.rs:409."""

    def filter(self, batch, sites, sample_names):
        return np.ones(batch.n_loci, bool)


class ContaminationCandidateFilter(CandidateFilter):
    """estimation/contamination.rs:404-428: SNVs whose contaminant pileup has >= 10 observations that are all ref support
    (prob_ref > prob_alt, read_observation.rs:439-441) and whose sample pileup has >= 10 observations with at least one strong
    alt support (Bayes factor alt:ref above 20, read_observation.rs:429-432)."""

    def filter(self, batch, sites, sample_names):
        S = batch.n_samples
        ci, si = list(sample_names).index("contaminant"), list(sample_names).index("sample")
        off = batch.obs_offset.astype(np.int64)
        pa, pr = batch.columns["prob_alt"].astype(np.float64), batch.columns["prob_ref"].astype(np.float64)
        ref_support = pr > pa
        with np.errstate(invalid="ignore"):   # (-inf) - (-inf)
            strong_alt = (pa - pr) > np.log(20.0)
        cs = np.concatenate([[0], np.cumsum(~ref_support)])
        sa = np.concatenate([[0], np.cumsum(strong_alt)])
        L = batch.n_loci
        c0, c1 = off[np.arange(L) * S + ci], off[np.arange(L) * S + ci + 1]
        s0, s1 = off[np.arange(L) * S + si], off[np.arange(L) * S + si + 1]
        has_snv = (batch.locus["locus_flags"] & abi.LOCUS_HAS_SNV) != 0
        return has_snv & (c1 - c0 >= 10) & (cs[c1] - cs[c0] == 0) & (s1 - s0 >= 10) & (sa[s1] - sa[s0] > 0)


class _PinnedResults:
    """Result buffers of one chunk carved out of recycled page-locked blocks (engine.host_array): the AFD lists of a chunk are hundreds of
    megabytes — allocating and first-touching them per chunk costs more than the kernel, and from page-locked memory the device
    copies them by direct DMA."""

    def __init__(self):
        self.free, self.lock = [], threading.Lock()

    def results(self, n_loci, n_out, n_samples, afd_capacity, afd_text_capacity=0):
        need = (n_loci * (8 * (n_out + 1 + n_samples) + abi.N_BIAS + 8) + (n_loci * n_samples * (4 + 16 * afd_capacity) if afd_capacity else 0)
                + (afd_text_capacity + n_loci * n_samples * 8 if afd_capacity else 0) + 64 * 16)
        block = None
        with self.lock:
            for i, b in enumerate(self.free):
                if b.size >= need:
                    block = self.free.pop(i)
                    break
            if block is None and len(self.free) >= 4:
                self.free.pop(0)
        if block is None:
            block = engine.host_array(int(need * 1.15) + 4096, np.uint8)
        at = 0

        def alloc(shape, dtype):
            nonlocal at
            n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
            off = at
            at = (off + n + 63) & ~63
            return block[off:off + n].view(dtype).reshape(shape)
        res = CallResults(n_loci, n_out, n_samples, afd_capacity, alloc=alloc, afd_text_capacity=afd_text_capacity)
        res._pool_block = block
        return res

    def release(self, res):
        block = getattr(res, "_pool_block", None)
        if block is not None:
            res._pool_block = None
            with self.lock:
                self.free.append(block)


_RESULT_POOL = None


def _shared_result_pool():
    global _RESULT_POOL
    if _RESULT_POOL is None:
        _RESULT_POOL = _PinnedResults()
    return _RESULT_POOL


def _fixed_fields(res):
    """Copy of the fixed-size result fields (the AFD lists stay with the chunk's own buffers)."""
    out = CallResults(res.n_loci, res.n_out, res.n_samples, 0)
    for f in FIELDS[:6]:
        getattr(out, f)[...] = getattr(res, f)
    return out


def _part_path(output: str, rank: int) -> str:
    """Part file of a sharded run (ends in .bcf: the native writer picks the container by the suffix)."""
    return "%s.part%d.bcf" % (output, rank)


class _CrossesShards(Exception):
    """a chunk of a sharded run holds records whose evaluation needs records of other shards"""


@dataclass(frozen=True)
class Switches:
    """The environment switches of the driver, read once per call_variants call (never at import: tests set them just before)."""
    native: bool                 # VLR_INGEST=native (default; the `ingest` argument wins): the native streaming driver; else the Python restatement
    host_reader: bool            # VLR_INGEST_HOST=1: the host reader even for files the device reader takes
    sharded: bool                # VLR_INGEST_SHARDED=0 keeps the older multi-rank path (every rank reads everything, results all-gathered)
    summaries: bool              # VLR_INGEST_SUMMARIES=0: the calls writer reads the host columns instead of the device's pileup summaries
    afd_text: bool               # VLR_AFD_TEXT=0: AFD lists come down as numbers only, no FORMAT/AFD text from the device
    chunk: int                   # VLR_CLI_CHUNK: records per reader request (0: the reader's own rule)
    queue: int                   # VLR_CLI_QUEUE: chunks that may wait between two stages of the pipeline (2)
    shard_report: Optional[str]  # VLR_INGEST_SHARD_REPORT: path prefix of what each rank of a sharded run read (tests, tools)

    @classmethod
    def from_env(cls, ingest: str = None) -> "Switches":
        env = os.environ.get
        return cls(native=(ingest or env("VLR_INGEST", "native")) == "native", host_reader=env("VLR_INGEST_HOST", "0") != "0",
                   sharded=env("VLR_INGEST_SHARDED", "1") != "0", summaries=env("VLR_INGEST_SUMMARIES", "1") != "0",
                   afd_text=env("VLR_AFD_TEXT", "1") != "0", chunk=int(env("VLR_CLI_CHUNK", "0")), queue=int(env("VLR_CLI_QUEUE", "2")),
                   shard_report=env("VLR_INGEST_SHARD_REPORT") or None)


class ModelCache:
    """The scenario of every (contig, model mode) of a run.  `scenario`: a Scenario, or a callable contig -> Scenario.
    The reference keeps one model (and one `last_rid`) per model mode = the tuple of check_* flags of the work item
    (calling.rs:414-443): each mode installs the variant-specific prior of ITS first record on a contig."""

    def __init__(self, scenario, obs_paths: Dict[str, str]):
        self.scenario, self.obs_paths = scenario, obs_paths
        self.per_contig = scenario if callable(scenario) else (lambda contig: scenario)
        self.scen: Dict[tuple, Scenario] = {}
        self.first_of_contig: Dict[tuple, tuple] = {}
        # samples are ordered by name (BTreeMap, grammar/mod.rs:137), independent of the contig
        self.sample_order = scenario.sample_names if not callable(scenario) else sorted(obs_paths)
        if not callable(scenario):   # the sample-name checks, before anything is opened
            self.resolve("all")
            self.scen.clear()

    def resolve(self, contig, mode=0):
        key = (contig, mode)
        if key not in self.scen:
            sc = self.per_contig(contig)
            if callable(self.scenario) or key in self.first_of_contig:
                sc = copy.copy(sc)
            # variant-specific priors are installed with the contig's model, from its first record (calling.rs:643-713)
            het, som = self.first_of_contig.get(key, (None, None))
            if het is not None:
                sc.variant_heterozygosity_ln = het
            if som is not None:
                sc.variant_somatic_effective_mutation_rate_ln = som
            for name in sc.sample_names:
                if name not in self.obs_paths:
                    raise SystemExit("no observations given for sample %r" % name)
            for name in self.obs_paths:
                if name not in sc.sample_names:
                    raise SystemExit("invalid observation sample name %r" % name)  # errors::Error::InvalidObservationSampleName
            self.scen[key] = sc
        return self.scen[key]

    def record_first(self, key, contig_names, het, som):
        """Remember the prior overrides of the first record of every (contig, mode) among `key` that was not seen before."""
        for k_, first in zip(*np.unique(key, return_index=True)):
            self.first_of_contig.setdefault(_contig_mode(k_, contig_names), (
                None if het[first] != het[first] else float(het[first]), None if som[first] != som[first] else float(som[first])))

    def header_for(self, names, contigs):
        scenario0 = self.resolve(contigs[0] if contigs else "all")
        return callsfmt.header(names or scenario0.out_names(), scenario0.sample_names, sorted(set(contigs))), scenario0


class PlanCache:
    """One plan per scenario signature, kept across the chunks of a run.  A plan owns device buffers (staging slots, scratch rows,
    AFD log): keep a handful."""

    def __init__(self, device: int = 0, afd_capacity: int = 0, plan_class=None):
        self.plans: Dict[tuple, "engine.Plan"] = {}
        self.device, self.afd_capacity, self.plan_class = device, afd_capacity, plan_class or engine.Plan
        self.reserve_loci = 0   # request size of an open device reader

    def get(self, sig, sc):
        if sig not in self.plans:
            while len(self.plans) >= 4:
                self.plans.pop(next(iter(self.plans))).close()
            self.plans[sig] = self.plan_class(sc, device=self.device)
            if self.reserve_loci:   # size the plan's buffers once for the reader's request size: no growth (hipFree + hipMalloc) between chunks
                self.plans[sig].reserve(self.reserve_loci, self.afd_capacity)
        return self.plans[sig]

    def close_all(self):
        for p_ in self.plans.values():
            p_.close()
        self.plans.clear()


def scatter(res, r, loci):
    """Rows of the sub-result `r` go to the records `loci` of the chunk's result."""
    for f in FIELDS:
        a = getattr(res, f)
        if a is not None:
            a[loci] = getattr(r, f)


def fan_out(res, group_rep):
    """Every record of a group gets the result of the group's representative."""
    for f in FIELDS:
        a = getattr(res, f)
        if a is not None:
            a[:] = a[group_rep]


def carry_breakends(res, group_key, carried: Dict[int, dict]):
    """Breakend events whose first record sat in an EARLIER chunk of the streaming reader: the reference hands the first breakend's
    event probabilities and sample infos to every later record of the event across the whole file (calling.rs:569-580,
    726-741); `carried`: key = vlr_obs_sites.group_key, value = that record's result row."""
    for l in np.nonzero(group_key != 0)[0]:
        k_ = int(group_key[l])
        row = carried.get(k_)
        if row is None:   # first record of the event in the file (a representative of this chunk)
            carried[k_] = {f: np.array(getattr(res, f)[l]) for f in FIELDS if getattr(res, f) is not None}
        else:             # the event began in an earlier chunk: its first record's result
            for f, v in row.items():
                getattr(res, f)[l] = v


def warn_hard_status(status):
    """the reference panics on NaN (assert!(!p.is_nan())): say so instead of writing `.` silently"""
    hard = status & (abi.LOCUS_NAN | abi.LOCUS_UNDERFLOW | abi.LOCUS_TABLE_FULL | abi.LOCUS_TOO_DEEP)
    for bit, what in ((abi.LOCUS_NAN, "a likelihood became NaN"), (abi.LOCUS_UNDERFLOW, "an observation likelihood is outside the f64 range"),
                      (abi.LOCUS_TABLE_FULL, "visited-point table overflow"), (abi.LOCUS_TOO_DEEP, "pileup above the LDS budget and the deep pool")):
        n_bad = int(((hard & bit) != 0).sum())
        if n_bad:
            print("warning: %d record(s) without a result: %s" % (n_bad, what), file=sys.stderr)


def regroup_representatives(group_key):
    """Representatives among the records a candidate filter left: the first kept record of every group (key 0: no group)."""
    rep = np.arange(len(group_key))
    first_of: Dict[int, int] = {}
    for j_, k_ in enumerate(group_key):
        if k_:
            rep[j_] = first_of.setdefault(int(k_), j_)
    return rep


class Evaluator:
    """Results of one batch of records (the whole file, or one chunk of the streaming reader)."""

    def __init__(self, models: ModelCache, plans: PlanCache, rank=0, world=1, device=0, afd_capacity=0, result_pool=None, switches: Switches = None):
        self.models, self.plans, self.rank, self.world, self.device, self.afd_capacity = models, plans, rank, world, device, afd_capacity
        self.result_pool, self.switches = result_pool, switches
        self.sharded = False   # the sharded front door (Pipeline.open_reader): this rank reads, evaluates and writes its own share
        self.carried: Dict[int, dict] = {}   # see carry_breakends

    def evaluate(self, batch, contig_names, contig_of, het, som, group_rep, group_key=None):
        L = batch.n_loci
        modes = model_modes(batch.locus["locus_flags"]) if L else np.zeros(0, np.int64)
        key = contig_of * 256 + modes  # (contig, model mode): one model, one `last_rid`, one variant-specific prior (calling.rs:413-443)
        self.models.record_first(key, contig_names, het, som)
        # breakends of one event share a pileup and a result: evaluate the first record of every event only and copy its
        # event probabilities / sample info to the others (calling.rs:569-580, 726-741, 820-839)
        reps = np.nonzero(group_rep == np.arange(L))[0]
        res, names = None, None
        for sig, sc, loci in self.group_by_model(key, reps, contig_names):
            r = self.run_group(batch, sig, sc, loci, len(reps), group_key)
            if names is None:
                names = sc.out_names()
            if len(loci) == L:
                res = r
                break
            if res is None:
                res = CallResults(L, r.n_out, r.n_samples, self.afd_capacity)
            scatter(res, r, loci)
        if res is not None:
            if len(reps) < L:
                fan_out(res, group_rep)
            if group_key is not None and L:
                carry_breakends(res, group_key, self.carried)
            if self.rank == 0 or self.sharded:
                warn_hard_status(res.status)
        return res, names

    def group_by_model(self, key, reps, contig_names):
        """[(signature, scenario, sorted loci)]: the representatives `reps`, grouped by the signature of their model's scenario"""
        groups: Dict[tuple, List] = {}
        sig_scenario: Dict[tuple, Scenario] = {}
        for k_ in np.unique(key[reps]) if len(reps) else []:
            sc = self.models.resolve(*_contig_mode(k_, contig_names))
            sig = _scenario_signature(sc)
            sig_scenario.setdefault(sig, sc)
            groups.setdefault(sig, []).append(reps[key[reps] == k_])
        return [(sig, sig_scenario[sig], np.sort(np.concatenate(parts))) for sig, parts in groups.items()]

    def run_group(self, batch, sig, sc, loci, n_reps, group_key):
        """Results of the records `loci` of `batch`, which share the scenario `sc`."""
        L, afd_capacity = batch.n_loci, self.afd_capacity
        n_out_, S_ = sc.n_out, len(sc.sample_names)
        gather = self.world > 1 and not self.sharded
        if gather:
            # loci shard across the ranks (one process per GPU); the results are reassembled by one all-gather of
            # fixed-size records (+ one for the AFD lists), every rank ends up with the full result
            lo, hi = vdist.shard_range(len(loci), self.rank, self.world)
            mine = loci[lo:hi]
        else:
            lo, hi, mine = 0, len(loci), loci
        if len(mine):
            plan = self.plans.get(sig, sc)
            table = batch.extra.get("native_table") if getattr(batch, "extra", None) else None
            on_dev = table is not None and getattr(table, "on_device", False)
            if on_dev and len(mine) != L:
                # several models (or ranks) in one chunk: the sub-batches are cut from the HOST columns, which a device reader with
                # detached copies may still be filling — wait for them before the first select
                table.fetch_columns()
            sub = batch if len(mine) == L else batch.select(mine)
            # observation files are already capped by preprocess's --max-depth: size the LDS budget to the deepest record
            # (deeper records than the LDS holds take the deep launch); the depth comes from the offsets, never from the columns
            plan.fit_max_obs(sub.obs_offset)
            if len(mine) == L and on_dev:
                # the columns were decoded on the device (device reader): nothing to stage but the results, which land in recycled
                # page-locked memory when the calls writer is the only consumer (it hands the block back after the chunk is written)
                # the FORMAT/AFD text is written on the device (vlr_results.afd_text, 8 bytes per slot of the lists' capacity; a list
                # that does not fit comes down as numbers) unless results are copied between records afterwards — breakend events
                # (group fan-out, rows carried across chunks) index the arrays.  VLR_AFD_TEXT=0: numbers only.
                text_cap = 0
                if afd_capacity and n_reps == L and (group_key is None or not np.any(group_key)) and self.switches.afd_text:
                    text_cap = min(L * S_ * 8 * afd_capacity, 0xffff0000)
                # (device text only where the native calls writer is the sole consumer of the lists — the pooled path and the sharded
                #  writer: a list that was formatted on the device is not copied down as numbers, and a caller of call_variants() that
                #  gets the CallResults of a single chunk back reads afd_vaf / afd_lnprob)
                buf = (self.result_pool.results(L, n_out_, S_, afd_capacity, text_cap) if self.result_pool is not None
                       else (CallResults(L, n_out_, S_, afd_capacity, afd_text_capacity=text_cap) if (text_cap and self.sharded) else None))
                r = plan.call_table_device(table, afd_capacity=afd_capacity, results=buf)
            else:
                r = plan.call_host(sub, afd_capacity=afd_capacity)
        else:
            r = CallResults(0, n_out_, S_, afd_capacity)
        if gather:
            r = vdist.gather_call_results(r, lo, hi, len(loci), n_out_, S_, afd_capacity)
        return r


class Pipeline:
    """The product path: BGZF inflate, BCF/VCF parse, the v15 decoder and the calls writer in native code (csrc/vlr_ingest.cpp), a
    bounded number of records at a time; reader, evaluation and writer of consecutive chunks overlap (three threads: the
    native calls release the GIL)."""

    def __init__(self, ev: Evaluator, paths, omit_mask, output, processor, candidate_filter, allow_shards, t_begin):
        self.ev, self.sw, self.paths, self.omit_mask, self.output = ev, ev.switches, paths, omit_mask, output
        self.processor, self.candidate_filter, self.allow_shards, self.t_begin = processor, candidate_filter, allow_shards, t_begin
        self.is_text = any(not (p_.endswith(".bcf") or p_.endswith(".bcf.gz")) for p_ in paths)
        self.reader = self.open_reader()
        self.q_in: "queue.Queue" = queue.Queue(maxsize=self.sw.queue)
        self.q_out: "queue.Queue" = queue.Queue(maxsize=self.sw.queue)
        self.stage = {"read_s": 0.0, "call_s": 0.0, "write_s": 0.0, "n_loci": 0, "n_obs": 0}
        self.errors: List[BaseException] = []      # of the reader and writer threads, handed to the main thread
        self.loop_exc: List[BaseException] = []    # sharded run: what went wrong on THIS rank (the others must hear of it before anybody waits)
        self.stop = threading.Event()
        self.tw, self.writer, self.writer_tmp, self.writer_path = None, None, None, None   # the writer thread and its lazily opened CallsWriter
        self.proc_setup = False
        self.collected: List = []
        self.names, self.used_contigs, self.t_loop_end = None, [], None

    def open_reader(self):
        """The device reader where it can take the files, else the host reader; sets Evaluator.sharded and the plans' reserve size.

        Sharded front door (several ranks, device reader, BCF output): every rank inflates, decodes, evaluates and WRITES its own
        contiguous share of the records (ingest.ObsReader(shard=...): about 1 / N of the members of every file per rank) and rank 0 puts
        the parts of the calls file together — no rank ever holds the whole file, nothing but a few counters crosses between the ranks.
        VLR_INGEST_SHARDED=0 keeps the older path (every rank reads everything, results all-gathered)."""
        ev, sw, paths, processor, candidate_filter, output = self.ev, self.sw, self.paths, self.processor, self.candidate_filter, self.output
        world, rank = ev.world, ev.rank
        if not self.is_text and not sw.host_reader:
            # BGZF inflate, record split and v15 decode as kernels (csrc/vlr_inflate.hip, csrc/vlr_decode.hip): the compressed members
            # cross PCIe, the columns are born in device memory and the evaluation reads them there.  Files it does not read (plain
            # gzip, uncompressed BCF) go to the host reader.
            want_shards = (world > 1 and processor is None and candidate_filter is None and bool(output) and str(output).endswith(".bcf")
                           and sw.sharded and self.allow_shards)
            try:
                # records per request: 32 768, and 65 536 for inputs above a gigabyte (tools/cli_sweep.sh, 1 M records per step: 1.66 -> 1.75 M
                # records/s; 131 072: 1.42 M — too few chunks for the three stages to overlap —, 16 384: 1.25 M)
                big = sum(os.path.getsize(p_) for p_ in paths) >= (1 << 30)
                reader = vingest.ObsReader(paths, omit_bias_mask=self.omit_mask, chunk_records=sw.chunk or (65536 if big else 32768), device=ev.device,
                                           shard=(rank, world) if want_shards else None,
                                           # the observation columns stay on the device and the calls writer takes the OBS text, the SAOBS / SROBS letters
                                           # and the DP runs of every pileup from obs_text_kernel (vlr_obs_reader_set_host_columns(0)); a processor, a
                                           # candidate filter and the unsharded multi-rank path read the host columns.  VLR_INGEST_SUMMARIES=0: columns.
                                           host_columns=(processor is not None or candidate_filter is not None or not (world == 1 or want_shards)
                                                         or not sw.summaries),
                                           # the evaluation reads the device side of a table; only the writer (which waits) needs the host copy of the columns
                                           # (several ranks: every rank inflates and decodes the files on its own device instead of sharing the
                                           # node's CPUs between N host readers; its shard is cut from the host copy of the columns)
                                           async_columns=(processor is None and candidate_filter is None and (world == 1 or want_shards)))
                ev.sharded = want_shards
                ev.plans.reserve_loci = reader.chunk_records
                return reader
            except engine.EngineError as ex:
                if ex.code != abi.ERR_UNSUPPORTED:
                    raise
        # text VCF: contigs are only known at the end
        return vingest.ObsReader(paths, omit_bias_mask=self.omit_mask, chunk_records=sw.chunk or (1 << 62 if self.is_text else 16384))

    def read_loop(self):
        try:
            while not self.stop.is_set():
                t0 = time.perf_counter()
                item = self.reader.next()
                self.stage["read_s"] += time.perf_counter() - t0
                while not self.stop.is_set():
                    try:
                        self.q_in.put(item, timeout=0.2)
                        break
                    except queue.Full:
                        pass
                if item is None:
                    return
        except BaseException as ex:  # noqa: BLE001 (handed to the main thread)
            self.errors.append(ex)
            self.q_in.put(None)

    def write_loop(self):
        ev = self.ev
        try:
            while True:
                item = self.q_out.get()
                if item is None:
                    return
                table, res_, names_, contigs_ = item
                t0 = time.perf_counter()
                if self.writer is None:
                    hdr, _ = ev.models.header_for(names_, contigs_)
                    target = self.output
                    if not target:
                        self.writer_tmp = tempfile.TemporaryDirectory()
                        target = os.path.join(self.writer_tmp.name, "calls.vcf")
                    if ev.sharded:
                        target = _part_path(self.output, ev.rank)
                    self.writer = vingest.CallsWriter(target, hdr, part=(ev.rank, ev.world) if ev.sharded else None)
                    self.writer_path = target
                self.writer.append(table, res_, list(names_))
                if ev.result_pool is not None:
                    ev.result_pool.release(res_)
                self.stage["write_s"] += time.perf_counter() - t0
        except BaseException as ex:  # noqa: BLE001
            self.errors.append(ex)
            while self.q_out.get() is not None:
                pass

    def run(self):
        """Reads, evaluates and hands on every chunk; returns with the threads joined, the reader and the plans closed."""
        ev = self.ev
        tr = threading.Thread(target=self.read_loop, daemon=True)
        self.tw = threading.Thread(target=self.write_loop, daemon=True) if ((ev.rank == 0 or ev.sharded) and self.processor is None) else None
        self.stage["setup_s"] = time.perf_counter() - self.t_begin
        tr.start()
        if self.tw:
            self.tw.start()
        try:
            try:
                while True:
                    item = self.q_in.get()
                    if item is None or self.errors:
                        break
                    self.process(*item)
            except BaseException as ex:  # noqa: BLE001
                if not ev.sharded:
                    raise
                self.loop_exc.append(ex)
        finally:
            self.t_loop_end = time.perf_counter()
            if self.tw:
                self.q_out.put(None)
                self.tw.join()
            self.stage["drain_writer_s"] = time.perf_counter() - self.t_loop_end   # the writer's last chunk(s)
            self.stop.set()
            tr.join()
            if ev.sharded and self.sw.shard_report:
                # what this rank read (tests, tools): its record range and the bytes it inflated
                with open("%s.%d" % (self.sw.shard_report, ev.rank), "w") as fh_:
                    json.dump({"rank": ev.rank, "world": ev.world, "first_record": self.reader.first_record, "n_records": self.reader.n_records,
                               "total_records": getattr(self.reader, "total_records", None), "device_reader": vingest.device_timings()}, fh_)
            t_c0 = time.perf_counter()
            self.reader.close()
            self.stage["drain_reader_close_s"] = time.perf_counter() - t_c0
            t_c0 = time.perf_counter()
            ev.plans.close_all()
            self.stage["drain_plans_close_s"] = time.perf_counter() - t_c0

    def process(self, batch, sites):
        """One chunk of the reader: filter, evaluate, hand the results to the processor or the writer thread."""
        ev, stage, processor, sample_order = self.ev, self.stage, self.processor, self.ev.models.sample_order
        t0 = time.perf_counter()
        contig_names = list(sites.contig_names)
        contig_of = np.asarray(sites.contig, np.int64)
        het_, som_ = batch.extra["prior_het_ln"], batch.extra["prior_som_ln"]
        grep_, gkey_ = np.asarray(batch.extra["group_representative"], np.int64), np.asarray(batch.extra["group_key"], np.uint64)
        if ev.sharded and ((gkey_ != 0).any() or np.isfinite(np.asarray(het_, np.float64)).any() or np.isfinite(np.asarray(som_, np.float64)).any()):
            # breakend events hand the FIRST record's result to the later ones, and per-variant prior overrides are installed from
            # the first record of a contig (calling.rs:569-580, 643-713): both reach across shard boundaries.  This rank stops
            # here; after the collective of finish_sharded ALL ranks drop their parts and take the file again on the unsharded path
            # (every rank reads everything, results all-gathered), which carries both.
            raise _CrossesShards()
        loci_ = np.arange(batch.n_loci)
        ebatch = batch
        if self.candidate_filter is not None:   # calling.rs:409: work items the filter rejects are not processed at all
            keep = np.asarray(self.candidate_filter.filter(batch, sites, sample_order), bool)
            if not keep.all():
                loci_ = np.nonzero(keep)[0]
                ebatch = batch.select(loci_)
                contig_of, het_, som_, gkey_ = contig_of[loci_], np.asarray(het_)[loci_], np.asarray(som_)[loci_], gkey_[loci_]
                grep_ = regroup_representatives(gkey_)
        res, nm = (ev.evaluate(ebatch, contig_names, contig_of, het_, som_, grep_, gkey_) if ebatch.n_loci else (None, None))
        self.names = names = self.names or nm
        stage["call_s"] += time.perf_counter() - t0
        stage["n_loci"] += batch.n_loci
        stage["n_obs"] += batch.n_obs
        if not self.used_contigs:
            self.used_contigs = contig_names if not self.is_text else [contig_names[int(c_)] for c_ in np.unique(np.asarray(sites.contig))]
        self.collected.append(_fixed_fields(res) if (ev.result_pool is not None and getattr(res, "_pool_block", None) is not None) else res)
        if processor is not None:
            if res is not None and ev.rank == 0:
                if not self.proc_setup:
                    processor.setup(list(names), list(sample_order))
                    self.proc_setup = True
                processor.process_calls(CallChunk(ebatch, sites, res, list(names), list(sample_order), loci_, stage["n_loci"] - batch.n_loci))
        elif self.tw and res is not None:
            self.q_out.put((batch.extra["native_table"], res, names, self.used_contigs))

    def finish_processor(self):
        """setup (when no chunk had records) and finalize of the processor, on rank 0"""
        if self.ev.rank == 0:
            if not self.proc_setup:
                contig = self.used_contigs[0] if self.used_contigs else "all"
                self.processor.setup(list(self.names or self.ev.models.resolve(contig).out_names()), list(self.ev.models.sample_order))
            self.processor.finalize()

    def drop_part(self, quiet=False):
        """A sharded run that does not come through: close and remove this rank's part of the calls file."""
        if self.writer is not None:
            try:
                self.writer.close()
            except Exception:  # noqa: BLE001 (already failing)
                if not quiet:
                    raise
        try:
            os.remove(_part_path(self.output, self.ev.rank))
        except OSError:
            pass


def finish_sharded(p: Pipeline) -> bool:
    """The ending of a sharded run: True when the calls file was assembled, False when ALL ranks have dropped their parts and take
    the file again on the unsharded path.

    One collective tells every rank whether ALL ranks came through and what the file's header holds (a rank that
    fails alone leaves the others at the barrier below until the RCCL timeout; a rank without records cannot know the contigs
    and output names the other parts index).  Nothing is written unless every rank succeeded; parts are removed otherwise."""
    import torch.distributed as tdist
    rank, world, errors, loop_exc = p.ev.rank, p.ev.world, p.errors, p.loop_exc
    crosses = bool(loop_exc) and isinstance(loop_exc[0], _CrossesShards)
    mine_failed = bool(errors or loop_exc) and not crosses
    info: List = [None] * world
    tdist.all_gather_object(info, (mine_failed, list(p.names) if p.names else None, list(p.used_contigs), crosses))
    if any(i_[3] for i_ in info) and not any(i_[0] for i_ in info):
        # records that reach across shard boundaries (seen by at least one rank): the whole file again, unsharded
        p.drop_part()
        if rank == 0:
            print("note: breakend events or per-variant prior overrides in the input: %d ranks read the whole file (results all-gathered) "
                  "instead of a share each" % world, file=sys.stderr)
        tdist.barrier()
        return False
    if any(i_[0] for i_ in info):
        p.drop_part(quiet=True)
        if loop_exc and not crosses:
            raise loop_exc[0]
        if errors:
            raise errors[0]
        raise SystemExit("rank(s) %s of the sharded run failed: no calls file was written" % ", ".join(str(k_) for k_, i_ in enumerate(info) if i_[0]))
    # the same header on every rank: names and contigs of the first rank that saw records
    names = next((i_[1] for i_ in info if i_[1]), p.names)
    used_contigs = next((i_[2] for i_ in info if i_[2]), p.used_contigs)
    # every rank closes its part (a rank without records writes an empty one: the header, on rank 0); rank 0 assembles the file
    if p.writer is None:
        hdr, _ = p.ev.models.header_for(names, used_contigs)
        vingest.CallsWriter(_part_path(p.output, rank), hdr, part=(rank, world)).close()
    else:
        p.writer.close()
    tdist.barrier()
    if rank == 0:
        vingest.concat_parts(p.output, [_part_path(p.output, k_) for k_ in range(world)])
    tdist.barrier()
    return True


def finish_single(p: Pipeline, out):
    """The ending of an unsharded run on rank 0: the calls file is closed, or copied to `out` when there is no output path."""
    if p.writer is None:  # no records at all: the header alone
        hdr, _ = p.ev.models.header_for(p.names, p.used_contigs)
        if p.output:
            vingest.CallsWriter(p.output, hdr).close()
        else:
            print(hdr, file=out)
    else:
        p.writer.close()
        if not p.output:
            with open(p.writer_path) as fh:
                out.write(fh.read())
            p.writer_tmp.cleanup()


def concat_fixed(collected):
    """What call_variants returns of the chunks' results: None, the single result, or the fixed-size fields concatenated (the AFD
    lists went to the file chunk by chunk)."""
    collected = [r_ for r_ in collected if r_ is not None]
    if len(collected) == 1:
        return collected[0]
    if not collected:
        return None
    tot = CallResults(sum(r_.n_loci for r_ in collected), collected[0].n_out, collected[0].n_samples, 0)
    o = 0
    for r_ in collected:
        for f in FIELDS[:6]:
            getattr(tot, f)[o:o + r_.n_loci] = getattr(r_, f)
        o += r_.n_loci
    return tot


def call_python(ev: Evaluator, paths, omit_mask, out, output, timings, t_begin):
    """The Python restatement of the same decoder and formatter (obsfmt.py / bcfio.py / callsfmt.py); the tests compare the two."""
    batch, sites = obsfmt.read_observation_vcf(paths, omit_bias_mask=omit_mask)
    contig_names = sorted(set(s_[0] for s_ in sites))
    cidx = {c: i for i, c in enumerate(contig_names)}
    contig_of = np.array([cidx[s_[0]] for s_ in sites], np.int64)
    pri = batch.extra.get("prior_overrides") or []
    het = np.array([np.nan if p_[0] is None else p_[0] for p_ in pri], np.float64)
    som = np.array([np.nan if p_[1] is None else p_[1] for p_ in pri], np.float64)
    reps_, source_ = obsfmt.haplotype_groups(batch.extra.get("haplotype") or [None] * batch.n_loci)
    group_rep = np.asarray(reps_, np.int64)[np.asarray(source_, np.int64)] if batch.n_loci else np.zeros(0, np.int64)
    L = batch.n_loci
    t_read = time.perf_counter()
    try:
        res, names = ev.evaluate(batch, contig_names, contig_of, het, som, group_rep)
    finally:
        ev.plans.close_all()
    t_call = time.perf_counter()
    header, scenario0 = ev.models.header_for(names, contig_names if L else [])
    names = names or scenario0.out_names()
    if ev.rank != 0:
        return res
    if output and output.endswith(".bcf"):  # binary calls file (reference: bcf::Writer, calling.rs:296-304)
        from .bcfio import BcfWriter
        with BcfWriter(output, header) as wr:
            for l in range(L):
                wr.write_line(callsfmt.format_record(sites[l], batch, res, l, names, scenario0.sample_names))
    else:
        if output:
            out = open(output, "w")
        print(header, file=out)
        for l in range(L):
            print(callsfmt.format_record(sites[l], batch, res, l, names, scenario0.sample_names), file=out)
        if output:
            out.close()
    if timings is not None:
        t_end = time.perf_counter()
        timings.update({"read_s": t_read - t_begin, "call_s": t_call - t_read, "write_s": t_end - t_call, "n_loci": L, "n_obs": batch.n_obs, "wall_s": t_end - t_begin, "chunks": 1})
    return res


def _world_rank():
    try:
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized():
            return tdist.get_world_size(), tdist.get_rank()
    except ImportError:
        pass
    return 1, 0


def call_variants(scenario, obs_paths: Dict[str, str], omit_mask: int = 0, afd_capacity: int = 128, out=sys.stdout,
                  device: int = 0, output: str = None, ingest: str = None, timings: dict = None,
                  processor: "CallProcessor" = None, candidate_filter: "CandidateFilter" = None, _allow_shards: bool = True):
    """`scenario`: a Scenario, or a callable contig -> Scenario (contig-specific universes / ploidies: one plan per
    distinct resolution, as the reference re-configures its model on contig change, calling.rs:343-356).
    `processor` / `candidate_filter`: the driver's two plug points (calling.rs:964-1020); with a processor no calls file is
    written (the processor IS the consumer, as CallWriter is in the reference); a candidate filter needs a processor."""
    if candidate_filter is not None and processor is None:
        raise ValueError("a candidate filter comes with its own call processor (calling.rs:1022-1040: call_generic takes both)")
    models = ModelCache(scenario, obs_paths)
    paths = [obs_paths[name] for name in models.sample_order if name in obs_paths]
    sw = Switches.from_env(ingest)
    if processor is not None and not sw.native:
        raise ValueError("call processors plug into the native streaming driver (VLR_INGEST=native)")
    world, rank = _world_rank()
    # (one pool per process: page-locking its blocks again for every run costs tens of milliseconds)
    result_pool = _shared_result_pool() if (sw.native and processor is None and rank == 0 and world == 1 and output) else None
    ev = Evaluator(models, PlanCache(device, afd_capacity), rank, world, device, afd_capacity, result_pool, sw)
    t_begin = time.perf_counter()
    if not sw.native:
        return call_python(ev, paths, omit_mask, out, output, timings, t_begin)
    p = Pipeline(ev, paths, omit_mask, output, processor, candidate_filter, _allow_shards, t_begin)
    p.run()
    if ev.sharded and not finish_sharded(p):
        return call_variants(scenario, obs_paths, omit_mask=omit_mask, afd_capacity=afd_capacity, out=out, device=device, output=output,
                             ingest=ingest, timings=timings, processor=processor, candidate_filter=candidate_filter, _allow_shards=False)
    if p.errors:
        raise p.errors[0]
    if processor is not None:
        p.finish_processor()
    elif rank == 0 and not ev.sharded:
        finish_single(p, out)
    if timings is not None:
        timings.update(dict(p.stage, wall_s=time.perf_counter() - t_begin, chunks=len(p.collected), drain_s=time.perf_counter() - p.t_loop_end))
    return concat_fixed(p.collected)
