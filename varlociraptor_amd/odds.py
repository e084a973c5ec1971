"""Filtering calls by posterior odds: `filter-calls posterior-odds` (reference src/filtration/posterior_odds.rs:19-82).

An allele is kept while the evidence AGAINST the chosen events — the Bayes factor of all other events of the header over the
chosen ones, on the Kass-Raftery scale — stays below `--odds`.  Both probabilities are ln-sums over
PROB_* INFO tags as utils::tags_prob_sum forms them (restated in fdr.py).  The per-allele decision has a HIP kernel behind the C
ABI (`vlr_posterior_odds_keep`, csrc/vlr_callstats.hip) and the whole command runs in the engine (`vlr_calls_filter_odds`,
csrc/vlr_callsfile.cpp); next to them is the host restatement (`device="cpu"`) that the CPU suite and the comparisons use.

Deviation: the reference trims the removed alleles of a kept record; here a kept record passes through untrimmed, which is the
same thing for the single-ALT records `call variants` writes.  Not checkable here: the reference's spelling of the `--odds`
values (bio's KassRaftery parser is not in the reference tree); this command takes none, barely, positive, strong, very-strong.
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import fdr

LEVELS = ("none", "barely", "positive", "strong", "very-strong")  # KassRaftery in declaration order = VLR_ODDS_*


def event_tags(header_lines: Sequence[str]) -> List[Tuple[str, str]]:
    """(ID, Description) of every PROB_* INFO line, in header order (utils::get_event_tags, utils/mod.rs:429-446)."""
    out = []
    for l in header_lines:
        if not l.startswith("##INFO=<"):
            continue
        m = re.search(r"(?:<|,)ID=([^,>]+)", l)
        if not m or not m.group(1).startswith("PROB_"):
            continue
        d = re.search(r'Description="([^"]*)"', l) or re.search(r"Description=([^,>]*)", l)
        out.append((m.group(1), d.group(1) if d else ""))
    return out


def is_phred_scaled(header_lines: Sequence[str]) -> bool:
    """utils/mod.rs:421-426 (a description without closing parenthesis passes, for backward compatibility)."""
    return all(d.endswith("(PHRED)") or not d.endswith(")") for _, d in event_tags(header_lines))


def target_tags(events: Sequence[str]) -> List[str]:
    """utils::events_to_tags: the tag upper-cases the event name (lib.rs:52-54)."""
    return ["PROB_" + e.upper() for e in events]


def other_tags(header_lines: Sequence[str], events: Sequence[str]) -> List[str]:
    """posterior_odds.rs:39-52: the PROB_* tags whose suffix equals none of the event names AS GIVEN — an event typed in lower
    case excludes nothing, so its tag is summed on both sides (mirrored, and tested)."""
    return [t for t, _ in event_tags(header_lines) if t[5:] not in events]


def level(k: float) -> int:
    """bio evidence_kass_raftery; a NaN factor fails every comparison."""
    return 0 if k <= 1.0 else 1 if k <= 3.0 else 2 if k <= 20.0 else 3 if k <= 150.0 else 4


def allele_sums(rec: dict, targets: Sequence[str], others: Sequence[str]) -> List[Tuple[Optional[float], Optional[float]]]:
    """(ln_target, ln_other) per typed variant of a record; None = no value (utils::tags_prob_sum(.., None))."""
    return list(zip(fdr.tags_prob_sum(rec, targets, None), fdr.tags_prob_sum(rec, others, None)))


def keep_bits(ln_target, ln_other, valid, min_level: int, device="cpu") -> np.ndarray:
    """keep[i] = both valid && level(e^(ln_other - ln_target)) < min_level (posterior_odds.rs:66-78).  valid: bit 0 target,
    bit 1 other.  device="cpu": numpy restatement; an int or "cuda[:k]": vlr_posterior_odds_keep."""
    lt = np.ascontiguousarray(ln_target, np.float64)
    lo = np.ascontiguousarray(ln_other, np.float64)
    va = np.ascontiguousarray(valid, np.uint8)
    if not (len(lt) == len(lo) == len(va)):
        raise ValueError("ln_target, ln_other and valid differ in length")
    if not 0 <= int(min_level) <= 4:
        raise ValueError("min_level outside [0, 4]")
    if device == "cpu":
        with np.errstate(invalid="ignore", over="ignore"):
            k = np.exp(lo - lt)
            lev = np.where(k <= 1.0, 0, np.where(k <= 3.0, 1, np.where(k <= 20.0, 2, np.where(k <= 150.0, 3, 4))))
        return (((va & 3) == 3) & (lev < int(min_level))).astype(np.uint8)
    from . import engine
    L = engine.lib()
    keep = np.zeros(len(lt), np.uint8)
    engine.check(L.vlr_posterior_odds_keep(_device_index(device), len(lt), lt.ctypes.data, lo.ctypes.data, va.ctypes.data, int(min_level), keep.ctypes.data))
    return keep


def _device_index(device) -> int:
    s = str(device)
    if s.startswith("cuda"):
        return int(s.split(":")[1]) if ":" in s else 0
    return int(s)


def filter_by_odds(records: Sequence[dict], header_lines: Sequence[str], events: Sequence[str], min_level: int, device="cpu") -> List[dict]:
    """The command on parsed records: the kept ones (a record is kept when any of its alleles is)."""
    if not is_phred_scaled(header_lines):
        raise ValueError("Event probabilities are not PHRED scaled, aborting.")
    targets, others = target_tags(events), other_tags(header_lines, events)
    lt, lo, va, first = [], [], [], [0]
    for rec in records:
        for t, o in allele_sums(rec, targets, others):
            lt.append(0.0 if t is None else t)
            lo.append(0.0 if o is None else o)
            va.append((0 if t is None else 1) | (0 if o is None else 2))
        first.append(len(lt))
    keep = keep_bits(lt, lo, va, min_level, device=device)
    return [rec for i, rec in enumerate(records) if keep[first[i]:first[i + 1]].any()]


def filter_calls_native(in_path: str, out_path: str, events: Sequence[str], min_level: int, device: int = 0, threads: int = 0) -> Tuple[int, int]:
    """vlr_calls_filter_odds (include/vlr.h): the whole command in the engine.  Returns (kept, total)."""
    import ctypes as C
    from . import engine
    L = engine.lib()
    ev = (C.c_char_p * len(events))(*[e.encode() for e in events])
    kept, total = C.c_int64(), C.c_int64()
    engine.check(L.vlr_calls_filter_odds(in_path.encode(), out_path.encode(), len(events), ev, int(min_level), int(device), int(threads), C.byref(kept), C.byref(total)))
    return int(kept.value), int(total.value)

