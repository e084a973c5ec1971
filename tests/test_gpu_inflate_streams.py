"""vlr_inflate_kernel (csrc/vlr_inflate.hip) on DEFLATE streams zlib's compressor never emits: the catalogue of tests/deflate_cases.py
— codes of 11 to 15 bits in every class of symbol and tokens of 48 bits, every overlap of distance and length up to 258, matches at
the edge of the 4 KiB ring and beyond it up to distance 32 768 at all sixteen output shifts, dynamic headers in their rare forms,
hundreds of tiny blocks, stored blocks at every bit phase, block headers across the 256-byte input windows — and on streams that
must be refused, each for its own INFL_* reason.

The expected bytes are zlib's (tests/test_deflate_cases_host.py shows, without a GPU, that zlib inflates every accepted member and
refuses every refused one, and that each case reaches the path it is named for); they are compared with ==.  Both symbol loops
run (VLR_INFLATE_BATCH = 0 / 1).  Every refused case was read along its path through the kernel before it was put here: LDS
accesses go through the ring mask, a far copy reads nothing unless the distance lies inside the member, nothing goes to HBM
beyond lim = ISIZE, and the input is read at most one block header and one flush interval (a few KiB) beyond the member, inside
kInflateInputSlack."""
import contextlib
import os
import re

import pytest

import deflate_cases as dc
from varlociraptor_amd import engine, ingest

pytestmark = pytest.mark.gpu

MODES = {"symbol loop": "0", "speculative batches": "1"}


@contextlib.contextmanager
def _mode(value):
    """VLR_INFLATE_BATCH is read at every launch."""
    old = os.environ.get("VLR_INFLATE_BATCH")
    os.environ["VLR_INFLATE_BATCH"] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ["VLR_INFLATE_BATCH"]
        else:
            os.environ["VLR_INFLATE_BATCH"] = old


@pytest.fixture(params=list(MODES.values()), ids=list(MODES))
def inflate_mode(request):
    """Both symbol loops of vlr_inflate_kernel."""
    with _mode(request.param):
        yield request.param


@pytest.fixture(scope="module")
def cat():
    return dc.catalogue()


_ALONE = {}


def _alone(cat, mode):
    """Every accepted case inflated alone in one mode, once per module: the bytes, or the error."""
    if mode not in _ALONE:
        got = []
        with _mode(mode):
            for c in cat.accepted:
                try:
                    got.append(ingest.bgzf_inflate(c.data))
                except engine.EngineError as e:
                    got.append(e)
        _ALONE[mode] = got
    return _ALONE[mode]


def _refusal(data):
    """(INFL_* code, member index) of the refusal of `data` (vlr_bgzf_inflate: code * 1000000 + member index)."""
    with pytest.raises(engine.EngineError) as ei:
        ingest.bgzf_inflate(data)
    m = re.search(r"corrupt DEFLATE stream \(code (\d+)\)", str(ei.value))
    assert m, str(ei.value)
    return divmod(int(m.group(1)), 1000000)


def _reasons(c):
    return c.reason if isinstance(c.reason, frozenset) else frozenset([c.reason])


@pytest.mark.parametrize("group", ["long codes", "overlap grid", "ring edge and far matches", "dynamic-header forms", "block structure"])
def test_accepted_members_equal_zlib(cat, inflate_mode, group):
    got = _alone(cat, inflate_mode)
    n = 0
    for c, g in zip(cat.accepted, got):          # each case alone: a failure names it
        if c.group != group:
            continue
        assert not isinstance(g, Exception), "%r: %s" % (c, g)
        assert g == c.payload, "%r: first difference at byte %d of %d" % (c, next((i for i, (a, b) in enumerate(zip(g, c.payload)) if a != b), min(len(g), len(c.payload))), len(c.payload))
        n += 1
    assert n == len(cat.group(group)) > 0
    # the group as one stream: other output offsets, many members in flight
    cs = cat.group(group)
    assert ingest.bgzf_inflate(b"".join(c.data for c in cs)) == b"".join(c.payload for c in cs)


def test_both_symbol_loops_agree_on_every_accepted_case(cat):
    a, b = _alone(cat, "0"), _alone(cat, "1")
    for c, x, y in zip(cat.accepted, a, b):
        assert not isinstance(x, Exception) and not isinstance(y, Exception), c
        assert x == y, c


def test_refused_members_are_refused_for_their_reason(cat, inflate_mode):
    for c in cat.refused:
        code, index = _refusal(c.data)
        assert code in _reasons(c) and index == 0, "%r: code %d, member %d" % (c, code, index)


def test_a_refused_member_between_two_accepted_ones_fails_the_call_with_its_index(cat, inflate_mode):
    small = sorted(cat.group("dynamic-header forms"), key=lambda c: len(c.data))[:6]
    for i, c in enumerate(cat.refused):
        before, after = small[i % 6], small[(i + 1) % 6]
        assert ingest.bgzf_inflate(before.data + after.data) == before.payload + after.payload
        code, index = _refusal(before.data + c.data + after.data)
        assert code in _reasons(c) and index == 1, "%r: code %d, member %d" % (c, code, index)


def test_a_mixed_stream_is_refused_in_both_modes_with_the_same_code(cat):
    ok = sorted(cat.group("dynamic-header forms") + cat.group("block structure")[:12], key=lambda c: len(c.data))[:12]
    for i, c in enumerate(cat.refused):
        three, more = [ok[(i + k) % 12] for k in range(3)], [ok[(i + 3 + k) % 12] for k in range(3)]
        data = b"".join(x.data for x in three) + c.data + b"".join(x.data for x in more)
        got = []
        for mode in MODES.values():
            with _mode(mode):
                got.append(_refusal(data))
        assert got[0] == got[1], "%r: %r" % (c, got)
        assert got[0][0] in _reasons(c) and got[0][1] == 3, "%r: %r" % (c, got)
