"""GPU parity for the way the engine is used in production: one long-lived
engine that is reset and fed again over a table still holding the previous
count, and device feeds cut into segments (staged tails, borrowed input,
a 0xFF byte right behind a cut).

Every comparison is exact, against the CPU oracle of that step's bytes alone.
"""
import functools

import numpy as np
import pytest

import findkmer_amd as fk
import oracle
from conftest import golden_input
from test_gpu_parity import _dense_records, mixed_input

pytestmark = pytest.mark.gpu

ALLOW = (fk.FK_OK, fk.FK_E_EMPTY, fk.FK_E_UNTERMINATED_HEADER)
SEG = 65536          # FINDKMER_TUNE seg_kb=64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if fk.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


# ---- inputs ---------------------------------------------------------------

def random_fasta(seed, nbytes, width, header_at=()):
    """uniform random ACGT in lines of `width` bases, a '>' line in front of
    each line whose number is in header_at (ascending)"""
    rng = np.random.default_rng(seed)
    nlines = nbytes // (width + 1)
    lines = np.full((nlines, width + 1), 10, dtype=np.uint8)
    lines[:, :width] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(nlines, width))]
    out, prev = [], 0
    for i, at in enumerate(header_at):
        out += [lines[prev:at].tobytes(), b">rec%d ACGT x\n" % i]
        prev = at
    out.append(lines[prev:].tobytes())
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def dirty_input(which):
    """1.5 MB (0) / 1.25 MB (1) of 80-column random FASTA: windows all over
    the index space, so every slice, coarse slice and part holds nonzero
    bins.  (The second is 1.25 MB, not 1 MB: 1 MB of 80-column FASTA has
    fewer than 2^20 windows, and test_reuse_dirty_table asks both for more
    than 2^20 distinct k-mers at k >= 12.)"""
    if which == 0:
        return random_fasta(20260, 1_500_000, 80, header_at=(0, 4000, 12000))
    return random_fasta(20261, 1_250_000, 80, header_at=(0, 7000))


@functools.lru_cache(maxsize=None)
def no_windows_input():
    """bases inside comment lines only, then a run shorter than any k used here"""
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return b"".join(b">" + acgt[rng.integers(0, 4, size=20_000)].tobytes() + b"\n" for _ in range(3)) + b"ACG\n"


@functools.lru_cache(maxsize=None)
def mixed_no_ff(seed, n):
    return mixed_input(seed, n).replace(b"\xff", b"Z")


@functools.lru_cache(maxsize=None)
def dense_records(seed, n):
    return _dense_records(seed, n)


def to_device(data, lead=0):
    """data at byte `lead` of a fresh device buffer with 16 spare bytes behind
    it; returns (tensor to keep alive, device address of the data)"""
    import torch
    dev = torch.zeros(lead + len(data) + 16, dtype=torch.uint8, device="cuda")
    if len(data):
        dev[lead:lead + len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + lead


def host(data):
    return np.frombuffer(bytes(data), dtype=np.uint8).copy()


# ---- comparisons ----------------------------------------------------------

def device_table_nonzero(e, k, scratch=None):
    """The dense table's nonzero bins (uint64 codes ascending, uint32 counts)
    without reading the table through the host: a device copy in API index
    order (fk_engine_table_to_device), nonzero() over 2^28-bin pieces."""
    import torch
    n = 1 << (2 * k)
    t = scratch if scratch is not None else torch.empty(n, dtype=torch.int32, device="cuda")
    assert t.numel() == n and t.dtype == torch.int32
    e.table_to_device(t.data_ptr())
    step = 1 << 28
    codes, cnts = [], []
    for first in range(0, n, step):
        piece = t[first:first + step]
        idx = piece.nonzero().flatten()
        codes.append((idx + first).cpu().numpy().astype(np.uint64))
        cnts.append(piece[idx].cpu().numpy().view(np.uint32))
    return np.concatenate(codes), np.concatenate(cnts)


def table_scratch(k):
    """a 4^k int32 device tensor for device_table_nonzero (12 <= k <= 16:
    16 GiB at k = 16, so one per test and not one per comparison)"""
    if not 12 <= k <= 16:
        return None
    import torch
    return torch.empty(1 << (2 * k), dtype=torch.int32, device="cuda")


@pytest.fixture(autouse=True)
def _release_device_memory():
    """give the tests' device buffers back to the driver (torch caches them)"""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=4)
def _sparse_oracle(data, k):
    return oracle.count_sparse(data, k, cap=len(data) + 16)


def _unknown_bytes_of(data):
    return oracle.count_dense(data, 3, unknown_cap=1 << 20)[2]   # they do not depend on k


def check(e, data, k, r_g, want_nodes=True, scratch=None):
    """An engine that was fed `data` and finished (r_g: finish's result)
    against the oracle: the whole table and every scalar.
    k <= 11: e.table() vs the dense oracle (as assert_same);
    12 <= k <= 16: the table's nonzero bins, taken on the device, vs the
    sparse oracle (the scalars of _assert_same_sparse_view);
    k >= 17: e.sparse() vs the sparse oracle (as assert_same_sparse)."""
    if k <= 11:
        t_o, r_o, ub_o = oracle.count_dense(data, k, unknown_cap=1 << 20)
        t_g = e.table()
        bad = np.nonzero(t_o != t_g)[0]
        assert len(bad) == 0, f"k={k}: {len(bad)} bins differ, first {bad[:8]} oracle={t_o[bad[:8]]} gpu={t_g[bad[:8]]}"
    else:
        codes_o, cnt_o, r_o = _sparse_oracle(bytes(data), k)
        ub_o = _unknown_bytes_of(data)
        if k <= 16:
            codes_g, cnt_g = device_table_nonzero(e, k, scratch)
        else:
            codes_g, cnt_g = e.sparse()
        assert len(codes_g) == len(codes_o), (k, len(codes_g), len(codes_o))
        bad = np.nonzero(codes_g != codes_o)[0]
        assert len(bad) == 0, f"k={k}: nonzero bins differ, first at {bad[:4]}: oracle={codes_o[bad[:4]]} gpu={codes_g[bad[:4]]}"
        bad = np.nonzero(cnt_g != cnt_o)[0]
        assert len(bad) == 0, f"k={k}: {len(bad)} counts differ, bins {codes_o[bad[:4]]} oracle={cnt_o[bad[:4]]} gpu={cnt_g[bad[:4]]}"
        assert r_o.distinct == len(codes_o)
    assert list(r_g.base_count) == list(r_o.base_count)
    assert r_g.valid_bases == r_o.valid_bases
    assert r_g.windows == r_o.windows
    assert r_g.distinct == r_o.distinct
    assert list(r_g.depth1) == list(r_o.depth1)
    assert r_g.unknown_chars == r_o.unknown_chars
    assert e.unknown_bytes() == ub_o
    assert r_g.hit_eof_byte == r_o.hit_eof_byte
    assert r_g.unterminated_header == r_o.unterminated_header
    assert r_g.scanned_bytes == r_o.scanned_bytes
    if want_nodes:
        assert r_g.nodes == r_o.nodes
    return r_o


# ---- B. reuse over a dirty table ------------------------------------------

def _assert_dirty_enough(data, k):
    """the dirty inputs reach the whole index space"""
    if k <= 8:
        assert (oracle.count_dense(data, k)[0] > 0).all()
    elif k >= 12:
        assert _sparse_oracle(data, k)[2].distinct > 2 ** 20


def _reuse_steps(e, k, want_nodes, scratch, monkeypatch, steps):
    def done(data, allow=ALLOW):
        rc, r = e.finish(allow=allow)
        return check(e, data, k, r, want_nodes=want_nodes, scratch=scratch)

    dirty = dirty_input(0)
    dirty_dev, dirty_ptr = to_device(dirty)
    _assert_dirty_enough(dirty, k)

    if 1 in steps:   # dirty: every bin (k <= 8), every slice and part (k >= 12) nonzero
        e.reset()
        e.feed_device(dirty_ptr, len(dirty))
        done(dirty)

    if 2 in steps:   # tiny, from the host: a fresh count in which nearly every part has no entry
        data = golden_input("test.txt")
        e.reset()
        e.feed(host(data))
        done(data)

    if 3 in steps:   # no window at all: zero entries, and still an all-zero table
        data = no_windows_input()
        e.reset()
        e.feed(host(data))
        r_o = done(data)
        assert r_o.windows == 0 and r_o.distinct == 0

    if 4 in steps:   # one bin
        data = b"A" * 100_000
        dev, ptr = to_device(data)
        e.reset()
        e.feed_device(ptr, len(data))
        done(data)

    if 5 in steps:   # a fresh first segment (staged, shorter than a lane), then a segment that adds
        data = mixed_no_ff(2069, 300_000)
        assert all(c in b"ACGT" for c in data[:64])   # the 20 staged bytes start a run that goes on
        dev, ptr = to_device(data[20:], lead=32)
        assert ptr % 16 == 0
        e.reset()
        e.feed(host(data[:20]))
        e.feed_device(ptr, len(data) - 20)
        done(data)

    if 6 in steps:   # an abandoned count: its statistics and window list must not leak
        data = dense_records(2060, 200_000)
        e.reset()
        e.feed_device(dirty_ptr, len(dirty))
        e.reset()
        e.feed(host(data))
        done(data)

    if 7 in steps:   # end of stream at byte 0 of a device feed
        data = b"\xffACGT" * 1000
        dev, ptr = to_device(data)
        e.reset()
        e.feed_device(ptr, len(data))
        r_o = done(data)
        assert r_o.hit_eof_byte == 1 and r_o.windows == 0 and r_o.distinct == 0 and r_o.scanned_bytes == 0

    if 8 in steps:   # reset and nothing else
        e.reset()
        r_o = done(b"", allow=(fk.FK_E_EMPTY, fk.FK_OK))
        assert r_o.windows == 0 and r_o.distinct == 0

    if 9 in steps:   # dirty again with other bytes, the feed cut into segments
        # (seg_kb is read by segment_budget at every device feed, so the knob
        # applies to this engine from here on)
        data = dirty_input(1)
        _assert_dirty_enough(data, k)
        dev, ptr = to_device(data)
        monkeypatch.setenv("FINDKMER_TUNE", "seg_kb=272")
        e.reset()
        e.feed_device(ptr, len(data))
        done(data)


@pytest.mark.parametrize("k", [7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 20])
def test_reuse_dirty_table(k, monkeypatch):
    """reset(); feed; finish() over and over on ONE engine, every count checked
    whole against the oracle of its own bytes.  After the first step every bin
    (k <= 8) or every slice, coarse slice and part (k >= 12) of the table is
    nonzero, so a reset that leaves a bin behind shows in the next, nearly
    empty, counts: k = 8..11 are zeroed by k_zero (the benchmark's cycle);
    for k = 12..16 the first segment after a reset is a fresh table that the
    counting kernels must write whole, parts without any entry included
    (k_pair_fold, k_bucket16, k_count_parts; general tiles from the list);
    k >= 17 clears its retained segments and reuses their buffers."""
    scratch = table_scratch(k)
    with fk.Engine(k, want_nodes=True, collect_unknown=True) as e:
        _reuse_steps(e, k, True, scratch, monkeypatch, range(1, 10))


@pytest.mark.parametrize("k", [6, 7])
def test_reuse_dirty_table_onepass_reset(k, monkeypatch):
    """without nodeCounter the one-pass k_count does the pending reset itself
    (`fresh` in count_segment; with want_nodes the same k take flush_zero)"""
    with fk.Engine(k, want_nodes=False, collect_unknown=True) as e:
        _reuse_steps(e, k, False, None, monkeypatch, (1, 2, 4))


# ---- C. device-feed cuts, staging tails, borrowed input ---------------------

TAIL_AT = 3 * SEG


@functools.lru_cache(maxsize=None)
def tail_input():
    """~400 KB of mixed input with 2 KiB of plain random ACGT around the third
    64 KiB cut (a '\\n' in front of it ends any comment line), so the bytes
    behind the cut lie in a run and enter k-mers"""
    data = bytearray(mixed_no_ff(3030, 400_000))
    rng = np.random.default_rng(3031)
    data[TAIL_AT - 1025:TAIL_AT - 1024] = b"\n"
    data[TAIL_AT - 1024:TAIL_AT + 1024] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=2048)].tobytes()
    return bytes(data)


@pytest.mark.parametrize("r", [0, 1, 7, 16, 31, 32])
@pytest.mark.parametrize("borrow", [False, True])
@pytest.mark.parametrize("k", [17, 20])
def test_sparse_borrowed_segment_tail(k, borrow, r, monkeypatch):
    """A device feed whose last segment is shorter than a lane: the engine
    moves those r bytes into its staging buffer, and the next staged feeds
    overwrite them there.  With borrow_input the finish re-reads borrowed
    segments from where they were counted, so this tail must have been
    copied, not borrowed.  r = 0 and r = 32 never stage (controls)."""
    data = tail_input()
    n1 = TAIL_AT + r
    rest = data[n1 + 5:]
    assert len(rest) > 100_000
    # what the staging buffer holds at finish where the tail was: the last
    # staged feed's first bytes
    if r >= 1:
        assert data[TAIL_AT:n1] != rest[:r]
    assert all(c in b"ACGT" for c in data[TAIL_AT - 1024:TAIL_AT + 40])
    dev, ptr = to_device(data)
    assert ptr % 16 == 0
    monkeypatch.setenv("FINDKMER_TUNE", "seg_kb=64")
    with fk.Engine(k, want_nodes=True, collect_unknown=True, borrow_input=borrow) as e:
        e.feed_device(ptr, n1)            # 3 segments of 64 KiB and one of r bytes
        e.feed_device(ptr + n1, 5)        # short: staged
        e.feed(host(rest))                # staged
        rc, res = e.finish(allow=ALLOW)
        r_o = check(e, data, k, res)
    assert r_o.hit_eof_byte == 0 and r_o.scanned_bytes == len(data)


@pytest.mark.parametrize("k,borrow", [(15, False), (17, False), (17, True), (20, False), (20, True)])
def test_device_feed_segments_large_k(k, borrow, monkeypatch):
    """test_device_feed_segments for the two-level partition (k = 15: only
    the first segment is a fresh table, the later ones add to it) and the
    sparse table (every segment retained, or borrowed)"""
    data = mixed_no_ff(621, 1_000_000)
    dev, ptr = to_device(data)
    monkeypatch.setenv("FINDKMER_TUNE", "seg_kb=272")
    scratch = table_scratch(k)
    with fk.Engine(k, want_nodes=True, collect_unknown=True, borrow_input=borrow) as e:
        e.feed_device(ptr, len(data))
        rc, res = e.finish(allow=ALLOW)
        check(e, data, k, res, scratch=scratch)


@functools.lru_cache(maxsize=None)
def eof_fasta():
    return random_fasta(4040, 200_000, 60, header_at=(300, 1500, 2500))


def _outside_header(data, p):
    j = data.rfind(b">", 0, p + 1)
    return j < 0 or (j < p and data.find(b"\n", j, p) >= 0)


@pytest.mark.parametrize("where", ["feed", "segment"])
@pytest.mark.parametrize("k", [6, 11, 15, 17, 20])
def test_eof_byte_near_device_feed_start(k, where, monkeypatch):
    """a 0xFF (end of stream) outside a comment line within a lane or so of
    the start of a device feed, or of its second segment: the prefix before
    it is counted again on the caller's buffer, shorter than a lane for the
    first offsets; one engine per (k, where), reset between the offsets"""
    base = eof_fasta()
    start = 0 if where == "feed" else SEG
    if where == "segment":
        monkeypatch.setenv("FINDKMER_TUNE", "seg_kb=64")
    scratch = table_scratch(k)
    with fk.Engine(k, want_nodes=True, collect_unknown=True) as e:
        for o in (0, 5, 31, 32, 33):
            p = start + o
            assert _outside_header(base, p) and base.count(b"\xff") == 0
            data = base[:p] + b"\xff" + base[p + 1:]
            dev, ptr = to_device(data)
            assert dev.numel() == len(data) + 16
            e.reset()
            e.feed_device(ptr, len(data))
            rc, res = e.finish(allow=ALLOW)
            try:
                r_o = check(e, data, k, res, scratch=scratch)
            except AssertionError as err:
                raise AssertionError(f"0xFF at offset {o} of the {where}: {err}") from err
            assert r_o.hit_eof_byte == 1 and r_o.scanned_bytes == p, (o, r_o.scanned_bytes)
