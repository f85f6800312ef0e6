"""The u32 counter edge on the device, the sparse merge against numpy, and the
one-shot entry points.

  - Rollover (FK_E_ROLLOVER, the reference's COUNTER ROLLOVER exit,
    findKmer.cpp:642-648) produced by real streams through the one-pass
    k_count (k <= 7): the `>=` at exactly 2^32, a bin that wraps, a wrap that
    only a merge of engines produces.  The expectations for these 2-6 GB
    poly-A streams come from tests/run_model.py (checked against the oracle
    on the CPU by tests/test_run_model_cpu.py).  Rollover at k >= 8 on a real
    stream is not covered: nobody has measured a multi-GB poly-A feed through
    k_part, and at k >= 17 one block counts a 2^32-window part for tens of
    seconds.
  - fk_engine_sparse_adopt (fks_merge_runs: run starts, merge-path rounds,
    equal keys summed, statistics) and the readers of the table it leaves
    (sparse_split, sparse_range, sparse_device) against a few lines of numpy.
  - fk_count / fk_count_multi, fk_engine_table_from_device, and the refusals
    of fk_engine_merge_from.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import findkmer_amd as fk
import oracle
import run_model
from test_gpu_parity import mixed_input

pytestmark = pytest.mark.gpu

R = (1 << 31) - 1    # the longest run before the reference's int32 seqSize wraps (:977)
A, N, NL = ord("A"), ord("N"), ord("\n")
DONE = (fk.FK_OK, fk.FK_E_EMPTY, fk.FK_E_UNTERMINATED_HEADER, fk.FK_E_ROLLOVER)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if fk.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    yield
    for e in _FINISHED.values():
        e.close()
    _FINISHED.clear()


# ---- 2. real rollover on the device path (k <= 7) ---------------------------

@contextlib.contextmanager
def poly_a(nbytes, other):
    """the address of a device buffer of `nbytes` 'A' with the single bytes
    {offset: byte}; freed on exit, before the next test allocates its own"""
    import torch
    buf = torch.full((nbytes,), A, dtype=torch.uint8, device="cuda")
    try:
        for at, byte in other.items():
            buf[at:at + 1].fill_(byte)
        torch.cuda.synchronize()
        yield buf.data_ptr()
    finally:
        del buf
        torch.cuda.empty_cache()


def assert_is_model(r, table, m, k, what, table_fields=True):
    """every parity field of fk_result and the whole table against the model;
    table_fields=False leaves out the fields fk_engine_finish derives from
    sums over the u32 table (after a bin wrapped they describe the wrapped
    table, include/findkmer.h)"""
    assert r.windows == m.windows, what
    assert r.valid_bases == m.valid_bases, what
    assert r.unknown_chars == m.unknown_chars, what
    assert r.scanned_bytes == m.scanned_bytes, what
    assert r.hit_eof_byte == 0 and r.unterminated_header == 0, what
    assert r.rollover == int(m.rollover), what
    if table_fields:
        assert list(r.base_count) == m.base_count, what
        assert list(r.depth1) == m.depth1, what
        assert r.distinct == m.distinct, what
    want = run_model.table_u32(m, k)
    bad = np.nonzero(table != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} bins differ, first {bad[:8]} model={want[bad[:8]]} gpu={table[bad[:8]]}"


@pytest.mark.parametrize("k", [2, 6, 7])
def test_rollover_threshold(k):
    """A^R N A^R N A A: without its last byte depth1[A] is 2^32 - 1 (FK_OK),
    with it exactly 2^32 (the reference's exit, :642) while no bin has
    wrapped -- fk_engine_finish's `>=`, which the table total cannot stand in
    for here."""
    n = 2 * R + 4
    below = run_model.model([(b"A", R), (b"A", R), (b"A", 1)], k)
    at = run_model.model([(b"A", R), (b"A", R), (b"A", 2)], k)
    assert below.depth1[0] == (1 << 32) - 1 and at.depth1[0] == 1 << 32
    assert max(at.bins.values()) < 1 << 32
    with poly_a(n, {R: N, 2 * R + 1: N}) as ptr, fk.Engine(k) as e:
        e.feed_device(ptr, n - 1)
        rc, r = e.finish(allow=DONE)
        assert rc == fk.FK_OK, f"k={k}: depth1[A] = 2^32 - 1 is no rollover, got rc {rc} depth1 {list(r.depth1)}"
        assert_is_model(r, e.table(), below, k, f"k={k} below")
        e.reset()
        e.feed_device(ptr, n)
        rc, r = e.finish(allow=DONE)
        assert rc == fk.FK_E_ROLLOVER, f"k={k}: depth1[A] = 2^32 is the rollover, got rc {rc} depth1 {list(r.depth1)}"
        assert r.depth1[0] == 4294967296
        assert_is_model(r, e.table(), at, k, f"k={k} at")
        # the same stream with its last byte as a feed of its own (staged: it
        # is shorter than a lane): the counter crosses 2^32 between two feeds
        e.reset()
        e.feed_device(ptr, n - 1)
        e.feed_device(ptr + n - 1, 1)
        rc, r = e.finish(allow=DONE)
        assert rc == fk.FK_E_ROLLOVER and r.depth1[0] == 4294967296
        assert_is_model(r, e.table(), at, k, f"k={k} at, two feeds")


@pytest.mark.parametrize("k", [2, 6])
def test_rollover_bin_wrap(k):
    """A^R N A^R N A^R \\n: bin 0 holds 3(R - k + 1) >= 2^32 windows and wraps,
    the table total falls 2^32 short of the windows (fk_engine_finish's second
    test).  base_count, depth1 and distinct are computed from the wrapped
    table and are not compared (include/findkmer.h at FK_E_ROLLOVER)."""
    n = 3 * R + 3
    m = run_model.model([(b"A", R)] * 3, k, tail_newlines=1)
    with poly_a(n, {R: N, 2 * R + 1: N, n - 1: NL}) as ptr, fk.Engine(k) as e:
        e.feed_device(ptr, n)
        rc, r = e.finish(allow=DONE)
        t = e.table()
    assert rc == fk.FK_E_ROLLOVER and r.rollover == 1
    assert r.windows == 3 * (R - k + 1)
    assert int(t[0]) == r.windows - (1 << 32)
    assert int(t.sum(dtype=np.uint64)) == r.windows - (1 << 32)
    assert_is_model(r, t, m, k, f"k={k} wrap", table_fields=False)


def test_rollover_by_merge():
    """three k = 6 engines, A^R each: two merged stay below 2^32 in every
    counter, the third merge wraps bin 0 (fk_engine_merge_from's u32 adds)"""
    k = 6
    engines = [fk.Engine(k) for _ in range(3)]
    try:
        with poly_a(R, {}) as ptr:
            for e in engines:
                e.feed_device(ptr, R)
            e0 = engines[0]
            assert fk.lib().fk_engine_merge_from(e0.h, engines[1].h) == fk.FK_OK
            rc, r = e0.finish(allow=DONE)
            t = e0.table()
            two = run_model.model([(b"A", R)] * 2, k)
            assert rc == fk.FK_OK and r.rollover == 0
            assert int(t[0]) == 2 * (R - 5)
            assert r.windows == two.windows and r.valid_bases == two.valid_bases
            assert list(r.base_count) == two.base_count and list(r.depth1) == two.depth1 and r.distinct == 1
            assert np.array_equal(t, run_model.table_u32(two, k))
            assert fk.lib().fk_engine_merge_from(e0.h, engines[2].h) == fk.FK_OK
            rc, r = e0.finish(allow=DONE)
            t = e0.table()
            three = run_model.model([(b"A", R)] * 3, k)
            assert rc == fk.FK_E_ROLLOVER and r.rollover == 1
            assert r.windows == three.windows == 3 * (R - 5) and r.valid_bases == three.valid_bases
            assert int(t[0]) == 3 * (R - 5) - (1 << 32)
            assert np.array_equal(t, run_model.table_u32(three, k))
    finally:
        for e in engines:
            e.close()


# ---- 3. fk_engine_sparse_adopt and its readers against numpy ----------------

_FINISHED = {}


def finished_engine(k):
    """a finished sparse engine (adopt and the readers need one), one per k
    for the module: every adopt replaces its whole table"""
    if k not in _FINISHED:
        e = fk.Engine(k)
        e.feed(np.frombuffer(b"ACGT" * 10, dtype=np.uint8).copy())
        e.finish()
        _FINISHED[k] = e
    return _FINISHED[k]


def to_device(keys, cnts):
    """uint64 keys / uint32 counts as torch.int64 / torch.int32 device tensors
    (one element when empty, so that the pointers are real)"""
    import torch
    kd = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64).copy()).cuda() if len(keys) \
        else torch.zeros(1, dtype=torch.int64, device="cuda")
    cd = torch.from_numpy(np.ascontiguousarray(cnts, dtype=np.uint32).view(np.int32).copy()).cuda() if len(keys) \
        else torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return kd, cd


def adopt(e, keys, cnts):
    kd, cd = to_device(keys, cnts)
    return e.sparse_adopt(kd.data_ptr(), cd.data_ptr(), len(keys))


def merged(keys, cnts):
    """the reference: (distinct keys ascending, their summed counts mod 2^32,
    the exact total)"""
    keys = np.asarray(keys, dtype=np.uint64)
    cnts = np.asarray(cnts, dtype=np.uint32)
    keys_o, inv = np.unique(keys, return_inverse=True)
    c64 = np.zeros(len(keys_o), dtype=np.uint64)
    np.add.at(c64, inv.reshape(-1), cnts.astype(np.uint64))
    cnt_o = (c64 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return keys_o, cnt_o, int(cnts.sum(dtype=np.uint64))


def assert_adopt(k, keys, cnts, what):
    keys = np.asarray(keys, dtype=np.uint64)
    cnts = np.asarray(cnts, dtype=np.uint32)
    assert len(keys) == len(cnts) and (len(keys) == 0 or int(keys.max()) < 1 << (2 * k))
    keys_o, cnt_o, exact = merged(keys, cnts)
    e = finished_engine(k)
    st = adopt(e, keys, cnts)
    keys_g, cnt_g = e.sparse()
    assert len(keys_g) == len(keys_o), f"{what}: {len(keys_g)} keys, numpy has {len(keys_o)}"
    bad = np.nonzero(keys_g != keys_o)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} keys differ, first at {bad[:4]} numpy={keys_o[bad[:4]]} gpu={keys_g[bad[:4]]}"
    bad = np.nonzero(cnt_g != cnt_o)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} counts differ, first at {bad[:4]} numpy={cnt_o[bad[:4]]} gpu={cnt_g[bad[:4]]}"
    total = int(cnt_o.sum(dtype=np.uint64))
    assert st == (len(keys_o), total), f"{what}: stats {st}, numpy {(len(keys_o), total)}"
    # the header's contract: short of the exact total by whole wraps only
    assert exact >= st[1] and (exact - st[1]) % (1 << 32) == 0, what
    return keys_o, cnt_o


def universe(rng, k, n):
    """n distinct keys spread over [0, 4^k), ascending"""
    u = np.unique(rng.integers(0, 1 << (2 * k), size=n + n // 8, dtype=np.uint64))
    assert len(u) >= n
    return np.sort(rng.choice(u, size=n, replace=False))


def sources(rng, univ, lens):
    """one ascending source per length, drawn without replacement from univ,
    concatenated; counts 1..1000"""
    parts = [np.sort(rng.choice(univ, size=n, replace=False)) for n in lens]
    keys = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
    return keys.astype(np.uint64), rng.integers(1, 1001, size=len(keys), dtype=np.uint32)


def ragged(rng, total, s, cap):
    """s ragged lengths <= cap that sum to total"""
    assert total <= s * cap
    while True:
        cuts = np.sort(rng.integers(0, total + 1, size=s - 1))
        lens = np.diff(np.concatenate([[0], cuts, [total]]))
        if lens.max() <= cap:
            return [int(x) for x in lens]


WORLDS = [1, 2, 3, 5, 7, 8]


def owner_edges(k):
    """r*S - 1, r*S, r*S + 1 for every owner bound of every world in WORLDS
    (S = ceil(4^k / world)), inside [0, 4^k)"""
    nb = 1 << (2 * k)
    out = set()
    for world in WORLDS:
        S = (nb + world - 1) // world
        for r in range(world + 1):
            out.update(x for x in (r * S - 1, r * S, r * S + 1) if 0 <= x < nb)
    return np.array(sorted(out), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def big_case(k):
    """about 300 000 entries: 8 ragged ascending sources over a universe of
    60 000 keys (3000 keys would cap 8 sources at 24 000 entries; most keys
    still occur in several sources), and the owner bounds' neighbours as a
    ninth.  Shared by the shapes test and the readers' test; read-only."""
    rng = np.random.default_rng(300 + k)
    univ = universe(rng, k, 60_000)
    keys, cnts = sources(rng, univ, ragged(rng, 300_000, 8, 60_000))
    edges = owner_edges(k)
    keys = np.concatenate([keys, edges])
    cnts = np.concatenate([cnts, rng.integers(1, 1001, size=len(edges), dtype=np.uint32)])
    keys.setflags(write=False)
    cnts.setflags(write=False)
    return keys, cnts


def shape_case(k, name):
    rng = np.random.default_rng(1000 * k + sum(map(ord, name)))
    univ = universe(rng, k, 3000)
    if name == "empty":
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    if name == "one_key":
        return univ[1500:1501].copy(), np.array([77], dtype=np.uint32)
    if name == "big":
        return big_case(k)
    if name == "empty_and_one_element_sources":
        return sources(rng, univ, [1000, 0, 1, 1047, 0])
    if name == "fused_sources":
        # the second source lies wholly above the first: one natural run; the
        # third overlaps both (2 runs from 3 sources, 2049 entries)
        lo, _ = sources(rng, univ[:1500], [700])
        hi, _ = sources(rng, univ[1500:], [600])
        mid, _ = sources(rng, univ, [749])
        keys = np.concatenate([lo, hi, mid])
        assert int(hi[0]) > int(lo[-1])
        return keys, rng.integers(1, 1001, size=len(keys), dtype=np.uint32)
    s, total = name.split("x")
    return sources(rng, univ, ragged(rng, int(total), int(s), 3000))


# <sources>x<total>: totals around the 2048-output merge block (256 threads x
# MP_PER) and the 4096-item selection tile (FKS_TILE); odd and even run counts
SHAPES = ["empty", "one_key", "1x2047", "2x2048", "3x2049", "5x4095", "8x4096", "3x4097", "5x2048", "2x4097",
          "empty_and_one_element_sources", "fused_sources", "big"]


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("k", [17, 20])
def test_adopt_shapes(k, name):
    keys, cnts = shape_case(k, name)
    if "x" in name:
        assert len(keys) == int(name.split("x")[1])
    keys_o, _ = assert_adopt(k, keys, cnts, f"k={k} {name}")
    if name == "empty":
        assert len(keys_o) == 0
    elif name not in ("one_key", "1x2047"):
        assert len(keys_o) < len(keys)       # sources share keys


@pytest.mark.parametrize("k", [17, 20])
def test_adopt_identical_sources(k):
    rng = np.random.default_rng(k)
    run = universe(rng, k, 5000)
    c = rng.integers(1, 1001, size=5000, dtype=np.uint32)
    keys_o, cnt_o = assert_adopt(k, np.tile(run, 8), np.tile(c, 8), f"k={k} 8 identical sources")
    assert np.array_equal(keys_o, run) and np.array_equal(cnt_o, c * np.uint32(8))


@pytest.mark.parametrize("order", ["descending", "shuffled"])
@pytest.mark.parametrize("k", [17, 20])
def test_adopt_any_order(k, order):
    """the header promises any order: 5000 one-key natural runs, and 20 000
    shuffled entries with repeats"""
    rng = np.random.default_rng(7 * k)
    if order == "descending":
        keys = universe(rng, k, 5000)[::-1].copy()
        assert np.all(keys[1:] < keys[:-1])
    else:
        keys = rng.choice(universe(rng, k, 3000), size=20_000, replace=True)
    assert_adopt(k, keys, rng.integers(1, 1001, size=len(keys), dtype=np.uint32), f"k={k} {order}")


@pytest.mark.parametrize("k", [17, 20])
def test_adopt_key_space_edges(k):
    rng = np.random.default_rng(11 * k)
    nb = 1 << (2 * k)
    univ = universe(rng, k, 3000)
    x = int(univ[1000]) & ~3                      # x, x + 3: differ only in their last base
    y = int(univ[2000]) % (1 << (2 * (k - 1)))    # y, y + 3 * 4^(k-1): only in their first base
    special = np.array([0, nb - 1, x, x + 3, y, y + 3 * (1 << (2 * (k - 1)))], dtype=np.uint64)
    parts = []
    for i, n in enumerate([900, 1200, 1, 700, 1100]):
        own = special if i != 2 else special[:2]      # keys 0 and 4^k - 1 in every source
        parts.append(np.unique(np.concatenate([rng.choice(univ, size=n, replace=False), own])))
    keys = np.concatenate(parts)
    keys_o, _ = assert_adopt(k, keys, rng.integers(1, 1001, size=len(keys), dtype=np.uint32), f"k={k} edges")
    assert keys_o[0] == 0 and keys_o[-1] == nb - 1 and set(special.tolist()) <= set(keys_o.tolist())


@pytest.mark.parametrize("k", [17, 20])
def test_adopt_u32_edge(k):
    """summed counts of 2^32 - 1 (stays), exactly 2^32 (count 0, the key stays
    in the table) and 2^32 + 7 (count 7): the u32 frequency of the reference
    (:110), and stats[1] short of the exact total by whole wraps"""
    rng = np.random.default_rng(13 * k)
    univ = universe(rng, k, 3000)
    a, b, c = (np.uint64(int(univ[i])) for i in (17, 1500, 2990))
    give = {int(a): [1 << 31, 1 << 30, (1 << 30) - 1], int(b): [1 << 31, 1 << 30, 1 << 30],
            int(c): [0xFFFFFFFF, 5, 3]}
    rest = np.setdiff1d(univ, np.array([a, b, c], dtype=np.uint64))
    ks, cs = [], []
    for i, n in enumerate([1500, 800, 2000]):
        body = rng.choice(rest, size=n, replace=False)
        src = np.sort(np.concatenate([body, np.array([a, b, c], dtype=np.uint64)]))
        cnt = rng.integers(1, 1001, size=len(src), dtype=np.uint32)
        for key, vals in give.items():
            cnt[src == np.uint64(key)] = vals[i]
        ks.append(src)
        cs.append(cnt)
    keys, cnts = np.concatenate(ks), np.concatenate(cs)
    keys_o, cnt_o = assert_adopt(k, keys, cnts, f"k={k} u32 edge")
    at = {int(key): int(cnt_o[np.searchsorted(keys_o, np.uint64(key))]) for key in give}
    assert at == {int(a): 4294967295, int(b): 0, int(c): 7}
    assert int(cnts.sum(dtype=np.uint64)) - int(cnt_o.sum(dtype=np.uint64)) == 2 << 32


def np_range(keys_o, cnt_o, lo, hi):
    i, j = np.searchsorted(keys_o, np.uint64(lo)), np.searchsorted(keys_o, np.uint64(hi))
    return keys_o[i:j], cnt_o[i:j]


@pytest.mark.parametrize("k", [17, 20])
def test_adopted_table_readers(k):
    """sparse_split, sparse_range and sparse_device over the adopted table of
    about 300 000 entries that holds every owner bound and its neighbours"""
    import torch
    nb = 1 << (2 * k)
    keys, cnts = big_case(k)
    keys_o, cnt_o, _ = merged(keys, cnts)
    n = len(keys_o)
    e = finished_engine(k)
    try:
        assert adopt(e, keys, cnts)[0] == n
        for world in WORLDS:
            S = (nb + world - 1) // world
            want = np.bincount((keys_o // np.uint64(S)).astype(np.int64), minlength=world)
            assert e.sparse_split(world) == want.tolist(), f"k={k} world={world}"
            assert min(want) > 0
        mid = int(keys_o[n // 2])
        ranges = [(0, nb), (0, 0), (mid, mid), (mid + 1, mid + 1),              # lo == hi, on a key and off
                  (int(keys_o[100]), int(keys_o[n - 100])),                      # both on present keys: hi exclusive
                  (int(keys_o[100]), int(keys_o[100]) + 1), (int(keys_o[100]) + 1, int(keys_o[101])),
                  (int(keys_o[-1]), nb), (int(keys_o[-1]) + 1 if int(keys_o[-1]) + 1 < nb else nb, nb),
                  (nb, nb), (0, int(keys_o[0])), (0, int(keys_o[0]) + 1)]
        for lo, hi in ranges:
            kg, cg = e.sparse_range(lo, hi)
            kw, cw = np_range(keys_o, cnt_o, lo, hi)
            assert np.array_equal(kg, kw) and np.array_equal(cg, cw), f"k={k} range [{lo}, {hi}): {len(kg)} vs {len(kw)}"
        assert len(e.sparse_range(int(keys_o[100]), int(keys_o[n - 100]))[0]) == n - 200
        with pytest.raises(fk.FindKmerError) as err:
            e.sparse_range(mid + 1, mid)
        assert err.value.code == fk.FK_E_INVALID
        # a short host buffer takes the first `cap` entries and still reports n
        cap, got = 1000, ctypes.c_uint64()
        hk, hc = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        assert fk.lib().fk_engine_sparse_range(e.h, 0, nb, hk.ctypes.data_as(fk._U64P), hc.ctypes.data_as(fk._U32P),
                                               cap, ctypes.byref(got)) == fk.FK_OK
        assert got.value == n and np.array_equal(hk, keys_o[:cap]) and np.array_equal(hc, cnt_o[:cap])
        # sparse_device: the whole table into device buffers with room to spare
        dk = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda")
        dc = torch.full((n + 8,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert e.sparse_device(dk.data_ptr(), dc.data_ptr(), n + 8) == n
        hk, hc = dk.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint32)
        sk, sc = e.sparse()
        assert np.array_equal(hk[:n], sk) and np.array_equal(hc[:n], sc) and np.array_equal(sk, keys_o)
        assert np.all(hk[n:] == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(hc[n:] == np.uint32(0xFFFFFFFF))
        # exactly n fits; NULL buffers ask for n alone
        assert e.sparse_device(dk.data_ptr(), dc.data_ptr(), n) == n
        assert e.sparse_device(None, None, 0) == n
        # cap < n: FK_E_INVALID, n still reported, nothing copied (sparse_copy)
        dk.fill_(-1)
        dc.fill_(-1)
        torch.cuda.synchronize()
        got = ctypes.c_uint64()
        assert fk.lib().fk_engine_sparse_device(e.h, dk.data_ptr(), dc.data_ptr(), n - 1, ctypes.byref(got)) \
            == fk.FK_E_INVALID
        assert got.value == n
        assert bool((dk == -1).all()) and bool((dc == -1).all())
        del dk, dc
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [17, 20])
def test_sparse_split_one_owner_and_empty(k):
    nb = 1 << (2 * k)
    rng = np.random.default_rng(5 * k)
    e = finished_engine(k)
    S = (nb + 4) // 5
    keys = np.unique(rng.integers(2 * S, 3 * S, size=500, dtype=np.uint64))      # owner 2 of 5 holds them all
    keys = np.union1d(keys, np.array([2 * S, 3 * S - 1], dtype=np.uint64))
    adopt(e, keys, np.ones(len(keys), dtype=np.uint32))
    assert e.sparse_split(5) == [0, 0, len(keys), 0, 0]
    assert e.sparse_split(1) == [len(keys)]
    assert len(e.sparse_range(3 * S, nb)[0]) == 0            # lo past the last key
    assert len(e.sparse_range(2 * S, 3 * S)[0]) == len(keys)
    assert adopt(e, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)) == (0, 0)
    for world in WORLDS:
        assert e.sparse_split(world) == [0] * world
    kg, cg = e.sparse_range(0, nb)
    assert len(kg) == 0 and len(cg) == 0 and len(e.sparse()[0]) == 0


# ---- 4. the one-shot entry points and the table's way back -----------------

def assert_count_is_oracle(rc, t, r, data, k, nodes):
    t_o, r_o, _ = oracle.count_dense(data, k)
    assert rc == (fk.FK_E_UNTERMINATED_HEADER if r_o.unterminated_header else fk.FK_OK)
    bad = np.nonzero(t != t_o)[0]
    assert len(bad) == 0, f"k={k}: {len(bad)} bins differ, first {bad[:8]} oracle={t_o[bad[:8]]} gpu={t[bad[:8]]}"
    assert list(r.base_count) == list(r_o.base_count)
    assert r.valid_bases == r_o.valid_bases and r.windows == r_o.windows and r.distinct == r_o.distinct
    assert list(r.depth1) == list(r_o.depth1)
    assert r.unknown_chars == r_o.unknown_chars and r.scanned_bytes == r_o.scanned_bytes
    assert r.hit_eof_byte == r_o.hit_eof_byte and r.unterminated_header == r_o.unterminated_header
    assert r.rollover == 0
    if nodes:
        assert r.nodes_valid == 1 and r.nodes == r_o.nodes


@pytest.mark.parametrize("k", [3, 11, 13])
def test_count_one_shot(k):
    data = mixed_input(4100 + k, 300_000)
    rc, t, r = fk.count(data, k, want_nodes=True)
    assert_count_is_oracle(rc, t, r, data, k, nodes=True)
    # ngpu = 2: fk_count_multi where two GPUs are visible, else its fall-back
    # to the single path; the same table either way (nodeCounter's short walks
    # belong to the last shard, as in assert_same)
    rc2, t2, r2 = fk.count(data, k, ngpu=2)
    assert_count_is_oracle(rc2, t2, r2, data, k, nodes=False)
    assert np.array_equal(t, t2)


def test_count_one_shot_empty_and_open_header():
    rc, t, r = fk.count(b"", 6)
    assert rc == fk.FK_E_EMPTY and not t.any() and r.windows == 0 and r.scanned_bytes == 0
    rc, t, r = fk.count(b">abc", 6)
    assert rc == fk.FK_E_UNTERMINATED_HEADER and r.unterminated_header == 1
    assert not t.any() and r.windows == 0 and r.scanned_bytes == 4
    # the table is copied out in this case: a caller's stale buffer is overwritten
    stale = np.full(1 << 12, 7, dtype=np.uint32)
    buf = np.frombuffer(b">abc", dtype=np.uint8).copy()
    o = fk.FkOpts()
    o.device = -1
    rc = fk.lib().fk_count(buf.ctypes.data, 4, 6, ctypes.byref(o), stale.ctypes.data_as(fk._U32P), None)
    assert rc == fk.FK_E_UNTERMINATED_HEADER and not stale.any()


@pytest.mark.parametrize("k", [6, 12])
def test_table_to_and_from_device(k):
    import torch
    data = mixed_input(4200 + k, 300_000)
    t_o, _, _ = oracle.count_dense(data, k)
    dev = torch.zeros(1 << (2 * k), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with fk.Engine(k) as a, fk.Engine(k) as b:
        a.feed(np.frombuffer(data, dtype=np.uint8).copy())
        a.finish(allow=DONE)
        a.table_to_device(dev.data_ptr())
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), t_o)
        b.feed(np.frombuffer(b"TTTTTTTTTTTTTTTTTTTTTTTT", dtype=np.uint8).copy())   # replaced, not added to
        b.table_from_device(dev.data_ptr())
        assert np.array_equal(b.table(), t_o)
        assert np.array_equal(b.table_range(5, 1000), t_o[5:1005])
        assert np.array_equal(a.table(), t_o)
    with fk.Engine(17) as s:
        for call in (s.table_from_device, s.table_to_device):
            with pytest.raises(fk.FindKmerError) as err:
                call(dev.data_ptr())
            assert err.value.code == fk.FK_E_INVALID
    del dev
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [3, 6, 11])
def test_merge_from_with_nodes(k):
    """two finished want_nodes engines merged (tables, counters and short-walk
    counts added): what one stream `first N second` gives, nodeCounter and the
    prefix-only walks at both streams' ends included"""
    first = mixed_input(4400 + k, 120_000).replace(b"\xff", b"Z") + b"\nAC"
    second = mixed_input(4500 + k, 90_000).replace(b"\xff", b"Z") + b"\nT"
    t_o, r_o, _ = oracle.count_dense(first + b"N" + second, k)
    with fk.Engine(k, want_nodes=True) as a, fk.Engine(k, want_nodes=True) as b:
        a.feed(np.frombuffer(first, dtype=np.uint8).copy())
        b.feed(np.frombuffer(second, dtype=np.uint8).copy())
        assert a.finish(allow=DONE)[0] == fk.FK_OK and b.finish(allow=DONE)[0] == fk.FK_OK
        assert fk.lib().fk_engine_merge_from(a.h, b.h) == fk.FK_OK
        rc, r = a.finish(allow=DONE)
        t = a.table()
    assert rc == fk.FK_OK and np.array_equal(t, t_o)
    assert list(r.base_count) == list(r_o.base_count) and list(r.depth1) == list(r_o.depth1)
    assert r.valid_bases == r_o.valid_bases and r.windows == r_o.windows and r.distinct == r_o.distinct
    assert r.unknown_chars == r_o.unknown_chars
    assert r.nodes_valid == 1 and r.nodes == r_o.nodes


def test_merge_from_refusals():
    """different k, want_nodes on one side only, a sparse engine on either
    side: FK_E_INVALID, the destination's table as it was"""
    data = np.frombuffer(mixed_input(4300, 100_000), dtype=np.uint8).copy()
    merge = fk.lib().fk_engine_merge_from

    def fed(k, **kw):
        e = fk.Engine(k, **kw)
        e.feed(data)
        e.finish(allow=DONE)
        return e

    k6, k5, k6n, k6n2 = fed(6), fed(5), fed(6, want_nodes=True), fed(6, want_nodes=True)
    s17, s17b = fed(17), fed(17)
    try:
        t6, t6n = k6.table(), k6n.table()
        sk, sc = s17.sparse()
        assert t6.any() and len(sk)
        for dst, src in [(k6, k5), (k5, k6), (k6, k6n), (k6n, k6), (k6, s17), (s17, k6), (s17, s17b)]:
            assert merge(dst.h, src.h) == fk.FK_E_INVALID
        assert merge(k6.h, None) == fk.FK_E_INVALID and merge(None, k6.h) == fk.FK_E_INVALID
        assert np.array_equal(k6.table(), t6) and np.array_equal(k6n.table(), t6n)
        sk2, sc2 = s17.sparse()
        assert np.array_equal(sk, sk2) and np.array_equal(sc, sc2)
        rc, r = k6.finish(allow=DONE)
        assert int(k6.table().sum(dtype=np.uint64)) == r.windows
        # two engines that both keep short-walk counts do merge: the table doubles
        assert merge(k6n.h, k6n2.h) == fk.FK_OK
        assert np.array_equal(k6n.table(), t6n * np.uint32(2))
    finally:
        for e in (k6, k5, k6n, k6n2, s17, s17b):
            e.close()
