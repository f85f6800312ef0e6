"""Closed-form model of the scan over streams of periodic runs.

A stream here is a list of runs separated by one 'N' each; a run is a unit of
one or two bases repeated and cut to `length` bases (length 0: an empty run,
two separators side by side).  For such a stream everything the oracle
(oracle/fk_oracle.c, the restatement of findKmer.cpp:962-1069) reports follows
from the run lengths alone, so a test can state exact expectations for a
multi-GB input without an oracle pass over its bytes:

  - a run of L >= k bases has L - k + 1 windows; its first window counts k
    bases and every later one its new base (:1035-1057), so the run adds all
    its L bases to baseCounter and base_count; a shorter run adds nothing;
  - every window adds 1 to depth1[its first base]; the run's first
    min(L, k - 1) bases are prefix-only walks (:1059-1062, fk_oracle.c:135-137)
    and add 1 each to depth1[the run's first base];
  - a unit of p bases has at most p different windows: the window starting at
    base j is the one of residue j mod p.

Counts are exact Python ints (a u32 table holds them mod 2^32: table_u32).
tests/test_run_model_cpu.py checks the model against the oracle on real bytes.
"""
from collections import namedtuple

CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
MAX_RUN = (1 << 31) - 1   # the reference's int32 seqSize wraps past this (:977): out of scope

Model = namedtuple("Model", "windows valid_bases base_count depth1 distinct bins rollover unknown_chars "
                            "scanned_bytes")


def _check(runs, k):
    assert k >= 1
    for unit, length in runs:
        assert len(unit) in (1, 2) and all(c in CODE for c in unit), unit
        assert 0 <= length <= MAX_RUN, f"run length {length}: longer than 2^31 - 1 is out of scope"


def model(runs, k, tail_newlines=0):
    """runs: [(unit: bytes of 1 or 2 bases, length)], one 'N' between runs,
    `tail_newlines` '\\n' bytes after the last run (transparent, :1011).
    Returns a Model; bins = {k-mer index: exact count} of the nonzero bins."""
    _check(runs, k)
    windows = valid = 0
    base_count = [0, 0, 0, 0]
    depth1 = [0, 0, 0, 0]
    bins = {}
    for unit, L in runs:
        p = len(unit)
        u = [CODE[c] for c in unit]
        depth1[u[0]] += min(L, k - 1)
        if L < k:
            continue
        W = L - k + 1
        windows += W
        valid += L
        for r in range(p):
            base_count[u[r]] += (L + p - 1 - r) // p          # bases i < L with i mod p == r
            nw = (W + p - 1 - r) // p                          # windows j < W with j mod p == r
            if not nw:
                continue
            depth1[u[r]] += nw
            code = 0
            for i in range(k):
                code = (code << 2) | u[(r + i) % p]
            bins[code] = bins.get(code, 0) + nw
    nbytes = sum(L for _, L in runs) + max(0, len(runs) - 1) + tail_newlines
    return Model(windows=windows, valid_bases=valid, base_count=base_count, depth1=depth1, distinct=len(bins),
                 bins=bins, rollover=any(d >= 1 << 32 for d in depth1), unknown_chars=0, scanned_bytes=nbytes)


def table_u32(m, k):
    """The model's bins as the u32 table holds them (counts mod 2^32, the
    reference's `unsigned int frequency`, :110), numpy uint32[4^k]."""
    import numpy as np
    t = np.zeros(1 << (2 * k), dtype=np.uint32)
    for code, c in m.bins.items():
        t[code] = c & 0xFFFFFFFF
    return t


def render(runs, tail_newlines=0):
    """The stream's bytes (small runs only: the CPU check of the model)."""
    _check(runs, 1)
    return b"N".join((unit * (L // len(unit) + 1))[:L] for unit, L in runs) + b"\n" * tail_newlines
