"""The closed-form run model (tests/run_model.py) against the oracle on real
bytes, field by field and over the whole table -- what lets
tests/test_gpu_counter_edge.py state expectations for 4-6 GB inputs without an
oracle pass over them.  No GPU."""
import itertools

import numpy as np
import pytest

import oracle
import run_model

UNITS = [b"A", b"T", b"AC"]
# three-run streams take every length triple with these unit triples (the
# one- and two-run streams take every unit combination)
UNIT_TRIPLES = [(b"A", b"T", b"AC"), (b"AC", b"AC", b"A"), (b"T", b"T", b"T"), (b"A", b"AC", b"A")]


def lengths(k):
    return sorted({0, 1, k - 1, k, k + 1, 37, 1000})


def streams(k):
    ls = lengths(k)
    for n in (1, 2):
        for us in itertools.product(UNITS, repeat=n):
            for lt in itertools.product(ls, repeat=n):
                yield list(zip(us, lt))
    for us in UNIT_TRIPLES:
        for lt in itertools.product(ls, repeat=3):
            yield list(zip(us, lt))


def assert_model_is_oracle(runs, k, tail_newlines=0):
    data = run_model.render(runs, tail_newlines)
    m = run_model.model(runs, k, tail_newlines)
    t_o, r_o, _ = oracle.count_dense(data, k)
    what = f"k={k} runs={runs}"
    assert m.windows == r_o.windows, what
    assert m.valid_bases == r_o.valid_bases, what
    assert m.base_count == list(r_o.base_count), what
    assert m.depth1 == list(r_o.depth1), what
    assert m.distinct == r_o.distinct, what
    assert int(m.rollover) == r_o.rollover, what
    assert m.unknown_chars == r_o.unknown_chars, what
    assert m.scanned_bytes == r_o.scanned_bytes == len(data), what
    # the whole table, zero bins included
    assert np.array_equal(run_model.table_u32(m, k), t_o), what
    assert all(c > 0 for c in m.bins.values()), what


@pytest.mark.parametrize("k", range(1, 8))
def test_model_matches_oracle(k):
    n = 0
    for runs in streams(k):
        assert_model_is_oracle(runs, k)
        n += 1
    assert n >= len(UNITS) + len(UNITS) ** 2 + len(UNIT_TRIPLES)


@pytest.mark.parametrize("k", [2, 6, 7])
def test_model_trailing_newline_and_no_runs(k):
    assert_model_is_oracle([(b"A", 1000), (b"AC", k), (b"T", 37)], k, tail_newlines=1)
    assert_model_is_oracle([], k)
    assert_model_is_oracle([(b"A", 0), (b"A", 0)], k)   # the stream "N"


def test_model_refuses_runs_past_int32():
    run_model.model([(b"A", run_model.MAX_RUN)], 6)
    with pytest.raises(AssertionError):
        run_model.model([(b"A", run_model.MAX_RUN + 1)], 6)


@pytest.mark.parametrize("k", [2, 6, 7])
def test_model_at_the_u32_edge(k):
    """The streams of tests/test_gpu_counter_edge.py: what the model says at
    the sizes no oracle pass reaches (plain arithmetic, stated here once)."""
    R = run_model.MAX_RUN
    below = run_model.model([(b"A", R), (b"A", R), (b"A", 1)], k)
    at = run_model.model([(b"A", R), (b"A", R), (b"A", 2)], k)
    assert below.depth1 == [(1 << 32) - 1, 0, 0, 0] and not below.rollover
    assert at.depth1 == [1 << 32, 0, 0, 0] and at.rollover
    w = 2 * (R - k + 1) + (1 if k == 2 else 0)
    assert at.windows == w and at.bins == {0: w} and w < 1 << 32      # no bin has wrapped
    assert at.scanned_bytes == below.scanned_bytes + 1 == 2 * R + 4
    wrap = run_model.model([(b"A", R)] * 3, k, tail_newlines=1)
    assert wrap.windows == 3 * (R - k + 1) >= 1 << 32 and wrap.rollover
    assert int(run_model.table_u32(wrap, k)[0]) == wrap.windows - (1 << 32)
    assert wrap.scanned_bytes == 3 * R + 3
