"""The string restatement that tests/test_gpu_unitigs.py compares the device against, checked on the CPU before it is trusted there: on
the oracle's solid rows (global order) it must give the numbers fixed for these inputs -- rows, unitigs, longest, single nodes, cycles,
palindromes -- and its stream, counted again by the oracle, must give back exactly the rows, each once."""
import os

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU module imports it at the top)
from tests.test_gpu_unitigs import GOLDEN, PINNED, Restatement, circles_stream, handmade_stream      # noqa: E402


def solid_rows(oracle, stream, k, amin):
    ref = oracle.count(stream, k)
    pairs = sorted((int(v), int(a)) for v, a in zip(ref.values(), ref.ab) if a >= amin)
    return [p[0] for p in pairs], [p[1] for p in pairs]


def check(oracle, stream, k, amin, pinned):
    values, ab = solid_rows(oracle, stream, k, amin)
    exp = Restatement(values, ab, k)
    s = exp.stats
    assert (exp.n, s["n_unitigs"], s["max_nodes"], s["n_single"], s["n_cycles"], exp.n_palindromes) == pinned
    back = oracle.count(exp.stream.copy(), k)
    assert sorted(int(v) for v in back.values()) == values and (np.asarray(back.ab) == 1).all()
    assert int(exp.ab_sum.sum()) == sum(ab)
    return exp


@pytest.mark.parametrize("k", sorted(k for kind, k in PINNED if kind == "hand"))
def test_handmade_stream(oracle, k):
    check(oracle, handmade_stream(k), k, 1, PINNED[("hand", k)])


@pytest.mark.parametrize("k", [31, 96])
def test_golden_reads(oracle, golden_dir, k):
    stream = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
    check(oracle, stream, k, 2, PINNED[("golden", k)])


def test_long_chain_and_two_circles(oracle):
    exp = check(oracle, circles_stream(31), 31, 1, (28193, 3, 20000, 0, 2, 0))
    assert sorted(len(p) for p, _ in exp.paths) == [4096, 4097, 20000]
    for path, cyc in exp.paths:
        if cyc:                                                              # a cycle starts at its smallest row, forward
            assert path[0] == 2 * min(p >> 1 for p in path)
