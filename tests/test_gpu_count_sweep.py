"""The sweep of the list-free count kernels (k_count1v3, k_count2v3) at the shapes that decide its passes.

After a sub-partition's inserts every wave holds the table slots its lanes claimed (one per distinct k-mer); it ranks them by ballot,
packs the slot indices into a list of its own and sweeps them 64 at a time: ceil(T / 64) passes for the T claims of a wave.  A mean
sub-partition gives a wave about 180 keys, so the streams here set T by how many of those keys are distinct:

  all distinct    independent random reads: every key claims, T ~ 180, three passes with full lanes
  repeats         ~100x coverage of a small genome: ~30 distinct k-mers per sub-partition, most waves have T = 0, the rest a few lanes
  mixed           ~3x coverage with 1 % errors: six (k = 31) or eight (k = 63) keys of ten are distinct, T ~ 110 and ~ 130 in a full
                  wave, fewer in the waves that hold a sub-partition's last keys: the pass boundaries at 64 and 128

each at k = 31 (k_count1v3) and k = 63 (k_count2v3), on two levels.  Every comparison is exact against the CPU oracle, as in
tests/test_gpu_abundance_edges.py: rows in the oracle's order, abundances, the whole histogram, n_kmers, n_distinct, n_solid.
"""
import numpy as np
import pytest

from tests.test_gpu_abundance_edges import ACGT, MAX, RL, check_exact, run_count

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HMAX = 10000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


def as_stream(reads):
    return np.concatenate([reads, np.full((len(reads), 1), ord("\n"), np.uint8)], axis=1).reshape(-1)


def random_reads(rng, n_reads):
    return as_stream(rng.choice(ACGT, size=(n_reads, RL)))


def genome_reads(rng, n_reads, genome_len, error_rate=0.0):
    """reads of one strand of a random genome; error_rate: the share of bases replaced by a different one"""
    genome = rng.choice(ACGT, size=genome_len)
    idx = rng.integers(0, genome_len - RL, size=n_reads)[:, None] + np.arange(RL)[None, :]
    code = np.searchsorted(ACGT, genome)[idx]
    if error_rate:
        err = rng.random(code.shape) < error_rate
        code = np.where(err, (code + rng.integers(1, 4, size=code.shape)) & 3, code)
    return as_stream(np.sort(ACGT)[code])


# name: (k, abundance_min, stream)
STREAMS = {
    "all_distinct_k31": (31, 1, lambda rng: random_reads(rng, 32_000)),
    "all_distinct_k63": (63, 1, lambda rng: random_reads(rng, 36_000)),
    "repeats_k31": (31, 2, lambda rng: genome_reads(rng, 30_000, 36_000)),
    "repeats_k63": (63, 2, lambda rng: genome_reads(rng, 36_000, 36_000)),
    "mixed_k31": (31, 2, lambda rng: genome_reads(rng, 32_000, 32_000 * RL // 3, 0.01)),
    "mixed_k63": (63, 2, lambda rng: genome_reads(rng, 32_000, 32_000 * RL // 3, 0.01)),
}
_cases = {}


def case_of(oracle, name):
    """-> (k, abundance_min, stream, oracle count), made once"""
    if name not in _cases:
        k, amin, make = STREAMS[name]
        stream = make(np.random.default_rng(11))
        _cases[name] = (k, amin, stream, oracle.count(stream, k))
    return _cases[name]


def count_and_check(dev, k, amin, stream, ref):
    got = run_count(torch.from_numpy(np.ascontiguousarray(stream)).to(dev), k, amin, MAX, HMAX)
    st = got[3]
    assert st["n_levels"] == 2 and st["n_retries"] == 0
    check_exact(ref, k, got, amin, MAX, HMAX)
    return st


@pytest.mark.parametrize("name", ["all_distinct_k31", "all_distinct_k63"])
def test_every_key_claims(oracle, dev, name):
    k, amin, stream, ref = case_of(oracle, name)
    assert ref.distinct == ref.total                     # every key claims a slot
    st = count_and_check(dev, k, amin, stream, ref)
    assert st["n_solid"] == ref.total                    # abundance-min 1: every k-mer is a row


@pytest.mark.parametrize("name", ["repeats_k31", "repeats_k63"])
def test_most_waves_claim_nothing(oracle, dev, name):
    k, amin, stream, ref = case_of(oracle, name)
    assert ref.total / ref.distinct >= 50                # a sub-partition of ~2900 keys holds well under 64 distinct k-mers in 16 waves
    assert int(ref.ab.max()) < 4000                      # no k-mer fills a region by itself: no region chains
    count_and_check(dev, k, amin, stream, ref)


@pytest.mark.parametrize("name", ["mixed_k31", "mixed_k63"])
def test_claims_cross_a_pass_boundary(oracle, dev, name):
    k, amin, stream, ref = case_of(oracle, name)
    # a full wave's ~180 keys (k = 31; ~160 at k = 63) hold distinct / total of that many claims -- ~110 and ~130: the last pass is
    # partly filled at k = 31 and T lies on both sides of 128 at k = 63; the waves at the end of a sub-partition hold fewer keys
    # and come down to 64
    assert 0.5 < ref.distinct / ref.total < 0.9
    assert 0 < int((ref.ab >= amin).sum()) < ref.distinct            # rows and non-rows share the passes
    count_and_check(dev, k, amin, stream, ref)
