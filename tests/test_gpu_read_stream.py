"""The read stream and the bank ends across the calls that change them: dskgpu_push_reads / _push_raw / _reserve_reads / _rewind_reads /
_set_reads_device on one side (csrc/reads.hip), dskgpu_next_bank / _set_banks and the per-bank count on the other (csrc/banks.hip).

Each owns its state, and each of these sequences makes one of them act on what the other holds: a rewind drops bank ends, a new device
read set clears them, next_bank finishes a pending raw ingest, a per-bank count borrows the context's configuration and read stream and
gives them back.  Expected values: the CPU oracle, per bank through the numpy restatement of the solidity kinds (_bank_reference).
"""
import numpy as np
import pytest

from tests.test_gpu_parity import _bank_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

AMAX = 2**31 - 1
N_READS, READ_LEN, GENOME = 2000, 100, 10_000      # 20x of a 10 kbp genome per stream: A and B share most of their k-mers


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def streams(dev):
    """A, B and a third stream that only ever gets rewound away: uint8 arrays, every read followed by its newline"""
    from dsk_amd import synth
    genome = synth.make_genome(GENOME, dev)
    return [synth.make_reads(genome, N_READS, READ_LEN, seed=synth.SEED + 1 + i).cpu().numpy() for i in range(3)]


@pytest.fixture(scope="module")
def references(oracle, streams):
    """computed once, read by several cases: (k, kind, amin) -> _bank_reference of [A, B]"""
    memo = {}

    def get(k, kind, amin):
        if (k, kind, amin) not in memo:
            memo[(k, kind, amin)] = _bank_reference(oracle, streams[:2], k, kind, amin, AMAX, 0)
        return memo[(k, kind, amin)]
    return get


def keys_of(kmers, k):
    """the rows' k-mers as _bank_reference has them: the low word for k <= 32, Python integers above"""
    if k <= 32:
        return kmers[:, 0]
    return np.array([(int(h) << 64) | int(l) for l, h in zip(kmers[:, 0], kmers[:, 1])], dtype=object)


def as_fasta(stream):
    return b"".join(b">r\n" + r + b"\n" for r in bytes(stream).split(b"\n")[:-1])


def check_banks(kc, k, want, with_2d):
    want_k, want_a, want_h, want_h2, want_total = want
    kmers, ab = kc.rows()
    st = kc.stats()
    assert st["n_kmers"] == want_total and st["n_solid"] == len(want_k)
    assert (keys_of(kmers, k) == want_k).all() and (ab == want_a).all()
    assert (kc.histogram() == want_h).all()
    if with_2d:
        assert (kc.histogram2d() == want_h2).all()


@pytest.mark.parametrize("k", [27, 41])
def test_rewind_forgets_the_banks_beyond_it(streams, references, k):
    """A | other | rewind to the end of A | B: two banks.  A bank end left behind by the rewound reads would make three banks, one of them
    empty, and "min" would then keep no row at all."""
    from dsk_amd import KmerCounter
    A, B, other = streams
    want = references(k, "min", 1)
    assert len(want[0]) > 0
    with KmerCounter(kmer_size=k, abundance_min=1, solidity_kind="min", histo2d=True) as kc:
        kc.push_reads(A)
        kc.next_bank()
        mark = kc.stream_bytes()
        assert mark == len(A) + 1
        kc.push_reads(other)
        kc.next_bank()
        kc.rewind_reads(mark)
        kc.push_reads(B)
        kc.next_bank()
        kc.count()
        check_banks(kc, k, want, True)


@pytest.mark.parametrize("k", [27, 41])
def test_new_device_reads_forget_the_banks_and_the_job_restores_the_configuration(oracle, dev, streams, references, k):
    """A per-bank count runs its banks with the abundance window 1 .. max and unsorted rows.  The plain count after it, on a read set given
    anew and without banks, must see abundance_min = 3 and sorted rows again, and no bank end of the old read set."""
    from dsk_amd import KmerCounter
    A, B, _ = streams
    whole_np = np.concatenate([A, B])
    whole = torch.from_numpy(whole_np).to(dev)
    with KmerCounter(kmer_size=k, abundance_min=3, solidity_kind="max") as kc:
        kc.set_reads_device(whole.data_ptr(), whole.numel())
        kc.set_banks([len(A), len(A) + len(B)])
        kc.count()
        check_banks(kc, k, references(k, "max", 3), False)
        kc.set_reads_device(whole.data_ptr(), whole.numel())
        kc.count()
        kmers, ab = kc.rows()
        st = kc.stats()
    ref = oracle.count(whole_np, k)
    _, _, rab = ref.solid(3)
    keep = ref.ab >= 3
    assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct and st["n_solid"] == len(rab)
    assert kmers.shape == (len(rab), (k + 31) // 32)
    assert (kmers == ref.words()[keep]).all()      # the oracle's order: ascending
    assert (ab == rab).all()


@pytest.mark.parametrize("k", [27, 41])
def test_raw_text_bank_by_bank(streams, references, k):
    """The same two banks as FASTA text: next_bank must finish the raw ingest before it reads the stream's length."""
    from dsk_amd import KmerCounter
    want = references(k, "min", 1)
    with KmerCounter(kmer_size=k, abundance_min=1, solidity_kind="min", histo2d=True) as kc:
        for s in streams[:2]:
            kc.push_raw(as_fasta(s), kc.RAW_FASTA, new_file=True)
            kc.next_bank()
        kc.count()
        check_banks(kc, k, want, True)


def test_mixed_growth_keeps_the_stream(oracle, streams):
    """The stream buffer grows under each of its three callers with reads in it.  A push never allocates less than 256 MB, so the raw
    push has to bring more than that to grow the buffer again: a FASTA header line of 257 MB, of which the stream keeps one newline."""
    from dsk_amd import KmerCounter
    A, B, other = streams
    k, cut = 27, 40 * (READ_LEN + 1)            # (between two reads)
    pad = np.full((257 << 20) + 2, ord("h"), np.uint8)
    pad[0], pad[-1] = ord(">"), ord("\n")
    raw = np.concatenate([pad, np.frombuffer(as_fasta(B)[len(b">r\n"):], np.uint8)])      # B's first record under the long header
    with KmerCounter(kmer_size=k, abundance_min=1) as kc:
        kc.reserve_reads(8 << 10)
        kc.push_reads(A[:cut])                  # fits what was reserved
        kc.push_reads(A[cut:])                  # outgrows it: 256 MB
        kc.push_raw(raw, kc.RAW_FASTA, new_file=True)      # outgrows that
        nbytes, records = kc.raw_finish()
        assert records == N_READS
        kc.reserve_reads(1 << 20)               # smaller: nothing happens
        assert kc.stream_bytes() == nbytes
        kc.push_reads(other)
        kc.reserve_reads(600 << 20)             # larger than everything so far: grows with all three parts in it
        kc.count()
        kmers, ab = kc.rows()
        st = kc.stats()
        hist = kc.histogram()
    ref = oracle.count(np.concatenate([A, B, other]), k)
    _, _, rab = ref.solid(1)
    assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
    assert (kmers == ref.words()).all() and (ab == rab).all()
    assert (hist == ref.histogram(10000)).all()
