"""Dense inputs at small k for the graph layer: read streams whose k-mers fill a large share of the 4^k / 2 canonical k-mers, so that the
structures the graph kernels' guards and tie-breaks exist for -- palindromic rows, self-loops, hairpin edges, several edges between the same
two unitigs, ends with 4 targets, full flanks, ambiguous corrections -- occur many times in one input and all at once.  Used by
tests/test_dense_restatement.py (the restatements alone, on the CPU) and tests/test_gpu_dense.py (the device against them).

dense_stream(k, seed) is deterministic from np.random.default_rng and is meant to be counted with abundance_min = 1.  What it is made of:

  pieces       two (k <= 4) or three tiny isolated chains of fewer than 2 k rows, chosen first.  Their k-mers and every k-mer next to one of
               them are FORBIDDEN for everything below, which is what keeps them isolated in a graph that is otherwise one tangle: every
               random letter below is drawn among the letters that complete no forbidden window.
  G            the main genome, linear: three times the canonical space in windows at k <= 4 (it holds nearly all that is allowed), half the
               space at k = 5 and 6, and what the row cap leaves from k = 7 on (1 400 windows up to k = 8, 1 200 beyond: 18 % of the space
               at k = 7, 5 % at k = 8, less beyond).  Written twice forward and once as its reverse complement.
  planted      5 to 40 reads of 4 k - 1 letters round random positions of G, each written once, in turn: one substitution, a deletion of
               1 .. 3, an insertion of 1 .. 3, a dead end of 1 .. k - 1 letters, an exact copy.
  designed     at sites of G that are 3 k away from each other and that the planted reads keep 2 k + 3 letters away from (random positions
               where G is too short for that): a substitution written as often as G (a bubble of equally strong branches where G's windows
               occur nowhere else), a substitution written twice and a third allele written once (two trusted alternatives: an ambiguous
               correction), a stem off G that forks into two unequal dead ends (an outranked tip); from k = 8 on two substitutions 3 apart
               and a substitution next to an insertion (MULTI and COMPLEX); up to k = 6 three dead ends of one letter whose window no
               other read holds (a tail gap of one window, where most letters are trusted).
  circle       a second genome of 3 k letters written as a circle: a cycle unitig wherever its k-mers meet no other.
  degenerate   poly-A, the AT repeat, the AC repeat and, at even k, one explicit palindrome with four letters on either side.
"""
import numpy as np

# (k, seed) of every dense input; about ROW_CAP rows at the most, which holds the full restatement of one input to a few seconds
DENSE_CASES = [(3, 1), (4, 1), (5, 1), (6, 1), (6, 2), (7, 1), (8, 1), (9, 1), (9, 2), (10, 1), (12, 1), (14, 1)]
ROW_CAP = 2000

_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canon(s):
    r = revcomp(s)
    return s if s < r else r


def kmers_of(s, k):
    return [canon(s[i: i + k]) for i in range(len(s) - k + 1)]


def beside(kmer):
    """the canonical forms of the 8 k-mers next to one"""
    return {canon(kmer[1:] + b) for b in "ACGT"} | {canon(b + kmer[:-1]) for b in "ACGT"}


def space(k):
    return (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2


class Dense:
    """reads: every read in the order of the stream; the named parts as strings or lists of strings; forbidden: the set of canonical k-mers
    that only the pieces may touch"""


_made = {}


def dense_parts(k, seed):
    if (k, seed) in _made:
        return _made[(k, seed)]
    assert k >= 3
    rng = np.random.default_rng(31000 + 100 * k + seed)

    def rnd(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))

    def other(c):
        return "ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) & 3]

    degenerate = ["A" * (k + 5), "AT" * ((k + 21) // 2), "AC" * ((k + 21) // 2)]
    fixed = {x for r in degenerate for x in kmers_of(r, k)}

    # ---- the pieces and what they forbid
    pieces, own, forbidden = [], set(), set()
    for _ in range(2 if k <= 4 else 3):
        for _ in range(1000):
            rows = 1 if k <= 4 else int(rng.integers(1, 2 * k))
            p = rnd(k - 1 + rows)
            mine = set(kmers_of(p, k))
            near = set().union(*(beside(x) for x in mine)) - mine
            chain = all(len(beside(x) & mine) == (1 if i in (0, rows - 1) else 2) for i, x in enumerate(kmers_of(p, k))) if rows > 1 else True
            if len(mine) == rows and chain and not (mine | near) & (fixed | own) and not mine & forbidden:
                break
        else:
            raise AssertionError("no isolated piece found")
        pieces.append(p)
        own |= mine
        forbidden |= mine | near

    def ok(s):
        return not any(x in forbidden for x in kmers_of(s, k))

    def gen(n):
        """n random letters, none of which completes a forbidden window"""
        s = []
        while len(s) < n:
            allowed = [c for c in "ACGT" if len(s) < k - 1 or canon("".join(s[len(s) - k + 1:]) + c) not in forbidden]
            if allowed:
                s.append(allowed[int(rng.integers(0, len(allowed)))])
            else:                                                            # a dead end of the allowed k-mers: take the last window back
                del s[max(0, len(s) - k):]
        return "".join(s)

    def tried(make):
        """make() until it touches nothing forbidden; None when 200 draws all do"""
        for _ in range(200):
            r = make()
            if r is not None and ok(r):
                return r
        return None

    sp = space(k)
    n_main = 3 * sp if k <= 4 else min(sp // 2, (ROW_CAP * 7) // 10 if k <= 8 else (ROW_CAP * 6) // 10)
    G = gen(n_main + k - 1)
    n = len(G)
    reads = [G, G, revcomp(G)]

    # ---- the sites of the designed reads, 3 k apart, where G is long enough: the planted reads keep 2 k + 3 letters away from them
    grid = [int(x) for x in rng.permutation(np.arange(3 * k, n - 3 * k, 3 * k))] if n > 9 * k else []
    sites = grid[: 5 if k >= 8 else 3] if len(grid) >= 10 else []

    def spot():
        for _ in range(50):
            p = int(rng.integers(2 * k, n - 2 * k)) if n > 4 * k + 1 else int(rng.integers(k, n - k))
            if all(abs(p - s) > 2 * k + 3 for s in sites):
                break
        return p

    def left(p):
        return G[max(0, p - 2 * k + 1): p]

    # ---- planted reads, one of each kind in turn
    def planted_read(kind):
        p = spot()
        if kind == 0:
            return left(p) + other(G[p]) + G[p + 1: p + 2 * k]
        if kind == 1:
            d = int(rng.integers(1, 4))
            return left(p) + G[p + d: p + d + 2 * k - 1]
        if kind == 2:
            d = int(rng.integers(1, 4))
            return left(p) + rnd(d) + G[p: p + 2 * k - 1]
        if kind == 3:
            t = int(rng.integers(1, k))
            return left(p) + other(G[p]) + rnd(t - 1)
        return G[max(0, p - 2 * k + 1): p + 2 * k]

    n_planted = max(5, min(40, n_main // 40 * 5))
    planted = []
    for i in range(n_planted):
        r = tried(lambda: planted_read(i % 5))
        if r is not None:
            planted.append(r)
    reads += planted

    # ---- designed reads, each at a site of its own (a random position where G is too short for sites)
    places = list(sites)

    def place():
        return places.pop() if places else spot()

    designed = []
    p = place()                                                              # a substitution written as often as G: only the windows that hold it
    r = tried(lambda: G[max(0, p - (k - 1)): p] + other(G[p]) + G[p + 1: p + k])
    designed += [r] * 3 if r else []

    p = place()                                                              # one allele written twice, another once

    def two_alleles():
        x = other(G[p])
        y = [c for c in "ACGT" if c not in (G[p], x)][int(rng.integers(0, 2))]
        return left(p) + x + G[p + 1: p + 2 * k] + "\n" + left(p) + y + G[p + 1: p + 2 * k]
    r = tried(two_alleles)
    if r:
        strong, weak = r.split("\n")
        designed += [strong, strong, weak]

    p = place()                                                              # a stem off G that forks into two unequal dead ends

    def fork():
        stem = G[max(0, p - (k - 1)): p] + other(G[p]) + rnd(max(1, k // 2))
        a = rnd(1)
        return stem + a + rnd(max(0, k // 4 - 1)) + "\n" + stem + other(a) + rnd(max(1, k // 2) - 1)
    r = tried(fork)
    if r:
        short, long_ = r.split("\n")
        designed += [short, long_, long_]
    if k >= 8:
        p = place()                                                          # two substitutions 3 apart
        r = tried(lambda: left(p) + other(G[p]) + G[p + 1: p + 3] + other(G[p + 3]) + G[p + 4: p + 2 * k + 3])
        designed += [r] if r else []
        p = place()                                                          # a substitution and two inserted letters
        r = tried(lambda: left(p) + other(G[p]) + rnd(2) + G[p + 1: p + 2 * k])
        designed += [r] if r else []
    if k <= 6:                                                               # dead ends of one letter whose window no read so far holds
        seen = {x for r in reads + designed for x in kmers_of(r, k)}
        for _ in range(3):
            def lone_tail():
                q = spot()
                r = left(q) + other(G[q])
                return r if canon(r[-k:]) not in seen else None
            r = tried(lone_tail)
            if r:
                designed.append(r)
                seen.add(canon(r[-k:]))
    reads += designed

    # ---- the circle, the pieces, the degenerate reads
    C = gen(3 * k)
    circle = tried(lambda: C + C[: k - 1]) or C
    reads.append(circle)
    reads += pieces
    palindrome = None
    if k % 2 == 0:
        def pal():
            h = rnd(k // 2)
            return rnd(4) + h + revcomp(h) + rnd(4)
        palindrome = tried(pal)
        assert palindrome is not None
        degenerate = degenerate + [palindrome]
    reads += degenerate

    out = Dense()
    out.k, out.seed, out.reads, out.forbidden = k, seed, reads, forbidden
    out.G, out.planted, out.designed, out.circle, out.pieces, out.degenerate, out.palindrome = G, planted, designed, circle, pieces, degenerate, palindrome
    out.stream = np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy()
    _made[(k, seed)] = out
    return out


def dense_stream(k, seed):
    """the read stream (np.uint8, reads ended by a newline) of the dense input (k, seed); the same array every time, never to be changed"""
    return dense_parts(k, seed).stream
