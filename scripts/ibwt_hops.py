"""Host model of the inverse BWT's splitter geometry (csrc/ibwt.hip, main path) for one block given as
any byte string L and any primary index pi < len(L): the transform, the splitter step, the hop every
splitter walks, the cycle through pi, the overflow chunks the walk claims and k_ib_scan's verdict on
two-step walking.  Plain numpy; imports nothing from the library.  The tests use it to say which
kernel paths an input reaches (tests/ibwt_cases.py) and what bra_gpu_debug_ibwt_path must report.

    python scripts/ibwt_hops.py random N ALPHABET PI [SEED]
    python scripts/ibwt_hops.py rotation N A PI          L = 1^A 0^(N-A): T(y) = y + A mod N
"""
import sys
from dataclasses import dataclass

import numpy as np

IB_MAXS = 16385   # splitters per block: 16384 regular ones and the primary index
IB_CHUNK = 256    # bytes of an overflow chunk
PAIR_SHIFT = 6    # a batch whose largest shift is above this launches the two-step walk kernels


def geometry(n: int):
    """(shift, ns): the splitter step S = 2^shift and the number of regular splitters 0, S, 2S, ..."""
    shift = 6
    while ((n + (1 << shift) - 1) >> shift) > IB_MAXS - 1:
        shift += 1
    return shift, (n + (1 << shift) - 1) >> shift


def transform(L: np.ndarray) -> np.ndarray:
    """The reference's transform: T[first[c] + k] = position of the k-th c in L."""
    return np.argsort(np.asarray(L, np.uint8), kind="stable")


def suits_pairs(L: np.ndarray) -> bool:
    """k_ib_scan's rule: bytes that hold at most 1/32 of the positions each are rare; a block in which
    the rare bytes together hold a quarter of the positions or more is walked one step per load."""
    cnt = np.bincount(np.asarray(L, np.uint8), minlength=256).astype(np.int64)
    n = int(cnt.sum())
    rare = int(cnt[32 * cnt <= n].sum())
    return not 4 * rare >= n


def pool_capacity(nsplit: int) -> int:
    """Overflow chunks a context holds whose largest batch so far had nsplit splitters in all
    (IbwtWorkspace::reserve_main)."""
    c = nsplit + nsplit // 8 + 64
    return c // 8 + 256


def walk_mode(blocks) -> str:
    """"one" / "two" / "one_if" for a batch of Hops: what the walk kernels of one call do."""
    if max(h.shift for h in blocks) <= PAIR_SHIFT:
        return "one"
    return "two" if all(h.pairs for h in blocks) else "one_if"


@dataclass
class Hops:
    n: int
    pi: int
    shift: int
    ns: int
    T: np.ndarray          # the transform
    hop_len: np.ndarray    # per splitter id (ns + 1 entries; id ns = the primary index when it is no
    hop_next: np.ndarray   # regular splitter, else unused: length 0, next -1): bytes walked, next id
    primary: int           # id of the primary splitter
    cycle: int             # length of the cycle through pi
    chain: np.ndarray      # ids of the hops on that cycle, in output order
    chunks: int            # overflow chunks claimed by all walked hops
    pairs: bool            # suits_pairs(L)

    @property
    def S(self) -> int:
        return 1 << self.shift

    @property
    def nsplit(self) -> int:
        return self.ns + 1


def hops(L: np.ndarray, pi: int) -> Hops:
    L = np.asarray(L, np.uint8)
    n = int(L.size)
    assert 0 <= pi < n
    shift, ns = geometry(n)
    S = 1 << shift
    T = transform(L)
    split = np.zeros(n, bool)
    split[::S] = True
    split[pi] = True
    extra = pi % S != 0
    start = np.arange(0, n, S, dtype=np.int64)
    if extra:
        start = np.append(start, pi)
    # f = T with the splitters made absorbing; after k rounds jump = f^(2^k) and steps counts the
    # positions before absorption among the first 2^k of the orbit.  Every start lies on a cycle
    # with a splitter (itself), so its successor is absorbed after at most log2(n) + 1 rounds.
    first = T[start]
    jump = np.where(split, np.arange(n, dtype=np.int64), T)
    steps = (~split).astype(np.int64)
    while not split[jump[first]].all():
        steps = steps + steps[jump]
        jump = jump[jump]
    end = jump[first]
    hop_len = np.zeros(ns + 1, np.int64)
    hop_next = np.full(ns + 1, -1, np.int64)
    ids = np.where((end == pi) & extra, ns, end >> shift)
    hop_len[: start.size] = 1 + steps[first]
    hop_next[: start.size] = ids
    primary = ns if extra else pi >> shift
    chain, k, cycle = [], primary, 0
    while True:
        chain.append(k)
        cycle += int(hop_len[k])
        k = int(hop_next[k])
        if k == primary:
            break
    over = np.maximum(hop_len - 4 * S, 0)
    chunks = int(((over + IB_CHUNK - 1) // IB_CHUNK).sum())
    return Hops(n, pi, shift, ns, T, hop_len, hop_next, primary, cycle, np.asarray(chain, np.int64), chunks, suits_pairs(L))


def decode(L: np.ndarray, h: Hops) -> np.ndarray:
    """The block's decoded bytes from the model's own hops (n steps from pi, the cycle repeated): a
    check of the model against a plain inverse BWT, not an expected value for the library."""
    L = np.asarray(L, np.uint8)
    k, cyc = h.pi, np.empty(h.cycle, np.int64)
    for i in range(h.cycle):
        k = cyc[i] = h.T[k]
    return L[cyc][np.arange(h.n) % h.cycle]


def rotation(n: int, a: int) -> np.ndarray:
    """L = 1^a 0^(n-a): T(y) = y + a mod n."""
    L = np.zeros(n, np.uint8)
    L[:a] = 1
    return L


def describe(h: Hops) -> str:
    walked = h.hop_len[h.hop_len > 0]
    return (f"n {h.n} pi {h.pi}: S {h.S}, {h.ns} regular splitters, primary splitter {h.primary}; cycle {h.cycle} in {h.chain.size} hops"
            f"{'' if h.cycle == h.n else ' (n %% cycle = %d)' % (h.n % h.cycle)}; hops: longest {int(walked.max())}, "
            f"{int((walked > 4 * h.S).sum())} past the slot, {h.chunks} overflow chunks (a one-block context holds {pool_capacity(h.nsplit)}); "
            f"residues mod 16 seen {np.unique(walked % 16).size}; suits two-step walking: {h.pairs}")


if __name__ == "__main__":
    kind, n, x, pi = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    if kind == "rotation":
        blk = rotation(n, x)
    else:
        blk = np.random.default_rng(int(sys.argv[5]) if len(sys.argv) > 5 else 0).integers(0, x, n, dtype=np.uint8)
    print(describe(hops(blk, pi)))
